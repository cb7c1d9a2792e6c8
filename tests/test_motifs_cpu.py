"""Host side of motif mining (cg_window_keep, cg_window_pool, cg_kmeans_step and codonlm_amd.motifs):
the ABI additions, the argument checks that return before any launch, and the host logic -- PCA,
PWM / consensus / report, and the k-means driver (seeding, Lloyd loop, empty-cluster rule, stopping
rule) against an fp64 numpy restatement, with ops.kmeans_step replaced by a numpy stub.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
FAKE = 4096  # a non-NULL pointer value: every call below returns before anything reads it


# ------------------------------------------------------------------ ABI
def test_symbols_struct_mirror_and_version():
    from codonlm_amd import _lib as L
    for name in ("cg_window_keep", "cg_window_pool", "cg_kmeans_step", "cg_kmeans_workspace"):
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert L.lib.cg_struct_bytes(b"cg_kmeans_desc") == ctypes.sizeof(L.KMeansDesc) > 0
    assert L.lib.cg_version().decode() == "codonlm_hip 0.6 gfx950"  # additions only
    header = (ROOT / "include" / "codonlm_hip.h").read_text()
    assert int(re.search(r"#define CG_KMEANS_CHUNK (\d+)", header).group(1)) == L.KMEANS_CHUNK


def test_window_keep_argument_checks():
    from codonlm_amd import _lib as L
    mask = (ctypes.c_uint32 * 8)()

    def call(idx=FAKE, B=2, T=40, window=9, stride=3, m=mask, keep=FAKE):
        return L.lib.cg_window_keep(idx, B, T, window, stride, m, keep, None)
    assert call(idx=None) == L.CG_EINVAL and call(keep=None) == L.CG_EINVAL and call(m=None) == L.CG_EINVAL
    assert call(window=0) == L.CG_EINVAL and call(stride=0) == L.CG_EINVAL
    assert call(B=-1) == L.CG_EINVAL and call(T=-1) == L.CG_EINVAL
    assert call(B=0) == L.CG_OK and call(B=0, idx=None, keep=None) == L.CG_OK
    assert call(T=8) == L.CG_OK  # T < window: no window, nothing to launch
    assert call(B=0, window=0) == L.CG_EINVAL  # a bad window stays an error


def test_window_pool_argument_checks():
    from codonlm_amd import _lib as L

    def call(dt=L.CG_F32, h=FAKE, ldh=64, B=2, T=40, d=64, window=9, stride=3, dst=FAKE, out=FAKE, ldo=64, rows=22):
        return L.lib.cg_window_pool(dt, h, ldh, B, T, d, window, stride, dst, out, ldo, rows, None)
    assert call(h=None) == L.CG_EINVAL and call(dst=None) == L.CG_EINVAL and call(out=None) == L.CG_EINVAL
    assert call(ldh=63) == L.CG_EINVAL and call(ldo=63) == L.CG_EINVAL
    assert call(window=0) == L.CG_EINVAL and call(stride=0) == L.CG_EINVAL and call(rows=-1) == L.CG_EINVAL
    assert call(dt=L.CG_BF16X2) == L.CG_EUNSUPPORTED
    assert call(B=0) == L.CG_OK and call(B=0, h=None, dst=None, out=None) == L.CG_OK
    assert call(T=8) == L.CG_OK and call(d=0, ldh=0, ldo=0) == L.CG_OK


def test_kmeans_step_argument_checks():
    from codonlm_amd import _lib as L
    need = L.lib.cg_kmeans_workspace(1000, 50, 10)
    assert need > 0 and L.lib.cg_kmeans_workspace(10000, 50, 10) > need
    assert L.lib.cg_kmeans_workspace(0, 50, 10) == 0

    def call(**kw):
        a = dict(x=FAKE, ldx=50, n=1000, d=50, centers=FAKE, ldc=50, k=10, labels=FAKE, dist2=FAKE, sums=FAKE,
                 counts=FAKE, inertia=FAKE, workspace=FAKE, ws_bytes=need)
        a.update(kw)
        p = L.KMeansDesc()
        for f, v in a.items():
            setattr(p, f, v)
        return L.lib.cg_kmeans_step(ctypes.byref(p), None)
    assert L.lib.cg_kmeans_step(None, None) == L.CG_EINVAL
    for f in ("x", "centers", "labels", "workspace"):
        assert call(**{f: None}) == L.CG_EINVAL, f
    assert call(ldx=49) == L.CG_EINVAL and call(ldc=49) == L.CG_EINVAL and call(n=-1) == L.CG_EINVAL
    assert call(counts=None) == L.CG_EINVAL  # sums without counts
    assert call(k=0) == L.CG_EUNSUPPORTED and call(k=257) == L.CG_EUNSUPPORTED
    assert call(d=0) == L.CG_EUNSUPPORTED and call(d=1025, ldx=1025, ldc=1025) == L.CG_EUNSUPPORTED
    assert call(ws_bytes=need - 1) == L.CG_EINVAL and call(ws_bytes=0) == L.CG_EINVAL
    assert call(workspace=FAKE + 4) == L.CG_EINVAL  # not 16-byte aligned
    assert call(n=0) == L.CG_OK and call(n=0, x=None, centers=None, labels=None, workspace=None, ws_bytes=0) == L.CG_OK


# ------------------------------------------------------------------ PCA, PWM, report
def test_pca_project_against_numpy_svd():
    from codonlm_amd import motifs as M
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 7)) * np.array([5.0, 3.0, 2.0, 1.0, 0.5, 0.2, 0.1]) + rng.standard_normal(7)
    Y, comp, mean = M.pca_project(torch.from_numpy(X), 4, chunk=64)  # several row chunks
    assert Y.dtype == torch.float64 and tuple(Y.shape) == (200, 4) and tuple(comp.shape) == (4, 7)
    Xc = X - X.mean(0)
    _, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    want_var = S[:4] ** 2 / 199
    got_var = Y.numpy().var(0, ddof=1)
    assert np.abs(got_var - want_var).max() <= 1e-10 * want_var.max()
    assert np.abs(got_var / want_var - 1).max() <= 1e-10
    assert np.abs(mean.numpy() - X.mean(0)).max() <= 1e-13
    V = Vt[:4] * np.sign(Vt[:4][np.arange(4), np.abs(Vt[:4]).argmax(1)])[:, None]  # the stated sign rule
    assert np.abs(comp.numpy() - V).max() <= 1e-9
    c = comp.numpy()
    assert (c[np.arange(4), np.abs(c).argmax(1)] > 0).all()
    assert np.abs(Y.numpy() - Xc @ V.T).max() <= 1e-9
    # the cap min(n_components, d, N), and fp32 in -> fp32 out
    Y3, comp3, _ = M.pca_project(torch.from_numpy(X[:3].astype(np.float32)), 50)
    assert tuple(Y3.shape) == (3, 3) and Y3.dtype == torch.float32 and tuple(comp3.shape) == (3, 7)
    assert tuple(M.pca_project(torch.from_numpy(X), 50)[0].shape) == (200, 7)


def test_pwm_and_consensus_hand_counted():
    from codonlm_amd import motifs as M
    vocab = ["<PAD>", "AAA", "CCC", "GGG"]
    seqs = [["AAA", "CCC", "GGG"], ["AAA", "GGG", "GGG"], ["CCC", "CCC", "XXX"], ["AAA", "GGG", "AAA"]]
    pwm = M.calculate_pwm(seqs, vocab)
    want = np.array([[0, 0, 0], [3, 0, 1], [1, 2, 0], [0, 2, 2]]) / 4.0  # XXX is outside the vocabulary
    assert pwm.shape == (4, 3) and np.array_equal(pwm, want)
    assert M.get_consensus(pwm, vocab) == "AAACCCGGG"  # position 1 ties CCC / GGG: first in vocabulary order
    assert M.calculate_pwm([], vocab).size == 0 and M.get_consensus(M.calculate_pwm([], vocab), vocab) == ""


def test_report_orders_clusters_by_size_then_first_appearance():
    from codonlm_amd import motifs as M
    labels = np.array([2, 0, 0, 1, 1, 2, 2, 2, 2, 2, 2])
    assert M.cluster_order(labels) == [2, 0, 1]
    vocab = ["<PAD>", "AAA", "CCC"]
    windows = [["AAA", "CCC"] if i % 2 else ["CCC", "CCC"] for i in range(len(labels))]
    rep = M.build_report("r1", 4, labels, windows, vocab, "kmeans", -1)
    lines = rep.split("\n")
    assert lines[:7] == ["# Motif Mining Report: r1", "", "- **Sequences sampled:** 4", "- **Total windows:** 11",
                         "- **Method:** kmeans", "- **Layer:** -1", ""]
    heads = [ln for ln in lines if ln.startswith("## ")]
    assert heads == ["## Cluster 2 (size=7)", "## Cluster 0 (size=2)", "## Cluster 1 (size=2)"]
    sizes = [int(re.search(r"size=(\d+)", h).group(1)) for h in heads]
    assert sum(sizes) == len(labels)
    first = lines.index("## Cluster 2 (size=7)")
    assert lines[first + 1] == "**Consensus:** `CCCCCC`" and lines[first + 3] == "**Top 5 Examples:**"
    assert lines[first + 4:first + 10] == ["- `CCC CCC`", "- `AAA CCC`", "- `CCC CCC`", "- `AAA CCC`", "- `CCC CCC`", ""]
    meta = np.array([[0, 0, 2], [1, 1, 3]])
    assert M.window_tokens(np.array([[1, 2, 0], [0, 2, 7]]), meta, vocab) == [["AAA", "CCC"], ["CCC", "tok_7"]]
    assert np.array_equal(M.window_meta(np.array([[1, 0, 1], [0, 0, 1]]), 9, 3),
                          [[0, 0, 9], [0, 6, 15], [1, 6, 15]])


def test_unsupported_requests_fail_clearly(capsys):
    from codonlm_amd import mine_motifs as C
    from codonlm_amd import motifs as M
    with pytest.raises(ValueError, match="not on the MI355X path"):
        M.check_method("hdbscan")
    with pytest.raises(ValueError, match="not on the MI355X path"):
        M.mine(None, np.zeros((1, 9), np.int64), method="hdbscan")
    with pytest.raises(SystemExit):
        C.main(["--run_dir", "nowhere", "--data_npz", "none.npz", "--method", "hdbscan"])
    assert "not on the MI355X path" in capsys.readouterr().err
    with pytest.raises(ValueError, match="lists of layers"):
        M.window_embeddings(None, np.zeros((1, 9), np.int64), 9, 3, layer=[0, 1])
    a = C.build_parser().parse_args(["--run_id", "r", "--data_npz", "d.npz"])
    assert (a.n_samples, a.window_size, a.stride, a.n_clusters, a.method, a.pca, a.layer, a.seed) == \
        (100, 9, 3, 10, "kmeans", 50, -1, 42)
    toks = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>", "AAA", "<eog>"]
    assert sorted(C.special_ids(toks)) == [0, 1, 2, 3, 5]


# ------------------------------------------------------------------ the k-means driver against numpy
def np_step(X, Cn):
    """The contract of cg_kmeans_step in fp64 from fp32 operands: lowest index on ties."""
    X64, C64 = X.astype(np.float64), Cn.astype(np.float64)
    d2 = ((X64[:, None, :] - C64[None]) ** 2).sum(-1)
    lab = d2.argmin(1)
    dist = d2[np.arange(len(X)), lab].astype(np.float32)
    k = len(Cn)
    sums = np.zeros((k, X.shape[1]))
    np.add.at(sums, lab, X64)
    return lab.astype(np.int32), dist, sums, np.bincount(lab, minlength=k).astype(np.int64)


@pytest.fixture
def stub_step(monkeypatch):
    from codonlm_amd import ops
    calls = []

    def step(x, centers, *, want_dist2=True, want_stats=True, want_inertia=True, workspace=None):
        lab, dist, sums, counts = np_step(x.numpy(), centers.numpy())
        calls.append((want_dist2, want_stats, want_inertia))
        r = ops.KMeansStep(labels=torch.from_numpy(lab))
        if want_dist2:
            r.dist2 = torch.from_numpy(dist)
        if want_stats:
            r.sums, r.counts = torch.from_numpy(sums), torch.from_numpy(counts)
        if want_inertia:
            r.inertia = torch.tensor(float(dist.astype(np.float64).sum()), dtype=torch.float64)
        return r
    monkeypatch.setattr(ops, "kmeans_step", step)
    return calls


def ref_pp(X, k, seed):
    N = len(X)
    u = np.random.default_rng(seed).random(k)
    chosen = [min(int(np.floor(u[0] * N)), N - 1)]
    mind = np_step(X, X[chosen[-1:]])[1]
    for c in range(1, k):
        cum = np.cumsum(mind.astype(np.float64))
        if cum[-1] > 0:
            i = min(int(np.searchsorted(cum, u[c] * cum[-1], side="right")), N - 1)
        else:
            i = min(j for j in range(N) if j not in chosen)
        chosen.append(i)
        mind = np.minimum(mind, np_step(X, X[i:i + 1])[1])
    return X[chosen].copy(), chosen


def ref_kmeans(X, k, seed=42, max_iter=300, tol=1e-4, init=None):
    """Lloyd's algorithm as the issue states it, restated on numpy arrays."""
    Cn = (ref_pp(X, k, seed)[0] if init is None else np.asarray(init)).astype(np.float32)
    tol_abs = tol * X.astype(np.float64).var(0).mean()
    prev = np.full(len(X), -1)
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        lab, dist, sums, counts = np_step(X, Cn)
        empty = np.nonzero(counts == 0)[0]
        if len(empty):
            far = np.argsort(-dist, kind="stable")[:len(empty)]
            for e, i in zip(empty, far):
                sums[lab[i]] -= X[i]
                counts[lab[i]] -= 1
                sums[e], counts[e] = X[i], 1
        new = Cn.astype(np.float64)
        new[counts > 0] = sums[counts > 0] / counts[counts > 0, None]
        new = new.astype(np.float32)
        shift = ((new.astype(np.float64) - Cn) ** 2).sum()
        changed = (lab != prev).any()
        Cn, prev = new, lab
        if not changed or (not len(empty) and shift <= tol_abs):
            break
    lab, dist, _, _ = np_step(X, Cn)
    return lab, Cn, float(dist.astype(np.float64).sum()), n_iter


def _blobs(N=300, d=5, seed=1):
    rng = np.random.default_rng(seed)
    planted = np.arange(N) % 3
    means = np.array([[0.0] * d, [20.0] * d, [-20.0, 20.0] + [0.0] * (d - 2)])
    X = (means[planted] + rng.standard_normal((N, d))).astype(np.float32)
    init = (means + 3.0 * rng.standard_normal((3, d))).astype(np.float32)
    return X, planted, init


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_lloyd_driver_with_init_matches_the_restatement(stub_step):
    from codonlm_amd import motifs as M
    X, planted, init = _blobs()
    lab, cen, inertia, n_iter = M.kmeans(torch.from_numpy(X), 3, init=torch.from_numpy(init))
    rl, rc, ri, rn = ref_kmeans(X, 3, init=init)
    assert lab.dtype == torch.int32 and cen.dtype == torch.float32 and isinstance(inertia, float)
    assert np.array_equal(lab.numpy(), rl) and np.array_equal(cen.numpy(), rc) and n_iter == rn and inertia == ri
    assert np.array_equal(lab.numpy(), planted)  # init row c lies next to blob c
    # one step with statistics per iteration, one assign-only step at the end
    assert stub_step == [(True, True, False)] * n_iter + [(True, False, True)]
    # labels and inertia belong to the returned centres
    l2, d2, _, _ = np_step(X, cen.numpy())
    assert np.array_equal(l2, lab.numpy()) and inertia == float(d2.astype(np.float64).sum())


def test_lloyd_driver_matches_sklearn_partition(stub_step):
    cluster = pytest.importorskip("sklearn.cluster")
    from codonlm_amd import motifs as M
    X, planted, init = _blobs()
    lab = M.kmeans(torch.from_numpy(X), 3, init=torch.from_numpy(init))[0].numpy()
    sk = cluster.KMeans(n_clusters=3, init=init, n_init=1, algorithm="lloyd").fit(X)
    assert _same_partition(lab, sk.labels_) and np.array_equal(lab, sk.labels_)


def test_kmeans_pp_seeding(stub_step):
    from codonlm_amd import motifs as M
    rng = np.random.default_rng(5)
    X = rng.standard_normal((157, 4)).astype(np.float32)
    for seed in (42, 0, 9):
        want, chosen = ref_pp(X, 6, seed)
        got = M.kmeans_pp_init(torch.from_numpy(X), 6, seed).numpy()
        assert np.array_equal(got, want) and len(set(chosen)) == 6
        assert chosen[0] == int(np.floor(np.random.default_rng(seed).random(6)[0] * 157))
    # seeded runs: the same seed gives the same result, and the whole run equals the restatement
    a = M.kmeans(torch.from_numpy(X), 6, seed=9)
    b = M.kmeans(torch.from_numpy(X), 6, seed=9)
    r = ref_kmeans(X, 6, seed=9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    assert np.array_equal(a[0].numpy(), r[0]) and np.array_equal(a[1].numpy(), r[1]) and a[2:] == r[2:]
    # all points equal: every total is 0, so the lowest row not yet chosen follows
    Z = np.ones((10, 3), np.float32)
    first = int(np.floor(np.random.default_rng(3).random(4)[0] * 10))
    assert ref_pp(Z, 4, 3)[1] == [first] + [j for j in range(10) if j != first][:3]
    Zd = np.concatenate([Z, 2 * Z[:2]])  # two values only: the total is 0 again once both are centres
    got = M.kmeans_pp_init(torch.from_numpy(Zd), 4, 3).numpy()
    assert np.array_equal(got, ref_pp(Zd, 4, 3)[0])
    assert np.array_equal(M.kmeans_pp_init(torch.from_numpy(Z), 4, 3).numpy(), Z[:4])


def test_empty_cluster_takes_the_farthest_point(stub_step):
    from codonlm_amd import motifs as M
    X, _, init = _blobs(N=90)
    far_init = np.concatenate([init, np.full((2, 5), 1e4, np.float32)])  # two centres that win no point
    lab0, dist0, _, counts0 = np_step(X, far_init)
    assert counts0[3] == 0 and counts0[4] == 0
    # after one iteration: cluster 3 is the farthest point, cluster 4 the second farthest
    cen1 = M.kmeans(torch.from_numpy(X), 5, init=torch.from_numpy(far_init), max_iter=1)[1].numpy()
    order = np.argsort(-dist0, kind="stable")
    assert np.array_equal(cen1[3], X[order[0]]) and np.array_equal(cen1[4], X[order[1]])
    # the donors lost those points
    for c in range(3):
        members = [i for i in np.nonzero(lab0 == c)[0] if i not in order[:2]]
        assert np.array_equal(cen1[c], X[members].astype(np.float64).mean(0).astype(np.float32))
    got = M.kmeans(torch.from_numpy(X), 5, init=torch.from_numpy(far_init))
    want = ref_kmeans(X, 5, init=far_init)
    assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]) and got[3] == want[3]
    assert np.bincount(got[0].numpy(), minlength=5).min() >= 1
    # ties in dist2 go to the lowest index
    T = np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)
    init_t = np.array([[0, 0], [50, 50]], np.float32)
    cen_t = M.kmeans(torch.from_numpy(T), 2, init=torch.from_numpy(init_t), max_iter=1)[1].numpy()
    assert np.array_equal(cen_t[1], T[1])  # rows 1..4 are all at distance 1: row 1 wins


def test_stopping_rule(stub_step):
    from codonlm_amd import motifs as M
    rng = np.random.default_rng(11)
    X = rng.standard_normal((400, 3)).astype(np.float32)
    Xt = torch.from_numpy(X)
    init = X[:7].copy()
    full = M.kmeans(Xt, 7, init=torch.from_numpy(init), tol=0.0)  # only "no label changed" can stop it
    ref = ref_kmeans(X, 7, init=init, tol=0.0)
    assert full[3] == ref[3] > 3 and np.array_equal(full[0].numpy(), ref[0])
    # a huge tolerance stops after the first update, max_iter caps the loop
    assert M.kmeans(Xt, 7, init=torch.from_numpy(init), tol=1e9)[3] == 1
    assert M.kmeans(Xt, 7, init=torch.from_numpy(init), tol=0.0, max_iter=2)[3] == 2
    # a tolerance in between stops where the restatement does, and earlier than tol = 0
    mid = M.kmeans(Xt, 7, init=torch.from_numpy(init), tol=1e-2)
    rmid = ref_kmeans(X, 7, init=init, tol=1e-2)
    assert mid[3] == rmid[3] < full[3] and np.array_equal(mid[1].numpy(), rmid[1])
    # inertia never grows with more iterations
    inert = [M.kmeans(Xt, 7, init=torch.from_numpy(init), tol=0.0, max_iter=i)[2] for i in range(0, 6)]
    assert all(b <= a for a, b in zip(inert, inert[1:]))
    with pytest.raises(ValueError, match="n_clusters"):
        M.kmeans(Xt[:5], 6)
    with pytest.raises(ValueError, match="n_clusters"):
        M.kmeans(Xt, 0)
