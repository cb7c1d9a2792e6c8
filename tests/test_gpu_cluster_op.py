"""cg_window_keep, cg_window_pool and cg_kmeans_step against fp64 numpy restatements of their
contracts (include/codonlm_hip.h).

Bounds (u = 2^-24, the fp32 unit roundoff):
  window_pool   a window's sum is `window` fp32 additions and one division: (window + 2) u sum|h| / window.
  labels        the kernel ranks centres by |c|^2 - 2 x.c in fp32; each score is off by at most
                (d + 2) u (|x|^2 + max|c|^2), so a label may differ from the fp64 argmin only where the
                fp64 gap of the two smallest squared distances is at most 4 (d + 2) u (|x|^2 + max|c|^2).
  dist2         d fp32 products and additions of non-negative terms: 2 (d + 2) u relative.
  sums          at most CG_KMEANS_CHUNK fp32 additions per partial, then fp64: (n 2^-53 + CHUNK u) sum|x|
                over the cluster's members, per column; the same form for the inertia over dist2.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nwin(T, window, stride):
    return (T - window) // stride + 1 if T >= window else 0


# ------------------------------------------------------------------ window_keep
@pytest.mark.parametrize("T", [5, 40])
def test_window_keep_is_exact(T):
    from codonlm_amd import ops
    rng = np.random.default_rng(T)
    idx = rng.integers(4, 68, size=(7, T)).astype(np.int64)
    special = [0, 3, 255, 256, 10 ** 12]
    for b in range(7):  # every row gets one or two of the special values
        for v in rng.choice(special, size=1 + b % 2, replace=False):
            idx[b, rng.integers(0, T)] = v
    idx[6, :] = rng.integers(4, 68, size=T)
    idx[6, T - 1] = 256  # 256 and 10^12 alias ids 0 and 0x...00 modulo 256: they must not be excluded
    idx[5, 0] = 10 ** 12
    exclude = (0, 3, 255)
    for window in (1, 9, T, T + 1):
        for stride in (1, 3, 50):
            nwin = _nwin(T, window, stride)
            want = np.zeros((7, nwin), np.int32)
            for b in range(7):
                for j in range(nwin):
                    want[b, j] = not any(int(t) in exclude for t in idx[b, j * stride:j * stride + window])
            got = ops.window_keep(_dev(idx), window, stride, exclude)
            assert got.dtype == torch.int32 and tuple(got.shape) == (7, nwin)
            assert np.array_equal(got.cpu().numpy(), want), (window, stride)
            if nwin:
                none = ops.window_keep(_dev(idx), window, stride, ())
                assert bool((none == 1).all())
    with pytest.raises(ValueError):
        ops.window_keep(_dev(idx), 9, 3, (256,))


# ------------------------------------------------------------------ window_pool
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [6, 64, 200])
def test_window_pool_matches_fp64(dtype, d):
    from codonlm_amd import ops
    B, T = 3, 40
    rng = np.random.default_rng(d)
    for window, stride in ((9, 3), (1, 1), (40, 5), (7, 50)):
        nwin = _nwin(T, window, stride)
        ldh, ldo = d + 5, d + 3
        hbuf = torch.full((B, T, ldh), float("nan"), dtype=dtype, device=DEV)
        hbuf[:, :, :d] = _dev(rng.standard_normal((B, T, d)).astype(np.float32) * 3).to(dtype)
        h64 = hbuf[:, :, :d].to(torch.float64).cpu().numpy()  # the bf16 input widened exactly
        nw = B * nwin
        rows = nw + 4
        perm = rng.permutation(nw).astype(np.int32)
        dst = perm.copy()
        dst[rng.choice(nw, size=max(1, nw // 5), replace=False)] = -1
        if nw > 2:
            dst[1], dst[2] = rows, 2 ** 31 - 1  # past the output: skipped
        obuf = torch.full((rows, ldo), float("nan"), device=DEV)
        obuf[:, :d] = -77.0  # the sentinel of rows no window selects
        out = ops.window_pool(hbuf[:, :, :d], window, stride, _dev(dst.reshape(B, nwin)), obuf[:, :d])
        got = obuf.cpu().numpy()
        assert out.data_ptr() == obuf.data_ptr()
        assert np.isnan(got[:, d:]).all()  # the pad columns of out are untouched (and h's NaN pads never read)
        written = np.zeros(rows, bool)
        worst = 0.0
        for b in range(B):
            for j in range(nwin):
                r = int(dst[b * nwin + j])
                if r < 0 or r >= rows:
                    continue
                seg = h64[b, j * stride:j * stride + window]
                bound = (window + 2) * U * np.abs(seg).sum(0) / window
                err = np.abs(got[r, :d].astype(np.float64) - seg.sum(0) / window)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all(), (window, stride, b, j)
                written[r] = True
        assert (got[~written, :d] == -77.0).all()
        print(f"[window_pool {dtype} d={d} w={window} s={stride}] max err/bound {worst:.3f}")


# ------------------------------------------------------------------ kmeans_step
def _chunk():
    from codonlm_amd import _lib as L
    return L.KMEANS_CHUNK


def _case(n, d, k, dup, seed=7):
    """x = 1.5 N(0,1) + one N(0,1) row offset; the centres are k distinct points + 0.05 N(0,1), centre 0
    exactly a point; dup: centres 3 and 7 identical."""
    rng = np.random.default_rng(seed)
    x = (1.5 * rng.standard_normal((n, d)) + rng.standard_normal((1, d))).astype(np.float32)
    pick = rng.choice(n, size=k, replace=False)
    c = (x[pick] + 0.05 * rng.standard_normal((k, d))).astype(np.float32)
    c[0] = x[pick[0]]
    if dup:
        c[7] = c[3]
    return x, c


def _padded(a, pad):
    """a view of the matrix inside a wider buffer whose pad columns hold NaN"""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device=DEV)
    buf[:, :a.shape[1]] = _dev(a)
    return buf[:, :a.shape[1]] if pad else buf


def _reference(x, c):
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    d2 = np.empty((len(x), len(c)))
    for j in range(len(c)):
        d2[:, j] = ((x64 - c64[j]) ** 2).sum(1)
    return d2


KM_CASES = [
    # n, d, k, duplicate centres, pad columns of x / centres.  The kernel stages 16-byte pieces when
    # d and the row strides are multiples of 4 and single elements otherwise, and keeps 1, 2, 4 or 8
    # accumulator tiles for k <= 32, 64, 128, 256: both staging paths meet every tile count.
    (1, 6, 1, False, 3),
    (63, 8, 1, False, 0),
    (63, 50, 33, False, 0),
    (63, 512, 2, False, 3),
    (1031, 200, 100, False, 4),
    (1031, 50, 100, False, 1),
    (1031, 6, 256, False, 1),
    (1031, 64, 256, False, 0),
    (1031, 512, 33, True, 0),
    ("2chunk+37", 50, 256, False, 3),
    ("2chunk+37", 200, 33, True, 5),
]


@pytest.mark.parametrize("n,d,k,dup,pad", KM_CASES)
def test_kmeans_step_matches_fp64(n, d, k, dup, pad):
    from codonlm_amd import ops
    CH = _chunk()
    if isinstance(n, str):
        n = 2 * CH + 37
    x, c = _case(n, d, k, dup)
    d2 = _reference(x, c)
    ref_lab = d2.argmin(1)
    xt, ct = _padded(x, pad), _padded(c, pad)
    r = ops.kmeans_step(xt, ct)
    lab = r.labels.cpu().numpy().astype(np.int64)
    rows = np.arange(n)
    assert lab.min() >= 0 and lab.max() < k
    # labels: differences only inside the near-tie allowance, and the inputs keep the allowance rare
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    allow = 4 * (d + 2) * U * ((x64 ** 2).sum(1) + (c64 ** 2).sum(1).max())
    if k > 1:
        two = np.partition(d2, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
        if dup:  # the twin of centre 3 is a tie by construction, not a near-tie of the data
            d2x = np.delete(d2, 7, axis=1)
            two = np.partition(d2x, 1, axis=1)[:, :2]
            gap = two[:, 1] - two[:, 0]
    else:
        gap = np.full(n, np.inf)
    near = gap <= allow
    print(f"[kmeans n={n} d={d} k={k}] near-tie share {near.mean():.4f}, labels differing {int((lab != ref_lab).sum())}")
    assert near.mean() <= 0.02
    diff = lab != ref_lab
    assert (d2[rows, lab][diff] - d2[rows, ref_lab][diff] <= allow[diff]).all()
    assert not (diff & ~near).any()
    if dup:
        assert not (lab == 7).any() and (ref_lab == 3).any()  # an exact tie goes to the lowest index
    assert lab[np.nonzero((x == c[0]).all(1))[0][0]] == 0
    # dist2 of the returned label
    dist = r.dist2.cpu().numpy().astype(np.float64)
    want = d2[rows, lab]
    assert (np.abs(dist - want) <= 2 * (d + 2) * U * want).all()
    assert (dist[(x == c[0]).all(1)] == 0).all()  # centre 0 is exactly a point
    # counts exact, sums and inertia to the bound, from the returned labels
    counts = r.counts.cpu().numpy()
    assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(lab, minlength=k))
    sums64, absum = np.zeros((k, d)), np.zeros((k, d))
    np.add.at(sums64, lab, x64)
    np.add.at(absum, lab, np.abs(x64))
    rel = n * 2.0 ** -53 + CH * U
    sums = r.sums.cpu().numpy()
    assert sums.dtype == np.float64 and (np.abs(sums - sums64) <= rel * absum).all()
    assert (sums[counts == 0] == 0).all()
    tot = float(dist.sum())
    assert abs(float(r.inertia) - tot) <= rel * tot
    # bitwise reproducible, with and without the optional outputs
    r2 = ops.kmeans_step(xt, ct)
    for f in ("labels", "dist2", "sums", "counts", "inertia"):
        assert torch.equal(getattr(r, f), getattr(r2, f)), f
    r3 = ops.kmeans_step(xt, ct, want_dist2=False, want_stats=False, want_inertia=False)
    assert torch.equal(r3.labels, r.labels) and r3.dist2 is None and r3.sums is None and r3.inertia is None
    r4 = ops.kmeans_step(xt, ct, want_dist2=False, want_inertia=False)
    assert torch.equal(r4.sums, r.sums) and torch.equal(r4.counts, r.counts)
    r5 = ops.kmeans_step(xt, ct, want_stats=False)
    assert torch.equal(r5.dist2, r.dist2) and torch.equal(r5.inertia, r.inertia)
    assert not torch.isnan(r.sums).any() and not torch.isnan(r.dist2).any()  # the NaN pads poisoned nothing


def test_kmeans_step_limits_and_empty_input():
    from codonlm_amd import ops
    x = torch.zeros(4, 1025, device=DEV)
    with pytest.raises(ValueError, match="unsupported"):
        ops.kmeans_step(x, x[:2])
    with pytest.raises(ValueError, match="unsupported"):
        ops.kmeans_step(torch.zeros(300, 4, device=DEV), torch.zeros(257, 4, device=DEV))
    r = ops.kmeans_step(torch.zeros(0, 4, device=DEV), torch.zeros(2, 4, device=DEV))
    assert r.labels.numel() == 0 and float(r.inertia) == 0 and int(r.counts.sum()) == 0
