"""cg_attr_reduce and cg_attr_seed against fp64 numpy restatements of their contracts
(include/codonlm_hip.h).

Bounds.  cg_attr_reduce forms fp32 dot products of length d as FMA chains plus a 6-step butterfly:
each value is held to the forward bound of an fp32 dot product, (d + 2) 2^-24 sum_k |a_k b_k| (d
for the sum in any order, 2 for the roundings around it); gnorm is compared as its square, the sum
before the root, the root's own rounding being one of those 2.  cg_attr_seed rounds an fp64 value
once: the fp32 layout is held to 4 ulp, the split bf16 layout (hi + lo) to 2^-16 of the row's
largest |d| (bf16 keeps 8 bits, hi + lo 16).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(a, pad):
    """A device copy of the 2-D fp32 array whose row stride is a.shape[1] + pad; the pad columns hold
    NaN, which no result may pick up."""
    rows, d = a.shape
    buf = torch.full((rows, d + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :d] = _dev(a)
    return buf[:, :d]


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ cg_attr_reduce
REDUCE_V = 37


@pytest.fixture(scope="module")
def reduce_case():
    """Operands shared by every attr_reduce test, sliced per (rows, d): g, x0 [300][512], a table
    [37][512] and token ids of which about one in six lies outside the table."""
    rng = np.random.default_rng(101)
    g = (rng.standard_normal((300, 512)) * np.exp(rng.standard_normal((300, 1)))).astype(np.float32)
    x0 = rng.standard_normal((300, 512)).astype(np.float32)
    tok = rng.standard_normal((REDUCE_V, 512)).astype(np.float32)
    idx = rng.integers(0, REDUCE_V, size=300)
    idx[rng.random(300) < 1 / 6] = -1
    idx[7], idx[64], idx[299] = REDUCE_V, 10 ** 12, -5
    idx[0] = 3  # the single-row case reads the table
    return g, x0, tok, idx.astype(np.int64)


def _reduce_ref(g, x0, tok, idx):
    g64, x64, t64 = g.astype(np.float64), x0.astype(np.float64), tok.astype(np.float64)
    ok = (idx >= 0) & (idx < tok.shape[0])
    e = np.where(ok[:, None], t64[np.where(ok, idx, 0)], 0.0)
    return {"gxt": ((g64 * e).sum(1), np.abs(g64 * e).sum(1)), "gxi": ((g64 * x64).sum(1), np.abs(g64 * x64).sum(1)),
            "gnorm2": ((g64 * g64).sum(1), (g64 * g64).sum(1)), "ok": ok}


@pytest.mark.parametrize("rows", [1, 65, 300])
@pytest.mark.parametrize("d", [6, 64, 100, 512])
def test_attr_reduce_matches_fp64(reduce_case, rows, d):
    from codonlm_amd import ops
    g, x0, tok, idx = reduce_case
    g, x0, tok, idx = g[:rows, :d], x0[:rows, :d], tok[:, :d], idx[:rows]
    ref = _reduce_ref(g, x0, tok, idx)
    got = {}
    # strides d + 4 (16-byte rows where d % 4 == 0: the vector loads) and d + 3 (element loads)
    for pad in (4, 3):
        r = ops.attr_reduce(_strided(g, pad), _dev(idx), _strided(tok, pad), _strided(x0, pad))
        got[pad] = r
        vals = {"gxt": r.gxt.cpu().numpy().astype(np.float64), "gxi": r.gxi.cpu().numpy().astype(np.float64),
                "gnorm2": r.gnorm.cpu().numpy().astype(np.float64) ** 2}
        for k, v in vals.items():
            want, mag = ref[k]
            err = np.abs(v - want)
            bound = (d + 2) * U * mag
            print(f"[attr_reduce rows={rows} d={d} pad={pad}] {k}: max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert np.isfinite(v).all() and (err <= bound).all(), (k, pad)
        assert (vals["gxt"][~ref["ok"]] == 0).all()  # ids outside the table
    # the two load paths add in the same order
    for k in ("gxt", "gxi", "gnorm"):
        assert np.array_equal(_bits(getattr(got[4], k)), _bits(getattr(got[3], k))), k
    # the same launch again gives the same bits
    again = ops.attr_reduce(_strided(g, 4), _dev(idx), _strided(tok, 4), _strided(x0, 4))
    for k in ("gxt", "gxi", "gnorm"):
        assert np.array_equal(_bits(getattr(got[4], k)), _bits(getattr(again, k))), k


@pytest.mark.parametrize("d", [6, 64, 100, 512])
def test_attr_reduce_rows_are_independent_of_the_batch(reduce_case, d):
    from codonlm_amd import ops
    g, x0, tok, idx = reduce_case
    gd, xd, td, idd = _strided(g[:, :d], 4), _strided(x0[:, :d], 4), _strided(tok[:, :d], 4), _dev(idx)
    full = ops.attr_reduce(gd, idd, td, xd)
    for r in (0, 3, 64, 65, 255, 299):
        one = ops.attr_reduce(gd[r:r + 1], idd[r:r + 1], td, xd[r:r + 1])
        for k in ("gxt", "gxi", "gnorm"):
            assert _bits(getattr(one, k))[0] == _bits(getattr(full, k))[r], (k, r)
    part = ops.attr_reduce(gd[:65], idd[:65], td, xd[:65])
    for k in ("gxt", "gxi", "gnorm"):
        assert np.array_equal(_bits(getattr(part, k)), _bits(getattr(full, k))[:65]), k


def test_attr_reduce_optional_outputs_and_empty_input(reduce_case):
    from codonlm_amd import ops
    g, x0, tok, idx = reduce_case
    gd, idd = _dev(g[:9, :64]), _dev(idx[:9])
    full = ops.attr_reduce(gd, idd, _dev(tok[:, :64]), _dev(x0[:9, :64]))
    only = ops.attr_reduce(gd, idd, want=("gnorm",))  # neither table nor x0 needed
    assert only.gxt is None and only.gxi is None and np.array_equal(_bits(only.gnorm), _bits(full.gnorm))
    only = ops.attr_reduce(gd, idd, _dev(tok[:, :64]), want=("gxt",))
    assert only.gnorm is None and np.array_equal(_bits(only.gxt), _bits(full.gxt))
    with pytest.raises(ValueError, match="tok_emb"):
        ops.attr_reduce(gd, idd, want=("gxt",))
    with pytest.raises(ValueError, match="x0"):
        ops.attr_reduce(gd, idd, _dev(tok[:, :64]), want=("gxi",))
    empty = ops.attr_reduce(gd[:0], idd[:0], _dev(tok[:, :64]), _dev(x0[:0, :64]))
    assert empty.gxt.shape == (0,) and empty.gnorm.shape == (0,)


# ------------------------------------------------------------------ cg_attr_seed
def _seed_case(V, rows=37):
    rng = np.random.default_rng(1000 + V)
    ld = V + 5
    z = np.full((rows, ld), 1e30, np.float32)  # columns past V are not logits: never read
    z[:, :V] = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    y = rng.integers(0, V, size=rows).astype(np.int64)
    w = rng.standard_normal(rows).astype(np.float32)
    y[2], y[9], y[20] = -1, V, V + 5
    w[4], w[9] = 0.0, 0.0
    z[6, y[6]] = 40.0    # a peaked row: 1 - p_y is about e^-37, far below an ulp of p_y
    z[11, :V] = -50.0    # a row of equal logits
    z[12, (y[12] + 1) % V] = 60.0  # a row whose class has a vanishing probability
    return z, y, w


def _seed_ref(z, y, w, V, mode):
    rows = z.shape[0]
    z64 = z[:, :V].astype(np.float64)
    live = (y >= 0) & (y < V) & (w != 0)
    yy = np.where(live, y, 0)
    onehot = np.zeros((rows, V))
    onehot[np.arange(rows), yy] = 1.0
    w64 = w.astype(np.float64)[:, None]
    if mode == "logit":
        d = w64 * onehot
    else:
        e = np.exp(z64 - z64.max(1, keepdims=True))
        rest = (e * (1.0 - onehot)).sum(1, keepdims=True)  # 1 - p_y without cancellation
        ey = (e * onehot).sum(1, keepdims=True)
        d = w64 * np.where(onehot > 0, rest, -e) / (rest + ey)
    return np.where(live[:, None], d, 0.0), live


@pytest.mark.parametrize("mode", ["logprob", "logit"])
@pytest.mark.parametrize("V", [68, 16, 128])
def test_attr_seed_fp32_layout(V, mode):
    from codonlm_amd import ops
    z, y, w = _seed_case(V)
    ref, live = _seed_ref(z, y, w, V, mode)
    ldd = (V + 15) // 16 * 16 + 16
    got = ops.attr_seed(_dev(z), _dev(y), _dev(w), V=V, mode=mode, pad_to=ldd).cpu().numpy()
    assert got.shape == (z.shape[0], ldd) and (got[:, V:] == 0).all()  # the pad columns
    assert (got[~live] == 0).all()  # y = -1, y >= V, w = 0: the whole row
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got[:, :V].astype(np.float64) - ref)
    print(f"[attr_seed fp32 V={V} {mode}] max err {float((err / ulp).max()):.2f} ulp")
    assert (err <= 4 * ulp).all()
    if mode == "logprob":
        s = np.abs(got[:, :V].astype(np.float64).sum(1))
        print(f"[attr_seed fp32 V={V}] max |row sum| / |w| {float((s[live] / np.abs(w[live])).max()):.2e}")
        assert (s <= 1e-6 * np.abs(w)).all()
    # no weights = weight 1
    one, _ = _seed_ref(z, y, np.ones_like(w), V, mode)
    got1 = ops.attr_seed(_dev(z), _dev(y), None, V=V, mode=mode, pad_to=ldd).cpu().numpy()
    assert (np.abs(got1[:, :V] - one) <= 4 * np.spacing(np.abs(one).astype(np.float32))).all()


@pytest.mark.parametrize("mode", ["logprob", "logit"])
@pytest.mark.parametrize("V", [68, 16, 128])
def test_attr_seed_split_bf16_layout(V, mode):
    """hi + lo against fp64 at 2^-16 of the row's largest |d|.  The row sums: hi + lo carries a
    relative error of up to 2^-18 + 2^-24 per element (lo = bf16 of a residual below 2^-9 |d|), and
    sum_c |d_c| <= 2 |w|, so the split rows can only be held to 2^-16 |w|; the 1e-6 |w| of the fp32
    layout is below what 16 bits can represent."""
    from codonlm_amd import ops
    z, y, w = _seed_case(V)
    ref, live = _seed_ref(z, y, w, V, mode)
    half = ((V + 15) // 16 * 16 + 31) // 32 * 32  # the engine's Vh
    got = ops.attr_seed(_dev(z), _dev(y), _dev(w), V=V, mode=mode, pad_to=2 * half, split=True)
    assert got.dtype == torch.bfloat16 and got.shape == (z.shape[0], 2 * half)
    g = got.float().cpu().numpy().astype(np.float64)
    hi, lo = g[:, :half], g[:, half:]
    assert (hi[:, V:] == 0).all() and (lo[:, V:] == 0).all()
    assert (hi[~live] == 0).all() and (lo[~live] == 0).all()
    val = hi[:, :V] + lo[:, :V]
    err = np.abs(val - ref)
    scale = np.abs(ref).max(1, keepdims=True)
    print(f"[attr_seed split V={V} {mode}] max err / row max {float((err[live] / scale[live]).max()):.2e} (2^-16 = {2.0 ** -16:.2e})")
    assert (err <= 2.0 ** -16 * scale).all()
    if mode == "logprob":
        s = np.abs(val.sum(1))
        print(f"[attr_seed split V={V}] max |row sum| / |w| {float((s[live] / np.abs(w[live])).max()):.2e}")
        assert (s <= 2.0 ** -16 * np.abs(w)).all()


def test_attr_seed_many_rows_and_empty():
    """More rows than one grid pass of 4 waves x 4096 workgroups covers: the grid-stride loop."""
    from codonlm_amd import ops
    V, rows = 16, 4 * 4096 + 37
    rng = np.random.default_rng(8)
    z = rng.standard_normal((rows, V)).astype(np.float32)
    y = rng.integers(-1, V + 1, size=rows).astype(np.int64)
    ref, live = _seed_ref(z, y, np.ones(rows, np.float32), V, "logprob")
    got = ops.attr_seed(_dev(z), _dev(y), None, mode="logprob").cpu().numpy()
    assert got.shape == (rows, V)
    assert (np.abs(got - ref) <= 4 * np.spacing(np.abs(ref).astype(np.float32))).all() and (got[~live] == 0).all()
    assert ops.attr_seed(_dev(z[:0]), _dev(y[:0]), None).shape == (0, V)
    with pytest.raises(ValueError, match="mode"):
        ops.attr_seed(_dev(z[:4]), _dev(y[:4]), None, mode="prob")
