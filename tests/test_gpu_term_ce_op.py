"""cg_term_ce_fwd / cg_term_ce_bwd (the fused termination-head loss) against an fp64 numpy restatement
of their contract (include/codonlm_hip.h).  A bf16 input is widened exactly, so the reference reads
the same numbers.

Bounds (u = 2^-24, the fp32 unit roundoff; S_r = max_c (sum_j |x_rj W_cj| + |b_c|), Z_r = max_c |z_rc|):
  logit   d fma per class spread over 64 lanes, a 6-level butterfly and the bias: e_z = (d + 8) u S_r.
  nll     lse = max + log(sum exp(z - max)), nll = lse - z_y: the logit errors enter three times (the
          max, the sum, z_y), exp / log / the C-term sum and the subtractions each add a few u of a
          value bounded by 1 + 2 Z_r (|lse| <= Z_r + log 16): e_nll = 3 e_z + (C + 16) u (1 + 2 Z_r).
  loss    a ratio of two fp64 sums of fp32 terms w nll (one rounding each) and w (exact), rounded
          once: sum_r w_r (e_nll + u nll_r) / sum_r w_r + 2 u |loss|.
  p       exp(z - lse) <= 1: e_p = 2 e_nll.
  g       coef_r = scale w_y / sum w costs five roundings, the product one: |coef_r| (e_p + 6 u).
  dW, db  at most 64 fp32 fma per chunk partial, the partials added in fp64, one rounding:
          sum_r |x_rj| |coef_r| (e_p + 80 u) (x = 1 for db), plus u |result| when accumulating.
  dx      C fma: |coef_r| sum_c |W_cj| (e_p + (C + 8) u), plus u |result| when accumulating.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
IGN = -100


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(a, ld, dtype=torch.float32):
    """a (rows, d) inside a NaN-poisoned (rows, ld) buffer: the view and its fp64 value"""
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=dtype, device=DEV)
    buf[:, :a.shape[1]] = _dev(a).to(dtype)
    v = buf[:, :a.shape[1]]
    return v, v.to(torch.float64).cpu().numpy()


def _reference(x, W, b, labels, cw, scale):
    """fp64 loss, sums, dW, db, dx and their bounds (module docstring)"""
    rows, d = x.shape
    C = W.shape[0]
    valid = (labels != IGN) & (labels >= 0) & (labels < C)
    y = labels[valid].astype(np.int64)
    xv = x[valid]
    z = xv @ W.T + b
    S = (np.abs(xv) @ np.abs(W).T + np.abs(b)).max(axis=1) if len(y) else np.zeros(0)
    Z = np.abs(z).max(axis=1) if len(y) else np.zeros(0)
    mx = z.max(axis=1, keepdims=True) if len(y) else np.zeros((0, 1))
    lse = (mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True)))[:, 0]
    nll = lse - z[np.arange(len(y)), y]
    w = cw[y] if cw is not None else np.ones(len(y))
    num, den = float((w * nll).sum()), float(w.sum())
    r = {"n": int(len(y)), "num": num, "den": den}
    e_z = (d + 8) * U * S
    e_nll = 3 * e_z + (C + 16) * U * (1 + 2 * Z)
    e_p = 2 * e_nll
    if len(y) == 0:
        r["loss"] = float("nan")
        r["dW"], r["db"], r["dx"] = np.zeros((C, d)), np.zeros(C), np.zeros((rows, d))
        r["b_dW"], r["b_db"], r["b_dx"] = np.zeros((C, d)), np.zeros(C), np.zeros((rows, d))
        return r
    r["loss"] = num / den
    r["b_loss"] = float((w * (e_nll + U * np.abs(nll))).sum()) / den + 2 * U * abs(r["loss"])
    p = np.exp(z - lse[:, None])
    onehot = np.zeros_like(p)
    onehot[np.arange(len(y)), y] = 1.0
    coef = scale * w / den
    g = coef[:, None] * (p - onehot)
    r["dW"], r["db"] = g.T @ xv, g.sum(axis=0)
    r["dx"] = np.zeros((rows, d))
    r["dx"][valid] = g @ W
    eg = np.abs(coef) * (e_p + 80 * U)
    r["b_dW"] = np.broadcast_to((eg[:, None] * np.abs(xv)).sum(axis=0), (C, d)).copy()
    r["b_db"] = np.full(C, eg.sum())
    r["b_dx"] = np.zeros((rows, d))
    r["b_dx"][valid] = (np.abs(coef) * (e_p + (C + 8) * U))[:, None] * np.abs(W).sum(axis=0)[None, :]
    return r


def _labels(rng, rows, C, how):
    lab = np.full(rows, IGN, np.int64)
    if how == "all":
        lab[:] = rng.integers(0, C, size=rows)
    elif how == "sparse":  # ~6 %
        pick = rng.random(rows) < 0.06
        lab[pick] = rng.integers(0, C, size=int(pick.sum()))
    elif how == "one":
        lab[rng.integers(0, rows)] = rng.integers(0, C)
    return lab


def _check(got, want, bound, what):
    got = got.to(torch.float64).cpu().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    assert (err <= bound + 1e-300).all(), (what, float(err.max()), float(bound.max()))


def _problem(rng, rows, d, C, ld, dtype):
    x, x64 = _padded(rng.standard_normal((rows, d)).astype(np.float32) * 1.5, ld, dtype)
    W, W64 = _padded((rng.standard_normal((C, d)) / np.sqrt(d)).astype(np.float32) * 2, ld)
    b = rng.standard_normal(C).astype(np.float32)
    return x, x64, W, W64, b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("aligned", [False, True], ids=["ld_odd", "ld_vec"])
@pytest.mark.parametrize("C", [1, 5, 16])
@pytest.mark.parametrize("d", [6, 64, 200])
@pytest.mark.parametrize("rows", [1, 67, 300])
def test_loss_and_gradients_match_fp64(rows, d, C, aligned, dtype):
    """ld = d + 5 (element loads only) and a 16-byte aligned ld (16-byte loads with an element tail at
    d = 6); pad columns are NaN; every labelling, with and without class weights."""
    from codonlm_amd import ops
    rng = np.random.default_rng(1000 * rows + 10 * d + C)
    ld = (d + 7) // 4 * 4 if aligned else d + 5
    x, x64, W, W64, b = _problem(rng, rows, d, C, ld, dtype)
    cw = (0.25 + 2 * rng.random(C)).astype(np.float32)
    for how in ("all", "sparse", "one", "none"):
        lab = _labels(rng, rows, C, how)
        for cwi in (None, cw):
            ref = _reference(x64, W64, b.astype(np.float64), lab, None if cwi is None else cwi.astype(np.float64), 1.0)
            st = ops.term_ce_fwd(x, W, _dev(b), _dev(lab), class_w=None if cwi is None else _dev(cwi), ignore_index=IGN)
            dxbuf = torch.full((rows, ld), float("nan"), dtype=torch.float32, device=DEV)
            dWbuf = torch.full((C, ld), float("nan"), dtype=torch.float32, device=DEV)
            sentinel_dx, sentinel_dW = dxbuf[:, :d], dWbuf[:, :d]
            sentinel_dx.zero_()
            sentinel_dW.zero_()
            dW, db, dx = ops.term_ce_bwd(st)
            # the same into padded outputs (accumulating into zeros): pad columns stay NaN
            ops.term_ce_bwd(st, dW=sentinel_dW, dx=sentinel_dx, want=())
            loss = float(st.loss.item())
            sums = st.sums.to(torch.float64).cpu().numpy()
            print(rows, d, C, how, cwi is not None, "loss", loss, ref["loss"], "n", ref["n"])
            if ref["n"] == 0:
                assert np.isnan(loss)
                assert sums[0] == 0.0 and sums[1] == 0.0
                for t in (dW, db, dx, sentinel_dW, sentinel_dx):
                    assert bool((t == 0).all())
                continue
            assert abs(loss - ref["loss"]) <= ref["b_loss"], (how, loss, ref["loss"], ref["b_loss"])
            assert abs(sums[1] - ref["den"]) <= 2 * U * ref["den"]
            assert abs(sums[0] - ref["num"]) <= ref["b_loss"] * ref["den"] + 2 * U * abs(ref["num"])
            _check(dW, ref["dW"], ref["b_dW"], ("dW", how))
            _check(db, ref["db"], ref["b_db"], ("db", how))
            _check(dx, ref["dx"], ref["b_dx"], ("dx", how))
            unl = torch.from_numpy(~((lab != IGN) & (lab >= 0) & (lab < C))).to(DEV)
            assert bool((dx[unl] == 0).all())  # unlabelled rows written as exact zeros
            _check(sentinel_dW, ref["dW"], ref["b_dW"], ("dW padded", how))
            _check(sentinel_dx, ref["dx"], ref["b_dx"], ("dx padded", how))
            assert bool(torch.isnan(dxbuf[:, d:]).all()) and bool(torch.isnan(dWbuf[:, d:]).all())


def test_none_labelled_leaves_accumulated_outputs_unchanged():
    from codonlm_amd import ops
    rng = np.random.default_rng(5)
    rows, d, C = 67, 64, 5
    x, _, W, _, b = _problem(rng, rows, d, C, d + 5, torch.float32)
    st = ops.term_ce_fwd(x, W, _dev(b), _dev(np.full(rows, IGN, np.int64)))
    assert bool(torch.isnan(st.loss))
    pre = [torch.randn(C, d, device=DEV), torch.randn(C, device=DEV), torch.randn(rows, d, device=DEV)]
    out = [t.clone() for t in pre]
    ops.term_ce_bwd(st, dW=out[0], db=out[1], dx=out[2], want=())
    for a, p in zip(out, pre):
        assert torch.equal(a, p)
    for t in ops.term_ce_bwd(st):
        assert bool((t == 0).all())


@pytest.mark.parametrize("C", [5, 16])
def test_out_of_range_labels_are_ignored(C):
    """C, -1 and 10**12 behave as ignore_index does: bit-identical results."""
    from codonlm_amd import ops
    rng = np.random.default_rng(C)
    rows, d = 67, 64
    x, _, W, _, b = _problem(rng, rows, d, C, d + 5, torch.float32)
    lab = _labels(rng, rows, C, "all")
    bad = rng.choice(rows, size=9, replace=False)
    clean = lab.copy()
    clean[bad] = IGN
    dirty = lab.copy()
    dirty[bad] = np.array([C, -1, 10 ** 12] * 3, np.int64)
    res = []
    for l in (clean, dirty):
        st = ops.term_ce_fwd(x, W, _dev(b), _dev(l))
        res.append((st.loss, st.sums) + ops.term_ce_bwd(st))
    assert bool(torch.isfinite(res[0][0]))
    for a, b_ in zip(*res):
        assert torch.equal(a, b_)
    assert bool((res[1][4][torch.from_numpy(bad).to(DEV)] == 0).all())


def test_scale_host_device_and_both():
    from codonlm_amd import ops
    rng = np.random.default_rng(11)
    rows, d, C = 300, 64, 5
    x, x64, W, W64, b = _problem(rng, rows, d, C, d + 5, torch.float32)
    lab = _labels(rng, rows, C, "sparse")
    cw = (0.25 + 2 * rng.random(C)).astype(np.float32)
    st = ops.term_ce_fwd(x, W, _dev(b), _dev(lab), class_w=_dev(cw))
    sd = torch.tensor([-1.75], dtype=torch.float32, device=DEV)
    for kw, s in ((dict(scale=0.375), 0.375), (dict(scale_dev=sd), -1.75), (dict(scale=0.375, scale_dev=sd), -0.65625)):
        ref = _reference(x64, W64, b.astype(np.float64), lab, cw.astype(np.float64), s)
        dW, db, dx = ops.term_ce_bwd(st, **kw)
        _check(dW, ref["dW"], ref["b_dW"], ("dW", s))
        _check(db, ref["db"], ref["b_db"], ("db", s))
        _check(dx, ref["dx"], ref["b_dx"], ("dx", s))
        assert float(db.abs().max()) > 0


@pytest.mark.parametrize("which", ["dW", "db", "dx"])
def test_each_accumulate_flag(which):
    """One output accumulates into a prefilled tensor, the other two are overwritten."""
    from codonlm_amd import ops
    rng = np.random.default_rng(17)
    rows, d, C = 67, 200, 5
    x, x64, W, W64, b = _problem(rng, rows, d, C, d + 5, torch.bfloat16)
    lab = _labels(rng, rows, C, "sparse")
    lab[3] = 2
    st = ops.term_ce_fwd(x, W, _dev(b), _dev(lab))
    ref = _reference(x64, W64, b.astype(np.float64), lab, None, 1.0)
    shapes = {"dW": (C, d), "db": (C,), "dx": (rows, d)}
    pre = torch.randn(shapes[which], device=DEV)
    out = dict(zip(("dW", "db", "dx"), ops.term_ce_bwd(st, **{which: pre.clone()})))
    for name in shapes:
        want = ref[name] + (pre.to(torch.float64).cpu().numpy() if name == which else 0.0)
        bound = ref["b_" + name] + (U * np.abs(want) if name == which else 0.0)
        _check(out[name], want, bound, (which, name))
    if which == "dx":  # unlabelled rows of an accumulating dx are not touched
        unl = torch.from_numpy(lab == IGN).to(DEV)
        assert torch.equal(out["dx"][unl], pre[unl])


def test_more_than_16_classes_is_unsupported():
    from codonlm_amd import ops
    x = torch.randn(8, 32, device=DEV)
    W = torch.randn(17, 32, device=DEV)
    with pytest.raises(ValueError, match="CG_EUNSUPPORTED"):
        ops.term_ce_fwd(x, W, torch.zeros(17, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bitwise_reproducible(dtype):
    from codonlm_amd import ops
    rng = np.random.default_rng(23)
    rows, d, C = 300, 200, 5
    x, _, W, _, b = _problem(rng, rows, d, C, d + 4, dtype)
    lab = _labels(rng, rows, C, "all")
    runs = []
    for _ in range(2):
        st = ops.term_ce_fwd(x, W, _dev(b), _dev(lab))
        runs.append((st.loss, st.sums) + ops.term_ce_bwd(st, scale=0.5))
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)
