"""cg_score_rows against an fp64 numpy restatement of its contract (include/codonlm_hip.h).

The kernel evaluates every row quantity in fp64 from the fp32 logits and rounds once, so each
fp32 output must lie within 1 fp32 ulp of the restatement (whose own error is orders below an
fp32 ulp); the integer outputs are exact; the fp64 sums differ from the restatement in summation
order only (relative 1e-12).  Every output buffer and the workspace are followed by sentinel
guard bytes that must come back untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
SENT = 0x7FC0DEAD  # a NaN bit pattern no kernel writes
F32_OUT = ("lse", "logp", "entropy")
I32_OUT = ("argmax", "rank")


def _L():
    from codonlm_amd import _lib as L
    return L


class Guarded:
    """`nbytes` of device memory (8-byte aligned) followed by GUARD sentinel bytes."""

    def __init__(self, nbytes, fill=None):
        self.n = int(nbytes)
        self.words = (self.n + 3) // 4
        self.buf = torch.full((self.words + GUARD // 4 + 2,), SENT, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 8 == 0
        self.ptr = self.buf.data_ptr()
        if fill is not None:
            self.buf[:self.words] = fill

    def intact(self):
        return bool((self.buf[self.words:] == SENT).all())

    def array(self, dtype, shape):
        return self.buf[:self.words].cpu().numpy().view(dtype).reshape(shape).copy()


# ------------------------------------------------------------------ the fp64 restatement
def restate(z32, targets, V, ignore=0, eps=0.0, sel=None, T=0):
    """Row outputs, class deltas, sequence sums and the four accumulator terms of rows z32[:, :V]."""
    z = z32[:, :V].astype(np.float64)
    rows = z.shape[0]
    cols = np.arange(V)
    amax = z.argmax(1)  # numpy returns the first of equal maxima
    m = z[np.arange(rows), amax]
    dz = m[:, None] - z  # >= 0; +inf where z = -inf
    e = np.exp(-dz)
    e[np.arange(rows), amax] = 0.0  # that term is exactly 1: lse - max = log1p(sum of the others)
    s1 = e.sum(1)
    lgs = np.log1p(s1)
    lse = m + lgs
    with np.errstate(invalid="ignore"):
        ent = lgs + np.where(e > 0, e * dz, 0.0).sum(1) / (1.0 + s1)
    if targets is None:
        valid = np.zeros(rows, bool)
        y = np.zeros(rows, np.int64)
    else:
        valid = (targets != ignore) & (targets >= 0) & (targets < V)
        y = np.where(valid, targets, 0)
    zy = z[np.arange(rows), y]
    logp = np.where(valid, (zy - m) - lgs, 0.0)
    rank = (z > zy[:, None]).sum(1) + ((z == zy[:, None]) & (cols[None, :] < y[:, None])).sum(1)
    rank = np.where(valid, rank, -1)
    out = {"lse": lse, "logp": logp, "entropy": ent, "argmax": amax, "rank": rank, "valid": valid}
    if sel is not None:
        ok = (sel >= 0) & (sel < V)
        zs = z[:, np.where(ok, sel, 0)]
        base = np.where(valid, zy, lse)  # (z_s - lse) - (z_y - lse) = z_s - z_y on a valid row
        out["delta"] = np.where(ok[None, :], zs - base[:, None], -np.inf)
    nll = -logp
    e64 = float(np.float32(eps))
    with np.errstate(invalid="ignore"):
        obj = (1.0 - e64) * nll + (e64 / V) * (lse[:, None] - z).sum(1) if e64 != 0.0 else nll
    out["acc"] = np.array([nll[valid].sum(), obj[valid].sum(), valid.sum(), (valid & (amax == y)).sum()], np.float64)
    if T:
        out["seq_logp"] = logp.reshape(-1, T).sum(1)
        out["seq_count"] = valid.reshape(-1, T).sum(1)
    return out


# ------------------------------------------------------------------ the launch
def launch(z32, V, targets=None, *, ignore=0, eps=0.0, sel=None, T=0, acc=None, want_acc=True, ws_short=0,
           outputs=F32_OUT + I32_OUT):
    """cg_score_rows over z32 [rows][ldl] with every buffer guarded: (status, outputs as numpy)."""
    L = _L()
    rows, ldl = z32.shape
    zd = torch.from_numpy(z32).to(DEV)
    d = L.ScoreDesc()
    d.logits, d.ldl, d.rows, d.V = zd.data_ptr(), ldl, rows, V
    keep = [zd]
    if targets is not None:
        td = torch.from_numpy(np.asarray(targets, np.int64)).to(DEV)
        keep.append(td)
        d.targets = td.data_ptr()
    d.ignore_index, d.smoothing, d.T = ignore, eps, T
    bufs = {}
    for name in outputs:
        bufs[name] = Guarded(rows * 4)
        setattr(d, name, bufs[name].ptr)
    if sel is not None:
        sd = torch.from_numpy(np.asarray(sel, np.int32)).to(DEV)
        keep.append(sd)
        bufs["delta"] = Guarded(rows * len(sel) * 4)
        d.sel, d.n_sel, d.delta, d.ld_delta = sd.data_ptr(), len(sel), bufs["delta"].ptr, len(sel)
    if T:
        bufs["seq_logp"] = Guarded(rows // T * 8)
        bufs["seq_count"] = Guarded(rows // T * 4)
        d.seq_logp, d.seq_count = bufs["seq_logp"].ptr, bufs["seq_count"].ptr
    if acc is None and want_acc:
        acc = Guarded(32, fill=0)
    if acc is not None:
        d.acc = acc.ptr
        bufs["acc"] = acc
    need = int(L.lib.cg_score_workspace(rows))
    ws = Guarded(need)
    d.workspace, d.ws_bytes = ws.ptr, need - ws_short
    status = L.lib.cg_score_rows(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ws.intact(), "workspace guard"
    out = {}
    for name, g in bufs.items():
        assert g.intact(), f"guard after {name}"
        if name in F32_OUT:
            out[name] = g.array(np.float32, (rows,))
        elif name in I32_OUT:
            out[name] = g.array(np.int32, (rows,))
        elif name == "delta":
            out[name] = g.array(np.float32, (rows, len(sel)))
        elif name == "seq_logp":
            out[name] = g.array(np.float64, (rows // T,))
        elif name == "seq_count":
            out[name] = g.array(np.int32, (rows // T,))
        else:
            out[name] = g.array(np.float64, (4,))
    return status, out


def within_ulp(got32, ref64, extra=0.0):
    """|got - ref| <= 1 fp32 ulp at ref (+ extra); infinities must match exactly."""
    got = got32.astype(np.float64)
    inf = np.isinf(ref64)
    assert np.array_equal(got[inf], ref64[inf])
    assert not np.isnan(got).any()
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(ref64[~inf]).astype(np.float32)).astype(np.float64)
    err = np.abs(got[~inf] - ref64[~inf])
    bad = err > ulp + extra
    assert not bad.any(), (float(err[bad].max()), float(ulp[bad].min()), int(bad.sum()))


def compare(out, ref, z32, V, sel=None, T=0, acc0=None):
    zmax = float(np.abs(z32[:, :V][np.isfinite(z32[:, :V])]).max())
    within_ulp(out["lse"], ref["lse"])
    within_ulp(out["logp"], ref["logp"])
    within_ulp(out["entropy"], ref["entropy"], extra=1e-12 * max(1.0, zmax))
    assert np.array_equal(out["argmax"], ref["argmax"])
    assert np.array_equal(out["rank"], ref["rank"])
    if sel is not None:
        within_ulp(out["delta"], ref["delta"])
    if T:
        assert np.array_equal(out["seq_count"], ref["seq_count"])
        np.testing.assert_allclose(out["seq_logp"], ref["seq_logp"], rtol=1e-12, atol=0)
    if "acc" in out:
        exp = ref["acc"] + (acc0 if acc0 is not None else 0.0)
        assert out["acc"][2] == exp[2] and out["acc"][3] == exp[3]
        np.testing.assert_allclose(out["acc"][:2], exp[:2], rtol=1e-12, atol=0)


def make_logits(rng, rows, V, wide, scale):
    """N(0,1) * scale logits; with `wide`, ldl = round_up(V, 16) + 16 and pad columns of NaN / +inf."""
    ldl = (V + 15) // 16 * 16 + 16 if wide else V
    z = np.empty((rows, ldl), np.float32)
    z[:, :V] = (rng.standard_normal((rows, V)) * scale).astype(np.float32)
    pad = np.where(np.arange(ldl - V) % 2 == 0, np.float32(np.nan), np.float32(np.inf))
    z[:, V:] = pad
    return z


def make_targets(rng, rows, V, ignore=0):
    """In-range targets with some ignored rows and some out-of-range ones (negative and >= V)."""
    t = rng.integers(0, V, size=rows).astype(np.int64)
    k = rng.random(rows)
    t[k < 0.15] = ignore
    t[(k >= 0.15) & (k < 0.20)] = V + rng.integers(0, 5)
    t[(k >= 0.20) & (k < 0.25)] = -3
    return t


def sel_for(V):
    # classes in and out of the vocabulary, one negative: the mutation map's 64 codon ids
    return np.array([1, 0, V - 1, V, -1, V + 7] + list(range(2, min(V, 60))), np.int32)


VS = [5, 64, 65, 68, 128, 129, 1000, 1024]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("V", VS)
def test_rows_against_fp64(V, wide):
    rng = np.random.default_rng(1000 * V + wide)
    for rows in (1, 3, 4, 5):
        for scale in (1.0, None):
            z = make_logits(rng, rows, V, wide, 1.0)
            if scale is None:  # scaled to +-400: the magnitude full-depth fp32 logits reach
                z[:, :V] *= np.float32(400.0) / np.abs(z[:, :V]).max()
            t = make_targets(rng, rows, V)
            t[0] = 1 % V if V > 1 else 0  # at least one valid row
            sel = sel_for(V)
            st, out = launch(z, V, t, eps=0.05, sel=sel, T=rows)
            assert st == 0
            compare(out, restate(z, t, V, eps=0.05, sel=sel, T=rows), z, V, sel=sel, T=rows)


@pytest.mark.parametrize("rows", [16387, 70001])
def test_many_rows_pass_the_grid_cap(rows):
    V = 68
    rng = np.random.default_rng(rows)
    z = make_logits(rng, rows, V, True, 3.0)
    t = make_targets(rng, rows, V)
    T = 7 if rows % 7 == 0 else 1  # 16387 = 7 * 2341
    st, out = launch(z, V, t, eps=0.1, sel=sel_for(V), T=T)
    assert st == 0
    compare(out, restate(z, t, V, eps=0.1, sel=sel_for(V), T=T), z, V, sel=sel_for(V), T=T)


def test_unsupported_and_short_workspace():
    L = _L()
    z = np.zeros((4, 1025), np.float32)
    st, _ = launch(z, 1025, np.ones(4, np.int64))
    assert st == L.CG_EUNSUPPORTED
    z = np.zeros((5, 68), np.float32)
    st, out = launch(z, 68, np.ones(5, np.int64), ws_short=1)
    assert st == L.CG_EINVAL
    assert np.array_equal(out["acc"], np.zeros(4))  # refused before any launch
    assert int(L.lib.cg_score_rows(C.byref(L.ScoreDesc(rows=0, V=68)), 0)) == L.CG_OK


def test_all_ignored_call_changes_nothing():
    V, rows = 68, 9
    rng = np.random.default_rng(5)
    z = make_logits(rng, rows, V, True, 1.0)
    t = np.zeros(rows, np.int64)
    acc = Guarded(32)
    start = np.array([1.5, -2.25, 7.0, 3.0])
    acc.buf[:8] = torch.from_numpy(start.view(np.int32)).to(DEV)
    st, out = launch(z, V, t, eps=0.05, sel=sel_for(V), T=3, acc=acc)
    assert st == 0
    assert np.array_equal(out["acc"].view(np.int64), start.view(np.int64))
    assert np.array_equal(out["logp"], np.zeros(rows, np.float32)) and (out["rank"] == -1).all()
    assert np.array_equal(out["seq_logp"], np.zeros(3)) and (out["seq_count"] == 0).all()
    for k in ("lse", "entropy", "delta"):
        assert not np.isnan(out[k]).any()
    compare(out, restate(z, t, V, eps=0.05, sel=sel_for(V), T=3), z, V, sel=sel_for(V), T=3, acc0=start)


@pytest.mark.parametrize("V", [5, 68, 129, 1000])
def test_ties_and_minus_infinity(V):
    rng = np.random.default_rng(V)
    rows = 8
    z = make_logits(rng, rows, V, True, 2.0)
    t = rng.integers(0, V, size=rows).astype(np.int64)
    hi = np.float32(np.abs(z[:, :V]).max() + 1)
    z[0, [V - 1, 1, V // 2]] = hi              # three maxima: argmax is the lowest index
    t[0] = V // 2                               # ... and the target ties with them
    z[1, :V] = np.float32(0.25)                 # a flat row: every class ties
    t[1] = V - 1
    z[2, [0, 3]] = z[2, t[2]]                   # ties at the target's value, on both sides of it
    z[3, :V][np.arange(V) % 3 == 0] = -np.inf   # some non-target logits are -inf
    t[3] = 1
    z[4, :V] = -np.inf                          # all but two classes are -inf
    z[4, [1, V - 2]] = [0.5, -1.0]
    t[4] = V - 2
    z[5, 1:V] = -np.inf                         # a single finite class: entropy 0, logp 0
    t[5] = 0
    st, out = launch(z, V, t, sel=sel_for(V), T=4)
    assert st == 0
    ref = restate(z, t, V, sel=sel_for(V), T=4)
    assert ref["argmax"][0] == 1 and ref["rank"][0] == 1 and ref["rank"][1] == V - 1
    assert out["entropy"][5] == 0.0 and out["logp"][5] == 0.0
    compare(out, ref, z, V, sel=sel_for(V), T=4)


def test_without_targets():
    V, rows = 129, 6
    rng = np.random.default_rng(8)
    z = make_logits(rng, rows, V, True, 5.0)
    st, out = launch(z, V, None, sel=sel_for(V), T=3)
    assert st == 0
    ref = restate(z, None, V, sel=sel_for(V), T=3)
    assert np.array_equal(out["acc"], np.zeros(4)) and (out["rank"] == -1).all()
    compare(out, ref, z, V, sel=sel_for(V), T=3)
    # delta with base 0 is log_softmax over the selected classes
    lsm = torch.log_softmax(torch.from_numpy(z[:, :V]).double(), -1).numpy()
    np.testing.assert_allclose(out["delta"][:, 0], lsm[:, 1], rtol=1e-6)


def test_two_launches_accumulate_and_runs_repeat():
    V, rows = 68, 4098
    rng = np.random.default_rng(21)
    z = make_logits(rng, rows, V, False, 2.0)
    t = make_targets(rng, rows, V)
    ref = restate(z, t, V, eps=0.05)
    acc = Guarded(32, fill=0)
    h = rows // 2
    for a, b in ((0, h), (h, rows)):
        st, out = launch(z[a:b].copy(), V, t[a:b], eps=0.05, acc=acc)
        assert st == 0
    assert out["acc"][2] == ref["acc"][2] and out["acc"][3] == ref["acc"][3]
    np.testing.assert_allclose(out["acc"][:2], ref["acc"][:2], rtol=1e-12, atol=0)
    # the same call twice: identical bits in every output
    _, o1 = launch(z, V, t, eps=0.05, sel=sel_for(V), T=2)
    _, o2 = launch(z, V, t, eps=0.05, sel=sel_for(V), T=2)
    for k in o1:
        assert np.array_equal(o1[k].view(np.uint8), o2[k].view(np.uint8)), k


def test_sequence_sum_is_independent_of_padding_and_neighbours():
    V = 68
    rng = np.random.default_rng(33)
    seq = make_logits(rng, 7, V, False, 2.0)
    tq = rng.integers(1, V, size=7).astype(np.int64)
    tq[3] = 0  # an ignored row inside the sequence
    # alone at T = 7 ...
    _, a = launch(seq, V, tq, T=7)
    # ... and as sequence 1 of 3 at T = 64, right-padded with ignored rows, beside other sequences
    z = make_logits(rng, 3 * 64, V, False, 2.0)
    t = rng.integers(1, V, size=3 * 64).astype(np.int64)
    z[64:71] = seq
    t[64:71] = tq
    t[71:128] = 0
    _, b = launch(z, V, t, T=64)
    assert a["seq_count"][0] == b["seq_count"][1] == 6
    assert a["seq_logp"].view(np.int64)[0] == b["seq_logp"].view(np.int64)[1]
    ref = restate(z, t, V, T=64)
    np.testing.assert_allclose(b["seq_logp"], ref["seq_logp"], rtol=1e-12, atol=0)


def test_ops_wrapper_and_T_above_64():
    """ops.score_rows allocates through cg_score_workspace; T = 130 rows per sequence (three per lane)."""
    from codonlm_amd import ops
    V, B, T = 68, 3, 130
    rng = np.random.default_rng(4)
    z = make_logits(rng, B * T, V, True, 2.0)
    t = make_targets(rng, B * T, V)
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    sel = torch.from_numpy(sel_for(V)).to(DEV)
    res = ops.score_rows(torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV), V=V, smoothing=0.05, sel=sel,
                         T=T, acc=acc, want=ops.SCORE_OUTPUTS)
    out = {k: getattr(res, k).cpu().numpy() for k in ops.SCORE_OUTPUTS + ("acc",)}
    compare(out, restate(z, t, V, eps=0.05, sel=sel_for(V), T=T), z, V, sel=sel_for(V), T=T)
