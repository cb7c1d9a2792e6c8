"""cg_ngram_count / cg_ngram_totals / cg_ngram_nll against the fp64 numpy restatement of their
contract (tests/context_restatement.py, tied to the reference by tests/test_context_cpu.py).

Count tables and totals are integers and must match exactly, however the rows are split into
launches.  The kernel evaluates every nll in fp64 and rounds once, so the per-token fp32 values lie
within 1 fp32 ulp of the restatement; the fp64 sums differ from it in summation order and in the
last bits of log only: 1e-12 of the sum of the terms' magnitudes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import context_restatement as CR
from test_gpu_score_op import within_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 0.01


@pytest.fixture(scope="module")
def splits():
    """Per T: the split, the restated tables and the restated baseline nll (computed once)."""
    out = {}
    for T in CR.TS:
        xtr, ytr, xte, yte, _ = CR.make_split(T)
        tables = CR.count_tables(xtr, ytr)
        out[T] = (xtr, ytr, xte, yte, tables, CR.ngram_nll(xte, yte, tables, ALPHA))
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fit(x, y, chunk=None, Vn=CR.V, reset=(CR.SEP,)):
    from codonlm_amd import ops
    tables = ops.NgramTables(Vn, DEV, CR.PAD, reset)
    step = chunk or len(x)
    for a in range(0, len(x), step):
        ops.ngram_count(tables, dev(x[a:a + step]), dev(y[a:a + step]))
    return ops.ngram_totals(tables)


def same_tables(tables, ref):
    uni, bi, tri, bad = ref
    assert np.array_equal(tables.uni.cpu().numpy(), uni)
    assert np.array_equal(tables.bi.cpu().numpy(), bi)
    assert np.array_equal(tables.tri.cpu().numpy(), tri)
    assert int(tables.n_bad) == bad
    tu, tb, tt = CR.totals(uni, bi, tri)
    assert np.array_equal(tables.uni_total.cpu().numpy(), tu)
    assert np.array_equal(tables.bi_total.cpu().numpy(), tb)
    assert np.array_equal(tables.tri_total.cpu().numpy(), tt)


@pytest.mark.parametrize("chunk", [None, 1, 3, 36])
@pytest.mark.parametrize("T", CR.TS)
def test_counts_and_totals_are_exact(splits, T, chunk):
    xtr, ytr, _, _, ref, _ = splits[T]
    same_tables(fit(xtr, ytr, chunk), ref)


@pytest.mark.parametrize("T", CR.TS)
def test_nll_against_fp64(splits, T):
    from codonlm_amd import ops
    xtr, ytr, xte, yte, _, ref = splits[T]
    tables = fit(xtr, ytr)
    acc = torch.zeros(5, dtype=torch.float64, device=DEV)
    res = ops.ngram_nll(tables, dev(xte), dev(yte), ALPHA, acc=acc, want=ops.NGRAM_OUTPUTS)
    within_ulp(res.tok_tri.cpu().numpy(), ref["tok"][3])
    assert (res.tok_tri.cpu().numpy()[~ref["counted"]] == 0).all()
    assert np.array_equal(res.row_count.cpu().numpy(), ref["row_count"])
    scale = np.abs(ref["tok"]).sum(-1).T  # [B][4]: the sum of a row's |terms|
    assert (np.abs(res.row_sums.cpu().numpy() - ref["row_sums"]) <= 1e-12 * scale).all()
    a = acc.cpu().numpy()
    assert a[4] == ref["acc"][4]
    assert (np.abs(a[:4] - ref["acc"][:4]) <= 1e-12 * ref["abs_terms"]).all()
    # a second launch adds to acc; the same call twice gives the same bits
    res2 = ops.ngram_nll(tables, dev(xte), dev(yte), ALPHA, acc=acc, want=ops.NGRAM_OUTPUTS)
    assert (np.abs(acc.cpu().numpy()[:4] - 2 * ref["acc"][:4]) <= 2e-12 * ref["abs_terms"]).all()
    for k in ops.NGRAM_OUTPUTS:
        assert torch.equal(getattr(res, k).view(torch.uint8), getattr(res2, k).view(torch.uint8)), k
    acc3 = torch.zeros(5, dtype=torch.float64, device=DEV)
    ops.ngram_nll(tables, dev(xte), dev(yte), ALPHA, acc=acc3, want=())
    assert np.array_equal(acc3.cpu().numpy().view(np.int64), a.view(np.int64))


def test_many_rows_pass_the_grid_cap():
    """More rows than the nll kernel's 4 * 1024 per pass, at the widest vocabulary (64 KB of LDS)."""
    from codonlm_amd import ops
    Vn, B, T = 128, 4500, 9
    rng = np.random.default_rng(9)
    x = rng.integers(0, Vn, size=(B, T)).astype(np.int64)
    y = rng.integers(0, Vn, size=(B, T)).astype(np.int64)
    y[rng.random((B, T)) < 0.1] = CR.PAD
    reset = (CR.SEP, 100)
    ref_t = CR.count_tables(x, y, Vn, CR.PAD, reset)
    tables = fit(x, y, Vn=Vn, reset=reset)
    same_tables(tables, ref_t)
    ref = CR.ngram_nll(x, y, ref_t, ALPHA, Vn, CR.PAD, reset)
    acc = torch.zeros(5, dtype=torch.float64, device=DEV)
    res = ops.ngram_nll(tables, dev(x), dev(y), ALPHA, acc=acc, want=ops.NGRAM_OUTPUTS)
    within_ulp(res.tok_tri.cpu().numpy(), ref["tok"][3])
    assert np.array_equal(res.row_count.cpu().numpy(), ref["row_count"])
    a = acc.cpu().numpy()
    assert a[4] == ref["acc"][4]
    assert (np.abs(a[:4] - ref["acc"][:4]) <= 1e-12 * ref["abs_terms"]).all()


def test_count_passes_its_grid_cap():
    """More positions than 1024 workgroups x 2048 take in one stride: every workgroup loops."""
    B, T = 2150, 1024
    rng = np.random.default_rng(31)
    x, y = CR.make_rows(rng, B, T)
    assert x.size > 1024 * 2048
    same_tables(fit(x, y), CR.count_tables(x, y))


def test_out_of_range_tokens_land_in_n_bad_only(splits):
    xtr, ytr, _, _, ref, _ = splits[65]
    x, y = xtr.copy(), ytr.copy()
    live = np.argwhere(y != CR.PAD)
    (b0, t0), (b1, t1), (b2, t2) = live[5], live[40], live[90]
    x[b0, t0] = CR.V          # previous out of range (and previous2 of the next position)
    y[b1, t1] = CR.V + 3      # target out of range
    x[b2, t2] = -1
    want = CR.count_tables(x, y)
    assert want[0].sum() < ref[0].sum()  # the skipped positions are counted nowhere
    tables = fit(x, y)
    same_tables(tables, want)
    assert int(tables.n_bad) == want[3] >= 3


def test_refusals():
    from codonlm_amd import _lib as L
    from codonlm_amd import ops
    with pytest.raises(ValueError):
        ops.NgramTables(129, DEV)
    z = torch.zeros(129 ** 2, dtype=torch.int64, device=DEV)
    xy = torch.ones(2, 4, dtype=torch.int64, device=DEV)
    mask = (C.c_uint32 * 8)()
    st = L.lib.cg_ngram_count(xy.data_ptr(), xy.data_ptr(), 2, 4, 129, 0, mask, z.data_ptr(), z.data_ptr(),
                              z.data_ptr(), None, None)
    assert st == L.CG_EUNSUPPORTED
    tables = fit(np.ones((2, 4), np.int64), np.ones((2, 4), np.int64))
    with pytest.raises(ValueError, match="CG_EINVAL"):
        ops.ngram_nll(tables, xy, xy, 0.0)
    with pytest.raises(ValueError, match="CG_EINVAL"):
        ops.ngram_nll(tables, xy, xy, -1.0)
    # rows == 0 touches nothing
    before = tables.tri.clone()
    ops.ngram_count(tables, xy[:0], xy[:0])
    torch.cuda.synchronize()
    assert torch.equal(before, tables.tri)
