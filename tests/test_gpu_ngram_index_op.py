"""cg_ngram_index_build / cg_ngram_coverage against the Python-set restatement of the reference's
window sets (tests/memorization_restatement.py).  Every comparison is exact integer equality: which
duplicate a slot holds is not defined, n_unique and the coverage outputs are."""
import ctypes

import numpy as np
import pytest
import torch

import memorization_restatement as MR

pytestmark = pytest.mark.gpu


def _mods():
    from codonlm_amd import _lib as L, memorization as M, ops
    return L, M, ops


def _index(seqs, n, capacity=None):
    _, M, ops = _mods()
    flat, offsets = M.pack_sequences(seqs)
    return ops.NgramIndex(torch.from_numpy(flat).cuda(), offsets, n, capacity=capacity)


def _check_queries(index, table, n, qs):
    """hit, n_hit and covered of every query equal the restatement's."""
    _, M, ops = _mods()
    flat, qoff = M.pack_sequences(qs)
    res = ops.ngram_coverage(index, torch.from_numpy(flat).cuda(), qoff, want=ops.COVERAGE_OUTPUTS)
    hit, n_hit, covered = res.hit.cpu().numpy(), res.n_hit.cpu().numpy(), res.covered.cpu().numpy()
    for q, seq in enumerate(qs):
        h, nh, nc = MR.coverage(seq, table, n)
        assert np.array_equal(hit[qoff[q]:qoff[q + 1]], h), q
        assert (int(n_hit[q]), int(covered[q])) == (nh, nc), q
    return n_hit, covered


@pytest.mark.parametrize("alphabet", MR.ALPHABETS)
@pytest.mark.parametrize("n", MR.BUILD_N)
def test_build_and_coverage_match_the_set(n, alphabet):
    _, _, ops = _mods()
    train = MR.training_set(n, alphabet)
    table = MR.build(train, n)
    q = MR.queries(n, alphabet, train)
    names, qs = list(q), list(q.values())

    one = ops.ngram_index_build(_index(train, n))  # default capacity, one launch
    assert int(one.n_unique.item()) == len(table) and int(one.n_dropped.item()) == 0
    if alphabet == 1:
        assert len(table) == 1
    n_hit, covered = _check_queries(one, table, n, qs)
    if len(q["copy"]) >= n:
        assert int(covered[names.index("copy")]) == len(q["copy"])
        assert int(covered[names.index("mutated")]) < len(q["mutated"])

    parts = _index(train, n)  # sequence by sequence: the same set
    for s in range(len(train)):
        ops.ngram_index_build(parts, s, s + 1)
        assert int(parts.n_unique.item()) == len(MR.build(train, n, 0, s + 1)), s
    ops.ngram_index_build(parts)  # every window again: all duplicates
    assert int(parts.n_unique.item()) == len(table) and int(parts.n_dropped.item()) == 0
    _check_queries(parts, table, n, qs)


@pytest.mark.parametrize("n", MR.BUILD_N)
def test_tight_capacity_with_distinct_windows(n):
    _, _, ops = _mods()
    train = MR.distinct_training_set(n)  # asserts distinctness on the CPU
    windows = MR.window_total(train, n)
    cap = MR.tight_capacity(windows)
    index = ops.ngram_index_build(_index(train, n, capacity=cap))
    assert index.capacity == cap and cap // 2 <= windows < cap
    assert int(index.n_unique.item()) == windows and int(index.n_dropped.item()) == 0
    filled = int((index.table != -1).sum().item())
    assert filled == windows
    table = MR.build(train, n)
    rng = np.random.default_rng(n)
    qs = [MR.longest(train).copy(), rng.integers(0, 251, size=300).astype(np.uint8),
          np.concatenate([train[-1], train[1]])]
    n_hit, covered = _check_queries(index, table, n, qs)
    assert int(covered[0]) == len(qs[0])


@pytest.mark.parametrize("n", (5, 10))
def test_partial_hits_over_four_symbols(n):
    _, _, ops = _mods()
    train, qs = MR.partial_hit_case(n)
    table = MR.build(train, n)
    for q in qs[:2]:
        hits = MR.coverage(q, table, n)[1]
        assert 0 < hits < len(q) - n + 1  # the case is not vacuous
    index = ops.ngram_index_build(_index(train, n))
    assert int(index.n_unique.item()) == len(table)
    _check_queries(index, table, n, qs)


def test_packed_rows_and_empty_work():
    """Packed rows [R][T] (offsets = r * T), a query set with no query, an index with no window."""
    _, M, ops = _mods()
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, size=(5, 64)).astype(np.uint8)
    X[3, 20:] = 0  # a pad run
    idx = M.TrainIndex.from_rows(torch.from_numpy(X.astype(np.int64)).cuda(), 10)
    table = MR.build(list(X), 10)
    assert idx.n_unique == len(table)
    _check_queries(idx.index, table, 10, [X[1], X[3], X.reshape(-1)[30:100]])
    before = idx.index.table.clone()
    ops.ngram_index_build(idx.index, 2, 2)  # zero work touches nothing
    assert torch.equal(before, idx.index.table) and idx.n_unique == len(table)
    res = ops.ngram_coverage(idx.index, torch.zeros(0, dtype=torch.uint8, device="cuda"), np.zeros(1, dtype=np.int64))
    assert res.n_hit.numel() == 0
    empty = ops.ngram_index_build(_index([np.zeros(3, dtype=np.uint8)], 10))
    assert int(empty.n_unique.item()) == 0
    _check_queries(empty, set(), 10, [np.zeros(40, dtype=np.uint8)])
    capped = M.TrainIndex.from_rows(X.astype(np.int64), 10, max_tokens=100)  # rows 0 and 1: 0 < 100, 64 < 100
    assert capped.rows_indexed == 2 and capped.n_unique == len(MR.build(list(X[:2]), 10))
    with pytest.raises(ValueError):
        M.TrainIndex.from_rows(np.full((2, 16), 256, dtype=np.int64), 4)


def test_argument_errors():
    """Host-side argument checks: nothing is launched."""
    L, _, ops = _mods()
    train = MR.training_set(10, 64)
    index = _index(train, 10)

    def desc(**kw):
        d = L.NgramIndexDesc()
        d.sym, d.n_sym = index.sym.data_ptr(), index.sym.numel()
        d.offsets, d.n_seq, d.seq_lo, d.seq_hi = index.offsets.data_ptr(), index.n_seq, 0, index.n_seq
        d.n, d.table, d.capacity = 10, index.table.data_ptr(), index.capacity
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    build = lambda d: L.lib.cg_ngram_index_build(ctypes.byref(d), None)  # noqa: E731
    assert build(desc(n=33)) == L.CG_EUNSUPPORTED
    assert build(desc(n=0)) == L.CG_EINVAL
    assert build(desc(capacity=index.capacity - 1)) == L.CG_EINVAL
    assert build(desc(capacity=3 * 1024)) == L.CG_EINVAL
    assert build(desc(table=None)) == L.CG_EINVAL
    assert build(desc(seq_hi=index.n_seq + 1)) == L.CG_EINVAL
    c = L.NgramCoverageDesc()
    c.sym, c.n_sym, c.n = index.sym.data_ptr(), index.sym.numel(), 10
    c.table, c.capacity = index.table.data_ptr(), index.capacity
    c.qsym, c.n_qsym, c.qoffsets, c.n_q = index.sym.data_ptr(), index.sym.numel(), index.offsets.data_ptr(), index.n_seq
    c.max_qlen = L.NGRAM_MAX_QUERY + 1
    assert L.lib.cg_ngram_coverage(ctypes.byref(c), None) == L.CG_EUNSUPPORTED
    c.max_qlen, c.n = 1000, 33
    assert L.lib.cg_ngram_coverage(ctypes.byref(c), None) == L.CG_EUNSUPPORTED
    c.n, c.table = 10, None
    assert L.lib.cg_ngram_coverage(ctypes.byref(c), None) == L.CG_EINVAL
    assert int((index.table != -1).sum().item()) == 0  # no call above inserted anything
    with pytest.raises(ValueError):
        ops.NgramIndex(index.sym, index.host_offsets, 33)
    with pytest.raises(ValueError):
        ops.NgramIndex(index.sym, index.host_offsets, 10, capacity=1024)  # not above the window count
    with pytest.raises(ValueError):
        ops.ngram_coverage(index, torch.zeros(L.NGRAM_MAX_QUERY + 1, dtype=torch.uint8, device="cuda"),
                           np.array([0, L.NGRAM_MAX_QUERY + 1]))
