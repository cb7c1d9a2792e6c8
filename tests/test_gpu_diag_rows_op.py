"""cg_diag_rows against the fp64 numpy restatement of its contract (tests/context_restatement.py,
tied to the reference by tests/test_context_cpu.py).

The segment positions, the slice counts, the calibration counts and the correct-sums are integers
and must match exactly.  Every fp32 output is the single rounding of an fp64 value: within 1 fp32
ulp of the restatement.  The fp64 sums differ from it in summation order only: 1e-12 relative (all
terms of a sum have one sign).  The test asserts that no restated confidence lies within 4 fp32
ulps of an interior bin edge, so bin membership is not a rounding question.
"""
import numpy as np
import pytest
import torch

import context_restatement as CR
from test_gpu_score_op import within_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_BINS = 15


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_case(T, B, Vz, seed=0):
    """B rows of the shared generator (tokens < 20 <= Vz) with its forced corners, wide logits with
    NaN pad columns, an all-equal row and a one-hot-dominant row."""
    rng = np.random.default_rng(7000 * T + 10 * B + Vz + seed)
    xs, ys = [], []
    while sum(len(a) for a in xs) < B:
        _, _, xte, yte, _ = CR.make_split(T, seed=len(xs) + seed)
        xs.append(xte)
        ys.append(yte)
    x, y = np.concatenate(xs)[:B], np.concatenate(ys)[:B].copy()
    if Vz > CR.V:
        # a third of the codon targets move into [20, Vz): targets, class lookups and z_y reads above
        # the generator's vocabulary, and in the lane's second logits register when Vz > 64
        move = (y >= 8) & (rng.random(y.shape) < 1 / 3)
        y[move] = rng.integers(CR.V, Vz, size=int(move.sum()))
    z = CR.make_logits(rng, x, y, Vz, wide=True)
    flat_y = y.reshape(-1)
    live = np.flatnonzero(flat_y != CR.PAD)
    if len(live) >= 2:
        z[live[0], :Vz] = np.float32(0.25)        # all equal: conf = 1 / V, the argmax tie goes to index 0
        z[live[-1], :Vz] = np.float32(-60.0)      # one-hot dominant: conf == 1.0, the last bin
        z[live[-1], flat_y[live[-1]]] = np.float32(60.0)
    flags = (np.arange(B) % 3 == 1).astype(np.uint8)
    cls = (np.arange(Vz) % 4).astype(np.uint8)
    cls[:CR.V] = CR.token_classes(CR.ITOS)
    return x, y, z, flags, cls


def run(x, y, z, Vz, flags, cls, edges, want=None):
    from codonlm_amd import ops
    nb = len(edges) - 1
    acc = {"slices": torch.zeros(13, 2, dtype=torch.float64, device=DEV),
           "calib": torch.zeros(nb, 3, dtype=torch.float64, device=DEV),
           "brier_acc": torch.zeros(2, dtype=torch.float64, device=DEV)}
    res = ops.diag_rows(dev(z), dev(x), dev(y), V=Vz, pad_id=CR.PAD, sep_id=CR.SEP, row_flag=dev(flags),
                        tok_class=dev(cls), edges=dev(edges), want=ops.DIAG_OUTPUTS if want is None else want, **acc)
    torch.cuda.synchronize()
    return res


def compare(res, ref):
    assert np.array_equal(res.segpos.cpu().numpy(), ref["segpos"])
    within_ulp(res.nll.cpu().numpy(), ref["nll"])
    within_ulp(res.conf.cpu().numpy(), ref["conf"])
    assert np.array_equal(res.row_count.cpu().numpy(), ref["row_count"])
    np.testing.assert_allclose(res.row_nll.cpu().numpy(), ref["row_nll"], rtol=1e-12, atol=0)
    s = res.slices.cpu().numpy()
    assert np.array_equal(s[:, 1], ref["slices"][:, 1])
    np.testing.assert_allclose(s[:, 0], ref["slices"][:, 0], rtol=1e-12, atol=0)
    c = res.calib.cpu().numpy()
    assert np.array_equal(c[:, [0, 2]], ref["calib"][:, [0, 2]])
    np.testing.assert_allclose(c[:, 1], ref["calib"][:, 1], rtol=1e-12, atol=0)
    b = res.brier_acc.cpu().numpy()
    assert b[1] == ref["brier_acc"][1]
    np.testing.assert_allclose(b[0], ref["brier_acc"][0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("Vz", [20, 68, 128])
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("T", CR.TS)
def test_rows_against_fp64(T, B, Vz):
    x, y, z, flags, cls = make_case(T, B, Vz)
    edges = torch.linspace(0, 1, steps=N_BINS + 1).numpy()
    ref = CR.diag_rows(z, x, y, Vz, row_flag=flags, tok_class=cls, edges=edges)
    assert ref["edge_ulps"] > 4, "a confidence sits on a bin edge: change the seed"
    flat = ref["valid"].reshape(-1)
    if flat.sum() >= 2:
        first, last = np.flatnonzero(flat)[[0, -1]]
        assert ref["conf64"][first] == 1.0 / Vz and not ref["correct"].reshape(-1)[first]  # argmax 0 = PAD
        assert np.float32(ref["conf64"][last]) == 1.0 and ref["bin"].reshape(-1)[last] == N_BINS - 1
    compare(run(x, y, z, Vz, flags, cls, edges), ref)


def test_segment_counter_corners():
    """Position 1 has a PAD target (no advance), 2 and 3 are adjacent separators, 5 is a separator
    under a PAD target (no reset); the same row again at positions 62..69, across the wave boundary."""
    from codonlm_amd import ops
    xr = [3, 5, 3, 3, 6, 3, 7, 8]
    yr = [5, 0, 3, 6, 0, 0, 8, 9]
    x = np.full((1, 72), 9, np.int64)
    y = np.full((1, 72), 9, np.int64)
    x[0, :8], y[0, :8] = xr, yr
    x[0, 62:70], y[0, 62:70] = xr, yr
    z = CR.make_logits(np.random.default_rng(1), x, y, CR.V)
    res = ops.diag_rows(dev(z), dev(x), dev(y), V=CR.V, sep_id=CR.SEP, want=("segpos",))
    want = [0, -1, 0, 0, -1, -1, 1, 2] + list(range(3, 57)) + [0, -1, 0, 0, -1, -1, 1, 2] + [3, 4]
    assert res.segpos.cpu().numpy().tolist() == [want]
    assert CR.segment_positions(x, y).tolist() == [want]


def test_launches_accumulate_and_runs_repeat():
    from codonlm_amd import ops
    T, B, Vz = 130, 70, 68
    x, y, z, flags, cls = make_case(T, B, Vz, seed=4)
    edges = torch.linspace(0, 1, steps=N_BINS + 1).numpy()
    ref = CR.diag_rows(z, x, y, Vz, row_flag=flags, tok_class=cls, edges=edges)
    assert ref["edge_ulps"] > 4
    a = run(x, y, z, Vz, flags, cls, edges)
    b = run(x, y, z, Vz, flags, cls, edges)
    for k in ops.DIAG_OUTPUTS + ("slices", "calib", "brier_acc"):
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k
    # the same rows in two launches into the same accumulators
    h = 33
    slices = torch.zeros(13, 2, dtype=torch.float64, device=DEV)
    calib = torch.zeros(N_BINS, 3, dtype=torch.float64, device=DEV)
    brier = torch.zeros(2, dtype=torch.float64, device=DEV)
    for lo, hi in ((0, h), (h, B)):
        ops.diag_rows(dev(z[lo * T:hi * T]), dev(x[lo:hi]), dev(y[lo:hi]), V=Vz, sep_id=CR.SEP, row_flag=dev(flags[lo:hi]),
                      tok_class=dev(cls), edges=dev(edges), slices=slices, calib=calib, brier_acc=brier)
    s = slices.cpu().numpy()
    assert np.array_equal(s[:, 1], ref["slices"][:, 1])
    np.testing.assert_allclose(s[:, 0], ref["slices"][:, 0], rtol=1e-12, atol=0)
    assert np.array_equal(calib.cpu().numpy()[:, [0, 2]], ref["calib"][:, [0, 2]])
    assert brier.cpu().numpy()[1] == ref["brier_acc"][1]


def test_rows_pass_the_grid_cap_and_optional_inputs():
    """More rows than the grid cap (2048), no row flags, no class table, no calibration."""
    from codonlm_amd import ops
    T, B, Vz = 5, 2100, 20
    rng = np.random.default_rng(12)
    x, y = CR.make_rows(rng, B, T, p_sep=0.2)
    z = CR.make_logits(rng, x, y, Vz)
    ref = CR.diag_rows(z, x, y, Vz)
    slices = torch.zeros(13, 2, dtype=torch.float64, device=DEV)
    res = ops.diag_rows(dev(z), dev(x), dev(y), V=Vz, sep_id=CR.SEP, slices=slices, want=("segpos", "row_nll"))
    assert np.array_equal(res.segpos.cpu().numpy(), ref["segpos"])
    np.testing.assert_allclose(res.row_nll.cpu().numpy(), ref["row_nll"], rtol=1e-12, atol=0)
    s = slices.cpu().numpy()
    assert np.array_equal(s[:, 1], ref["slices"][:, 1]) and s[2, 1] == 0 and (s[9:, 1] == 0).all()
    np.testing.assert_allclose(s[:9, 0], ref["slices"][:9, 0], rtol=1e-12, atol=0)


def test_refusals():
    from codonlm_amd import ops
    x = torch.ones(2, 4, dtype=torch.int64, device=DEV)
    z = torch.zeros(8, 129, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="CG_EUNSUPPORTED"):
        ops.diag_rows(z, x, x, V=129)
    with pytest.raises(ValueError, match="CG_EINVAL"):
        ops.diag_rows(z, x, x, V=20, edges=torch.linspace(0, 1, 34).to(DEV))
    ops.diag_rows(z[:0], x[:0], x[:0], V=20)  # rows == 0 is fine
