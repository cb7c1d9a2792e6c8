"""cg_gram_accum and cg_shape_targets against the fp64 numpy restatement of their contracts
(tests/probe_restatement.py).

Bound of a Gram entry: the inputs widen exactly and every product of two of them is exact in fp64
for integer data and rounds once otherwise; n_g products are added in some fixed order, and an
accumulating call adds one more rounding:  |got - ref| <= (n_g + 2) 2^-53 sum_r |z_ri| |z_rj|.
With integer |z| <= 2^10 every partial sum is an integer below 2^53, so the result is exact.
"""
import numpy as np
import pytest
import torch

import probe_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -53
SENT = -7.25  # what the pad columns of gram hold before a call
VOCAB = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _groups(rng, rows, G):
    """Group ids with every kind of skipped value in them (when there is room)."""
    grp = rng.integers(0, G, size=rows).astype(np.int32)
    for i, v in enumerate((-1, G, 2 ** 31 - 1, -2 ** 31)):
        if rows > 2 * (i + 1):
            grp[(3 * i + 1) % rows] = v
    return grp


def _call(h, y, m, grp, G, dtype, gram_buf=None, accumulate=False, workspace=None):
    """Runs ops.gram_accum on padded buffers: NaN in every pad column of h and y and in every skipped
    row, SENT in the pad columns of gram.  Returns the (G, P, ldg) buffer."""
    from codonlm_amd import ops
    rows, d = h.shape
    P = d + m + 1
    skipped = (grp < 0) | (grp >= G)
    # odd and even row strides
    hb = torch.full((rows, d + (3 if rows % 2 else 2)), float("nan"), dtype=TDT[dtype], device=DEV)
    hb[:, :d] = torch.from_numpy(h).to(DEV).to(TDT[dtype])
    hb[torch.from_numpy(skipped).to(DEV)] = float("nan")
    yv = None
    if y is not None:
        yb = torch.full((rows, y.shape[1] + 2), float("nan"), dtype=torch.float32, device=DEV)
        yb[:, :y.shape[1]] = torch.from_numpy(y).to(DEV)
        yb[torch.from_numpy(skipped).to(DEV)] = float("nan")
        yv = yb[:, :y.shape[1]]
    if gram_buf is None:
        gram_buf = torch.full((G, P, P + 5), SENT, dtype=torch.float64, device=DEV)
    out = ops.gram_accum(hb[:, :d], yv, torch.from_numpy(grp).to(DEV), G, gram_buf[:, :, :P], m=m if y is not None else None,
                         accumulate=accumulate, workspace=workspace)
    assert out.data_ptr() == gram_buf.data_ptr()
    return gram_buf


def _as_dtype(a, dtype):
    """The fp32 array rounded to what the dtype stores."""
    return torch.from_numpy(a).to(TDT[dtype]).to(torch.float32).numpy()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("d", [6, 64, 200])
@pytest.mark.parametrize("rows", [1, 5, 70, 300])
def test_gram_accum_against_the_restatement(rows, d, dtype):
    rng = np.random.default_rng(1000 * rows + d)
    r, c = np.arange(rows)[:, None], np.arange(d)[None, :]
    # exact integer data, asymmetric in row and column: x from 3c + r, y from r^2; bf16 stores multiples of 8
    step = 8 if dtype == "bf16" else 1
    xi = (((3 * c + r) * 37) % (2048 // step + 1) - 1024 // step) * step
    yi = ((r * r * 5 + 11 * np.arange(14)[None, :]) % 2049) - 1024
    assert np.abs(xi).max() <= 1024 and np.abs(yi).max() <= 1024
    xr = _as_dtype(rng.standard_normal((rows, d)).astype(np.float32) * 3 + 0.5, dtype)
    yr = (rng.standard_normal((rows, 14)) * 2 - 1).astype(np.float32)
    for m in (0, 14):
        for G in (1, 5):
            grp = _groups(rng, rows, G)
            P = d + m + 1
            # ---- integers: bitwise the int64 Gram
            xs = xi.astype(np.float32)
            assert np.array_equal(_as_dtype(xs, dtype), xs)
            buf = _call(xs, yi.astype(np.float32) if m else None, m, grp, G, dtype)
            got = buf[:, :, :P].cpu().numpy()
            zi = np.concatenate([xi] + ([yi] if m else []) + [np.ones((rows, 1), np.int64)], axis=1).astype(np.int64)
            for g in range(G):
                zg = zi[grp == g]
                assert np.array_equal(got[g], (zg.T @ zg).astype(np.float64)), (m, G, g)
                assert got[g, P - 1, P - 1] == (grp == g).sum()
            assert bool((buf[:, :, P:] == SENT).all())
            # ---- random data: the bound, symmetry, reproducibility
            buf = _call(xr, yr if m else None, m, grp, G, dtype)
            got = buf[:, :, :P].cpu().numpy()
            ref, mag, cnt = R.gram(xr, yr if m else None, m, grp, G)
            bound = (cnt[:, None, None] + 2) * EPS * mag
            assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all(), (m, G)
            assert np.array_equal(got, got.transpose(0, 2, 1))
            assert torch.equal(_call(xr, yr if m else None, m, grp, G, dtype), buf)
            assert bool((buf[:, :, P:] == SENT).all())
            # ---- accumulate = 1 over two half-batches against the one call
            if rows > 1:
                half = rows // 2
                acc = _call(xr[:half], yr[:half] if m else None, m, grp[:half], G, dtype)
                acc = _call(xr[half:], yr[half:] if m else None, m, grp[half:], G, dtype, gram_buf=acc, accumulate=True)
                two = acc[:, :, :P].cpu().numpy()
                assert (np.abs(two - ref) <= bound).all() and (np.abs(two - got) <= bound).all()
                assert np.array_equal(two, two.transpose(0, 2, 1)) and bool((acc[:, :, P:] == SENT).all())


def test_gram_accum_empty_groups_rows_and_slices():
    """accumulate = 0 clears an empty group; rows == 0 touches nothing with accumulate = 1 and zeroes
    without; several slices per group (rows >> 64 G) sum to the same Gram within the bound, and a
    reused workspace changes nothing."""
    from codonlm_amd import ops
    rng = np.random.default_rng(5)
    rows, d, m, G = 300, 6, 14, 5
    P = d + m + 1
    x = rng.standard_normal((rows, d)).astype(np.float32)
    y = rng.standard_normal((rows, m)).astype(np.float32)
    grp = rng.integers(0, 3, size=rows).astype(np.int32)  # groups 3 and 4 stay empty
    garbage = torch.full((G, P, P + 5), float("nan"), dtype=torch.float64, device=DEV)
    garbage[:, :, P:] = SENT
    buf = _call(x, y, m, grp, G, "fp32", gram_buf=garbage)
    got = buf[:, :, :P].cpu().numpy()
    assert (got[3:] == 0.0).all() and np.isfinite(got).all() and got[:3, P - 1, P - 1].sum() == rows
    before = buf.clone()
    e = torch.empty(0, d, device=DEV)
    ops.gram_accum(e, torch.empty(0, m, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), G, buf[:, :, :P],
                   accumulate=True)
    assert torch.equal(buf, before)
    ops.gram_accum(e, torch.empty(0, m, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), G, buf[:, :, :P])
    assert bool((buf[:, :, :P] == 0).all()) and bool((buf[:, :, P:] == SENT).all())
    # rows >> 64 G: the group's rows are cut into several slices
    rows = 3000
    x = rng.standard_normal((rows, d)).astype(np.float32)
    y = rng.standard_normal((rows, m)).astype(np.float32)
    grp = _groups(rng, rows, 2)
    ws = ops.gram_workspace(rows, d, m, 2, DEV)
    buf = _call(x, y, m, grp, 2, "fp32", workspace=ws)
    ref, mag, cnt = R.gram(x, y, m, grp, 2)
    got = buf[:, :, :P].cpu().numpy()
    assert (np.abs(got - ref) <= (cnt[:, None, None] + 2) * EPS * mag).all()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    assert torch.equal(_call(x, y, m, grp, 2, "fp32"), buf)
    # a 3-D hidden-state view (B, T, d) is taken as its B*T rows
    g3 = ops.gram_accum(torch.from_numpy(x).to(DEV).view(30, 100, d), torch.from_numpy(y).to(DEV),
                        torch.from_numpy(grp).to(DEV), 2)
    assert torch.equal(g3, buf[:, :, :P])
    # a view that starts at an odd column of a wider buffer: rows aligned to one element only
    wide = torch.full((rows, d + 2), float("nan"), device=DEV)
    wide[:, 1:d + 1] = torch.from_numpy(x).to(DEV)
    g4 = ops.gram_accum(wide[:, 1:d + 1], torch.from_numpy(y).to(DEV), torch.from_numpy(grp).to(DEV), 2)
    assert torch.equal(g4, buf[:, :, :P])


def test_gram_accum_wrapper_errors():
    from codonlm_amd import _lib as L
    from codonlm_amd import ops
    h = torch.zeros(8, 6, device=DEV)
    y = torch.zeros(8, 14, device=DEV)
    grp = torch.zeros(8, dtype=torch.int32, device=DEV)
    ok = ops.gram_accum(h, y, grp, 2)
    assert tuple(ok.shape) == (2, 21, 21) and float(ok[0, 20, 20]) == 8.0
    bad = [
        lambda: ops.gram_accum(h, y, grp.to(torch.int64), 2),            # grp dtype
        lambda: ops.gram_accum(h, y, grp[:7], 2),                        # grp length
        lambda: ops.gram_accum(h, y[:7], grp, 2),                        # y rows
        lambda: ops.gram_accum(h, y, grp, 0),                            # G < 1
        lambda: ops.gram_accum(h, y, grp, 2, m=15),                      # more columns than y has
        lambda: ops.gram_accum(h, y.double(), grp, 2),                   # y dtype
        lambda: ops.gram_accum(h, None, grp, 2, m=3),                    # m without y
        lambda: ops.gram_accum(h, y, grp, 2, accumulate=True),           # nothing to add to
        lambda: ops.gram_accum(h, y, grp, 2, torch.zeros(2, 21, 20, dtype=torch.float64, device=DEV)),
        lambda: ops.gram_accum(h, y, grp, 2, torch.zeros(2, 21, 21, dtype=torch.float32, device=DEV)),
        lambda: ops.gram_accum(h.double(), y, grp, 2),                   # dtype
        lambda: ops.gram_accum(h.t(), None, grp[:6], 2),                 # column stride
        lambda: ops.gram_accum(h, y, grp, 4097),                         # unsupported G
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    # the library's own checks surface as ValueError through the wrapper's status check
    ws = ops.gram_workspace(8, 6, 14, 2, DEV)
    g = torch.zeros(2, 21, 21, dtype=torch.float64, device=DEV)

    def raw(**kw):
        a = dict(dtype=L.CG_F32, h=h.data_ptr(), ldh=6, d=6, y=y.data_ptr(), ldy=14, m=14, grp=grp.data_ptr(), rows=8,
                 G=2, acc=0, gram=g.data_ptr(), ldg=21, ws=ws.data_ptr(), wsb=ws.numel())
        a.update(kw)
        L.check(L.lib.cg_gram_accum(a["dtype"], a["h"], a["ldh"], a["d"], a["y"], a["ldy"], a["m"], a["grp"], a["rows"],
                                    a["G"], a["acc"], a["gram"], a["ldg"], a["ws"], a["wsb"], L.stream_ptr(h.device)),
                "cg_gram_accum")
    raw()
    for kw in (dict(h=None), dict(y=None), dict(grp=None), dict(gram=None), dict(ws=None), dict(ldh=5), dict(ldy=13),
               dict(ldg=20), dict(rows=-1), dict(G=0), dict(acc=3), dict(wsb=16), dict(d=-1), dict(m=-1)):
        with pytest.raises(ValueError):
            raw(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ cg_shape_targets
def _targets(idx, itos, ldy=17):
    from codonlm_amd import ops
    from codonlm_amd.structure_probe import codon_table
    B, T = idx.shape
    out = torch.full((B * T, ldy), float("nan"), dtype=torch.float32, device=DEV)
    y, valid = ops.shape_targets(torch.from_numpy(idx).to(DEV), codon_table(itos), out=out[:, :14])
    assert y.data_ptr() == out.data_ptr() and valid.dtype == torch.int32
    return out.cpu().numpy(), valid.cpu().numpy()


def _check(idx, itos, want_y, want_valid):
    out, valid = _targets(idx, itos)
    assert np.array_equal(valid, want_valid)
    on = valid.astype(bool)
    assert np.array_equal(out[on, :14].view(np.uint32), want_y[on].view(np.uint32))
    assert np.isnan(out[~on]).all() and np.isnan(out[:, 14:]).all()  # rows and pad columns never written


def test_shape_targets_equal_the_reference_bitwise(golden):
    _, g = golden("shape_targets")
    stoi = {t: i for i, t in enumerate(VOCAB)}
    dna = [str(s) for s in g["dna"]]
    T = max(len(s) for s in dna) // 3
    idx = np.zeros((len(dna), T), dtype=np.int64)  # PAD after every string
    want = np.zeros((len(dna) * T, 14), dtype=np.float32)
    valid = np.zeros(len(dna) * T, dtype=np.int32)
    for i, s in enumerate(dna):
        n = len(s) // 3
        idx[i, :n] = [stoi[s[j:j + 3]] for j in range(0, len(s), 3)]
        want[i * T:i * T + n] = g[f"y_{i}"]
        valid[i * T:i * T + n] = 1
    _check(idx, VOCAB, want, valid)
    for i, s in enumerate(dna):  # each string alone, T = its length (1 and 2 among them)
        n = len(s) // 3
        _check(idx[i:i + 1, :n].copy(), VOCAB, g[f"y_{i}"], np.ones(n, np.int32))


@pytest.mark.parametrize("T", [1, 2, 40])
def test_shape_targets_with_specials_equal_the_restatement(T):
    rng = np.random.default_rng(T)
    stoi = {t: i for i, t in enumerate(VOCAB)}
    B = 12
    idx = rng.integers(4, 68, size=(B, T)).astype(np.int64)
    if T == 40:
        tract = [stoi[c] for c in ("AAA", "AAA", "GGC", "CGG", "CCA", "AAA", "ACG", "TAT")]
        for b in range(B):
            idx[b, 10:18] = tract
        idx[0, 0], idx[0, 39] = 1, 2                 # BOS at the start, EOS at the end
        idx[1, 0:2] = (1, 3)                          # specials adjacent to each other at the start
        idx[2, 37:40] = (2, 0, 0)                     # EOS then PAD at the end
        idx[3, 9], idx[3, 18] = 3, 3                  # SEP on both sides of the tract
        idx[4, 11], idx[4, 12] = 3, 2                 # specials inside the tract, adjacent
        idx[5, 13] = 0                                # PAD splitting GGC | CGG
        idx[6, 14] = 68                               # an id just past V
        idx[7, 15], idx[7, 16] = 255, 256             # the last id of the table's range, and one past it
        idx[8, 10], idx[8, 17] = 10 ** 12, -1         # far out of range, negative
        idx[9, :] = 0                                 # all PAD
        idx[10, 1::2] = 3                             # every run one codon long
    else:
        idx[0, 0] = 0
        idx[1, T - 1] = 3
        idx[2, 0] = 300
        idx[3, :] = 2
    want, valid = R.shape_targets(idx, VOCAB)
    assert 0 < valid.sum() < B * T
    _check(idx, VOCAB, want, valid)


def test_shape_targets_wrapper_errors():
    from codonlm_amd import ops
    idx = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    for f in (lambda: ops.shape_targets(idx, [0] * 257), lambda: ops.shape_targets(idx, [64] * 8),
              lambda: ops.shape_targets(idx[0], [0] * 8),
              lambda: ops.shape_targets(idx, [0] * 8, out=torch.zeros(8, 13, device=DEV)),
              lambda: ops.shape_targets(idx, [0] * 8, out=torch.zeros(7, 14, device=DEV)),
              lambda: ops.shape_targets(idx, [0] * 8, out=torch.zeros(8, 14, dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            f()
    y, valid = ops.shape_targets(torch.zeros(0, 4, dtype=torch.int64, device=DEV), [0] * 8)
    assert tuple(y.shape) == (0, 14) and valid.numel() == 0
