"""The LDS-DMA ring of the grouped dW kernel's 256 x 256 tile (cg_gemm_dw_grouped, tile code 512;
csrc/gemm_dw.h): 32-token stages on a 5-slot ring, fragments read one stage ahead.

The shapes are the ones at which a ring can go wrong and that test_gemm_dw_grouped_tiles
(K in {2048, 1023, 37}) does not reach: fewer stages than slots, token counts at the edges of a
32-token stage and of the 64-token k-unit, one workgroup walking every tile so that stages of
different tiles and products share the ring (max_wg), token splits with empty and ragged last
slices, a column-summing tile next to a plain one, and sentinels around every output.

Reference: the fp32 product of the same bf16 operands (dW = alpha dY^T X, the autograd of the
nn.Linear weights, model_tiny_gpt.py:85-93, 143-148).  Bound: the one of
test_gemm_dw_grouped_tiles, max error <= 1e-5 of the output scale."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 512
SENT = 1234.5
# exactly one tile; 2 x 3 tiles with partial edges; less than a tile: 8 tiles in all
SHAPES = [(256, 256), (264, 520), (72, 136)]
EDGE_K = [1, 8, 31, 32, 33, 63, 64, 65, 96, 97, 129, 160, 161]


def _ops():
    from codonlm_amd import ops
    return ops


def _products(K, seed, colsum_on=()):
    """-> (products, frames, refs, prevs): dy with row stride N_out + 8, alpha 0.5 + accumulate on
    the second product, every output a window of a larger sentinel-filled frame (ldc = K_out + 12,
    one extra row above and two below)."""
    g = torch.Generator().manual_seed(seed)
    prods, frames, refs = [], [], []
    for i, (n, k) in enumerate(SHAPES):
        dy = (torch.randn(K, n + 8, generator=g) + (0.3 if i in colsum_on else 0.0)).to(DEV, torch.bfloat16)[:, :n]
        x = torch.randn(K, k, generator=g).to(DEV, torch.bfloat16)
        alpha, acc = (0.5, True) if i == 1 else (1.0, False)
        frame = torch.full((n + 3, k + 12), SENT, device=DEV)
        out = frame[1:n + 1, 4:k + 4]
        prev = torch.randn(n, k, generator=g).to(DEV)
        if acc:
            out.copy_(prev)
        ref = alpha * (dy.float().t() @ x.float()) + (prev if acc else 0)
        p = [dy, x, out, alpha, acc]
        if i in colsum_on:
            p.append(torch.zeros(n, device=DEV))
        prods.append(tuple(p))
        frames.append(frame)
        refs.append(ref)
    return prods, frames, refs


def _check(prods, frames, refs, what):
    for (_, _, out, *_), frame, ref in zip(prods, frames, refs):
        n, k = out.shape
        err = ((out - ref).abs().max() / ref.abs().max()).item()
        print(what, (n, k), f"err/scale={err:.3e}")
        assert err <= 1e-5, (what, (n, k), err)
        around = frame.clone()
        around[1:n + 1, 4:k + 4] = SENT
        assert bool((around == SENT).all()), (what, (n, k), "wrote outside its output")


@pytest.mark.parametrize("K", EDGE_K)
def test_stage_edges(K):
    """Fewer stages than ring slots (K <= 128) and token counts around the 32-token stage and the
    64-token k-unit; nothing is written outside the outputs."""
    prods, frames, refs = _products(K, 100 + K)
    _ops().gemm_dw_grouped(prods, tile_m=TILE)
    torch.cuda.synchronize()
    _check(prods, frames, refs, f"K={K}")


@pytest.mark.parametrize("max_wg", [1, 3])
@pytest.mark.parametrize("K", [33, 97])
def test_seams_one_workgroup_walks_many_tiles(K, max_wg):
    """8 tiles on 1 or 3 workgroups: the ring holds stages of two or three tiles and products at
    once.  Every tile is still reduced in token order, so the result is bitwise the uncapped
    launch's."""
    free, frames0, refs = _products(K, 200 + K)
    capped, frames1, _ = _products(K, 200 + K)
    ops = _ops()
    ops.gemm_dw_grouped(free, tile_m=TILE)
    ops.gemm_dw_grouped(capped, tile_m=TILE, max_wg=max_wg)
    torch.cuda.synchronize()
    _check(capped, frames1, refs, f"K={K} max_wg={max_wg}")
    for f0, f1 in zip(frames0, frames1):
        assert torch.equal(f0, f1)


@pytest.mark.parametrize("K", [37, 100, 193])
@pytest.mark.parametrize("ksplit", [2, 3])
def test_token_split(ksplit, K):
    """Slices of whole 64-token k-units: empty last slices (K = 37) and ragged ones; the slabs'
    workspace is not written past its end; a rerun is bitwise equal."""
    ops = _ops()
    elems = (ksplit - 1) * sum(n * k for n, k in SHAPES)
    runs = []
    for _ in range(2):
        prods, frames, refs = _products(K, 300 + K)
        ws = torch.full((elems + 1024,), SENT, device=DEV)
        ops.gemm_dw_grouped(prods, tile_m=TILE, ksplit=ksplit, workspace=ws)
        torch.cuda.synchronize()
        _check(prods, frames, refs, f"K={K} ksplit={ksplit}")
        assert bool((ws[elems:] == SENT).all()), "wrote past the slabs"
        runs.append(frames)
    for f0, f1 in zip(*runs):
        assert torch.equal(f0, f1)


@pytest.mark.parametrize("K", [33, 161])
def test_colsum_tile_next_to_plain_tiles(K):
    """One workgroup walks a product with a column-sum output and then products without: a summing
    tile and a plain tile back to back in one ring.  dW bitwise as without the sums; the sums
    within 1e-5 of their scale."""
    ops = _ops()
    with_cs, frames1, refs = _products(K, 400 + K, colsum_on=(0,))
    plain, frames0, _ = _products(K, 400 + K, colsum_on=(0,))
    plain = [p[:5] for p in plain]
    ops.gemm_dw_grouped(with_cs, tile_m=TILE, max_wg=1)
    ops.gemm_dw_grouped(plain, tile_m=TILE, max_wg=1)
    torch.cuda.synchronize()
    _check(with_cs, frames1, refs, f"K={K} colsum")
    for f0, f1 in zip(frames0, frames1):
        assert torch.equal(f0, f1)
    dy, cs = with_cs[0][0], with_cs[0][5]
    ref = dy.float().sum(0)
    err = ((cs - ref).abs().max() / ref.abs().max()).item()
    print(f"K={K} colsum err/scale={err:.3e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("K", [97, 2048])
def test_same_summation_order_as_the_256x128_tile(K):
    """An output element is the sum of its 32-token MFMA blocks in token order in one accumulator,
    whatever the tile and the ring: tile codes 256 and 512 agree bitwise (they did with the 2-stage
    ring of 64-token stages too)."""
    ops = _ops()
    a, fa, refs = _products(K, 500 + K)
    b, fb, _ = _products(K, 500 + K)
    ops.gemm_dw_grouped(a, tile_m=256)
    ops.gemm_dw_grouped(b, tile_m=TILE)
    torch.cuda.synchronize()
    _check(b, fb, refs, f"K={K}")
    for f0, f1 in zip(fa, fb):
        assert torch.equal(f0, f1)
