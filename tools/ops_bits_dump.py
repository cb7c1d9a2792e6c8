"""Run the op wrappers of codonlm_amd/ops.py once on seeded inputs, at the smallest shapes that reach
each path of the shared csrc/common.h helpers (wave reductions, vector loaders, id mask, capped grid)
and each branch of the wrappers' own helpers (output tables, workspace policies, row-matrix and
per-row checks, the decode / sample / LayerNorm twins), and save every output to a .npz.  Two library
builds, or two versions of the Python binding over one library, can then be compared bit for bit:
    CG_LIB_PATH=<lib> python tools/ops_bits_dump.py out.npz"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "genomics-lm_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from codonlm_amd import _lib as L, ops  # noqa: E402

g = torch.Generator().manual_seed(0)
out = {}


def randn(*shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to("cuda", dtype)


def randint(lo, hi, shape, dtype=torch.int64):
    return torch.randint(lo, hi, shape, generator=g).to("cuda", dtype)


def put(name, t):
    if t is not None:
        t = t.detach()
        out[name] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


def put_all(prefix, res, names):
    for n in names:
        put(f"{prefix}.{n}", getattr(res, n))


f64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731

for V in (68, 300):  # score_rows: 2 and 8 column chunks per lane
    z, tg = randn(2 * 67, V, scale=3.0), randint(0, V, (2 * 67,))
    tg[::7], tg[5], tg[9] = 0, V + 5, -3  # ignored and out-of-range targets
    r = ops.score_rows(z, tg, smoothing=0.05, sel=randint(0, V, (5,), torch.int32), T=67, acc=f64(4),
                       want=ops.SCORE_OUTPUTS)
    put_all(f"score{V}", r, ops.SCORE_OUTPUTS + ("acc",))

B, T, V = 3, 300, 68  # diag_rows: two 256-position chunks with a tail
x, y = randint(4, V, (B, T)), randint(4, V, (B, T))
x[:, 40], x[1, 270], y[:, 290:], y[0, 3] = 3, 3, 0, 0
r = ops.diag_rows(randn(B * T, V, scale=3.0), x, y, row_flag=randint(0, 2, (B,), torch.uint8),
                  tok_class=randint(0, 5, (V,), torch.uint8), edges=torch.linspace(0, 1, 16).cuda(),
                  slices=f64(2 * len(L.DIAG_SLICES)), calib=f64(45), brier_acc=f64(2), want=ops.DIAG_OUTPUTS)
put_all("diag", r, ops.DIAG_OUTPUTS + ("slices", "calib", "brier_acc"))

x, y = randint(1, V, (5, 131)), randint(0, V, (5, 131))  # n-gram tables and baselines
tb = ops.ngram_totals(ops.ngram_count(ops.NgramTables(V, "cuda", reset_ids=(3,)), x, y))
put_all("ngram", tb, ("uni", "bi", "tri", "n_bad", "uni_total", "bi_total", "tri_total"))
put_all("ngram_nll", ops.ngram_nll(tb, x, y, acc=f64(5), want=ops.NGRAM_OUTPUTS), ops.NGRAM_OUTPUTS + ("acc",))

z, tg, w = randn(131, V, scale=3.0), randint(-2, V + 2, (131,)), randn(131)  # attr_seed / attr_reduce
w[::5] = 0
for mode in ("logprob", "logit"):
    put(f"attr_seed.f32.{mode}", ops.attr_seed(z, tg, w, mode=mode))
    put(f"attr_seed.split.{mode}", ops.attr_seed(z, tg, w, mode=mode, pad_to=192, split=True))
for d in (384, 50):  # 16-byte loads, and the element tail
    put_all(f"attr_reduce{d}", ops.attr_reduce(randn(131, d), tg, randn(V, d), randn(131, d)), ops.ATTR_OUTPUTS)

for d in (48, 50):  # kmeans_step
    r = ops.kmeans_step(randn(1000, d), randn(10, d))
    put_all(f"kmeans{d}", r, ("labels", "dist2", "sums", "counts", "inertia"))

idx = randint(0, V, (2, 64))  # window_keep / window_pool / pool_hidden
keep = ops.window_keep(idx, 9, 3, exclude_ids=(3, 7))
put("window_keep", keep)
dst = torch.arange(keep.numel(), dtype=torch.int32, device="cuda").view_as(keep).contiguous()
for dt in (torch.float32, torch.bfloat16):
    h = randn(2, 64, 48, dtype=dt)
    put(f"window_pool.{dt}", ops.window_pool(h, 9, 3, dst, torch.zeros(keep.numel(), 48, device="cuda")))
    put(f"pool_hidden.{dt}", ops.pool_hidden(h, idx, "mean_content", content_ids=range(4, 40)))

lab = randint(0, 5, (200,))  # term_ce: 16-byte bf16 rows, and fp32 rows with an element tail
lab[::3] = -100
for d, dt in ((384, torch.bfloat16), (50, torch.float32)):
    st = ops.term_ce_fwd(randn(200, d, dtype=dt), randn(5, d), randn(5), lab, class_w=randn(5).abs() + 0.5)
    for n, t in zip(("loss", "sums", "dW", "db", "dx"), (st.loss, st.sums) + ops.term_ce_bwd(st, scale=0.7)):
        put(f"term_ce{d}.{n}", t)

put("gram", ops.gram_accum(randn(300, 64), randn(300, 14), randint(-1, 5, (300,), torch.int32), 5))

z, tg, w = randn(131, V, scale=3.0), randint(0, V, (131,)), randn(V).abs() + 0.5  # cross_entropy
for name, kw in (("f32", {}), ("split", dict(pad_to=192, split=True))):
    loss, dl = ops.cross_entropy(z, tg, eps=0.05, weight=w, ignore_index=0, **kw)
    put(f"ce.{name}.loss", loss)
    put(f"ce.{name}.dl", dl)

for dt in (torch.bfloat16, torch.float32):  # swiglu: the 8-element vector kernels (Hp = 176, H = 170)
    gu, ds = randn(37, 352, dtype=dt), randn(37, 176, dtype=dt)
    put(f"swiglu_fwd.{dt}", ops.swiglu_fwd(gu, 170))
    put(f"swiglu_bwd.{dt}", ops.swiglu_bwd(gu, ds, 170))

x = randn(70, 96)  # LayerNorm forward and its dropout-mask twin
for name, r in (("ln", ops.layernorm_fwd(x, randn(96), randn(96))),
                ("ln_mask", ops.layernorm_fwd_mask(x, randn(96), randn(96), 2, 35, 4, 11, 0.1))):
    for n, t in zip(("y", "mean", "rstd", "mask"), r):
        put(f"{name}.{n}", t)

a, b = randn(70, 64, dtype=torch.bfloat16), randn(48, 64, dtype=torch.bfloat16)  # gemm workspaces, colsum
cs = torch.empty(48, device="cuda")
put("gemm.split_k", ops.gemm(randn(70, 64), randn(48, 64), split_k=2))
put("gemm.colsum_out.c", ops.gemm(a, b, colsum_out=cs))
put("gemm.colsum_out.s", cs)
put("colsum", ops.colsum(randn(300, 50)))

H, KV, hd, Tmax = 4, 2, 16, 40  # one-token attention: a shared position, and one per sequence
q, cache = randn(3, H * hd), randn(3, Tmax, 2 * KV * hd + 8)
seg = torch.tensor([0, 5, 17], dtype=torch.int32, device="cuda")
put("attn_decode", ops.attn_decode(q, cache, 17, H, KV, hd, segstate=seg, window=9))
pos = torch.tensor([39, -1, 17], dtype=torch.int32, device="cuda")
put("attn_decode_ragged", ops.attn_decode_ragged(q, cache, pos, H, KV, hd, segstate=seg))

B, T = 2, 70  # attn_stats: every output and both accumulators
idx = randint(4, V, (B, T))
idx[:, 30], idx[1, 60:] = 3, 0
r = ops.attn_stats(randn(B * T, (H + 2 * KV) * hd), ops.segment_starts(idx, 3), B, T, H, KV, hd, window=50, idx=idx,
                   pad_id=0, tok_class=randint(0, 4, (V,), torch.uint8), row_keep=randint(0, 2, (B, T), torch.uint8),
                   head_acc=f64(H * L.AS_NSTAT), n_rows=f64(1))
put_all("attn_stats", r, ops.ATTN_STATS_OUTPUTS + ("head_acc", "n_rows"))

sp = L.SampleParams(V=V, temperature=0.8, topk=5, target_codons=L.INT_MAX, max_codons=L.INT_MAX,  # sample_step twins
                    max_tokens=L.INT_MAX, seed=7, Tmax=L.INT_MAX)
tok_class = torch.zeros(V, dtype=torch.uint8, device="cuda")
sp.tok_class = tok_class.data_ptr()
z, logp = randn(5, V, scale=3.0), f64(10)
for name, step in (("sample_step", lambda *a: ops.sample_step(sp, *a)),  # no sets: the same draw, and its log-probs
                   ("sample_step_plan", lambda *a: ops.sample_step_plan(sp, L.SamplePlan(logp=logp.data_ptr()), *a))):
    state = torch.zeros(5, 8, dtype=torch.int32, device="cuda")  # cg_gen_state rows: pos0 = pos = 4, stream = row
    state[:, 0], state[:, 1], state[:, 6], state[:, 7] = 4, 4, -1, torch.arange(5, dtype=torch.int32, device="cuda")
    nxt, ids = torch.full((5,), -7, device="cuda"), torch.full((5, 8), -7, device="cuda")
    n_active = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    step(z, state, nxt, ids, n_active)
    for n, t in (("state", state), ("next_tok", nxt), ("out_ids", ids), ("n_active", n_active)):
        put(f"{name}.{n}", t)
put("sample_step_plan.logp", logp)

sym = randint(0, 4, (600,), torch.uint8)  # window index and coverage: hit is zero-filled, the counts are not
index = ops.ngram_index_build(ops.NgramIndex(sym[:400], [0, 150, 150, 400], 6))
put_all("ngram_index", index, ("n_unique", "n_dropped"))  # the table's slot order is the insertion race's
qsym = torch.cat([sym[100:180], sym[400:]])
put_all("ngram_coverage", ops.ngram_coverage(index, qsym, [0, 80, 83, 280], want=ops.COVERAGE_OUTPUTS),
        ops.COVERAGE_OUTPUTS)

torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print("saved", sys.argv[1], len(out), "arrays")
