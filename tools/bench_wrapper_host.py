#!/usr/bin/env python3
"""Host time of the op wrappers of codonlm_amd/ops.py: each wrapper is called 2000 times back to back at a tiny
shape (64 rows, V = 68; B = 8 for decode and sampling) without a sync in between, five times over, and the host
clock gives the median microseconds per call -- the wrapper's own Python plus the launch cost on the host, the
figure a change of the binding (not of the library) can move.  The device work is a few microseconds per call and
hides behind it.  Prints one JSON line.  Not wired into bench.py.

    python tools/bench_wrapper_host.py
"""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "genomics-lm_amd"))

import torch  # noqa: E402
from codonlm_amd import _lib as L, ops  # noqa: E402

dev, V, N = "cuda", 68, 2000
g = torch.Generator(device=dev).manual_seed(0)
z = torch.randn(64, V, device=dev, generator=g)
tg = torch.randint(1, V, (64,), device=dev, generator=g)
acc4, acc5 = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(5, dtype=torch.float64, device=dev)
ws_s = ops.score_workspace(64, dev)
x, y = torch.randint(4, V, (2, 32), device=dev, generator=g), torch.randint(4, V, (2, 32), device=dev, generator=g)
tb = ops.ngram_totals(ops.ngram_count(ops.NgramTables(V, dev, reset_ids=(3,)), x, y))
slices = torch.zeros(26, dtype=torch.float64, device=dev)
ws_d = ops.diag_workspace(2, dev)
H, KV, hd, Tmax = 4, 2, 16, 40
q, cache = torch.randn(8, H * hd, device=dev), torch.randn(8, Tmax, 2 * KV * hd, device=dev)
pos = torch.full((8,), 17, dtype=torch.int32, device=dev)
yout = torch.zeros(8, H * hd, device=dev)
sp = L.SampleParams(V=V, temperature=1.0, target_codons=L.INT_MAX, max_codons=L.INT_MAX, max_tokens=1, seed=7,
                    Tmax=L.INT_MAX)
cls = torch.zeros(V, dtype=torch.uint8, device=dev)
sp.tok_class = cls.data_ptr()
state = torch.zeros(8, 8, dtype=torch.int32, device=dev)
state[:, 4] = L.GEN_DONE  # finished rows: the launch runs and writes nothing
nxt, ids = torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(8, 4, dtype=torch.int64, device=dev)
zs = torch.randn(8, V, device=dev)
xk, ck = torch.randn(256, 16, device=dev), torch.randn(4, 16, device=dev)
calls = {
    "score_rows": lambda: ops.score_rows(z, tg, acc=acc4, want=("logp", "rank"), workspace=ws_s),
    "score_rows_own_ws": lambda: ops.score_rows(z, tg, want=("logp",)),
    "attr_seed": lambda: ops.attr_seed(z, tg),
    "ngram_nll": lambda: ops.ngram_nll(tb, x, y, acc=acc5),
    "diag_rows": lambda: ops.diag_rows(z, x, y, slices=slices, want=("row_nll",), workspace=ws_d),
    "attn_decode_ragged": lambda: ops.attn_decode_ragged(q, cache, pos, H, KV, hd, out=yout),
    "attn_decode": lambda: ops.attn_decode(q, cache, 17, H, KV, hd),
    "sample_step": lambda: ops.sample_step(sp, zs, state, nxt, ids),
    "kmeans_step": lambda: ops.kmeans_step(xk, ck),
    "layernorm_fwd": lambda: ops.layernorm_fwd(xk, ck[0], ck[1]),
}
out = {"what": "host_us_per_call"}
for name, fn in calls.items():
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(N):
            fn()
        us.append((time.perf_counter() - t0) / N * 1e6)
        torch.cuda.synchronize()
    out[name] = {"host_us": round(statistics.median(us), 3)}
print(json.dumps(out), flush=True)
