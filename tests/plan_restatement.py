"""fp64 numpy restatement of cg_sample_step_plan (include/codonlm_hip.h): the per-step set choice,
the two log-probabilities and the plan-end stop rule, on top of sampler_restatement's
sample_token / advance.  Shared by the plan sampler op test and the end-to-end recoding test.  Not a
test module."""
import numpy as np

import sampler_restatement as R

PLAN_END = 128


def new_plan(sets=None, plan=None, plan_len=None, end_with_plan=0):
    """sets uint8 [n_sets][>= V] or None, plan int [B][ld_plan], plan_len int [B]"""
    sets = np.zeros((0, 0), dtype=np.uint8) if sets is None else np.asarray(sets, dtype=np.uint8)
    return dict(sets=sets, n_sets=sets.shape[0], plan=None if plan is None else np.asarray(plan, dtype=np.int64),
                plan_len=None if plan_len is None else np.asarray(plan_len, dtype=np.int64),
                end_with_plan=int(end_with_plan))


def step_allowed(P, PL, b, st):
    """The mask step 2 uses for sequence b: its plan's set for generated token n_tokens when that set
    exists and allows a token < V, else P["allowed"]."""
    j = st["n_tokens"]
    plen = int(PL["plan_len"][b]) if PL["plan_len"] is not None else 0
    if PL["n_sets"] > 0 and 0 <= j < plen and j < PL["plan"].shape[1]:
        s = int(PL["plan"][b, j])
        if 0 <= s < PL["n_sets"]:
            row = PL["sets"][s, :P["V"]]
            if row.any():
                return (row != 0).astype(np.uint8)
    return P["allowed"]


def _draw_weights(P, allowed, l, biased):
    """Steps 2-4 on fp64 logits l: the kept weights and their total."""
    V = P["V"]
    if biased:
        l = l + np.where(P["tok_class"] & R.TOK_STOP, float(np.float32(P["stop_bias"])), 0.0)
    ok = np.ones(V, dtype=bool) if allowed is None else allowed.astype(bool)
    temp = max(1e-6, float(np.float32(P["temperature"])))
    with np.errstate(under="ignore", over="ignore"):
        w = np.where(ok, np.exp((l - l[ok].max()) / temp), 0.0)
    k = min(P["topk"], V) if P["topk"] > 0 else V
    if k < V:
        order = np.lexsort((np.arange(V), -w))
        keep = np.zeros(V, dtype=bool)
        keep[order[:k]] = True
        w = np.where(keep, w, 0.0)
    return w, w.sum()


def sample_token_plan(P, PL, b, logits, term, st):
    """Steps 1-5 for sequence b under its plan (st is updated by step 1).  Returns (token, boundary,
    gap, logp_model, logp_draw): the first three as sampler_restatement.sample_token, then
    l_tok - logsumexp over the V raw logits and log(w_tok / total) under the distribution drawn from."""
    V = P["V"]
    allowed = step_allowed(P, PL, b, st)
    steps_before = st["bias_steps"]
    tok, boundary, gap = R.sample_token(dict(P, allowed=allowed), logits, term, st)
    l = np.asarray(logits[:V], dtype=np.float32).astype(np.float64)
    m = l.max()
    lp_model = l[tok] - (m + np.log(np.exp(l - m).sum()))
    w, total = _draw_weights(P, allowed, l, st["bias_steps"] != steps_before)
    with np.errstate(divide="ignore"):
        lp_draw = np.log(w[tok] / total)
    return tok, boundary, gap, float(lp_model), float(lp_draw)


def advance_plan(P, PL, b, tok, st):
    """Steps 6-8 with the plan-end rule after step 7's last rule."""
    R.advance(dict(P, Tmax=R.INT_MAX), tok, st)  # steps 6-7; step 8 follows the plan rule
    if st["flags"] & R.DONE:
        return
    plen = int(PL["plan_len"][b]) if PL["plan_len"] is not None else 0
    if PL["end_with_plan"] and plen > 0 and st["n_tokens"] >= plen:
        st["flags"] |= PLAN_END | R.DONE
    elif st["pos"] >= P["Tmax"]:
        st["flags"] |= R.CONTEXT_FULL | R.DONE
    if st["flags"] & R.DONE:
        st["pos"] = -1


def device_plan(PL, dev, logp=None, tok_logp=None):
    """(_lib.SamplePlan, the device tensors it points to); logp fp64 [B][2] / tok_logp fp32 [B][n]
    device tensors (row-contiguous views are fine) or None."""
    import torch
    from codonlm_amd import _lib as L
    keep = []
    c = L.SamplePlan()
    c.n_sets = PL["n_sets"]
    if PL["n_sets"] > 0:
        keep.append(torch.from_numpy(np.ascontiguousarray(PL["sets"])).to(dev))
        c.sets, c.ld_sets = keep[-1].data_ptr(), keep[-1].stride(0)
    if PL["plan"] is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(PL["plan"], dtype=np.int32)).to(dev))
        c.plan, c.ld_plan = keep[-1].data_ptr(), keep[-1].stride(0)
    if PL["plan_len"] is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(PL["plan_len"], dtype=np.int32)).to(dev))
        c.plan_len = keep[-1].data_ptr()
    c.end_with_plan = PL["end_with_plan"]
    if logp is not None:
        c.logp = logp.data_ptr()
    if tok_logp is not None:
        c.tok_logp, c.ld_tok_logp = tok_logp.data_ptr(), tok_logp.stride(0)
    return c, keep
