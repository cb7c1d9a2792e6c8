"""fp64 numpy restatement of cg_sample_step (include/codonlm_hip.h): the termination bias, mask,
weights, top-k, counter-based draw and the stop machine, shared by the sampler op test and the
end-to-end generation test.  Not a test module."""
import numpy as np

from oracle import tinygpt_oracle as O

INT_MAX = 2 ** 31 - 1
TOK_CODON, TOK_STOP, TOK_EOS = 1, 2, 4
DONE, TERMINAL_STOP, EARLY_STOP, EOS, TARGET, CAP, CONTEXT_FULL = 1, 2, 4, 8, 16, 32, 64

# the generation tests' vocabulary: four specials, then the 64 codons in ACGT order
ITOS = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
STOI = {t: i for i, t in enumerate(ITOS)}
STOP_IDS = sorted(STOI[c] for c in ("TAA", "TAG", "TGA"))


def vocab_classes(V=68):
    cls = np.zeros(V, dtype=np.uint8)
    cls[4:68] = TOK_CODON
    cls[STOP_IDS] |= TOK_STOP
    cls[2] |= TOK_EOS
    return cls


def default_params(V, **kw):
    p = dict(V=V, tok_class=np.zeros(V, dtype=np.uint8), allowed=None, temperature=1.0, topk=0,
             target_codons=INT_MAX, max_codons=INT_MAX, max_tokens=INT_MAX, require_terminal_stop=0,
             stop_on_eos=0, stop_on_bio_stop=0, stop_bias=0.0, trigger_class_max=0, bias_window=0,
             n_term_classes=0, seed=0, Tmax=INT_MAX)
    p.update(kw)
    return p


def new_state(pos0, stream):
    return dict(pos0=int(pos0), pos=int(pos0), n_tokens=0, n_codons=0, flags=0, bias_steps=0, last_term_class=-1,
                stream=int(stream))


def draw_u(seed, stream, n_tokens):
    with np.errstate(over="ignore"):
        k = np.uint32(0x9E3779B1)
        row = O._fmix32(np.array([np.uint32(seed & 0xFFFFFFFF) ^ (np.uint32(stream & 0xFFFFFFFF) * k)], dtype=np.uint32))
        h = O._fmix32((row + np.uint32(n_tokens) * k).astype(np.uint32))
    return float(int(h[0]) >> 8) * 2.0 ** -24


def sample_token(P, logits, term, st):
    """Steps 1-5 for one sequence (st is updated by step 1).  Returns (token, boundary, gap):
    boundary = the distance of u*total from the nearest CDF boundary as a share of total, gap =
    the logit gap across the top-k cut (inf without a cut)."""
    V = P["V"]
    l = np.asarray(logits[:V], dtype=np.float32).astype(np.float64)
    cls = P["tok_class"]
    if (term is not None and P["stop_bias"] > 0 and P["n_term_classes"] > 0
            and st["n_codons"] >= max(0, P["target_codons"] - P["bias_window"])):
        c = int(np.argmax(np.asarray(term[:P["n_term_classes"]], dtype=np.float32)))  # first maximum
        st["last_term_class"] = c
        if c <= P["trigger_class_max"]:
            l = l + np.where(cls & TOK_STOP, float(np.float32(P["stop_bias"])), 0.0)
            st["bias_steps"] += 1
    ok = np.ones(V, dtype=bool) if P["allowed"] is None else P["allowed"].astype(bool)
    temp = max(1e-6, float(np.float32(P["temperature"])))
    with np.errstate(under="ignore", over="ignore"):  # (masked tokens above the allowed maximum)
        w = np.where(ok, np.exp((l - l[ok].max()) / temp), 0.0)
    gap = np.inf
    k = min(P["topk"], V) if P["topk"] > 0 else V
    if k < V:
        order = np.lexsort((np.arange(V), -w))  # by weight descending, then index ascending
        keep = np.zeros(V, dtype=bool)
        keep[order[:k]] = True
        if ok[order[k]] and ok[order[k - 1]]:
            gap = float(l[order[k - 1]] - l[order[k]])
        w = np.where(keep, w, 0.0)
    cum = np.cumsum(w)
    total = cum[-1]
    target = draw_u(P["seed"], st["stream"], st["n_tokens"]) * total
    hit = np.nonzero((cum > target) & (w > 0))[0]
    tok = int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1])
    edges = np.concatenate(([0.0], cum[w > 0]))
    boundary = float(np.abs(edges - target).min() / total)
    return tok, boundary, gap


def advance(P, tok, st):
    """Steps 6-8 for one sequence."""
    cls = int(P["tok_class"][tok])
    st["n_tokens"] += 1
    if cls & TOK_CODON:
        st["n_codons"] += 1
    at_target = st["n_codons"] >= P["target_codons"]
    req = bool(P["require_terminal_stop"])
    f = st["flags"]
    if (cls & TOK_STOP) and P["stop_on_bio_stop"]:
        if not at_target:
            f |= EARLY_STOP
            if not req:
                f |= TERMINAL_STOP | DONE
        else:
            f |= TERMINAL_STOP | DONE
    if not f & DONE and (cls & TOK_EOS) and P["stop_on_eos"] and (at_target or not req):
        f |= EOS | DONE
    if not f & DONE and at_target and not req:
        f |= TARGET | DONE
    if not f & DONE and (st["n_codons"] >= P["max_codons"] or st["n_tokens"] >= P["max_tokens"]):
        f |= CAP | DONE
    if not f & DONE:
        st["pos"] = st["pos0"] + st["n_tokens"] - 1
        if st["pos"] >= P["Tmax"]:
            f |= CONTEXT_FULL | DONE
    if f & DONE:
        st["pos"] = -1
    st["flags"] = f


def device_params(P, dev):
    """(_lib.SampleParams, the device tensors it points to)"""
    import torch
    from codonlm_amd import _lib as L
    keep = [torch.from_numpy(np.ascontiguousarray(P["tok_class"], dtype=np.uint8)).to(dev)]
    c = L.SampleParams()
    c.V = P["V"]
    c.tok_class = keep[0].data_ptr()
    if P["allowed"] is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(P["allowed"], dtype=np.uint8)).to(dev))
        c.allowed = keep[1].data_ptr()
    for k in ("temperature", "topk", "target_codons", "max_codons", "max_tokens", "require_terminal_stop",
              "stop_on_eos", "stop_on_bio_stop", "stop_bias", "trigger_class_max", "bias_window", "n_term_classes",
              "seed", "Tmax"):
        setattr(c, k, P[k])
    return c, keep


STATE_FIELDS = ("pos0", "pos", "n_tokens", "n_codons", "flags", "bias_steps", "last_term_class", "stream")


def states_to_array(states):
    a = np.array([[s[k] for k in STATE_FIELDS] for s in states], dtype=np.int64)
    return (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(len(states), 8)


def array_to_states(a):
    out = []
    for row in np.asarray(a):
        s = {k: int(v) for k, v in zip(STATE_FIELDS, row)}
        s["stream"] &= 0xFFFFFFFF
        out.append(s)
    return out
