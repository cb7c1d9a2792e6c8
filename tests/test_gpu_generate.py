"""Batched on-device generation end to end (codonlm_amd.generate) in fp32, verified by teacher
forcing: one full forward of every finished sequence gives the logits at each of its positions,
and the fp64 restatement of the sampler and the stop machine (tests/sampler_restatement.py)
replays the run on them.  Every token and every info field must match.

A draw is exempt only where the model's own fp32 error could move it: u*total within
(4 delta / temperature) * total of a CDF boundary, or a top-k cut whose logit gap is below
4 delta, with delta = max(1e-4, 5e-6 |logit|max) the fp32 bound of tests/test_gpu_model.py (a logit
error delta moves normalised cumulative mass by at most 2 delta / temperature; the margin is twice
that).  At most 12 % of a run's draws may be exempt."""
import functools

import numpy as np
import pytest
import torch

import sampler_restatement as R
from conftest import load_golden
from test_gpu_model import DEV, make_model

pytestmark = pytest.mark.gpu
SEED = 77
CONTEXTS = [[1] + list(range(10 + b, 10 + 2 * b)) for b in range(6)]
TARGET, HARD_CAP, RAW_NEW = 10, 19, 58
BIAS = dict(termination_bias_enabled=True, termination_stop_bias=3.0, termination_trigger_class_max=2,
            termination_bias_window=4)


@functools.lru_cache(maxsize=None)
def _model(case):
    cfgd, g = load_golden(case)
    m, cfg, params = make_model(cfgd, g)
    # the synthetic tied embedding gives |logit| ~ 55: no stop codon would ever be drawn
    m.load_state_dict({"tok_emb.weight": torch.from_numpy(params["tok_emb.weight"]) * 0.25}, strict=False)
    m.eval()
    return m


def _gen():
    from codonlm_amd import generate
    return generate


def _forward(m, ids, want_term):
    x = torch.tensor([ids], dtype=torch.long, device=DEV)
    with torch.no_grad():
        if want_term:
            logits, _, aux = m(x, return_aux=True)
            return logits[0].cpu().numpy(), aux["termination_logits"][0].float().cpu().numpy()
        logits, _ = m(x)
    return logits[0].cpu().numpy(), None


def _params(mode, temperature, topk, seed, bias=None):
    cls = R.vocab_classes(68)
    if mode == "raw":
        return R.default_params(68, tok_class=cls, temperature=temperature, topk=topk, seed=seed, Tmax=64,
                                max_tokens=RAW_NEW, stop_on_eos=1, stop_on_bio_stop=1)
    P = R.default_params(68, tok_class=cls, allowed=(cls & R.TOK_CODON).astype(np.uint8), temperature=temperature,
                         topk=topk, seed=seed, Tmax=64, target_codons=TARGET, max_codons=HARD_CAP,
                         max_tokens=3 * HARD_CAP, require_terminal_stop=int(mode == "constrained_req"),
                         stop_on_eos=1, stop_on_bio_stop=1)
    if bias:
        P.update(stop_bias=bias["termination_stop_bias"], trigger_class_max=bias["termination_trigger_class_max"],
                 bias_window=bias["termination_bias_window"], n_term_classes=5)
    return P


def _replay(m, P, ctx, ids, stream, want_term):
    """Teacher-forced replay of one finished sequence; returns (final restated state, exempt draw
    indices, number of draws).  Asserts every non-exempt token."""
    logits, term = _forward(m, ids, want_term)
    delta = max(1e-4, 5e-6 * float(np.abs(logits).max()))
    temp = max(1e-6, float(np.float32(P["temperature"])))
    st = R.new_state(len(ctx), stream)
    exempt = []
    n = len(ids) - len(ctx)
    for i in range(n):
        assert not st["flags"] & R.DONE, "tokens after the sequence was done"
        row = len(ctx) + i - 1
        tok, boundary, gap = R.sample_token(P, logits[row], None if term is None else term[row], st)
        if boundary <= 4 * delta / temp or gap < 4 * delta:
            exempt.append(i)
        else:
            assert ids[len(ctx) + i] == tok, (stream, i, ids[len(ctx) + i], tok, boundary, gap)
        R.advance(P, ids[len(ctx) + i], st)
    assert st["flags"] & R.DONE, "the sequence ended before a stop rule fired"
    return st, exempt, n


def _expected_info(mode, st, bias):
    f = st["flags"]
    if mode == "raw":
        reason = "biological_stop" if f & R.TERMINAL_STOP else "eos" if f & R.EOS else "max_new_tokens"
        return {"protocol": "raw_model", "cds_only": False, "require_terminal_stop": False, "guidance_components": [],
                "had_terminal_stop": bool(f & R.TERMINAL_STOP), "early_stop": False,
                "hit_hard_cap": reason == "max_new_tokens", "generated_codons": st["n_codons"],
                "generated_tokens": st["n_tokens"], "max_new_tokens": RAW_NEW, "stop_reason": reason}
    req = mode == "constrained_req"
    comps = (["termination_bias"] if bias else []) + (["forced_terminal_stop"] if req else [])
    return {"protocol": "guided" if comps else "cds_constrained", "guidance_components": comps,
            "had_terminal_stop": bool(f & R.TERMINAL_STOP), "early_stop": bool(f & R.EARLY_STOP),
            "hit_hard_cap": st["n_codons"] >= HARD_CAP, "target_codons": TARGET, "generated_codons": st["n_codons"],
            "termination_bias_enabled": bool(bias), "termination_bias_steps": st["bias_steps"],
            "termination_bias_window": bias["termination_bias_window"] if bias else 0,
            "last_termination_class": st["last_term_class"] if st["last_term_class"] >= 0 else None,
            "cds_only": True, "require_terminal_stop": req, "generated_tokens": st["n_tokens"]}


def _run(m, mode, temperature, topk, bias=None, poll_every=16, contexts=CONTEXTS, streams=None, seed=SEED):
    """The batch through the drop-in functions' shared path: [(ids, info)]."""
    G = _gen()
    if mode == "raw":
        res = G.generate_batch(m, contexts, R.STOI, R.ITOS, seed=seed, streams=streams, poll_every=poll_every,
                               max_tokens=RAW_NEW, temperature=temperature, topk=topk)
        return [(ids, G.raw_info(rec, RAW_NEW)) for ids, rec in res]
    kw = dict(termination_bias_enabled=False, termination_stop_bias=0.0, termination_trigger_class_max=0,
              termination_bias_window=0)
    kw.update(bias or {})
    return G._constrained_batch(m, contexts, R.STOI, R.ITOS, TARGET, HARD_CAP,
                                require_terminal_stop=mode == "constrained_req", temperature=temperature, topk=topk,
                                cds_only=True, seed=seed, streams=streams or list(range(len(contexts))),
                                poll_every=poll_every, **kw)


def _verify(m, mode, temperature, topk, bias=None):
    res = _run(m, mode, temperature, topk, bias)
    P = _params(mode, temperature, topk, SEED, bias)
    draws = n_exempt = 0
    exempt_at = []
    for b, (ids, info) in enumerate(res):
        assert ids[:len(CONTEXTS[b])] == CONTEXTS[b]
        st, exempt, n = _replay(m, P, CONTEXTS[b], ids, b, bool(bias))
        assert info == _expected_info(mode, st, bias), (b, info, st)
        draws += n
        n_exempt += len(exempt)
        exempt_at.append(exempt[0] if exempt else None)
    print(f"[{mode} T={temperature} k={topk} bias={bool(bias)}] {draws} draws, {n_exempt} exempt "
          f"({100.0 * n_exempt / draws:.1f} %), codons {[i['generated_codons'] for _, i in res]}")
    assert n_exempt <= 0.12 * draws, (n_exempt, draws)
    return res, exempt_at


@pytest.mark.parametrize("temperature,topk", [(1.0, 0), (0.8, 5), (1.5, 0)])
@pytest.mark.parametrize("mode", ["constrained", "constrained_req", "raw"])
def test_generation_replays_under_teacher_forcing(mode, temperature, topk):
    _verify(_model("mha_gelu_sep"), mode, temperature, topk)


@pytest.mark.parametrize("temperature,topk", [(1.0, 0), (0.8, 5), (1.5, 0)])
def test_guided_generation_with_termination_bias(temperature, topk):
    res, _ = _verify(_model("aux_heads"), "constrained_req", temperature, topk, bias=BIAS)
    assert all(i["protocol"] == "guided" and i["last_termination_class"] is not None for _, i in res)


def test_same_seed_and_any_poll_interval_give_the_same_output():
    m = _model("mha_gelu_sep")
    a = _run(m, "constrained_req", 0.8, 5, poll_every=16)
    assert _run(m, "constrained_req", 0.8, 5, poll_every=16) == a
    assert _run(m, "constrained_req", 0.8, 5, poll_every=1) == a
    assert _run(m, "constrained_req", 0.8, 5, poll_every=16, seed=SEED + 1) != a


def test_a_sequence_alone_equals_its_stream_in_the_batch():
    m = _model("mha_gelu_sep")
    res, exempt_at = _verify(m, "constrained_req", 1.0, 0)
    for b in (0, 3, 5):
        (ids, info), = _run(m, "constrained_req", 1.0, 0, contexts=[CONTEXTS[b]], streams=[b])
        n = len(CONTEXTS[b]) + (exempt_at[b] if exempt_at[b] is not None else 10 ** 6)
        assert ids[:n] == res[b][0][:n], b
        if exempt_at[b] is None:
            assert info == res[b][1]


def test_drop_in_functions_and_red_sampler():
    """generate_cds_constrained / generate_model_raw are the batch's rows for the same stream, and
    batch_red_sampler equals the reference's sequential loop run with the same seeds and streams."""
    G = _gen()
    m = _model("mha_gelu_sep")
    dev = torch.device(DEV)
    ids, info = G.generate_model_raw(m, dev, CONTEXTS[2], R.STOI, R.ITOS, RAW_NEW, temperature=0.8, topk=5, seed=SEED,
                                     stream=2)
    assert info["protocol"] == "raw_model" and info["generated_tokens"] == len(ids) - len(CONTEXTS[2])
    kw = dict(temperature=1.0, topk=0, cds_only=True)
    budget = 60
    solved, remaining, total = G.batch_red_sampler(m, dev, CONTEXTS, R.STOI, R.ITOS, TARGET, HARD_CAP, budget,
                                                   seed=SEED, **kw)
    # the reference's loop (generate.py:362-397), one prefix at a time
    active, want, spent, rnd = list(range(len(CONTEXTS))), {}, 0, 0
    while active and spent < budget:
        rnd += 1
        nxt = []
        for i in active:
            if spent >= budget:
                nxt.append(i)
                continue
            ids, info = G.generate_cds_constrained(m, dev, CONTEXTS[i], R.STOI, R.ITOS, TARGET, HARD_CAP,
                                                   require_terminal_stop=True, seed=G.round_seed(SEED, rnd), stream=i,
                                                   **kw)
            spent += info["generated_codons"]
            if info["had_terminal_stop"]:
                info["round"] = rnd
                want[i] = (ids, info)
            else:
                nxt.append(i)
        active = nxt
    assert (solved, remaining, total) == (want, active, spent)
    assert total >= budget or not remaining
    ids, info = G.generate_cds_red(m, dev, CONTEXTS[1], R.STOI, R.ITOS, TARGET, HARD_CAP, max_attempts=3, seed=SEED,
                                   stream=1, **kw)
    assert 1 <= info["attempts"] <= 3 and info["total_tokens_red"] >= info["generated_codons"]
    assert info["had_terminal_stop"] or info["attempts"] == 3
