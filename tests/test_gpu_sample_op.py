"""cg_sample_step alone: the fused sampler against the fp64 restatement of its contract
(tests/sampler_restatement.py: termination bias, mask, weights, top-k by rank, the counter-based
draw), and scripted sequences through the stop rules.

The kernel evaluates weights and cumulative sums in fp64 from the same fp32 logits, so tokens
must be EQUAL; a draw is exempt only where u*total lies within 1e-5*total of a CDF boundary
(expected share about 2e-5 * V of the draws), and at most 1 % of a case's draws may be exempt."""
import itertools

import numpy as np
import pytest
import torch

import sampler_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from codonlm_amd import ops
    return ops


def _run_step(P, logits, states, term=None, cap=8):
    """One cg_sample_step; returns (states after, next_tok, out_ids, n_active)."""
    cp, keep = R.device_params(P, DEV)
    B = logits.shape[0]
    st = torch.from_numpy(R.states_to_array(states)).to(DEV)
    nxt = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    out = torch.full((B, cap), -7, dtype=torch.int64, device=DEV)
    na = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    _ops().sample_step(cp, torch.from_numpy(logits).to(DEV), st, nxt, out, na,
                       term_logits=None if term is None else torch.from_numpy(term).to(DEV))
    torch.cuda.synchronize()
    return R.array_to_states(st.cpu().numpy()), nxt.cpu().numpy(), out.cpu().numpy(), int(na.item())


@pytest.mark.parametrize("V,B", [(68, 3), (68, 65), (69, 3), (69, 65), (257, 3), (257, 65)])
def test_sampler_matches_fp64_restatement(V, B):
    """Logits 3*N(0,1) with a duplicated row maximum; topk in {0, 1, 5, V, V+3}, temperature in
    {1, 0.7, 1e-9}, no mask / a random mask / a single allowed token; random streams and token
    counters.  topk = 1 must give the lowest index of the duplicated maximum."""
    rng = np.random.default_rng(V * 1000 + B)
    draws = exempt = 0
    for ci, (topk, temp, mask) in enumerate(itertools.product([0, 1, 5, V, V + 3], [1.0, 0.7, 1e-9],
                                                              ["none", "random", "single"])):
        logits = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
        allowed = None
        if mask == "random":
            allowed = (rng.random(V) < 0.6).astype(np.uint8)
            allowed[rng.integers(V)] = 1
        elif mask == "single":
            allowed = np.zeros(V, dtype=np.uint8)
            allowed[rng.integers(V)] = 1
        ok = np.ones(V, bool) if allowed is None else allowed.astype(bool)
        first_max = []
        for b in range(B):  # duplicate the maximum of the allowed tokens at a second allowed index
            cand = np.nonzero(ok)[0]
            top = cand[np.argmax(logits[b, cand])]
            other = cand[rng.integers(len(cand))]
            logits[b, other] = logits[b, top]
            first_max.append(min(top, other))
        P = R.default_params(V, allowed=allowed, temperature=temp, topk=topk, seed=int(rng.integers(2 ** 32)))
        states = [R.new_state(4, int(rng.integers(2 ** 32))) for _ in range(B)]
        for s in states:
            s["n_tokens"] = int(rng.integers(6))
        got_states, nxt, out, na = _run_step(P, logits, states)
        assert na == B
        for b in range(B):
            want = dict(states[b])
            tok, boundary, _ = R.sample_token(P, logits[b], None, want)
            draws += 1
            if topk == 1:
                assert tok == first_max[b]
            if boundary <= 1e-5 and nxt[b] != tok:
                exempt += 1
                continue
            assert nxt[b] == tok, (ci, topk, temp, mask, b, int(nxt[b]), tok, boundary)
            assert ok[tok]
            assert out[b, states[b]["n_tokens"]] == tok
            assert got_states[b]["n_tokens"] == states[b]["n_tokens"] + 1
    print(f"V={V} B={B}: {draws} draws, {exempt} exempt")
    assert exempt <= 0.01 * draws, (exempt, draws)


def test_large_vocabulary_is_unsupported():
    P = R.default_params(1025)
    with pytest.raises(ValueError):
        _run_step(P, np.zeros((1, 1025), dtype=np.float32), [R.new_state(1, 0)])


# ---------------------------------------------------------------------------
# scripted sequences: a logit of +50 forces the scripted token (every other token has a share of
# e^-50 of the mass, far below the 2^-24 step of u)
# ---------------------------------------------------------------------------
V0 = 68
CLS = R.vocab_classes(V0)
TAA, EOS_ID, COD = R.STOI["TAA"], R.STOI["<EOS_CDS>"], [R.STOI[c] for c in ("AAA", "AAC", "AAG", "AAT", "ACA")]


def _play(script, term=None, pos0=5, extra_steps=0, **kw):
    """Plays one scripted sequence; returns the list of (state, next_tok, n_active) per step and the
    final out_ids row."""
    P = R.default_params(V0, tok_class=CLS, seed=11, Tmax=64, **kw)
    cp, keep = R.device_params(P, DEV)
    st = torch.from_numpy(R.states_to_array([R.new_state(pos0, 3)])).to(DEV)
    nxt = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    out = torch.full((1, 16), -7, dtype=torch.int64, device=DEV)
    na = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    trace = []
    for i in range(len(script) + extra_steps):
        lg = np.zeros((1, V0), dtype=np.float32)
        lg[0, script[min(i, len(script) - 1)]] = 50.0
        tl = None if term is None else torch.tensor([term[min(i, len(term) - 1)]], dtype=torch.float32, device=DEV)
        _ops().sample_step(cp, torch.from_numpy(lg).to(DEV), st, nxt, out, na, term_logits=tl)
        torch.cuda.synchronize()
        trace.append((R.array_to_states(st.cpu().numpy())[0], int(nxt.item()), int(na.item())))
    return trace, out.cpu().numpy()[0]


def test_early_stop_codon_without_terminal_requirement():
    tr, out = _play([COD[0], TAA], target_codons=5, stop_on_bio_stop=1, stop_on_eos=1)
    assert tr[0][0]["flags"] == 0 and tr[0][0]["pos"] == 5 and tr[0][2] == 1
    s = tr[1][0]
    assert s["flags"] == R.EARLY_STOP | R.TERMINAL_STOP | R.DONE
    assert (s["n_tokens"], s["n_codons"], s["pos"]) == (2, 2, -1) and tr[1][2] == 0
    assert list(out[:3]) == [COD[0], TAA, -7]


def test_early_stop_codon_with_terminal_requirement_continues():
    tr, _ = _play([COD[0], TAA, COD[1], COD[2], COD[3], TAA], target_codons=5, require_terminal_stop=1,
                  stop_on_bio_stop=1, stop_on_eos=1)
    assert tr[1][0]["flags"] == R.EARLY_STOP and tr[1][0]["pos"] == 6 and tr[1][2] == 1
    assert tr[4][0]["flags"] == R.EARLY_STOP  # the target alone does not end a sequence that needs a stop
    s = tr[5][0]
    assert s["flags"] == R.EARLY_STOP | R.TERMINAL_STOP | R.DONE and s["n_codons"] == 6 and s["pos"] == -1


def test_stop_codon_ignored_without_the_flag():
    tr, _ = _play([TAA, COD[0]], target_codons=5, require_terminal_stop=1, stop_on_bio_stop=0)
    assert tr[1][0]["flags"] == 0 and tr[1][0]["n_codons"] == 2


def test_eos_before_and_after_target():
    tr, _ = _play([COD[0], EOS_ID, COD[1]], target_codons=3, require_terminal_stop=1, stop_on_eos=1,
                  stop_on_bio_stop=1)
    assert [t[0]["flags"] for t in tr] == [0, 0, 0] and tr[2][0]["n_codons"] == 2 and tr[2][0]["n_tokens"] == 3
    tr, _ = _play([COD[0], EOS_ID], target_codons=3, require_terminal_stop=0, stop_on_eos=1)
    assert tr[1][0]["flags"] == R.EOS | R.DONE
    tr, _ = _play([COD[0], COD[1], EOS_ID], target_codons=2, require_terminal_stop=1, stop_on_eos=1)
    assert tr[1][0]["flags"] == 0 and tr[2][0]["flags"] == R.EOS | R.DONE
    tr, _ = _play([COD[0], EOS_ID], target_codons=3, require_terminal_stop=0, stop_on_eos=0)
    assert tr[1][0]["flags"] == 0


def test_target_reached():
    tr, _ = _play([COD[0], COD[1], COD[2]], target_codons=3, stop_on_bio_stop=1, stop_on_eos=1)
    assert tr[1][0]["flags"] == 0 and tr[2][0]["flags"] == R.TARGET | R.DONE and tr[2][0]["pos"] == -1


def test_codon_cap():
    tr, _ = _play([COD[0], COD[1], COD[2], COD[3]], target_codons=2, require_terminal_stop=1, max_codons=4,
                  max_tokens=12)
    assert tr[2][0]["flags"] == 0 and tr[3][0]["flags"] == R.CAP | R.DONE


def test_token_cap_through_non_codon_tokens():
    tr, _ = _play([0, 0, 0], target_codons=2, require_terminal_stop=1, max_codons=5, max_tokens=3)
    assert tr[1][0]["flags"] == 0
    assert tr[2][0]["flags"] == R.CAP | R.DONE and tr[2][0]["n_codons"] == 0 and tr[2][0]["n_tokens"] == 3


def test_termination_bias_window_and_trigger():
    """target 4, window 2: the bias can act from n_codons = 2 on.  A bias of +100 on the three stop
    codons overrides the scripted +50, so a biased step draws a stop codon."""
    kw = dict(target_codons=4, require_terminal_stop=1, stop_on_bio_stop=1, stop_bias=100.0, bias_window=2,
              n_term_classes=5)
    term = [[0, 2, 1, 0, 0]]  # class 1
    tr, _ = _play([COD[0], COD[1], COD[2]], term=term, trigger_class_max=1, **kw)
    assert [t[1] for t in tr[:2]] == [COD[0], COD[1]]
    assert tr[1][0]["last_term_class"] == -1 and tr[1][0]["bias_steps"] == 0  # below the window edge
    assert tr[2][1] in R.STOP_IDS and tr[2][0]["bias_steps"] == 1 and tr[2][0]["last_term_class"] == 1
    assert tr[2][0]["flags"] == R.EARLY_STOP  # 3 codons < target, a stop is required: goes on
    tr, _ = _play([COD[0], COD[1], COD[2]], term=term, trigger_class_max=0, **kw)
    assert tr[2][1] == COD[2] and tr[2][0]["bias_steps"] == 0 and tr[2][0]["last_term_class"] == 1
    tr, _ = _play([COD[0], COD[1], COD[2]], term=[[3, 3, 0, 0, 0]], trigger_class_max=0, **kw)
    assert tr[2][1] in R.STOP_IDS and tr[2][0]["last_term_class"] == 0  # the lowest index of a tie
    off = dict(kw, stop_bias=0.0)
    tr, _ = _play([COD[0], COD[1], COD[2]], term=term, trigger_class_max=1, **off)
    assert tr[2][1] == COD[2] and tr[2][0]["bias_steps"] == 0 and tr[2][0]["last_term_class"] == -1
    tr, _ = _play([COD[0], COD[1], COD[2]], term=None, trigger_class_max=1, **kw)
    assert tr[2][1] == COD[2] and tr[2][0]["last_term_class"] == -1


def test_context_full():
    P = dict(target_codons=40, require_terminal_stop=1)
    tr, _ = _play([COD[0], COD[1], COD[2]], pos0=5, **P)  # Tmax 64: far away
    assert [t[0]["pos"] for t in tr] == [5, 6, 7]
    Pd = R.default_params(V0, tok_class=CLS, seed=11, Tmax=7, **P)
    states = [R.new_state(5, 3)]
    for i, want in enumerate([(5, 0), (6, 0), (-1, R.CONTEXT_FULL | R.DONE)]):
        lg = np.zeros((1, V0), dtype=np.float32)
        lg[0, COD[i]] = 50.0
        states, _, _, na = _run_step(Pd, lg, states)
        assert (states[0]["pos"], states[0]["flags"]) == want
    assert na == 0


def test_done_rows_stay_untouched_and_active_count():
    """Four sequences, two of them done: their state, next_tok and out_ids rows keep every byte,
    n_active counts the others."""
    P = R.default_params(V0, tok_class=CLS, seed=5, Tmax=64, target_codons=2, stop_on_bio_stop=1)
    states = [R.new_state(3, b) for b in range(4)]
    states[1].update(flags=R.TARGET | R.DONE, pos=-1, n_tokens=2, n_codons=2)
    states[3].update(flags=R.CAP | R.DONE, pos=-1, n_tokens=5, n_codons=1, bias_steps=2, last_term_class=4)
    lg = np.zeros((4, V0), dtype=np.float32)
    lg[:, COD[0]] = 50.0
    after, nxt, out, na = _run_step(P, lg, states)
    assert na == 2
    for b in (1, 3):
        assert after[b] == states[b] and nxt[b] == -7 and np.all(out[b] == -7)
    for b in (0, 2):
        assert after[b]["n_tokens"] == 1 and nxt[b] == COD[0] and out[b, 0] == COD[0] and after[b]["pos"] == 3
    lg[:, COD[0]] = 0.0
    lg[:, COD[1]] = 50.0
    after2, nxt2, _, na2 = _run_step(P, lg, after)
    assert na2 == 0 and all(s["flags"] & R.DONE for s in after2)
    assert after2[1] == states[1] and after2[3] == states[3]
    after3, nxt3, out3, na3 = _run_step(P, lg, after2)
    assert na3 == 0 and after3 == after2 and np.all(nxt3 == -7) and np.all(out3 == -7)
