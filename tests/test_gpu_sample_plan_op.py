"""cg_sample_step_plan alone: the sampler with a token set per step of every sequence against the
fp64 restatement of its contract (tests/plan_restatement.py), on random logits.

The kernel evaluates weights, cumulative sums and the log-probabilities in fp64 from the same fp32
logits, so tokens and states must be EQUAL (a draw within the restatement's own fp64 rounding,
about 1e-15 of the mass, of a CDF boundary would be the only way to differ; none of the seeded
cases below has one).  The fp64 logp sums differ from the restatement in summation order and exp /
log rounding only: relative 1e-12 plus 1e-12 * max(1, |z|max) absolute, the bound
tests/test_gpu_score_op.py holds fp64 sums to.  tok_logp is the single fp32 rounding of the fp64
value: within 1 fp32 ulp.  Every output sits between sentinel rows that must come back untouched."""
import itertools

import numpy as np
import pytest
import torch

import plan_restatement as PR
import sampler_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7


def _ops():
    from codonlm_amd import ops
    return ops


class Guarded:
    """A [rows][cols] device tensor between two sentinel rows."""

    def __init__(self, init, dtype):
        init = np.asarray(init)
        self.full = torch.full((init.shape[0] + 2,) + init.shape[1:], SENT, dtype=dtype, device=DEV)
        self.view = self.full[1:-1]
        self.view.copy_(torch.from_numpy(init).to(dtype))

    def read(self):
        full = self.full.cpu().numpy()
        assert np.all(full[0] == SENT) and np.all(full[-1] == SENT), "sentinel row overwritten"
        return full[1:-1]


def run_plan(P, PL, logits, states, term=None, cap=12, logp0=None, tok_cap=12, want_logp=True, want_tok=True,
             plan_struct=True):
    """One cg_sample_step_plan.  Returns dict(states, next_tok, out_ids, n_active, logp, tok_logp)."""
    cp, keep = R.device_params(P, DEV)
    B = logits.shape[0]
    st = Guarded(R.states_to_array(states), torch.int32)
    nxt = Guarded(np.full((B,), SENT), torch.int64)
    out = Guarded(np.full((B, cap), SENT), torch.int64)
    lp = Guarded(np.zeros((B, 2)) if logp0 is None else logp0, torch.float64)
    tl = Guarded(np.full((B, tok_cap), SENT), torch.float32)
    na = torch.full((3,), SENT, dtype=torch.int32, device=DEV)
    pl, keep2 = PR.device_plan(PL, DEV, logp=lp.view if want_logp else None, tok_logp=tl.view if want_tok else None)
    _ops().sample_step_plan(cp, pl if plan_struct else None, torch.from_numpy(logits).to(DEV), st.view, nxt.view,
                            out.view, na[1:2], term_logits=None if term is None else torch.from_numpy(term).to(DEV))
    torch.cuda.synchronize()
    na = na.cpu().numpy()
    assert na[0] == SENT and na[2] == SENT
    return dict(states=R.array_to_states(st.read()), next_tok=nxt.read(), out_ids=out.read(), n_active=int(na[1]),
                logp=lp.read(), tok_logp=tl.read())


def restate(P, PL, logits, states, term=None, cap=12, logp0=None, tok_cap=12):
    """The same step in fp64 numpy."""
    B = logits.shape[0]
    want = dict(states=[dict(s) for s in states], next_tok=np.full((B,), SENT, dtype=np.int64),
                out_ids=np.full((B, cap), SENT, dtype=np.int64),
                logp=np.zeros((B, 2)) if logp0 is None else np.array(logp0, dtype=np.float64),
                tok_logp=np.full((B, tok_cap), float(SENT)), touched=np.zeros((B, tok_cap), dtype=bool), n_active=0)
    for b, st in enumerate(want["states"]):
        if st["flags"] & R.DONE:
            continue
        j = st["n_tokens"]
        tok, _, _, lpm, lpd = PR.sample_token_plan(P, PL, b, logits[b], None if term is None else term[b], st)
        want["next_tok"][b] = tok
        if j < cap:
            want["out_ids"][b, j] = tok
        want["logp"][b] += (lpm, lpd)
        if j < tok_cap:
            want["tok_logp"][b, j] = lpm
            want["touched"][b, j] = True
        PR.advance_plan(P, PL, b, tok, st)
        want["n_active"] += 0 if st["flags"] & R.DONE else 1
    return want


def compare(got, want, logits, V, check_logp=True, check_tok=True):
    assert np.array_equal(got["next_tok"], want["next_tok"])
    assert np.array_equal(got["out_ids"], want["out_ids"])
    assert got["states"] == want["states"]
    assert got["n_active"] == want["n_active"]
    zmax = float(np.abs(logits[:, :V]).max())
    if check_logp:
        tol = 1e-12 * np.abs(want["logp"]) + 1e-12 * max(1.0, zmax)
        err = np.abs(got["logp"] - want["logp"])
        assert np.all(err <= tol), (float(err.max()), float(tol.min()))
    else:
        assert np.array_equal(got["logp"], want["logp"])
    if check_tok:
        t = want["touched"]
        w32 = want["tok_logp"][t].astype(np.float32)
        assert np.all(np.abs(got["tok_logp"][t].astype(np.float64) - w32.astype(np.float64))
                      <= np.spacing(np.abs(w32)).astype(np.float64))
        assert np.all(got["tok_logp"][~t] == SENT)
    else:
        assert np.all(got["tok_logp"] == SENT)


def make_case(rng, B, V, n_sets, ld_plan, pad):
    """Random sets (set 0 empty, set 1 and 2 one-token sets, pad columns all ones), a plan with
    entries from -1 to n_sets + 3, plan_len 0 on row 0 and ld_plan on row 1, a random allowed mask."""
    sets = np.zeros((n_sets, V + pad), dtype=np.uint8)
    sets[:, V:] = 1  # beyond V: never read
    for s in range(1, n_sets):
        if s <= 2:
            sets[s, rng.integers(V)] = 1
        else:
            sets[s, :V] = rng.random(V) < (0.08 if V > 8 else 0.5)
            sets[s, rng.integers(V)] = 1
    plan = rng.integers(-1, n_sets + 4, size=(B, ld_plan))
    plan[-1, 0], plan[-1, 1 % ld_plan] = -1, n_sets + 3
    if n_sets > 1:
        plan[-1, 2 % ld_plan] = 1  # a one-token set
        plan[-1, ld_plan - 1] = 0  # the empty set
    plan_len = rng.integers(0, ld_plan + 1, size=B)
    plan_len[0] = 0
    plan_len[1 % B] = ld_plan
    plan_len[-1] = ld_plan
    allowed = (rng.random(V) < 0.6).astype(np.uint8)
    allowed[rng.integers(V)] = 1
    return sets, plan, plan_len, allowed


SHAPES = [(7, 68, 23, 9, 0), (3, 1024, 2, 6, 16), (2, 5, 3, 4, 3)]


@pytest.mark.parametrize("B,V,n_sets,ld_plan,pad", SHAPES)
def test_plan_sampler_matches_fp64_restatement(B, V, n_sets, ld_plan, pad):
    """Every generated-token index 0 .. ld_plan + 1 of every row (so entries of -1, of n_sets + 3,
    the empty set, one-token sets, rows past their plan), temperature in {1, 0.8, 1.5}, topk in
    {0, 2, 40} (40 is larger than most sets), end_with_plan in {0, 1}, with and without an allowed
    mask and class bits for the stop rules."""
    rng = np.random.default_rng(B * 10007 + V)
    cls = R.vocab_classes(68)[:V] if V <= 68 else np.zeros(V, dtype=np.uint8)
    flagged = 0
    for temp, topk, ewp, masked in itertools.product([1.0, 0.8, 1.5], [0, 2, 40], [0, 1], [False, True]):
        sets, plan, plan_len, allowed = make_case(rng, B, V, n_sets, ld_plan, pad)
        PL = PR.new_plan(sets, plan, plan_len, end_with_plan=ewp)
        P = R.default_params(V, tok_class=cls, allowed=allowed if masked else None, temperature=temp, topk=topk,
                             seed=int(rng.integers(2 ** 32)), Tmax=64)
        for j in range(ld_plan + 2):
            logits = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
            states = [R.new_state(4, int(rng.integers(2 ** 32))) for _ in range(B)]
            for s in states:
                s.update(n_tokens=j, n_codons=j, pos=4 + j - 1 if j else 4)
            logp0 = rng.standard_normal((B, 2))
            got = run_plan(P, PL, logits, states, logp0=logp0)
            want = restate(P, PL, logits, states, logp0=logp0)
            compare(got, want, logits, V)
            for b in range(B):
                f = got["states"][b]["flags"]
                fires = bool(ewp) and plan_len[b] > 0 and j + 1 >= plan_len[b]
                assert bool(f & PR.PLAN_END) == fires, (b, j, f, plan_len[b])
                flagged += fires
                tok = int(got["next_tok"][b])
                mask = PR.step_allowed(P, PL, b, states[b])
                assert mask is None or mask[tok]
    assert flagged > 0


def test_allowed_logits_far_below_the_disallowed_ones():
    """Allowed logits near -400, disallowed ones near +400: the weights are taken against the
    allowed maximum, logp_model is about -800 and finite, logp_draw is an ordinary log-share."""
    rng = np.random.default_rng(5)
    B, V, n_sets = 4, 68, 6
    sets = np.zeros((n_sets, V), dtype=np.uint8)
    for s in range(n_sets):
        sets[s, rng.choice(V, size=1 + s, replace=False)] = 1
    plan = rng.integers(0, n_sets, size=(B, 3))
    PL = PR.new_plan(sets, plan, np.full(B, 3))
    for temp, topk in ((1.0, 0), (0.8, 2), (1.5, 40)):
        P = R.default_params(V, temperature=temp, topk=topk, seed=9, Tmax=64)
        states = [R.new_state(2, 100 + b) for b in range(B)]
        logits = np.empty((B, V), dtype=np.float32)
        for b in range(B):
            ok = sets[plan[b, 0]].astype(bool)
            logits[b] = np.where(ok, -400.0, 400.0) + rng.standard_normal(V)
        got = run_plan(P, PL, logits, states)
        want = restate(P, PL, logits, states)
        compare(got, want, logits, V)
        assert np.all(np.isfinite(got["logp"])) and np.all(got["logp"][:, 0] < -700) and np.all(got["logp"][:, 1] > -20)
        for b in range(B):
            assert sets[plan[b, 0], got["next_tok"][b]]


def test_termination_bias_under_a_plan():
    """The stop bias is part of the distribution drawn from (logp_draw) and not of logp_model."""
    rng = np.random.default_rng(17)
    B, V, n_sets, ld_plan, pad = SHAPES[0]
    sets, plan, plan_len, _ = make_case(rng, B, V, n_sets, ld_plan, pad)
    sets[3:, R.STOP_IDS[0]] = 1  # a stop codon in most sets
    PL = PR.new_plan(sets, plan, np.full(B, ld_plan), end_with_plan=1)
    P = R.default_params(V, tok_class=R.vocab_classes(68), seed=2, Tmax=64, target_codons=4, bias_window=4,
                         require_terminal_stop=1, stop_on_bio_stop=1, stop_bias=2.5, n_term_classes=3,
                         trigger_class_max=1)
    states = [R.new_state(3, 60 + b) for b in range(B)]
    biased = 0
    for _ in range(3):
        logits = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
        term = rng.standard_normal((B, 3)).astype(np.float32)
        got = run_plan(P, PL, logits, states, term=term)
        compare(got, restate(P, PL, logits, states, term=term), logits, V)
        biased += sum(g["bias_steps"] - s["bias_steps"] for g, s in zip(got["states"], states))
        states = got["states"]
    assert biased > 0


CLS = R.vocab_classes(68)
TAA, EOS_ID, AAA, AAC = R.STOI["TAA"], R.STOI["<EOS_CDS>"], R.STOI["AAA"], R.STOI["AAC"]


def _play(tokens, plan_len, end_with_plan, steps, **kw):
    """One sequence whose plan forces ``tokens`` through one-token sets; random logits.  Returns the
    flags after every step (kernel == restatement asserted at each)."""
    rng = np.random.default_rng(len(tokens) * 31 + plan_len)
    V = 68
    sets = np.zeros((V, V), dtype=np.uint8)
    sets[np.arange(V), np.arange(V)] = 1
    PL = PR.new_plan(sets, np.array([tokens]), np.array([plan_len]), end_with_plan=end_with_plan)
    P = R.default_params(V, tok_class=CLS, seed=3, **dict(dict(Tmax=64), **kw))
    states = [R.new_state(5, 8)]
    flags = []
    logp = np.zeros((1, 2))
    for i in range(steps):
        logits = (3.0 * rng.standard_normal((1, V))).astype(np.float32)
        got = run_plan(P, PL, logits, states, logp0=logp)
        want = restate(P, PL, logits, states, logp0=logp)
        compare(got, want, logits, V)
        if not states[0]["flags"] & R.DONE and i < plan_len:
            assert got["next_tok"][0] == tokens[i]
        states, logp = got["states"], got["logp"]
        flags.append(states[0]["flags"])
    return flags, states[0]


def test_plan_end_fires_exactly_at_plan_len():
    toks = [AAA, AAC, AAA, AAC, AAA]
    flags, st = _play(toks, 3, 1, 5)
    assert flags == [0, 0] + [PR.PLAN_END | R.DONE] * 3
    assert (st["n_tokens"], st["n_codons"], st["pos"]) == (3, 3, -1)  # the later steps touched nothing
    flags, st = _play(toks, 3, 0, 5)
    assert flags == [0] * 5 and st["n_tokens"] == 5  # past its plan the sequence samples on
    flags, st = _play(toks, 0, 1, 3)
    assert flags == [0] * 3  # plan_len 0: no plan, no end
    flags, st = _play(toks, 5, 1, 5)
    assert flags == [0] * 4 + [PR.PLAN_END | R.DONE]


def test_plan_end_comes_after_the_older_rules():
    toks = [AAA, AAC, TAA, AAA]
    # the stop codon at the plan's last step: the biological stop ends the sequence, not the plan
    flags, _ = _play(toks, 3, 1, 3, stop_on_bio_stop=1, target_codons=3)
    assert flags == [0, 0, R.TERMINAL_STOP | R.DONE]
    flags, _ = _play(toks, 3, 1, 3, stop_on_bio_stop=1, target_codons=9)
    assert flags == [0, 0, R.EARLY_STOP | R.TERMINAL_STOP | R.DONE]
    # an early stop that must go on (require_terminal_stop) still ends with the plan
    flags, _ = _play(toks, 3, 1, 3, stop_on_bio_stop=1, target_codons=9, require_terminal_stop=1)
    assert flags == [0, 0, R.EARLY_STOP | PR.PLAN_END | R.DONE]
    flags, _ = _play(toks, 3, 1, 3, max_tokens=3)
    assert flags == [0, 0, R.CAP | R.DONE]
    flags, _ = _play(toks, 4, 1, 4, target_codons=2)
    assert flags == [0] + [R.TARGET | R.DONE] * 3
    flags, _ = _play([AAA, EOS_ID, AAA], 2, 1, 2, stop_on_eos=1)
    assert flags == [0, R.EOS | R.DONE]
    # the plan ends the sequence before the context-full rule looks at the next position
    flags, st = _play(toks, 2, 1, 2, Tmax=6)
    assert flags == [0, PR.PLAN_END | R.DONE]
    flags, st = _play(toks, 3, 1, 2, Tmax=6)
    assert flags == [0, R.CONTEXT_FULL | R.DONE]


def test_done_rows_stay_untouched():
    """Rows already DONE (PLAN_END among them) keep every byte of state, next_tok, out_ids, logp and
    tok_logp; n_active counts the others."""
    rng = np.random.default_rng(11)
    B, V, n_sets, ld_plan, pad = SHAPES[0]
    sets, plan, plan_len, allowed = make_case(rng, B, V, n_sets, ld_plan, pad)
    plan_len[:] = ld_plan
    PL = PR.new_plan(sets, plan, plan_len, end_with_plan=1)
    P = R.default_params(V, tok_class=CLS, allowed=allowed, seed=5, Tmax=64)
    states = [R.new_state(3, b) for b in range(B)]
    states[1].update(flags=PR.PLAN_END | R.DONE, pos=-1, n_tokens=2, n_codons=2)
    states[4].update(flags=R.CAP | R.DONE, pos=-1, n_tokens=5, n_codons=1, bias_steps=2, last_term_class=4)
    logits = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    logp0 = rng.standard_normal((B, 2))
    got = run_plan(P, PL, logits, states, logp0=logp0)
    compare(got, restate(P, PL, logits, states, logp0=logp0), logits, V)
    assert got["n_active"] == B - 2
    for b in (1, 4):
        assert got["states"][b] == states[b] and got["next_tok"][b] == SENT and np.all(got["out_ids"][b] == SENT)
        assert np.array_equal(got["logp"][b].view(np.int64), logp0[b].view(np.int64))
        assert np.all(got["tok_logp"][b] == SENT)
    # without the optional outputs nothing of them is written
    got = run_plan(P, PL, logits, states, logp0=logp0, want_logp=False, want_tok=False)
    compare(got, restate(P, PL, logits, states, logp0=logp0) | dict(logp=logp0), logits, V, check_logp=False,
            check_tok=False)
    got = run_plan(P, PL, logits, states, logp0=logp0, want_tok=False)
    compare(got, restate(P, PL, logits, states, logp0=logp0), logits, V, check_tok=False)
    # a tok_logp row shorter than n_tokens: nothing written past it
    got = run_plan(P, PL, logits, [dict(s, n_tokens=3) if not s["flags"] else s for s in states], tok_cap=3)
    assert np.all(got["tok_logp"] == SENT)


def test_logp_accumulates_over_two_launches():
    rng = np.random.default_rng(21)
    B, V, n_sets, ld_plan, pad = SHAPES[0]
    sets, plan, plan_len, _ = make_case(rng, B, V, n_sets, ld_plan, pad)
    PL = PR.new_plan(sets, plan, plan_len)
    P = R.default_params(V, tok_class=CLS, temperature=0.8, topk=5, seed=6, Tmax=64)
    states = [R.new_state(3, 40 + b) for b in range(B)]
    l1 = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    l2 = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    g1 = run_plan(P, PL, l1, states)
    w1 = restate(P, PL, l1, states)
    compare(g1, w1, l1, V)
    g2 = run_plan(P, PL, l2, g1["states"], logp0=g1["logp"])
    w2 = restate(P, PL, l2, w1["states"], logp0=w1["logp"])
    compare(g2, w2, np.concatenate([l1, l2]), V)
    assert np.all(g2["logp"][:, 0] < g1["logp"][:, 0]) and np.all(g2["logp"][:, 1] <= g1["logp"][:, 1]) and all(s["n_tokens"] == 2 for s in g2["states"])


@pytest.mark.parametrize("V,B", [(68, 5), (257, 3)])
def test_no_sets_is_plain_sampling_with_log_probabilities(V, B):
    """n_sets == 0 (sets, plan and plan_len NULL) with logp: tokens and states equal cg_sample_step's."""
    rng = np.random.default_rng(V)
    cls = R.vocab_classes(68) if V == 68 else np.zeros(V, dtype=np.uint8)
    allowed = (rng.random(V) < 0.5).astype(np.uint8)
    allowed[3] = 1
    PL = PR.new_plan(None, None, None, end_with_plan=1)
    for temp, topk, mask in ((1.0, 0, None), (0.8, 5, allowed), (1.5, 0, allowed)):
        P = R.default_params(V, tok_class=cls, allowed=mask, temperature=temp, topk=topk, seed=12, Tmax=64,
                             stop_on_bio_stop=1, target_codons=1)
        states = [R.new_state(2, 7 * b) for b in range(B)]
        logits = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
        got = run_plan(P, PL, logits, states)
        compare(got, restate(P, PL, logits, states), logits, V)
        cp, keep = R.device_params(P, DEV)
        st = torch.from_numpy(R.states_to_array(states)).to(DEV)
        nxt = torch.full((B,), SENT, dtype=torch.int64, device=DEV)
        out = torch.full((B, 12), SENT, dtype=torch.int64, device=DEV)
        na = torch.zeros(1, dtype=torch.int32, device=DEV)
        _ops().sample_step(cp, torch.from_numpy(logits).to(DEV), st, nxt, out, na)
        torch.cuda.synchronize()
        assert np.array_equal(nxt.cpu().numpy(), got["next_tok"]) and np.array_equal(out.cpu().numpy(), got["out_ids"])
        assert R.array_to_states(st.cpu().numpy()) == got["states"] and int(na.item()) == got["n_active"]


def test_argument_checks():
    V = 68
    rng = np.random.default_rng(1)
    sets, plan, plan_len, _ = make_case(rng, 2, V, 3, 4, 0)
    logits = np.zeros((2, V), dtype=np.float32)
    states = [R.new_state(1, 0), R.new_state(1, 1)]
    P = R.default_params(V)
    good = PR.new_plan(sets, plan, plan_len)
    assert run_plan(P, good, logits, states)["n_active"] == 2
    with pytest.raises(ValueError, match="CG_EINVAL"):
        run_plan(P, good, logits, states, plan_struct=False)
    for drop in ("plan", "plan_len"):
        with pytest.raises(ValueError, match="CG_EINVAL"):
            run_plan(P, dict(good, **{drop: None}), logits, states)
    for field, value in (("sets", None), ("ld_sets", V - 1), ("n_sets", -1)):
        bad, keep2 = PR.device_plan(good, DEV)
        setattr(bad, field, value)
        cp, keep3 = R.device_params(P, DEV)
        st = torch.from_numpy(R.states_to_array(states)).to(DEV)
        nxt = torch.zeros(2, dtype=torch.int64, device=DEV)
        out = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError, match="CG_EINVAL"):
            _ops().sample_step_plan(cp, bad, torch.from_numpy(logits).to(DEV), st, nxt, out)
    with pytest.raises(ValueError, match="CG_EUNSUPPORTED"):
        big = PR.new_plan(np.ones((1, 1025), dtype=np.uint8), np.zeros((1, 2)), np.array([2]))
        run_plan(R.default_params(1025), big, np.zeros((1, 1025), dtype=np.float32), [R.new_state(1, 0)])
