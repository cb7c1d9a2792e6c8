"""Synonymous recoding end to end (codonlm_amd.generate / codonlm_amd.recode) in fp32, verified by
teacher forcing as tests/test_gpu_generate.py does: one full forward of every finished sequence
gives the logits at each of its positions, and the fp64 restatement of cg_sample_step_plan
(tests/plan_restatement.py) replays the run on them.

A draw is exempt only where the model's own fp32 error could move it: u*total within
(4 delta / temperature) * total of a CDF boundary, or a top-k cut whose logit gap is below 4 delta,
with delta = max(1e-4, 5e-6 |logit|max) (test_gpu_generate.py's rule).  At most 5 % of a run's draws
may be exempt.  logp_model must agree with score.token_logprobs of the finished sequence, summed
over the generated positions, within 2 delta * n_tokens: the decode-step logits and the full-forward
logits each carry delta, and a log-probability moves by at most twice its logits' error."""
import functools

import numpy as np
import pytest
import torch

import plan_restatement as PR
import sampler_restatement as R
from test_gpu_generate import _forward, _model
from test_gpu_model import DEV

pytestmark = pytest.mark.gpu
SEED = 77
ATG = R.STOI["ATG"]
PROTEINS = ["MKAQ", "MACDEFGHIKLMNPQRSTVWY", "MLLSRRXGGAVT", "MSSLPTTAW" * 3, "M", "MRRRRRRLLLLLLSSSSSS" + "AGV" * 8]
PROMPTS = [[1], [1, ATG], [1, 10, 11, 12, 13, 14], [1], [1, 20, 21], [1]]
SETTINGS = [(1.0, 0), (0.8, 3), (1.5, 0), (0.8, 1)]
N_DRAWS = sum(len(p) + 1 for p in PROTEINS)


def _mods():
    from codonlm_amd import generate, recode, score
    return generate, recode, score


def _plans(G):
    sets = G.TokenSets(R.STOI, R.ITOS, 68)
    plans = [G.synonymous_plan(sets, p) for p in PROTEINS]  # lenient: the X draws among all codon tokens
    return sets.array(), plans


def _run(m, temperature, topk, *, which=None, poll_every=16, seed=SEED, with_logp=True):
    """The six proteins (or the rows ``which``) as one batch, stream = index: [(ids, state)]."""
    G, _, _ = _mods()
    table, plans = _plans(G)
    which = list(range(len(PROTEINS))) if which is None else which
    return G.generate_batch(m, [PROMPTS[b] for b in which], R.STOI, R.ITOS, seed=seed, streams=which,
                            poll_every=poll_every, max_tokens=G.INT_MAX, temperature=temperature, topk=topk,
                            stop_on_eos=False, stop_on_bio_stop=False, token_sets=table,
                            plans=[plans[b] for b in which], end_with_plan=True, with_logp=with_logp)


def _translates(ids, b):
    G, _, _ = _mods()
    got = G.translate([R.ITOS[t] for t in ids[len(PROMPTS[b]):]])
    want = PROTEINS[b] + "_"
    return len(got) == len(want) and all(w == "X" or g == w for g, w in zip(got, want))


def _replay(m, P, PL, b, ids):
    """Teacher-forced replay of sequence b; returns (restated state, exempt draw indices, n draws,
    delta).  Asserts every non-exempt token."""
    ctx = PROMPTS[b]
    logits, _ = _forward(m, ids, False)
    delta = max(1e-4, 5e-6 * float(np.abs(logits).max()))
    temp = max(1e-6, float(np.float32(P["temperature"])))
    st = R.new_state(len(ctx), b)
    exempt = []
    n = len(ids) - len(ctx)
    for i in range(n):
        assert not st["flags"] & R.DONE, "tokens after the sequence was done"
        tok, boundary, gap, _, _ = PR.sample_token_plan(P, PL, b, logits[len(ctx) + i - 1], None, st)
        if boundary <= 4 * delta / temp or gap < 4 * delta:
            exempt.append(i)
        else:
            assert ids[len(ctx) + i] == tok, (b, i, ids[len(ctx) + i], tok, boundary, gap)
        PR.advance_plan(P, PL, b, ids[len(ctx) + i], st)
    return st, exempt, n, delta


@functools.lru_cache(maxsize=None)
def _verified(temperature, topk):
    """One verified run per setting, shared by the tests below: (results, first exempt index per row)."""
    G, _, S = _mods()
    m = _model("mha_gelu_sep")
    res = _run(m, temperature, topk)
    table, plans = _plans(G)
    ld = max(len(p) for p in plans)
    PL = PR.new_plan(table, [p + [-1] * (ld - len(p)) for p in plans], [len(p) for p in plans], end_with_plan=1)
    P = R.default_params(68, tok_class=R.vocab_classes(68), temperature=temperature, topk=topk, seed=SEED, Tmax=64)
    draws = n_exempt = 0
    exempt_at = []
    for b, (ids, rec) in enumerate(res):
        assert ids[:len(PROMPTS[b])] == PROMPTS[b]
        st, exempt, n, delta = _replay(m, P, PL, b, ids)
        draws += n
        n_exempt += len(exempt)
        exempt_at.append(exempt[0] if exempt else None)
        assert n == len(PROTEINS[b]) + 1 and _translates(ids, b), (b, ids)
        assert st["flags"] == PR.PLAN_END | R.DONE
        assert {k: rec[k] for k in R.STATE_FIELDS} == st, (b, rec, st)
        lp = S.token_logprobs(m, ids)[len(PROMPTS[b]) - 1:]
        assert len(lp) == n
        err = abs(rec["logp_model"] - float(lp.astype(np.float64).sum()))
        print(f"  row {b}: logp_model {rec['logp_model']:.6f} logp_draw {rec['logp_draw']:.6f} "
              f"|logp_model - scored| {err:.2e} (bound {2 * delta * n:.2e})")
        assert err <= 2 * delta * n, (b, err, delta, n)
        assert rec["logp_draw"] <= 1e-9 and rec["logp_model"] < 0
        if topk == 0 and temperature == 1.0:  # the same logits' share of a subset of the mass
            assert rec["logp_draw"] >= rec["logp_model"] - 1e-9
    print(f"[T={temperature} k={topk}] {draws} draws, {n_exempt} exempt")
    assert draws == N_DRAWS == 114
    assert n_exempt <= 0.05 * draws, (n_exempt, draws)
    return res, exempt_at


@pytest.mark.parametrize("temperature,topk", SETTINGS)
def test_recoding_replays_under_teacher_forcing(temperature, topk):
    _verified(temperature, topk)


def test_drop_in_equals_its_stream_and_returns_the_reference_record():
    G, _, _ = _mods()
    m = _model("mha_gelu_sep")
    temperature = 1.5  # (the drop-in has no top-k argument)
    res, exempt_at = _verified(temperature, 0)
    for b in (0, 2, 4):
        ids, info = G.generate_cds_synonymous(m, None, None, torch.device(DEV), PROMPTS[b], R.STOI, R.ITOS, PROTEINS[b],
                                              temperature=temperature, seed=SEED, stream=b)
        n = len(PROTEINS[b]) + 1
        assert ids[-1] == R.STOI["<EOS_CDS>"] and len(ids) == len(PROMPTS[b]) + n + 1
        upto = len(PROMPTS[b]) + (exempt_at[b] if exempt_at[b] is not None else n)
        assert ids[:upto] == res[b][0][:upto], b
        assert _translates(ids[:-1], b)
        assert info == {"protocol": "guided", "guidance_components": ["synonymous_template"],
                        "had_terminal_stop": True, "early_stop": False, "hit_hard_cap": False, "target_codons": n,
                        "generated_codons": n, "cds_only": True, "require_terminal_stop": True,
                        "generated_tokens": n + 1}
    # a critic with alpha = 0 is the plain path, named in the record as the reference names it
    ids0, info0 = G.generate_cds_synonymous(m, object(), None, torch.device(DEV), PROMPTS[0], R.STOI, R.ITOS, "mkaq",
                                            alpha=0.0, temperature=temperature, seed=SEED, stream=0)
    assert info0["guidance_components"] == ["synonymous_template", "critic"] and _translates(ids0[:-1], 0)


def test_a_candidate_alone_and_any_poll_interval_give_the_same_output():
    m = _model("mha_gelu_sep")
    res, exempt_at = _verified(1.0, 0)
    for b in (1, 3, 5):
        (ids, rec), = _run(m, 1.0, 0, which=[b])
        n = len(PROMPTS[b]) + (exempt_at[b] if exempt_at[b] is not None else 10 ** 6)
        assert ids[:n] == res[b][0][:n], b
        if exempt_at[b] is None:
            assert {k: rec[k] for k in R.STATE_FIELDS} == {k: res[b][1][k] for k in R.STATE_FIELDS}
    a = _run(m, 0.8, 3)
    assert _run(m, 0.8, 3, poll_every=16) == a
    assert _run(m, 0.8, 3, poll_every=1) == a
    assert _run(m, 0.8, 3, poll_every=7) == a
    assert [ids for ids, _ in _run(m, 0.8, 3, seed=SEED + 1)] != [ids for ids, _ in a]
    # without with_logp the states carry no log-probabilities and the tokens are the same
    plain = _run(m, 0.8, 3, with_logp=False)
    assert [ids for ids, _ in plain] == [ids for ids, _ in a] and "logp_model" not in plain[0][1]


def test_recode_proteins_ranks_candidates_and_uses_stream_i_n_plus_c():
    G, RC, _ = _mods()
    m = _model("mha_gelu_sep")
    proteins = ["MKAQ", "mllsrr", "M"]
    out = RC.recode_proteins(m, proteins, R.STOI, R.ITOS, n=5, seed=SEED, max_batch=4)  # 15 jobs in 4 batches
    assert len(out) == 3
    for i, cands in enumerate(out):
        assert sorted(c["stream"] for c in cands) == list(range(5 * i, 5 * i + 5))
        keys = [(-c["logp_model"], c["stream"]) for c in cands]
        assert keys == sorted(keys)
        for c in cands:
            assert set(c) == {"ids", "codons", "dna", "logp_model", "logp_draw", "stream"}
            assert G.translate(c["codons"]) == proteins[i].upper() + "_" and c["dna"] == "".join(c["codons"])
            assert c["ids"] == [1] + [R.STOI[x] for x in c["codons"]]
    # a candidate does not depend on its batch: one batch of all, another prefix-free call for one protein
    whole = RC.recode_proteins(m, proteins, R.STOI, R.ITOS, n=5, seed=SEED, max_batch=256)
    assert [[c["dna"] for c in cands] for cands in whole] == [[c["dna"] for c in cands] for cands in out]
    first = RC.recode_proteins(m, proteins[:1], R.STOI, R.ITOS, n=5, seed=SEED)
    assert [c["dna"] for c in first[0]] == [c["dna"] for c in out[0]]
    with_prefix = RC.recode_proteins(m, ["MKAQ"], R.STOI, R.ITOS, n=2, seed=SEED, prefix=[1, 20, 21])
    assert all(c["ids"][:3] == [1, 20, 21] and len(c["ids"]) == 8 for c in with_prefix[0])


def test_keep_ranges_stay_as_given():
    G, RC, _ = _mods()
    m = _model("mha_gelu_sep")
    dna = "ATGCTGCTAAGAAGCTCATTAGCGGGTGTCTGGTAA"  # M L L R S S L A G V W + stop
    keep = [(1, 3), (5, 7)]
    codons = RC.dna_codons(dna)
    cands = RC.recode_dna(m, dna.lower(), R.STOI, R.ITOS, n=12, seed=SEED, keep=keep)
    assert len(cands) == 12
    for c in cands:
        assert G.translate(c["codons"]) == "MLLRSSLAGVW_"
        for a, b in keep:
            assert c["codons"][a:b] == codons[a:b]
    free = [k for k in range(len(codons)) if not any(a <= k < b for a, b in keep)]
    assert any(c["codons"][k] != codons[k] for c in cands for k in free)  # the rest is really recoded
    assert len({c["dna"] for c in cands}) > 1
    everything = RC.recode_dna(m, dna, R.STOI, R.ITOS, n=3, seed=SEED, keep=[(0, len(codons))])
    assert all(c["codons"][:-1] == codons for c in everything)


def test_topk_1_is_one_greedy_recoding():
    _, RC, _ = _mods()
    m = _model("mha_gelu_sep")
    a = RC.recode_proteins(m, [PROTEINS[1]], R.STOI, R.ITOS, n=6, seed=1, topk=1)[0]
    b = RC.recode_proteins(m, [PROTEINS[1]], R.STOI, R.ITOS, n=2, seed=99, topk=1, temperature=0.8)[0]
    assert len({c["dna"] for c in a + b}) == 1
    assert all(c["logp_draw"] == 0.0 for c in a + b)  # the one kept token has all the mass
    assert sorted(c["stream"] for c in a) == list(range(6))


def test_bf16_run_keeps_the_structure():
    """bf16 logits differ from fp32 ones by far more than delta: structure only."""
    from conftest import load_golden
    from test_gpu_model import make_model
    G, _, _ = _mods()
    cfgd, g = load_golden("mha_gelu_sep")
    m, _, params = make_model(cfgd, g, dtype="bf16")
    m.load_state_dict({"tok_emb.weight": torch.from_numpy(params["tok_emb.weight"]) * 0.25}, strict=False)
    m.eval()
    res = _run(m, 1.0, 0)
    for b, (ids, rec) in enumerate(res):
        assert rec["flags"] == G.L.GEN_PLAN_END | G.L.GEN_DONE and rec["n_tokens"] == len(PROTEINS[b]) + 1
        assert _translates(ids, b) and R.ITOS[ids[-1]] in G.STOP_CODONS
        assert np.isfinite(rec["logp_model"]) and rec["logp_model"] < 0 and rec["logp_draw"] <= 1e-9


def test_cli_on_a_run_directory(tmp_path, capsys):
    from oracle import tinygpt_oracle as O
    G, RC, _ = _mods()
    cfg = O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=2, n_embd=128, sep_id=3)
    params = O.synthetic_params(cfg, seed=7)
    rd = tmp_path / "run"
    (rd / "checkpoints").mkdir(parents=True)
    (rd / "itos.txt").write_text("\n".join(R.ITOS) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["tok_emb.weight"] = sd["tok_emb.weight"] * 0.25
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 68, "block_size": 64, "n_layer": 2, "n_head": 2, "n_embd": 128, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    out = tmp_path / "o" / "recoded.tsv"
    cands = RC.main(["--run_dir", str(rd), "--protein", "MKLSRA", "--n", "8", "--seed", "3", "--top", "4",
                     "--out", str(out)])
    assert len(cands) == 8
    lines = out.read_bytes().decode().split("\r\n")
    assert lines[0].split("\t") == ["rank", "logp_model", "logp_draw", "dna"] and lines[-1] == "" and len(lines) == 6
    last = None
    for r, line in enumerate(lines[1:-1], start=1):
        f = line.split("\t")
        assert f[0] == str(r) and len(f) == 4 and f[3] == cands[r - 1]["dna"] and len(f[3]) == 21
        assert G.translate([f[3][i:i + 3] for i in range(0, 21, 3)]) == "MKLSRA_"
        assert f[1] == f"{cands[r - 1]['logp_model']:.4f}" and (last is None or float(f[1]) <= last)
        last = float(f[1])
    # --ckpt, --dna with --keep, standard output
    capsys.readouterr()
    cands = RC.main(["--ckpt", str(rd / "checkpoints" / "best.pt"), "--dna", "ATGAAACTGAGCCGTGCTTAA", "--keep", "2-4",
                     "--n", "4", "--top", "2"])
    text = [ln for ln in capsys.readouterr().out.splitlines() if "\t" in ln]
    assert len(text) == 3 and text[0].split("\t") == ["rank", "logp_model", "logp_draw", "dna"]
    assert all(c["codons"][2:4] == ["CTG", "AGC"] for c in cands) and text[1].split("\t")[3] == cands[0]["dna"]
