"""Host-side checks of synonymous recoding that need no GPU: the cg_sample_plan mirror, the genetic
code, plan building, the argument checks that come before any launch and the CLI surface."""
import ctypes

import numpy as np
import pytest

import sampler_restatement as R

CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV_Y_YSSSS_CWCLFLF"


def test_plan_struct_mirror_matches_the_library():
    from codonlm_amd import _lib as L
    assert L.lib.cg_struct_bytes(b"cg_sample_plan") == ctypes.sizeof(L.SamplePlan) > 0
    assert "cg_sample_step_plan" in L.SIGNATURES and hasattr(L.lib, "cg_sample_step_plan")
    assert L.GEN_PLAN_END == 128 and L.GEN_PLAN_END & (L.GEN_CONTEXT_FULL * 2 - 1) == 0
    assert L.lib.cg_version().decode().split()[1] == "0.6"


def test_genetic_code():
    from codonlm_amd import generate as G
    assert len(G.CODON_TABLE) == 64 and len(G.AA_TO_CODONS) == 21
    assert sum(len(v) for v in G.AA_TO_CODONS.values()) == 64
    for aa, n in (("L", 6), ("R", 6), ("S", 6), ("M", 1), ("W", 1)):
        assert len(G.AA_TO_CODONS[aa]) == n, aa
    assert G.AA_TO_CODONS["M"] == ["ATG"] and G.AA_TO_CODONS["W"] == ["TGG"]
    assert sorted(G.AA_TO_CODONS["_"]) == ["TAA", "TAG", "TGA"] == sorted(G.STOP_CODONS)
    codons = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
    assert "".join(G.CODON_TABLE[c] for c in codons) == CODE
    assert G.translate(["ATG", "AAA", "<SEP>", "TAA"]) == "MK?_"


class _Model:
    """What generate_batch reads before it launches anything."""
    block_size, vocab_size, sep_id, termination_aux = 64, 68, 3, False
    engine = None


def _sets():
    from codonlm_amd import generate as G
    return G.TokenSets(R.STOI, R.ITOS, 68)


def test_synonymous_plan_lenient_and_strict():
    from codonlm_amd import generate as G
    sets = _sets()
    plan = G.synonymous_plan(sets, "mkLXl")
    table = sets.array()
    assert table.dtype == np.uint8 and table.shape == (len(sets.rows), 68)
    assert len(plan) == 6 and plan[2] == plan[4]  # equal sets are stored once; lower case is accepted
    assert np.nonzero(table[plan[0]])[0].tolist() == [R.STOI["ATG"]]
    assert sorted(R.ITOS[i] for i in np.nonzero(table[plan[2]])[0]) == sorted(G.AA_TO_CODONS["L"])
    assert np.array_equal(table[plan[3]], G.cds_mask(R.ITOS))  # the unknown residue: every codon token
    assert sorted(np.nonzero(table[plan[5]])[0]) == R.STOP_IDS
    with pytest.raises(ValueError, match="unknown residue"):
        G.synonymous_plan(_sets(), "MKX", strict=True)
    with pytest.raises(ValueError):
        G.synonymous_plan(_sets(), "MK_A", strict=True)
    # a vocabulary without some codons: the sets hold only what it has
    itos = [t for t in R.ITOS if t not in ("CTA", "CTC", "TGG")]
    small = G.TokenSets({t: i for i, t in enumerate(itos)}, itos, 68)
    assert len(small.codon_ids("L")) == 4
    with pytest.raises(ValueError):
        small.residue("W", strict=True)
    w = small.residue("W")
    assert np.array_equal(small.array()[w][:len(itos)], G.cds_mask(itos))


def test_recode_is_strict_and_accepts_lower_case():
    from codonlm_amd import recode as RC
    with pytest.raises(ValueError, match="unknown residue"):
        RC.recode_proteins(_Model(), ["MKXA"], R.STOI, R.ITOS)
    with pytest.raises(ValueError, match="block_size"):  # 1 + 63 residues + stop = 65 tokens
        RC.recode_proteins(_Model(), ["m" + "k" * 62], R.STOI, R.ITOS)
    with pytest.raises(ValueError):
        RC.recode_proteins(_Model(), ["MK"], R.STOI, R.ITOS, n=0)


def test_dna_plans_and_keep_ranges():
    from codonlm_amd import generate as G
    from codonlm_amd import recode as RC
    assert RC.dna_codons("atg aaa gcu taa") == ["ATG", "AAA", "GCT"]
    assert RC.dna_codons("ATGAAAGCT") == ["ATG", "AAA", "GCT"]
    for bad in ("ATGAA", "ATGA", "ATGTAAGCT", "ATGNNNGCT"):
        with pytest.raises(ValueError):
            RC.dna_codons(bad)
    with pytest.raises(ValueError):
        RC.recode_dna(_Model(), "ATGAAAG", R.STOI, R.ITOS)
    sets = _sets()
    codons = RC.dna_codons("ATGCTGCTAAAAGCTTTATGA")
    protein, plan = RC.dna_plan(sets, codons, keep=[(1, 3), (5, 6)])
    table = sets.array()
    assert protein == "MLLKAL" and len(plan) == 7
    for k in (1, 2, 5):  # kept: one-token sets of the given codon
        assert np.nonzero(table[plan[k]])[0].tolist() == [R.STOI[codons[k]]]
    for k in (0, 3, 4):
        assert sorted(R.ITOS[i] for i in np.nonzero(table[plan[k]])[0]) == sorted(G.AA_TO_CODONS[protein[k]])
    assert sorted(np.nonzero(table[plan[6]])[0]) == R.STOP_IDS
    assert RC.dna_plan(_sets(), codons)[1] == G.synonymous_plan(_sets(), protein, strict=True)
    for bad in ([(0, 7)], [(3, 3)], [(-1, 2)]):
        with pytest.raises(ValueError, match="keep"):
            RC.dna_plan(_sets(), codons, keep=bad)
    assert RC.parse_keep("10-20,35-40") == [(10, 20), (35, 40)] and RC.parse_keep(None) == []


def test_fit_check_is_per_row_with_end_with_plan():
    from codonlm_amd import generate as G
    sets = _sets()
    table_plan = G.synonymous_plan(sets, "M" * 59)  # 60 generated tokens
    table = sets.array()
    ctx = [[1] * 4, [1] * 30]
    # each row fits (4 + 60, 30 + 10) although the longest prompt + the longest plan does not
    G._check_fit_plans(_Model(), ctx, [table_plan, table_plan[:10]])
    with pytest.raises(ValueError, match="block_size"):
        G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=G.INT_MAX, token_sets=table,
                         plans=[table_plan, table_plan[:35]], end_with_plan=True)
    with pytest.raises(ValueError, match="empty plan"):
        G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=G.INT_MAX, token_sets=table,
                         plans=[table_plan, []], end_with_plan=True)
    with pytest.raises(ValueError, match="block_size"):  # without end_with_plan: the older check
        G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=40, token_sets=table,
                         plans=[table_plan[:10], table_plan[:10]])
    with pytest.raises(ValueError, match="one plan per context"):
        G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=5, token_sets=table, plans=[table_plan])
    with pytest.raises(ValueError, match="token_sets"):
        G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=5, plans=[[0], [0]])
    for bad in (table.astype(np.int32), table[0], np.zeros((2, 69), dtype=np.uint8)):
        with pytest.raises(ValueError, match="token_sets is uint8"):
            G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=5, token_sets=bad, plans=[[0], [0]])


def test_critic_guidance_is_not_implemented():
    from codonlm_amd import generate as G
    for kw in (dict(critic_model=object(), ebm_model=None), dict(critic_model=None, ebm_model=object())):
        with pytest.raises(NotImplementedError):
            G.generate_cds_synonymous(_Model(), kw["critic_model"], None, None, [1], R.STOI, R.ITOS, "MK", alpha=0.5,
                                      ebm_model=kw["ebm_model"])
    with pytest.raises(ValueError, match="block_size"):  # no critic: reaches the fit check
        G.generate_cds_synonymous(_Model(), None, None, None, [1], R.STOI, R.ITOS, "M" * 64)
    info = G.synonymous_info(2, [1, 5] + [10] * 6, "MKAQ", critic=True)
    assert info == {"protocol": "guided", "guidance_components": ["synonymous_template", "critic"],
                    "had_terminal_stop": True, "early_stop": False, "hit_hard_cap": False, "target_codons": 5,
                    "generated_codons": 5, "cds_only": True, "require_terminal_stop": True, "generated_tokens": 6}
    assert G.synonymous_info(1, [1, 2], "", ebm=True)["guidance_components"] == ["synonymous_template", "ebm"]


def test_cli_parser_surface():
    from codonlm_amd import recode as RC
    ap = RC.build_parser()
    a = ap.parse_args(["--run_dir", "runs/x", "--protein", "MKAQ"])
    assert (a.run_dir, a.ckpt, a.protein, a.dna) == ("runs/x", None, "MKAQ", None)
    assert (a.n, a.seed, a.temperature, a.topk, a.keep, a.top, a.out, a.dtype) == (64, 0, 1.0, 0, None, 5, None, "fp32")
    a = ap.parse_args(["--ckpt", "best.pt", "--dna", "ATGAAATAA", "--n", "8", "--seed", "3", "--temperature", "0.8",
                       "--topk", "2", "--keep", "10-20,35-40", "--top", "3", "--out", "o.tsv", "--dtype", "bf16"])
    assert (a.ckpt, a.dna, a.n, a.seed, a.temperature, a.topk, a.keep, a.top, a.out, a.dtype) == \
        ("best.pt", "ATGAAATAA", 8, 3, 0.8, 2, "10-20,35-40", 3, "o.tsv", "bf16")
    for bad in ([], ["--run_dir", "r"], ["--protein", "MK"], ["--run_dir", "r", "--ckpt", "c", "--protein", "MK"],
                ["--run_dir", "r", "--protein", "MK", "--dna", "ATG"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    rows = RC.tsv_rows([{"logp_model": -1.25, "logp_draw": -0.5, "dna": "ATGTAA"},
                        {"logp_model": -2.0, "logp_draw": -0.75, "dna": "ATGTGA"}], top=1)
    assert rows == [["rank", "logp_model", "logp_draw", "dna"], [1, "-1.2500", "-0.5000", "ATGTAA"]]
    assert RC.read_protein("MKAQ") == "MKAQ"
