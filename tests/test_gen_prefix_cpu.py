"""The prefix-generation benchmark's host side, without a GPU.

* The restated metric functions of codonlm_amd.gen_prefix and the Python-set restatement of the window
  index (tests/memorization_restatement.py) equal what the REAL reference returned for the same inputs
  (tests/golden/gen_prefix.npz, written by make_golden_gen_prefix.py): integers and seeds exactly, floats
  within 1e-12.
* The closures the reference keeps inside main() -- aa_identity, syn_rate, usage_agree, gqs,
  ppl_stability -- cannot be imported from it, so they are held to hand-computed values stated here.
* translate_cds is NOT in the fixture (the reference's needs Biopython, which the fixture's maker does
  not have): the translation rule is checked against the hand-written cases below only.
"""
import ctypes
import json
import math

import numpy as np
import pytest

import memorization_restatement as MR

SPECIALS = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"]
CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
ITOS = SPECIALS + CODONS
STOI = {t: i for i, t in enumerate(ITOS)}

# the reference's SampleResult / ProtocolResult fields, in order
SAMPLE_HEADER = ["run_id", "gene_idx", "k", "sample_id", "aa_identity", "syn_rate", "stop_score", "frame_integrity",
                 "ppl_stability", "no_repeat", "usage_agree", "gqs", "gen_len", "valid_end", "early_stop",
                 "gen_len_codons", "had_terminal_stop", "hit_hard_cap", "target_codons", "termination_bias_steps",
                 "last_termination_class", "critic_stability", "critic_family_prob", "critic_function_prob", "raw_gqs",
                 "raw_gen_len", "raw_had_terminal_stop", "raw_hit_hard_cap", "raw_valid_end", "train_overlap_10",
                 "train_overlap_20"]
PROTOCOL_HEADER = ["run_id", "gene_idx", "k", "sample_id", "protocol", "sample_seed", "cds_only",
                   "require_terminal_stop", "guidance_components", "temperature", "topk", "target_codons",
                   "max_new_tokens", "generated_tokens", "aa_identity", "syn_rate", "stop_score", "frame_integrity",
                   "ppl_stability", "no_repeat", "usage_agree", "gqs", "gen_len_codons", "valid_end", "early_stop",
                   "had_terminal_stop", "hit_hard_cap", "stop_reason", "train_overlap_10", "train_overlap_20"]


@pytest.fixture(scope="module")
def doc():
    z = np.load(MR.__file__.replace("memorization_restatement.py", "golden/gen_prefix.npz"), allow_pickle=False)
    return json.loads(str(z["cases"]))


def _close(a, b):
    if isinstance(b, float) and math.isnan(b):
        return math.isnan(a)
    return abs(a - b) <= 1e-12


def test_seed_bootstrap_stop_and_repeat_equal_the_reference(doc):
    from codonlm_amd import gen_prefix as GP
    assert len(doc["sample_seed"]) >= 5
    for c in doc["sample_seed"]:
        assert GP.sample_seed(*c["args"]) == c["out"]
    for c in doc["bootstrap_interval"]:
        low, high = GP.bootstrap_interval(c["values"], statistic=c["statistic"], seed=c["seed"],
                                          n_resamples=c["n_resamples"])
        assert _close(low, c["out"][0]) and _close(high, c["out"][1]), c
    for c in doc["score_stop_behavior"]:
        score, valid_end, early = GP.score_stop_behavior(c["codons"], c["truth_len"])
        assert _close(score, c["out"][0]) and (valid_end, early) == (c["out"][1], c["out"][2]), c
    for c in doc["ngram_repeat_ratio"]:
        assert _close(GP.ngram_repeat_ratio(c["tokens"], n=c["n"]), c["out"]), c
    for c in doc["codon_to_aa"]:
        assert GP.codon_to_aa(c["codon"]) == c["out"], c


def test_restatement_coverage_equals_the_reference(doc):
    """The Python-set restatement the GPU tests compare the kernels with is itself the reference's
    _training_match_coverage, matching_substring_coverage, _coverage_from_index and
    _matched_query_windows."""
    n_pos = 0
    for c in doc["training_match_coverage"]:
        n = c["n"]
        train = [np.asarray(s, dtype=np.uint8) for s in c["training"]]
        table = MR.build(train, n)
        for q, out in zip(c["queries"], c["out"]):
            assert _close(MR.fraction(np.asarray(q, dtype=np.uint8), table, n), out)
            n_pos += out > 0
        for q, out in zip(c["queries"], c["out_empty_index"]):
            assert MR.fraction(np.asarray(q, dtype=np.uint8), set(), n) == out == 0.0
    assert n_pos >= 6
    for c in doc["leakage_audit"]:
        w = c["window"]
        sym = lambda s: np.frombuffer(s.encode("ascii"), dtype=np.uint8)  # noqa: E731
        table = MR.build([sym(s) for s in c["training"]], w)
        matched = set()
        for q, cov in zip(c["queries"], c["matching_substring_coverage"]):
            assert _close(MR.fraction(sym(q), table, w), cov), c["name"]
            hit = MR.coverage(sym(q), table, w)[0]
            matched.update(q[int(s):int(s) + w] for s in np.nonzero(hit)[0])
        assert sorted(matched) == c["matched_query_windows"], c["name"]
        sub = {m.encode("ascii") for m in matched}
        for q, cov in zip(c["queries"], c["coverage_from_index"]):
            assert _close(MR.fraction(sym(q), sub, w), cov), c["name"]
        assert 0 < len(matched)


def test_closures_of_main_on_hand_computed_cases():
    from codonlm_amd import gen_prefix as GP
    # aa_identity: over the shorter length; M and V agree out of 3
    assert GP.aa_identity(list("MKV"), list("MRVQ")) == 2 / 3
    assert GP.aa_identity([], ["M"]) == 0.0 and GP.aa_identity(list("MK"), list("MK")) == 1.0
    # syn_rate: ATG=ATG (M), AAA~AAG (K), TAA / TGA both stops (excluded), GGG~GGA (G): 3 of 4
    assert GP.syn_rate(["ATG", "AAA", "TAA", "GGG"], ["ATG", "AAG", "TGA", "GGA", "CCC"]) == 0.75
    assert GP.syn_rate(["ATG"], []) == 0.0
    assert GP.syn_rate(["AAA", "NNN"], ["CCC", "NNN"]) == 0.5  # unknown codons are both "?"
    # gqs: the weights 0.30 / 0.20 / 0.15 / 0.10 / 0.10 / 0.10 / 0.05, times 100
    assert GP.gqs(1.0, 0.5, 0.0, 1.0, 0.5, 0.0, 1.0) == pytest.approx(60.0, abs=1e-12)
    assert GP.gqs(0, 0, 0, 0, 0, 0, 0) == 0.0 and GP.gqs(1, 1, 1, 1, 1, 1, 1) == pytest.approx(100.0, abs=1e-12)
    assert GP.gqs(0, 0, 1, 0, 0, 0, 0) == pytest.approx(15.0, abs=1e-12)
    # usage_agree: the reference usage is AAA and CCC half each (the specials and other codons absent)
    usage = GP.UsageReference.from_lines(["AAACCC", "aaaccc", "AAACCCA"], ITOS, STOI)
    a, c = STOI["AAA"], STOI["CCC"]
    assert usage.unigram_cod[a] == usage.unigram_cod[c] == 0.5
    assert usage.usage_agree([a, c]) == pytest.approx(1.0, abs=1e-9)        # KL = 0
    assert usage.usage_agree([a, a]) == 0.0                                   # KL = ln 2 > KL0 = 0.5
    kl = 0.75 * math.log(1.5) + 0.25 * math.log(0.5)
    assert usage.usage_agree([a, a, a, c]) == pytest.approx(1.0 - kl / 0.5, abs=1e-9)
    assert usage.usage_agree([]) == 0.0 and usage.usage_agree([STOI["<SEP>"]]) == 0.0
    # a CDS file without a known codon: the flat fallback
    flat = GP.UsageReference.from_lines(["NNN"], ITOS, STOI)
    assert flat.unigram_cod[a] == pytest.approx(1 / 64) and flat.unigram_cod[0] == 0.0
    # frame_integrity
    assert GP.frame_integrity(["ATG", "TAA"]) == 1.0 and GP.frame_integrity(["ATG", "<SEP>"]) == 0.0
    # ppl_stability: fewer than 22 ids -> 1.0 whatever the losses
    assert GP.ppl_stability_from_losses(21, np.full(20, 9.0)) == 1.0
    # 22 ids, 21 losses, w = min(10, 21 // 4) = 5: first mean 1, last mean 1 + 1/64
    loss = np.ones(21, dtype=np.float32)
    loss[-5:] = 1.0 + 1.0 / 64
    assert GP.ppl_stability_from_losses(22, loss) == pytest.approx(math.exp(-(1.0 / 64) / 0.02), abs=1e-12)
    # last < first: the drift is clipped at 0
    assert GP.ppl_stability_from_losses(22, loss[::-1].copy()) == 1.0
    # 60 ids, 59 losses, w = 10: only the first and last ten count
    loss = np.full(59, 7.0, dtype=np.float32)
    loss[:10], loss[-10:] = 2.0, 2.0078125
    assert GP.ppl_stability_from_losses(60, loss) == pytest.approx(math.exp(-0.0078125 / 0.02), abs=1e-12)
    with pytest.raises(ValueError):
        GP.ppl_stability_from_losses(30, np.zeros(10))


def test_lengths_rows_and_guidance():
    from codonlm_amd import gen_prefix as GP
    s = GP.Settings(k_list=(1, 3), samples=2, max_new=300)
    # block 512: window 512 - 3 - 6 = 503; hard_cap = min(503, 400, 300); target = max(min(256, 300), 100)
    assert GP.length_plan(512, 3, s) == (300, 256)
    # block 128, k 10: window 112; hard_cap 112; target min(256, 112) = 112
    assert GP.length_plan(128, 10, s) == (112, 112)
    with pytest.raises(ValueError):
        GP.length_plan(100, 1, s)  # window 93 < min_aa_len 100
    small = GP.Settings(k_list=(1, 3), samples=2, max_new=20, min_aa_len=5, target_aa_len=12, max_aa_len=30)
    assert GP.length_plan(64, 3, small) == (20, 12)
    cds = ["ATGAAACCCGGGTTTTAA", "ATGCCC" + "AAA" * 3]
    rows = GP.plan_rows(cds, STOI, 64, small)
    assert [(r.gene_idx, r.k, r.sample_id) for r in rows] == [(g, k, i) for g in (0, 1) for k in (1, 3) for i in (0, 1)]
    assert rows[0].ctx_ids == [STOI["<BOS_CDS>"], STOI["ATG"]] and len(rows[2].ctx_ids) == 4
    assert all(r.seed == GP.sample_seed(small.seed, r.gene_idx, r.k, r.sample_id) for r in rows)
    assert GP.Settings().guidance() == []
    assert GP.Settings(allow_non_cds_tokens=True, termination_bias=True, require_terminal_stop=True,
                       multi_offset_prior=True).guidance() == ["termination_bias", "multi_offset_prior",
                                                               "forced_terminal_stop", "non_cds_tokens"]


def _protocol_row(GP, protocol, k, sample, gqs, length, stop):
    return GP.ProtocolResult(run_id="r", gene_idx=0, k=k, sample_id=sample, protocol=protocol, sample_seed=7, cds_only=True,
                             require_terminal_stop=False, guidance_components="[]", temperature=0.8, topk=5,
                             target_codons=12, max_new_tokens=20, generated_tokens=length, aa_identity=0.5, syn_rate=0.25,
                             stop_score=1.0, frame_integrity=1.0, ppl_stability=1.0, no_repeat=1.0, usage_agree=0.5,
                             gqs=gqs, gen_len_codons=length, valid_end=stop, early_stop=False, had_terminal_stop=stop,
                             hit_hard_cap=not stop, stop_reason="x", train_overlap_10=0.5, train_overlap_20=0.0)


def test_files_carry_the_reference_headers(tmp_path):
    import csv
    from codonlm_amd import gen_prefix as GP
    assert list(GP.SAMPLE_COLUMNS) == SAMPLE_HEADER and list(GP.PROTOCOL_COLUMNS) == PROTOCOL_HEADER
    s = GP.Settings(run_id="r", k_list=(1, 3), samples=2, ci_resamples=50)
    prot = [_protocol_row(GP, p, k, i, 40.0 + 10 * i + k, 10 + i, bool(i)) for k in (1, 3) for i in (0, 1)
            for p in ("raw_model", "cds_constrained")]
    samples = [GP.SampleResult("r", 0, r.k, r.sample_id, 0.5, 0.25, 1.0, 1.0, 1.0, 1.0, 0.5, r.gqs, r.gen_len_codons, r.valid_end,
                               False, gen_len_codons=r.gen_len_codons, had_terminal_stop=r.had_terminal_stop,
                               hit_hard_cap=r.hit_hard_cap, target_codons=12, termination_bias_steps=0,
                               last_termination_class=None, critic_function_prob=0.0, raw_gqs=r.gqs, train_overlap_10=0.5)
               for r in prot if r.protocol == "cds_constrained"]
    paths = GP.write_outputs(tmp_path / "out", samples, prot, [("raw_model_x", "ATGTAA"), ("empty", "")], s,
                             GP.manifest(s, "best.pt", {"status": "explicit_cds_file"}, [], False))
    assert sorted(p.name for p in paths.values()) == sorted(
        ["samples.csv", "protocol_samples.csv", "generated_protocols.fasta", "protocol_summary.csv",
         "protocol_manifest.json", "summary.csv"])
    head = lambda name: next(csv.reader(paths[name].open()))  # noqa: E731
    assert head("samples.csv") == SAMPLE_HEADER and head("protocol_samples.csv") == PROTOCOL_HEADER
    assert head("summary.csv") == list(GP.SUMMARY_COLUMNS) and head("summary.csv")[-1] == "n"
    assert head("protocol_summary.csv")[:6] == ["k", "protocol", "n", "median_gqs", "median_gqs_ci_low", "median_gqs_ci_high"]
    rows = list(csv.DictReader(paths["protocol_summary.csv"].open()))
    assert [(r["k"], r["protocol"]) for r in rows] == [("1", "raw_model"), ("1", "cds_constrained"), ("3", "raw_model"),
                                                        ("3", "cds_constrained")]
    assert float(rows[0]["median_gqs"]) == 46.0 and float(rows[0]["terminal_stop_rate"]) == 0.5
    assert float(rows[0]["median_gqs_ci_low"]) <= 46.0 <= float(rows[0]["median_gqs_ci_high"])
    srow = list(csv.DictReader(paths["summary.csv"].open()))[0]
    assert float(srow["median_gqs"]) == 46.0 and float(srow["train_overlap_10"]) == 0.5 and srow["n"] == "2"
    assert paths["generated_protocols.fasta"].read_text() == ">raw_model_x\nATGTAA\n"
    man = json.loads(paths["protocol_manifest.json"].read_text())
    assert set(man["protocols"]) == {"raw_model", "cds_constrained"} and man["base_seed"] == 1337
    assert man["sample_seed_derivation"] == "sha256(base_seed:gene_idx:k:sample_id)[0:4]"


def test_translation_rule_on_hand_written_cases():
    """The audit's protein rule: incomplete tail ignored, trailing stop dropped, internal stop or unknown
    codon -> X.  Hand-written only: the reference's translate_cds is not in the fixture."""
    from codonlm_amd import memorization as M
    assert M.translate_cds("ATGAAATAA") == "MK"
    assert M.translate_cds("atg aaa\nuaa") == "MK"          # whitespace, case, U
    assert M.translate_cds("ATGTAAAAATGA") == "MXK"          # internal stop -> X, trailing stop dropped
    assert M.translate_cds("ATGNNNAAAC") == "MXK"            # unknown codon -> X, tail C ignored
    assert M.translate_cds("ATGAAATAATAA") == "MKX"          # only the last stop is dropped
    assert M.translate_cds("AT") == "" and M.translate_cds("TAA") == ""
    assert M.normalize_cds(" acgu\tAC ") == "ACGTAC"
    with pytest.raises(ValueError):
        M.ids_to_symbols([3, 256])
    flat, off = M.pack_sequences([np.array([1, 2], dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.array([3], dtype=np.uint8)])
    assert flat.tolist() == [1, 2, 3] and off.tolist() == [0, 2, 2, 3]


def test_abi_of_the_window_index():
    """The new structs mirror the library's, and the argument checks answer on the host."""
    from codonlm_amd import _lib as L, ops
    assert L.lib.cg_struct_bytes(b"cg_ngram_index_desc") == ctypes.sizeof(L.NgramIndexDesc) > 0
    assert L.lib.cg_struct_bytes(b"cg_ngram_coverage_desc") == ctypes.sizeof(L.NgramCoverageDesc) > 0
    assert L.lib.cg_version().decode() == "codonlm_hip 0.6 gfx950"  # additions only
    d = L.NgramIndexDesc(n=33, n_seq=1, seq_hi=1, n_sym=64)
    assert L.lib.cg_ngram_index_build(ctypes.byref(d), None) == L.CG_EUNSUPPORTED
    d = L.NgramIndexDesc(n=0, n_seq=1, seq_hi=1, n_sym=64)
    assert L.lib.cg_ngram_index_build(ctypes.byref(d), None) == L.CG_EINVAL
    d = L.NgramIndexDesc(n=10, n_seq=1, seq_hi=1, n_sym=64, capacity=128)  # NULL sym / offsets / table
    assert L.lib.cg_ngram_index_build(ctypes.byref(d), None) == L.CG_EINVAL
    d = L.NgramIndexDesc(n=10, n_seq=4, seq_lo=2, seq_hi=2, n_sym=64)  # zero work: nothing is read
    assert L.lib.cg_ngram_index_build(ctypes.byref(d), None) == L.CG_OK
    c = L.NgramCoverageDesc(n=10, n_q=0)
    assert L.lib.cg_ngram_coverage(ctypes.byref(c), None) == L.CG_OK
    c = L.NgramCoverageDesc(n=10, n_q=1, max_qlen=L.NGRAM_MAX_QUERY + 1)
    assert L.lib.cg_ngram_coverage(ctypes.byref(c), None) == L.CG_EUNSUPPORTED
    assert ops.ngram_window_count(np.array([0, 0, 9, 19, 30]), 10) == 0 + 0 + 1 + 2


def test_cli_refuses_what_it_does_not_port():
    from codonlm_amd import eval_generation_prefix as E
    ap = E.build_parser()
    for flags in (["--critic_stability"], ["--critic_guidance"], ["--ebm_guidance"], ["--target_protein", "MK"]):
        with pytest.raises(SystemExit) as exc:
            E.settings_from(ap.parse_args(["--run_dir", "r", *flags]), "r", {})
        assert "gen-prefix" in str(exc.value)
    a = ap.parse_args(["--run_dir", "r"])
    assert (a.k_list, a.temperature, a.topk, a.seed, a.ci_resamples, a.batch_size, a.max_train_audit_tokens,
            a.memorization_n_list, a.out_label) == ("1,3,5,10", 0.8, 5, 1337, 1000, 256, 10000000, "10,20", "gen_prefix")
    s = E.settings_from(a, "r", {})
    assert (s.samples, s.max_new, s.k_list, s.guidance()) == (5, 300, (1, 3, 5, 10), [])
    s = E.settings_from(ap.parse_args(["--run_dir", "r", "--preset", "quick", "--samples", "7", "--termination_bias"]), "r", {})
    assert (s.samples, s.max_new, s.guidance()) == (7, 100, ["termination_bias"])
