"""The prefix-generation benchmark end to end on a tiny random model (vocabulary 68, block 64, 2 layers,
n_embd 64, termination head): batching does not change a row, every metric column is the CPU function of
the row's ids, the overlap columns are the Python-set restatement's, and the CLI writes the reference's
six files, twice the same bytes.

ppl_stability is the one column that is not a function of the ids alone: it reads fp32 losses.  The
library scores all rows in length-bucketed batches, the test one sequence at a time
(score.token_logprobs); with delta = 1e-4 the fp32 logit bound of tests/test_gpu_model.py, a loss moves
by at most 2 delta, the drift last - first by 4 delta, and exp(-drift / 0.02) by a factor exp(4 delta /
0.02) - 1 < 2.1e-2; gqs carries a tenth of it on a scale of 100 (0.21).  Every other column is compared
exactly."""
import csv
import functools

import numpy as np
import pytest
import torch

import memorization_restatement as MR
from test_gen_prefix_cpu import ITOS, PROTOCOL_HEADER, SAMPLE_HEADER, STOI

pytestmark = pytest.mark.gpu
STAB_RTOL = 2.1e-2
BIAS = dict(termination_bias=True, termination_stop_bias=3.0, termination_trigger_class_max=2,
            termination_bias_window=4, require_terminal_stop=True)
SENSE = [c for c in ITOS[4:] if c not in ("TAA", "TAG", "TGA")]


def _settings(**kw):
    from codonlm_amd import gen_prefix as GP
    return GP.Settings(run_id="run", k_list=(1, 3), samples=2, max_new=20, min_aa_len=5, target_aa_len=12,
                       max_aa_len=30, ci_resamples=50, **kw)


@functools.lru_cache(maxsize=None)
def _model():
    from codonlm_amd import TinyGPT
    torch.manual_seed(5)
    m = TinyGPT(68, 64, n_layer=2, n_head=4, n_embd=64, termination_aux=True, device="cuda")
    # the tied embedding at its initial scale makes the last token its own most likely successor and the
    # samples collapse into runs of one codon; a quarter of it leaves the top-5 draw close to uniform
    m.load_state_dict({"tok_emb.weight": m.state_dict()["tok_emb.weight"].clone() * 0.25}, strict=False)
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def _genes():
    rng = np.random.default_rng(9)
    return tuple("ATG" + "".join(SENSE[int(i)] for i in rng.integers(0, len(SENSE), size=24)) + "TAA" for _ in range(3))


@functools.lru_cache(maxsize=None)
def _generated():
    """{protocol: [(ids, info)]} of the guided settings, every (gene, k, sample) in one batch."""
    from codonlm_amd import gen_prefix as GP
    s = _settings(**BIAS)
    rows = GP.plan_rows(_genes(), STOI, 64, s)
    return rows, {p: GP.generate_protocol(_model(), rows, STOI, ITOS, s, p) for p in GP.PROTOCOLS}


def _train_matrix(extra=()):
    """Training rows [R][32]: the genes' codon ids, the first 14 codons of every third generated sequence
    (partial overlaps), random rows, ``extra`` id lists; PAD (0) to the right."""
    from codonlm_amd import gen_prefix as GP
    rows, gen = _generated()
    seqs = [[STOI[g[i:i + 3]] for i in range(0, len(g), 3)] for g in _genes()]
    for p in GP.PROTOCOLS:
        for ids, _ in gen[p][::3]:
            seqs.append([STOI[c] for c in GP.codons_of(ids, ITOS)][:14])
    rng = np.random.default_rng(2)
    seqs += [rng.integers(4, 68, size=32).tolist() for _ in range(4)] + [list(e) for e in extra]
    X = np.zeros((len(seqs), 32), dtype=np.int64)
    for r, sq in enumerate(seqs):
        X[r, :len(sq)] = sq
    return X


def test_every_row_equals_its_single_call():
    from codonlm_amd import generate as G
    m = _model()
    rows, gen = _generated()
    assert len(rows) == 12 and {r.hard_cap for r in rows} == {20} and {r.target_codons for r in rows} == {12}
    n_tokens = 0
    for j, r in enumerate(rows):
        ids, info = G.generate_model_raw(m, None, r.ctx_ids, STOI, ITOS, max_new_tokens=20, temperature=0.8, topk=5,
                                         seed=1337, stream=r.seed)
        assert (ids, info) == gen["raw_model"][j], ("raw_model", j)
        ids, info = G.generate_cds_constrained(m, None, r.ctx_ids, STOI, ITOS, target_codons=12, hard_cap=20,
                                               temperature=0.8, topk=5, seed=1337, stream=r.seed)
        assert (ids, info) == gen["cds_constrained"][j], ("cds_constrained", j)
        ids, info = G.generate_cds_constrained(m, None, r.ctx_ids, STOI, ITOS, target_codons=12, hard_cap=20,
                                               require_terminal_stop=True, temperature=0.8, topk=5,
                                               termination_bias_enabled=True, termination_stop_bias=3.0,
                                               termination_trigger_class_max=2, termination_bias_window=4, seed=1337,
                                               stream=r.seed)
        assert (ids, info) == gen["guided"][j], ("guided", j)
        assert info["protocol"] == "guided" and gen["cds_constrained"][j][1]["protocol"] == "cds_constrained"
        n_tokens += len(ids) - len(r.ctx_ids)
    assert n_tokens > 12
    # the paired design: a row's protocols share (seed, stream), and two samples of a prefix differ
    assert len({tuple(g[0]) for g in gen["cds_constrained"]}) > 6


def test_metric_and_overlap_columns():
    from codonlm_amd import gen_prefix as GP, memorization as M, score
    m, s = _model(), _settings(**BIAS)
    rows, gen = _generated()
    X = _train_matrix()
    indices = {n: M.TrainIndex.from_rows(X, n) for n in (10, 20)}
    tables = {n: MR.build([r.astype(np.uint8) for r in X], n) for n in (10, 20)}
    assert indices[10].n_unique == len(tables[10]) and indices[20].n_unique == len(tables[20])
    usage = GP.UsageReference.from_lines(_genes(), ITOS, STOI)
    overlaps, stab_diff, n_stab = [], 0.0, 0
    for p in GP.PROTOCOLS:
        out, _ = GP.score_rows(m, rows, gen[p], p, _genes(), STOI, ITOS, s, usage, indices, s.guidance() if p == "guided" else [])
        for r, (ids, info), res in zip(rows, gen[p], out):
            truth_codons, truth_aa = GP.truth_of(_genes()[r.gene_idx])
            codons = [ITOS[i] for i in ids if GP.is_codon(ITOS[i])]
            cont = codons[min(r.k, len(codons)):]
            stop_score, valid_end, early = GP.score_stop_behavior(codons, len(truth_codons))
            cids = [STOI[c] for c in codons]
            stab = 1.0
            if len(cids) >= 22:
                loss = -score.token_logprobs(m, cids)
                loss[np.asarray(cids[1:]) == 0] = 0.0
                stab = GP.ppl_stability_from_losses(len(cids), loss)
                n_stab += 1
            stab_diff = max(stab_diff, abs(res.ppl_stability - stab) / stab)
            exact = dict(aa_identity=GP.aa_identity(truth_aa[r.k:], GP.aa_seq(cont)), syn_rate=GP.syn_rate(truth_codons[r.k:], cont),
                         stop_score=stop_score, valid_end=valid_end, early_stop=early, frame_integrity=GP.frame_integrity(codons),
                         no_repeat=1.0 - GP.ngram_repeat_ratio(codons, 3), usage_agree=usage.usage_agree([STOI[c] for c in cont]),
                         gen_len_codons=len(codons), protocol=p, sample_seed=r.seed, target_codons=12, max_new_tokens=20,
                         generated_tokens=len(ids) - len(r.ctx_ids), had_terminal_stop=info["had_terminal_stop"],
                         hit_hard_cap=info["hit_hard_cap"], cds_only=p != "raw_model", require_terminal_stop=p == "guided",
                         train_overlap_10=MR.fraction(np.asarray(cids, dtype=np.uint8), tables[10], 10),
                         train_overlap_20=MR.fraction(np.asarray(cids, dtype=np.uint8), tables[20], 20))
            for key, want in exact.items():
                assert getattr(res, key) == want, (p, r, key)
            assert abs(res.ppl_stability - stab) <= STAB_RTOL * stab, (p, r)
            want_gqs = GP.gqs(stop_score, exact["aa_identity"], exact["syn_rate"], stab, exact["no_repeat"],
                              exact["usage_agree"], exact["frame_integrity"])
            assert abs(res.gqs - want_gqs) <= 10.0 * STAB_RTOL * stab + 1e-9, (p, r)
            overlaps.append(res.train_overlap_10)
    print(f"ppl_stability: {n_stab} rows of 22+ codons, max relative difference batched vs single {stab_diff:.3e}")
    assert any(0.0 < o < 1.0 for o in overlaps) and any(o == 0.0 for o in overlaps)  # the audit is not vacuous
    # the batched losses against the single-sequence scorer on sequences that all reach 22 ids
    rng = np.random.default_rng(4)
    seqs = [rng.integers(4, 68, size=k).tolist() for k in (22, 40, 63)] + [[7] * 30 + [0, 9, 0, 11]]
    for ids, loss in zip(seqs, GP.stability_losses(m, seqs, batch_size=2)):
        ref = -score.token_logprobs(m, ids)
        ref[np.asarray(ids[1:]) == 0] = 0.0
        assert loss.shape == ref.shape and np.abs(loss - ref).max() <= 2e-4  # 2 delta
        assert (loss[np.asarray(ids[1:]) == 0] == 0.0).all()
    assert GP.stability_losses(m, [[5] * 21]) == [None]


def test_a_pasted_generation_is_fully_covered():
    from codonlm_amd import gen_prefix as GP, memorization as M
    rows, gen = _generated()
    ids = max((GP.codons_of(g[0], ITOS) for g in gen["cds_constrained"]), key=len)
    ids = [STOI[c] for c in ids]
    assert 10 <= len(ids) <= 32
    before = M.training_match_coverage(M.TrainIndex.from_rows(_train_matrix()[:3], 10), [ids])  # the genes alone
    after = M.training_match_coverage(M.TrainIndex.from_rows(_train_matrix(extra=[ids]), 10), [ids, ids[:9]])
    assert before[0] < 1.0 and after[0] == 1.0 and after[1] == 0.0
    # the string form of the same audit
    dna = "".join(ITOS[i] for i in ids)
    rec = M.generated_coverage([{"sequence": g} for g in _genes()] + [{"sequence": dna}],
                               [{"source_id": "g", "sequence": dna}, {"source_id": "h", "sequence": _genes()[0][:40]}],
                               nucleotide_window=30, protein_window=10)
    assert rec[0]["nucleotide_training_match_coverage"] == 1.0
    assert rec[1]["source_id"] == "h" and rec[1]["nucleotide_training_match_coverage"] == 1.0
    genes_aa = [M.translate_cds(g) for g in _genes()]
    assert M.matched_windows([genes_aa[0][3:20]], genes_aa, 10) == {genes_aa[0][s:s + 10] for s in range(3, 11)}
    assert M.matching_substring_coverage([genes_aa[1], "MK"], genes_aa[:1], 10).tolist() == [
        MR.fraction(np.frombuffer(genes_aa[1].encode(), dtype=np.uint8),
                    MR.build([np.frombuffer(genes_aa[0].encode(), dtype=np.uint8)], 10), 10), 0.0]


def test_cli_writes_the_six_files_and_repeats_them(tmp_path):
    from codonlm_amd import eval_generation_prefix as E, gen_prefix as GP, memorization as M
    m = _model()
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    cfg = dict(vocab_size=68, block_size=64, n_layer=2, n_head=4, n_embd=64, termination_loss_enabled=True,
               termination_n_classes=5)
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}, "cfg": cfg}, run / "checkpoints" / "best.pt")
    (run / "itos.txt").write_text("\n".join(ITOS) + "\n")
    (tmp_path / "cds.txt").write_text("\n".join(_genes()) + "\nATGAA\n")
    X = _train_matrix()
    np.savez(tmp_path / "train.npz", X=X, Y=X)
    argv = ["--run_dir", str(run), "--cds_file", str(tmp_path / "cds.txt"), "--train_npz", str(tmp_path / "train.npz"),
            "--k_list", "1,3", "--samples", "2", "--max_genes", "3", "--max_new", "20", "--min_aa_len", "5",
            "--target_aa_len", "12", "--max_aa_len", "30", "--ci_resamples", "50", "--batch_size", "5",
            "--termination_bias", "--termination_stop_bias", "3.0", "--termination_trigger_class_max", "2",
            "--termination_bias_window", "4", "--require_terminal_stop"]
    a = E.main(argv)
    b = E.main(argv + ["--out_label", "again"])
    names = ["samples.csv", "protocol_samples.csv", "generated_protocols.fasta", "protocol_summary.csv",
             "protocol_manifest.json", "summary.csv"]
    assert sorted(a) == sorted(names) and a["samples.csv"].parent == run / "scores" / "gen_prefix"
    for name in names:
        assert a[name].exists() and a[name].read_bytes() == b[name].read_bytes(), name
    head = lambda name: next(csv.reader(a[name].open()))  # noqa: E731
    assert head("samples.csv") == SAMPLE_HEADER and head("protocol_samples.csv") == PROTOCOL_HEADER
    assert head("summary.csv") == list(GP.SUMMARY_COLUMNS)
    assert head("protocol_summary.csv") == list(GP.PROTOCOL_SUMMARY_COLUMNS)
    prot = list(csv.DictReader(a["protocol_samples.csv"].open()))
    assert len(prot) == 36 and [r["protocol"] for r in prot[:3]] == ["raw_model", "cds_constrained", "guided"]
    assert all(r["critic_stability"] == "0.0" for r in csv.DictReader(a["samples.csv"].open()))
    # chunks of 5 rows here, one batch of 12 in _generated(): the same sequences
    rows, gen = _generated()
    fasta = a["generated_protocols.fasta"].read_text().split("\n")
    want = {}
    for p in GP.PROTOCOLS:
        for r, (ids, _) in zip(rows, gen[p]):
            want[f"{p}_gene{r.gene_idx}_k{r.k}_sample{r.sample_id}_seed{r.seed}"] = "".join(GP.codons_of(ids, ITOS))
    got = {fasta[i][1:]: fasta[i + 1] for i in range(0, len(fasta) - 1, 2)}
    assert got == {k: v for k, v in want.items() if v}
    table = MR.build([r.astype(np.uint8) for r in X], 10)
    for r in prot:
        key = f"{r['protocol']}_gene{r['gene_idx']}_k{r['k']}_sample{r['sample_id']}_seed{r['sample_seed']}"
        ids = np.array([STOI[want[key][i:i + 3]] for i in range(0, len(want[key]), 3)], dtype=np.uint8)
        assert float(r["train_overlap_10"]) == MR.fraction(ids, table, 10), key
    assert len(list(csv.DictReader(a["protocol_summary.csv"].open()))) == 6
