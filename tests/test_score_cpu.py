"""Host side of batched scoring (codonlm_amd.score and its two CLIs): ABI additions, tokenisation,
batch order, TSV layout, argument checks and the sliding-window construction.  No GPU needed."""
import argparse
import ctypes
import io
import csv

import numpy as np
import pytest
import torch


def test_score_desc_mirror_and_workspace_query():
    from codonlm_amd import _lib as L
    assert L.lib.cg_struct_bytes(b"cg_score_desc") == ctypes.sizeof(L.ScoreDesc) > 0
    sizes = [int(L.lib.cg_score_workspace(r)) for r in (0, 1, 3, 4, 5, 64, 16384, 16387, 70001, 1 << 20)]
    assert sizes[0] > 0
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= (1 << 20) * 8  # an fp64 slot per row for the sequence sums
    assert {"cg_score_rows", "cg_score_workspace"} <= set(L.SIGNATURES)


def test_version_string_is_unchanged():
    from codonlm_amd import _lib as L
    assert L.lib.cg_version().decode() == "codonlm_hip 0.6 gfx950"


def test_tokenisation():
    from codonlm_amd import score as S
    stoi = {t: i for i, t in enumerate(S.DEFAULT_VOCAB)}
    assert len(S.DEFAULT_VOCAB) == 68 and S.CODONS[0] == "AAA" and S.CODONS[1] == "AAC" and S.CODONS[-1] == "TTT"
    # aug AAA nnn ccg UGA -> ATG AAA NNN CCG TGA: the unknown NNN is dropped, U reads as T
    assert S.dna_to_ids(" augAAAnnnccgUGA\n", stoi) == [1, stoi["ATG"], stoi["AAA"], stoi["CCG"], stoi["TGA"], 2]
    assert S.dna_to_ids("ATGAA", stoi) == [1, stoi["ATG"], 2]  # the partial codon is dropped
    assert S.dna_to_ids("", stoi) == [1, 2]
    small = {t: i for i, t in enumerate(t for t in S.DEFAULT_VOCAB if t != "CCC")}
    ids = S.codon_ids(small)
    assert len(ids) == 64 and ids[S.CODONS.index("CCC")] == -1 and sorted(i for i in ids if i >= 0) == list(range(4, 67))
    assert S.dna_to_ids("ATGCCCTAA", small) == [1, small["ATG"], small["TAA"], 2]


def test_batches_cover_every_sequence_once_in_length_buckets():
    from codonlm_amd import score as S
    rng = np.random.default_rng(0)
    lengths = rng.integers(1, 64, size=37)
    for bs in (1, 3, 8, 64):
        batches = S.batch_order(lengths, bs)
        flat = [i for b in batches for i in b]
        assert sorted(flat) == list(range(37)) and all(1 <= len(b) <= bs for b in batches)
        # scattering per-batch results by index restores input order
        out = [None] * 37
        for b in batches:
            for i in b:
                out[i] = int(lengths[i])
        assert out == [int(v) for v in lengths]
    # bucketed by length: a batch never spans more than one eighth of the length range (+1)
    width = (lengths.max() + 1 - lengths.min()) / 8
    for b in S.batch_order(lengths, 8):
        assert lengths[b].max() - lengths[b].min() <= width + 1
    assert S.batch_order(np.array([5, 5, 5]), 2) == [[0, 1], [2]]


def test_tsv_layout():
    from codonlm_amd import score as S
    from codonlm_amd import score_mutations as M
    itos = S.DEFAULT_VOCAB
    stoi = {t: i for i, t in enumerate(itos)}
    ids = S.dna_to_ids("ATGAAATAA", stoi)
    deltas = np.zeros((3, 64), np.float32)
    deltas[0, 0], deltas[0, 1], deltas[1, 5], deltas[2, 63] = -1.23456, 0.00004, -np.inf, 2.5
    rows = M.tsv_rows(ids, itos, deltas)
    assert rows[0] == ["pos", "wt"] + S.CODONS and len(rows) == 4
    assert [r[:2] for r in rows[1:]] == [[1, "ATG"], [2, "AAA"], [3, "TAA"]]
    assert rows[1][2:4] == ["-1.2346", "0.0000"] and rows[2][7] == "-inf" and rows[3][-1] == "2.5000"
    buf = io.StringIO()
    csv.writer(buf, delimiter="\t").writerows(rows)
    lines = buf.getvalue().split("\r\n")
    assert lines[0] == "pos\twt\t" + "\t".join(S.CODONS) and lines[1].startswith("1\tATG\t-1.2346\t0.0000\t")


def test_score_mutations_arguments(tmp_path, monkeypatch):
    from codonlm_amd import score_mutations as M
    ap = M.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--dna", "ATG"])  # neither --ckpt nor --run_dir
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt", "a.pt", "--run_dir", "r", "--dna", "ATG"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt", "a.pt"])  # --dna is required
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt", "a.pt", "--dna", "ATG", "--dtype", "fp16"])
    a = ap.parse_args(["--ckpt", "a.pt", "--dna", "ATG"])
    assert a.dtype == "fp32" and a.out is None
    # --dna: a short ACGTU string is the sequence itself, anything else names a file (raw or FASTA)
    assert M.read_dna("augTAA") == "augTAA"
    f = tmp_path / "one.fasta"
    f.write_text(">cds 1\nATGAAA\nCCCTAA\n")
    assert M.read_dna(str(f)) == "ATGAAACCCTAA"
    raw = tmp_path / "raw.txt"
    raw.write_text("ATGAAATAA\n")
    assert M.read_dna(str(raw)) == "ATGAAATAA"
    monkeypatch.delenv("RUN_ID", raising=False)
    assert M.default_output(str(raw), tmp_path / "best.pt").as_posix() == "outputs/scores/raw__best.tsv"
    monkeypatch.setenv("RUN_ID", "r7")
    assert M.default_output(str(raw), tmp_path / "best.pt").as_posix() == "outputs/scores/r7/raw__best.tsv"
    # the vocabulary: the run's itos.txt, else the tokenizer's fixed one
    (tmp_path / "itos.txt").write_text("<PAD>\n<BOS_CDS>\n<EOS_CDS>\n<SEP>\nAAA\n")
    assert M.load_vocab(None, tmp_path) == ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>", "AAA"]
    assert len(M.load_vocab(tmp_path / "x" / "y" / "best.pt", None)) == 68


def test_evaluate_test_arguments(tmp_path):
    from codonlm_amd import evaluate_test as E
    ap = E.build_parser()
    assert E.check_args(ap.parse_args(["--run_dir", "r"])) == "test"
    assert E.check_args(ap.parse_args(["--run_dir", "r", "--split", "validation"])) == "validation"
    assert E.check_args(ap.parse_args(["--run_dir", "r", "--metric-prefix", "ctrl_2"])) == "ctrl_2"
    with pytest.raises(ValueError, match="metric-prefix"):
        E.check_args(ap.parse_args(["--run_dir", "r", "--metric-prefix", "a-b"]))
    with pytest.raises(ValueError, match="--test_npz cannot be used with --split validation"):
        E.check_args(ap.parse_args(["--run_dir", "r", "--split", "validation", "--test_npz", "x.npz"]))
    with pytest.raises(ValueError, match="derived_provenance is not supported"):
        E.check_args(ap.parse_args(["--run_dir", "r", "--derived_provenance", "p.json"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--run_dir", "r", "--split", "train"])
    with pytest.raises(ValueError, match="either"):
        E.resolve_run(None, None)
    (tmp_path / "runA" / "checkpoints").mkdir(parents=True)
    assert E.resolve_run("other", str(tmp_path / "runA" / "checkpoints")) == ("runA", tmp_path / "runA")
    with pytest.raises(FileNotFoundError):
        E.resolve_run(None, str(tmp_path / "missing"))
    # dataset discovery
    cfg = {"block_size": 64}
    assert E.find_test_npz("r", cfg, tmp_path, tmp_path / "d") == tmp_path / "d" / "test_bs64.npz"
    assert E.find_test_npz("r", dict(cfg, test_npz=["a/t.npz", "b.npz"]), tmp_path, None) == tmp_path / "a/t.npz"
    assert E.find_test_npz("r", cfg, tmp_path, None) == tmp_path / "data/processed/test_bs64.npz"
    with pytest.raises(ValueError, match="val_npz"):
        E.find_validation_npz(cfg, tmp_path)
    assert E.find_validation_npz(dict(cfg, val_npz="/abs/v.npz"), tmp_path).as_posix() == "/abs/v.npz"
    # metrics merge keeps foreign keys and overwrites its own
    p = tmp_path / "scores" / "metrics.json"
    E.merge_metrics(p, {"a": 1, "test_nll": 2.0})
    merged = E.merge_metrics(p, {"test_nll": 3.0})
    import json
    assert merged == {"a": 1, "test_nll": 3.0} == json.loads(p.read_text())


@pytest.mark.parametrize("T,block", [(2, 8), (8, 8), (9, 8), (10, 8), (17, 8), (30, 4), (73, 64)])
def test_sliding_windows_match_the_literal_loop(T, block):
    """Every context of the streaming rule -- for t in 1..T-1: x[max(0, t - block):t] -- is a row
    prefix of `head` (t <= block) or the window block + 1 + j = t."""
    from codonlm_amd import score as S
    x = torch.arange(100, 100 + T)
    head, wins = S.sliding_windows(x, block)
    assert wins.shape == (max(0, T - 1 - block), block) and head.numel() == min(T - 1, block)
    for t in range(1, T):
        s = max(0, t - block)
        ctx = x[s:t]
        if t <= block:
            assert torch.equal(head[:t], ctx)  # row t - 1 of the head forward sees exactly ctx
        else:
            assert torch.equal(wins[t - block - 1], ctx)
    if T == 73:
        assert wins.shape[0] == 8  # with the head, the 9 full-length windows of a 73-token input
