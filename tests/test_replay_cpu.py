"""The replay data layer without a GPU: the restated GeneratedTerminationReplayDataset and label
function against what the reference returns for tests/golden/replay_fixture.jsonl
(replay_dataset.npz, made by tests/golden/make_golden_replay.py), their error cases, and the
builder's selection and record assembly with a stub generator."""
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import load_golden

GOLDEN = Path(__file__).resolve().parent / "golden"
RECORD_KEYS = {"source_run_id", "source_ckpt", "gene_idx", "k", "sample_id", "ids", "labels", "target_codons",
               "generated_codons", "hard_cap", "decoder", "synthetic_boundary", "last_termination_class"}


def test_term_ce_abi_and_host_side_validation():
    """The new struct mirrors match the library, and the argument checks that need no launch."""
    import ctypes as C
    from codonlm_amd import _lib as L
    assert L.lib.cg_struct_bytes(b"cg_term_ce_desc") == C.sizeof(L.TermCeDesc) > 0
    assert L.lib.cg_struct_bytes(b"cg_model") == C.sizeof(L.Model)
    ws = L.lib.cg_term_ce_workspace
    assert ws(0, 64, 5) == ws(8, 0, 5) == ws(8, 64, 0) == ws(8, 64, 17) == 0
    # header, loss partials, probabilities, db and dW partials of two 64-row chunks
    assert ws(67, 6, 5) == 16 + 32 + (67 * 5 * 4 + 15) // 16 * 16 + 128 + 2 * 5 * 6 * 4
    assert ws(67, 64, 16) > ws(67, 64, 5) > ws(1, 64, 5) % 16 == 0
    p = L.TermCeDesc()
    for fn in (L.lib.cg_term_ce_fwd, L.lib.cg_term_ce_bwd):
        assert fn(None, None) == L.CG_EINVAL
        p.x_dtype, p.rows, p.d, p.C, p.ldx, p.ldw = L.CG_F32, 8, 4, 17, 4, 4
        assert fn(C.byref(p), None) == L.CG_EUNSUPPORTED
        p.C = 5
        assert fn(C.byref(p), None) == L.CG_EINVAL  # NULL operands
        p.ldx = 3
        assert fn(C.byref(p), None) == L.CG_EINVAL
        p.ldx, p.rows = 4, 0
        assert fn(C.byref(p), None) == L.CG_OK  # nothing to do, nothing touched
        p.x_dtype = L.CG_BF16X2
        assert fn(C.byref(p), None) == L.CG_EUNSUPPORTED
    m = L.Model()
    assert L.lib.cg_model_term_loss(C.byref(m), None, None, None, None) == L.CG_EINVAL
    assert L.lib.cg_model_backward_heads(C.byref(m), 0, None) == L.CG_EINVAL
    assert L.lib.cg_model_forward_trunk(C.byref(m), None, 1, 8, 0, 0, 0, None) == L.CG_EINVAL


@pytest.mark.parametrize("block", [8, 16])
def test_dataset_reproduces_the_reference(block):
    from codonlm_amd.replay import GeneratedTerminationReplayDataset
    _, g = load_golden("replay_dataset")
    ds = GeneratedTerminationReplayDataset(GOLDEN / "replay_fixture.jsonl", block, n_classes=5)
    assert len(ds) == len(g[f"x_{block}"]) == 5
    for i in range(len(ds)):
        x, y = ds[i]
        assert x.dtype == y.dtype and str(x.dtype) == "torch.int64"
        assert np.array_equal(x.numpy(), g[f"x_{block}"][i]), i
        assert np.array_equal(y.numpy(), g[f"y_{block}"][i]), i
    assert (g[f"y_{block}"] != -100).any(axis=1).all()


def test_replay_labels_reproduce_the_reference():
    from codonlm_amd.replay import replay_labels
    _, g = load_golden("replay_dataset")
    cases = json.loads(str(g["label_cases"]))
    assert len(cases) >= 8
    for i, (n, prefix, window, edges) in enumerate(cases):
        got = np.array([[d["pos"], d["class"]] for d in replay_labels(n, prefix, window, edges)],
                       dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(got, g[f"labels_{i}"]), (i, n, prefix, window, edges)
    with pytest.raises(ValueError, match="sorted"):
        replay_labels(20, 3, 5, (3, 0))


def test_dataset_errors(tmp_path):
    from codonlm_amd.replay import GeneratedTerminationReplayDataset as DS
    with pytest.raises(FileNotFoundError):
        DS(tmp_path / "missing.jsonl", 8)
    empty = tmp_path / "empty.jsonl"
    empty.write_text('{"ids": [1, 2, 3]}\n\n{"ids": [], "labels": [{"pos": 0, "class": 0}]}\n'
                     '{"ids": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], "labels": [{"pos": 0, "class": 1}]}\n')
    with pytest.raises(ValueError, match="no usable records"):
        DS(empty, 8)  # the only labelled record loses its label to the left clip
    assert len(DS(empty, 16)) == 1
    bad = tmp_path / "bad.jsonl"
    bad.write_text('{"ids": [1, 2, 3], "labels": [{"pos": 1, "class": 5}]}\n')
    assert len(DS(bad, 8)) == 1  # as the reference: no class check unless asked for
    with pytest.raises(ValueError, match=r"outside \[0, 5\)"):
        DS(bad, 8, n_classes=5)
    broken = tmp_path / "broken.jsonl"
    broken.write_text('{"ids": [1, 2\n')
    with pytest.raises(ValueError, match="invalid JSONL"):
        DS(broken, 8)
    with pytest.raises(ValueError, match="positive"):
        DS(bad, 0)


def _args(**over):
    from codonlm_amd.build_replay import build_parser
    argv = ["--run_dir", "runs/x", "--dna", "cds.txt", "--min_aa_len", "4", "--target_aa_len", "6", "--max_aa_len", "8",
            "--max_new", "8", "--k_list", "1,3", "--samples", "2", "--replay_window", "3", "--batch", "3"]
    for k, v in over.items():
        argv += [f"--{k}"] + ([] if v is True else [str(v)])
    return build_parser().parse_args(argv)


def _stub(outcomes):
    """canned generator: job stream -> (hard cap?, stop?); ids = context + hard_cap tokens"""
    calls = []

    def generate(part):
        calls.append([job["stream"] for job in part])
        assert len({(j["hard_cap"], j["target_codons"]) for j in part}) == 1
        res = []
        for job in part:
            cap, stop = outcomes[job["stream"] % len(outcomes)]
            n = job["hard_cap"] if cap else job["hard_cap"] - 2
            res.append((job["ctx"] + [10 + job["stream"]] * n,
                        {"hit_hard_cap": cap, "had_terminal_stop": stop, "generated_codons": n,
                         "last_termination_class": 2 if cap else None}))
        return res
    return generate, calls


def test_builder_selects_and_assembles_records(tmp_path):
    from codonlm_amd import build_replay as BR
    from codonlm_amd.replay import GeneratedTerminationReplayDataset
    cds = ["ATGGCTGCTGCTGCTTAA", "ATGAAATAA"]
    outcomes = [(True, False), (True, True), (False, False), (False, True)]
    generate, calls = _stub(outcomes)
    args = _args()
    out = tmp_path / "sub" / "replay.jsonl"
    summary = BR.build(args, cds, 32, lambda dna: [1] + [4] * (len(dna) // 3), generate, out, "run-x")
    jobs = 2 * 2 * 2
    assert sorted(s for c in calls for s in c) == list(range(jobs)) and max(len(c) for c in calls) <= 3
    records = [json.loads(line) for line in out.read_text().splitlines()]
    kept = [s for s in range(jobs) if outcomes[s % 4] == (True, False)]
    assert [r["ids"][-1] - 10 for r in records] == kept  # only hard cap without a stop, in job order
    for r in records:
        assert set(r) == RECORD_KEYS
        assert r["source_run_id"] == "run-x" and r["decoder"] == "cds_constrained" and r["hard_cap"] == 8
        assert r["synthetic_boundary"] == "next_token_after_failed_prefix" and r["last_termination_class"] == 2
        assert r["labels"] == BR.replay_labels(len(r["ids"]), 1 + r["k"], 3, (0, 3, 10, 30))
        assert len(r["labels"]) == 4 and r["labels"][-1] == {"pos": len(r["ids"]) - 1, "class": 0}
    assert summary == json.loads(out.with_suffix(".summary.json").read_text())
    assert "source_provenance" not in summary
    assert summary["generated_samples"] == jobs and summary["records_written"] == len(kept) == 2
    assert summary["hard_cap_without_stop"] == 2 and summary["terminal_stops"] == 4
    assert sum(summary["label_class_counts"].values()) == sum(len(r["labels"]) for r in records)
    assert set(summary["label_class_counts"]) == {"0", "1", "2", "3", "4"}
    assert len(GeneratedTerminationReplayDataset(out, 32, n_classes=5)) == 2
    # batching does not change the output
    generate1, _ = _stub(outcomes)
    out1 = tmp_path / "one.jsonl"
    BR.build(_args(batch=1), cds, 32, lambda dna: [1] + [4] * (len(dna) // 3), generate1, out1, "run-x")
    assert out1.read_text() == out.read_text()


def test_builder_without_records_exits_nonzero(tmp_path):
    from codonlm_amd import build_replay as BR
    generate, _ = _stub([(True, True), (False, False)])
    to_ids = lambda dna: [1] + [4] * (len(dna) // 3)  # noqa: E731
    with pytest.raises(SystemExit) as exc:
        BR.build(_args(), ["ATGGCTGCTTAA"], 32, to_ids, generate, tmp_path / "none.jsonl", "run-x")
    assert exc.value.code not in (0, None)
    summary = BR.build(_args(allow_empty=True), ["ATGGCTGCTTAA"], 32, to_ids, generate, tmp_path / "ok.jsonl", "run-x")
    assert summary["records_written"] == 0 and (tmp_path / "ok.jsonl").read_text() == ""
    with pytest.raises(SystemExit):
        BR.build(_args(bucket_edges="3,0"), ["ATGGCTGCTTAA"], 32, to_ids, generate, tmp_path / "e.jsonl", "run-x")
    with pytest.raises(ValueError, match="block_size too small"):
        BR.build(_args(), ["ATGGCTGCTTAA"], 8, to_ids, generate, tmp_path / "s.jsonl", "run-x")
