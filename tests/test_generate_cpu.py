"""Host-side checks of batched generation that need no GPU: the new ABI structs, the argument
checks that come before any launch, the CLI surface and the info records."""
import ctypes

import numpy as np
import pytest

import sampler_restatement as R


def test_new_struct_mirrors_match_the_library():
    from codonlm_amd import _lib as L
    assert L.lib.cg_struct_bytes(b"cg_sample_params") == ctypes.sizeof(L.SampleParams)
    assert L.lib.cg_struct_bytes(b"cg_gen_state") == ctypes.sizeof(L.GenState) == 32
    assert L.GEN_STATE_FIELDS == R.STATE_FIELDS
    assert L.lib.cg_version().decode().split()[1] == "0.6"
    for name in ("cg_sample_step", "cg_model_prefill_ragged", "cg_model_decode_ragged", "cg_attn_decode_ragged",
                 "cg_decode_ragged_workspace_bytes"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)


def test_ragged_workspace_covers_the_decode_workspace():
    import ctypes as C
    from codonlm_amd import _lib as L
    from codonlm_amd.engine import EngineConfig
    cfg = EngineConfig(vocab_size=68, block_size=64, n_layer=2, n_head=4, n_embd=64).to_c()
    for B in (1, 65):
        base = L.lib.cg_decode_workspace_bytes(C.byref(cfg), B)
        ragged = L.lib.cg_decode_ragged_workspace_bytes(C.byref(cfg), B)
        assert ragged >= base + B * 68 * 4
    assert L.lib.cg_decode_ragged_workspace_bytes(C.byref(cfg), 0) == 0


class _Model:
    """What generate_batch reads before it launches anything."""
    block_size, vocab_size, sep_id, termination_aux = 64, 68, 3, False
    engine = None


def test_prompt_plus_cap_beyond_block_size_is_refused():
    from codonlm_amd import generate as G
    ctx = [[1] * 10, [1] * 3]
    with pytest.raises(ValueError, match="block_size"):
        G.generate_batch(_Model(), ctx, R.STOI, R.ITOS, seed=0, max_tokens=55)
    with pytest.raises(ValueError, match="block_size"):  # 3 * hard_cap = 57 tokens + 10
        G.generate_cds_constrained(_Model(), None, ctx[0], R.STOI, R.ITOS, 5, 19)
    with pytest.raises(ValueError, match="block_size"):
        G.generate_model_raw(_Model(), None, ctx[0], R.STOI, R.ITOS, 55)
    with pytest.raises(ValueError):
        G.generate_batch(_Model(), [[1], []], R.STOI, R.ITOS, seed=0, max_tokens=5)


def test_offset_priors_are_not_implemented():
    from codonlm_amd import generate as G
    with pytest.raises(NotImplementedError):
        G.generate_batch(_Model(), [[1]], R.STOI, R.ITOS, seed=0, max_tokens=5, multi_offset_prior_enabled=True)
    with pytest.raises(NotImplementedError):
        G.generate_cds_constrained(_Model(), None, [1], R.STOI, R.ITOS, 5, 10, multi_offset_prior_enabled=True,
                                   multi_offset_prior_weights={2: 0.5})


def test_token_classes_and_mask():
    from codonlm_amd import generate as G
    cls = G.token_classes(R.ITOS, R.STOI)
    assert np.array_equal(cls, R.vocab_classes(68))
    assert sorted(np.nonzero(cls & R.TOK_STOP)[0]) == R.STOP_IDS == [52, 54, 60]
    assert np.array_equal(G.cds_mask(R.ITOS), (cls & R.TOK_CODON).astype(np.uint8))
    assert G.round_seed(77, 1) != G.round_seed(77, 2) and 0 <= G.round_seed(2 ** 32 - 1, 3) < 2 ** 32


def test_cli_parser_surface():
    from codonlm_amd import sample as S
    ap = S.build_parser()
    a = ap.parse_args(["--run_dir", "runs/x"])
    assert (a.prompt, a.max_codons, a.stop_on_eos, a.stop_on_bio_stop) == ("", 300, False, False)
    assert (a.n, a.seed, a.temperature, a.topk, a.cds_only, a.dtype) == (1, 0, 1.0, 0, False, "fp32")
    a = ap.parse_args(["--run_dir", "r", "--prompt", "ATG GCT", "--max_codons", "40", "--stop_on_eos",
                       "--stop_on_bio_stop", "--n", "8", "--seed", "3", "--temperature", "0.8", "--topk", "5",
                       "--cds_only", "--dtype", "bf16"])
    assert (a.max_codons, a.stop_on_eos, a.stop_on_bio_stop, a.n, a.seed, a.topk, a.cds_only, a.dtype) == \
        (40, True, True, 8, 3, 5, True, "bf16")
    with pytest.raises(SystemExit):
        ap.parse_args([])  # --run_dir is required, as in the reference
    assert S.prompt_ids("atg gct nnn", R.STOI) == [1, R.STOI["ATG"], R.STOI["GCT"]]
    assert S.prompt_ids("", R.STOI) == [1]


def test_info_records_from_a_hand_made_state_array():
    from codonlm_amd import generate as G
    states = [R.new_state(4, 0), R.new_state(2, 2 ** 32 - 1), R.new_state(6, 7), R.new_state(1, 9)]
    states[0].update(n_tokens=12, n_codons=12, flags=R.TERMINAL_STOP | R.DONE, pos=-1, bias_steps=3, last_term_class=1)
    states[1].update(n_tokens=19, n_codons=19, flags=R.EARLY_STOP | R.CAP | R.DONE, pos=-1)
    states[2].update(n_tokens=4, n_codons=3, flags=R.EOS | R.DONE, pos=-1)
    states[3].update(n_tokens=58, n_codons=50, flags=R.CAP | R.DONE, pos=-1)
    recs = [G.state_record(r) for r in R.states_to_array(states)]
    assert recs == states  # (the uint32 stream survives the int32 column)
    kw = dict(target_codons=10, hard_cap=19, termination_bias_window=4, cds_only=True)
    a = G.constrained_info(recs[0], require_terminal_stop=True, termination_bias_enabled=True, **kw)
    assert a == {"protocol": "guided", "guidance_components": ["termination_bias", "forced_terminal_stop"],
                 "had_terminal_stop": True, "early_stop": False, "hit_hard_cap": False, "target_codons": 10,
                 "generated_codons": 12, "termination_bias_enabled": True, "termination_bias_steps": 3,
                 "termination_bias_window": 4, "last_termination_class": 1, "cds_only": True,
                 "require_terminal_stop": True, "generated_tokens": 12}
    b = G.constrained_info(recs[1], require_terminal_stop=False, termination_bias_enabled=False,
                           **dict(kw, termination_bias_window=0))
    assert (b["protocol"], b["guidance_components"], b["had_terminal_stop"], b["early_stop"], b["hit_hard_cap"],
            b["last_termination_class"]) == ("cds_constrained", [], False, True, True, None)
    c = G.constrained_info(recs[2], require_terminal_stop=False, termination_bias_enabled=False,
                           **dict(kw, cds_only=False))
    assert c["guidance_components"] == ["non_cds_tokens"] and c["protocol"] == "guided" and not c["hit_hard_cap"]
    r = G.raw_info(recs[0], 58)
    assert (r["stop_reason"], r["had_terminal_stop"], r["hit_hard_cap"], r["early_stop"]) == \
        ("biological_stop", True, False, False)
    assert G.raw_info(recs[2], 58)["stop_reason"] == "eos"
    r = G.raw_info(recs[3], 58)
    assert (r["stop_reason"], r["hit_hard_cap"], r["generated_tokens"], r["max_new_tokens"]) == \
        ("max_new_tokens", True, 58, 58)
    assert set(r) == {"protocol", "cds_only", "require_terminal_stop", "guidance_components", "had_terminal_stop",
                      "early_stop", "hit_hard_cap", "generated_codons", "generated_tokens", "max_new_tokens",
                      "stop_reason"}
