"""Host-side checks of multi-offset priors in batched generation that need no GPU: the new ABI,
the argument checks that come before any device work, the CLI surface and the info record."""
import ctypes as C

import pytest

import sampler_restatement as R

NEW = ("cg_xf_hist_bytes", "cg_model_prefill_hist", "cg_model_decode_ragged_hist", "cg_offset_prior_workspace",
       "cg_offset_prior_add")


def _cfg(dtype="fp32", offsets=(2, 4)):
    from codonlm_amd.engine import EngineConfig
    return EngineConfig(vocab_size=68, block_size=64, n_layer=2, n_head=4, n_embd=64, termination_aux=True,
                        multi_offset_targets=tuple(offsets), dtype=dtype)


def test_new_symbols_and_struct_mirror():
    from codonlm_amd import _lib as L
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert L.lib.cg_struct_bytes(b"cg_offset_prior") == C.sizeof(L.OffsetPrior) == 4 + 8 * 4 + 8 * 4
    assert L.lib.cg_version().decode() == "codonlm_hip 0.6 gfx950"


@pytest.mark.parametrize("dtype,elem", [("fp32", 4), ("bf16", 2)])
def test_hist_and_workspace_sizes(dtype, elem):
    from codonlm_amd import _lib as L
    cfg = _cfg(dtype).to_c()
    for B, Tmax in ((1, 1), (7, 64), (65, 33)):
        assert L.lib.cg_xf_hist_bytes(C.byref(cfg), B, Tmax) == B * Tmax * 64 * elem
        # u1 and u2 of up to 8 heads
        assert L.lib.cg_offset_prior_workspace(C.byref(cfg), B) >= 2 * 8 * B * 64 * elem
    assert L.lib.cg_xf_hist_bytes(C.byref(cfg), 0, 64) == 0
    assert L.lib.cg_xf_hist_bytes(C.byref(cfg), -3, 64) == 0
    assert L.lib.cg_offset_prior_workspace(C.byref(cfg), 0) == 0


def test_argument_checks_come_before_any_device_work():
    """Nothing here is device memory: every call must return CG_EINVAL from the checks alone."""
    from codonlm_amd import _lib as L
    m = L.Model()
    m.cfg = _cfg().to_c()
    buf = (C.c_char * 4096)()
    ptr = C.addressof(buf)
    ws = int(L.lib.cg_offset_prior_workspace(C.byref(m.cfg), 1))
    p = L.OffsetPrior()
    p.n, p.head[0], p.weight[0] = 1, 0, 0.5
    add = L.lib.cg_offset_prior_add
    ok = [C.byref(m), C.byref(p), ptr, 64, ptr, 1, ptr, 68, ptr, ws, None]
    for null_at in (0, 1, 2, 4, 6, 8):  # model, prior, hist, pos, logits, workspace
        a = list(ok)
        a[null_at] = None
        assert add(*a) == L.CG_EINVAL, null_at
    for n in (-1, 9):
        p.n = n
        assert add(*ok) == L.CG_EINVAL, n
    p.n = 2
    for head in (-1, 2, 8):  # the model has heads 0 and 1
        p.head[1] = head
        assert add(*ok) == L.CG_EINVAL, head
    p.n, p.head[1] = 1, 0
    for at, bad in ((7, 67), (9, ws - 1), (3, 0), (3, 65), (5, 0)):  # ldl < V, short ws, Tmax, B
        a = list(ok)
        a[at] = bad
        assert add(*a) == L.CG_EINVAL, (at, bad)
    m16 = L.Model()
    m16.cfg = _cfg("bf16").to_c()  # bf16 without the shadow weights
    assert add(C.byref(m16), *ok[1:]) == L.CG_EINVAL
    p.n = 0  # no heads: nothing to launch
    assert add(*ok) == L.CG_OK

    pre = L.lib.cg_model_prefill_hist
    ok = [C.byref(m), ptr, 1, 8, ptr, 64, None]
    for null_at in (0, 1, 4):
        a = list(ok)
        a[null_at] = None
        assert pre(*a) == L.CG_EINVAL, null_at
    for at, bad in ((2, 0), (3, 0), (5, 7), (5, 65)):  # B, T, Tmax < T, Tmax > block_size
        a = list(ok)
        a[at] = bad
        assert pre(*a) == L.CG_EINVAL, (at, bad)
    assert pre(*ok) == L.CG_EINVAL  # no prefill of that shape came before
    assert L.lib.cg_model_decode_ragged_hist(None, ptr, ptr, 1, ptr, 64, ptr, ptr, 4096, ptr, None, 0, ptr,
                                             None) == L.CG_EINVAL


class _Model:
    """What generate_batch reads before it launches anything (a model with offset heads)."""
    block_size, vocab_size, sep_id, termination_aux = 64, 68, 3, False
    multi_offset_targets = [2, 4]
    engine = None


def test_priors_with_logp_are_refused():
    from codonlm_amd import generate as G
    with pytest.raises(ValueError, match="with_logp"):
        G.generate_batch(_Model(), [[1]], R.STOI, R.ITOS, seed=0, max_tokens=5, multi_offset_prior_enabled=True,
                         multi_offset_prior_weights={2: 0.5}, with_logp=True)
    with pytest.raises(ValueError, match="with_logp"):  # the flag alone, as in the reference's info record
        G.generate_batch(_Model(), [[1]], R.STOI, R.ITOS, seed=0, max_tokens=5, multi_offset_prior_enabled=True,
                         with_logp=True)


def test_cli_flags_and_weight_resolution():
    from codonlm_amd import sample as S
    ap = S.build_parser()
    a = ap.parse_args(["--run_dir", "r"])
    assert (a.multi_offset_prior, a.multi_offset_prior_weights) == (False, None)
    a = ap.parse_args(["--run_dir", "r", "--multi_offset_prior", "--multi_offset_prior_weights",
                       '{"4": 0.25, "2": 0.5}'])
    assert a.multi_offset_prior is True
    w = S.resolve_offset_prior_weights(a.multi_offset_prior, a.multi_offset_prior_weights, {})
    assert w == {4: 0.25, 2: 0.5} and list(w) == [4, 2]  # the JSON's order is the heads' order
    res = S.resolve_offset_prior_weights
    assert res(False, '{"2": 1}', {"multi_offset_weights": {2: 1.0}}) is None
    assert res(True, None, {"multi_offset_weights": {"2": 0.5, 8: 1}}) == {2: 0.5, 8: 1.0}
    assert res(True, None, {"multi_offset_weights": [0.5, 0.25, 0.1], "multi_offset_targets": [2, 4]}) == \
        {2: 0.5, 4: 0.25}
    assert res(True, None, {"multi_offset_weights": [0.5]}) == {}  # no targets to zip with
    assert res(True, None, {}) == {} and res(True, None, {"multi_offset_weights": None}) == {}
    assert res(True, "", {"multi_offset_weights": {2: 1.0}}) == {2: 1.0}
    with pytest.raises(ValueError, match="multi_offset_prior_weights"):
        res(True, "{not json", {})


def test_constrained_info_lists_the_component():
    from codonlm_amd import generate as G
    rec = G.state_record(R.states_to_array([R.new_state(4, 0)])[0])
    kw = dict(target_codons=10, hard_cap=19, termination_bias_window=4, cds_only=True)
    a = G.constrained_info(rec, require_terminal_stop=True, termination_bias_enabled=True,
                           multi_offset_prior_enabled=True, **kw)
    assert a["guidance_components"] == ["termination_bias", "multi_offset_prior", "forced_terminal_stop"]
    b = G.constrained_info(rec, require_terminal_stop=False, termination_bias_enabled=False,
                           multi_offset_prior_enabled=True, **kw)
    assert b["guidance_components"] == ["multi_offset_prior"] and b["protocol"] == "guided"
    c = G.constrained_info(rec, require_terminal_stop=False, termination_bias_enabled=False, **kw)
    assert c["guidance_components"] == [] and c["protocol"] == "cds_constrained"
