"""CPU-side checks of the attention head analysis: the fp64 restatement of cg_attn_stats
(tests/attention_restatement.py) against the reference's own head statistics
(tests/golden/attention_heads.npz), the ABI mirror, and the host side of codonlm_amd.attention and
the analyze_attention CLI on fabricated statistics.  No GPU."""
import csv
import ctypes

import numpy as np
import pytest

import attention_restatement as AR

CLS = AR.token_classes(AR.ITOS)


@pytest.mark.parametrize("T", AR.GOLDEN_SHAPES)
def test_restatement_triple_equals_the_reference_head_stats(golden, T):
    """conference_attention._head_stats of the restatement's attention tensor (run in the build
    container, one call per batch row) = the triple taken from the restatement's fused row sums,
    within 1e-7: the reference adds 1e-12 inside its log and reads the tensor as fp32."""
    _, g = golden("attention_heads")
    idx, P = AR.golden_case(T)
    assert np.array_equal(g[f"T{T}/tokens"], idx)
    assert g[f"T{T}/attn"].shape == (AR.GOLDEN_L, AR.GOLDEN_B, AR.GOLDEN_H, T, T)
    assert np.abs(g[f"T{T}/attn"] - P).max() <= 1e-7
    want = g[f"T{T}/head_stats"]                       # (B, L, H, 3)
    assert want.shape == (AR.GOLDEN_B, AR.GOLDEN_L, AR.GOLDEN_H, 3)
    m = AR.attention_mask(idx, AR.GOLDEN_B, T, sep_id=AR.SEP)
    seen = np.zeros(3, bool)
    for layer in range(AR.GOLDEN_L):
        rows = AR.stats_from_probs(P[layer], m, idx=idx, pad_id=-1, tok_class=CLS)["rows"]
        for b in range(AR.GOLDEN_B):
            got = AR.reference_triple(rows[b], idx[b], CLS)
            assert np.abs(got - want[b, layer]).max() <= 1e-7, (T, layer, b)
            seen |= (want[b, layer] != 0).any(0)
    assert seen[0] and (T < 12 or seen.all())          # start and stop columns exist in the long case


@pytest.mark.parametrize("T,B,masked", [(1, 1, True), (5, 2, True), (130, 3, True), (130, 2, False)])
def test_restatement_masses_and_bins_sum_to_one(T, B, masked):
    H, KV, hd = 4, 2, 8
    idx = AR.make_tokens(B, T)
    r = AR.attn_stats(AR.make_qkv(B, T, H, KV, hd), B, T, H, KV, hd, idx=idx, sep_id=AR.SEP if masked else None,
                      window=70 if masked else 0, pad_id=AR.PAD, tok_class=CLS)
    rows, keep = r["rows"], r["keep"]
    k = np.broadcast_to(keep[:, None, :], rows.shape[:3])
    assert np.abs(rows[..., AR.MASS0:AR.MASS0 + 4].sum(-1) - 1)[k].max() <= 1e-12
    assert np.abs(rows[..., AR.DIST0:AR.DIST0 + 5].sum(-1) - 1)[k].max() <= 1e-12
    assert (rows[~np.broadcast_to(keep[:, None, :, None], rows.shape)] == 0).all()
    assert np.abs(r["received"].sum(-1) - keep.sum(1)[:, None]).max() <= 1e-9
    assert np.abs(r["head_acc"] - rows.sum((0, 2))).max() == 0 and r["n_rows"] == keep.sum()
    # a row whose only visible key is itself: entropy 0, all mass at distance 0 and on the sink
    one = (r["nvis"] == 1) & keep
    assert one.any()
    sel = np.broadcast_to(one[:, None, :], rows.shape[:3])
    assert (rows[..., AR.ENTROPY][sel] == 0).all() and (rows[..., AR.NORM_ENTROPY][sel] == 0).all()
    assert (rows[..., AR.DIST0][sel] == 1).all() and (rows[..., AR.FIRST][sel] == 1).all()
    if masked and T >= 130:
        x = idx[0]
        assert x[0] == AR.SEP and AR.SEP in (x[63], x[64]) and AR.SEP in (x[127], x[128]) and (x[2:4] == AR.SEP).all()
        assert (idx[1:, -1] == AR.PAD).all() and set(CLS[idx.reshape(-1)]) == {0, 1, 2, 3}
        assert r["nvis"].max() <= 70


def test_abi_mirror_and_host_side_refusals():
    from codonlm_amd import _lib as L
    assert L.lib.cg_struct_bytes(b"cg_attn_stats_desc") == ctypes.sizeof(L.AttnStatsDesc) > 0
    assert L.AS_NSTAT == len(L.AS_STATS) == AR.NSTAT and L.AS_STATS == AR.STATS
    assert (L.AS_MASS_SPECIAL, L.AS_DIST_0, L.AS_MEAN_DIST, L.AS_MAX_PROB, L.AS_FIRST) == \
        (AR.MASS0, AR.DIST0, AR.MEAN_DIST, AR.MAX_PROB, AR.FIRST)
    # [B H nqt][14] + [B nqt] doubles, then [B H nqt][T] floats; 128 queries per tile
    assert L.lib.cg_attn_stats_workspace(3, 300, 4) == 8 * (3 * 4 * 3 * 14 + 3 * 3) + 4 * 3 * 4 * 3 * 300
    assert L.lib.cg_attn_stats_workspace(0, 300, 4) == 0
    d = L.AttnStatsDesc(B=0, T=5, H=4, KV=2, hd=8)
    assert L.lib.cg_attn_stats(ctypes.byref(d), None) == L.CG_OK                 # empty: nothing to do
    d = L.AttnStatsDesc(B=1, T=5, H=4, KV=3, hd=8)
    assert L.lib.cg_attn_stats(ctypes.byref(d), None) == L.CG_EINVAL             # H % KV
    d = L.AttnStatsDesc(B=1, T=5, H=4, KV=2, hd=65, dtype=L.CG_F32)
    assert L.lib.cg_attn_stats(ctypes.byref(d), None) == L.CG_EUNSUPPORTED       # hd > 64
    d = L.AttnStatsDesc(B=1, T=5, H=4, KV=2, hd=8, dtype=L.CG_F32)
    assert L.lib.cg_attn_stats(ctypes.byref(d), None) == L.CG_EINVAL             # NULL qkv
    assert L.lib.cg_model_attn_stats(None, 0, ctypes.byref(d), None) == L.CG_EINVAL


def _fabricated(L_=3, H=4, n=10):
    from codonlm_amd import attention as A
    rng = np.random.default_rng(0)
    sums = rng.random((L_, H, len(A.STATS))) * n
    return A, A.HeadStats(sums, n)


def test_specialists_order_and_ties():
    A, st = _fabricated()
    ent, start = A.STATS.index("entropy"), A.STATS.index("mass_start")
    st.sums[:, :, ent] = 5.0
    st.sums[2, 1, ent] = st.sums[0, 3, ent] = 1.0        # a tie for the most focused head
    st.sums[1, 0, ent] = 2.0
    st.sums[:, :, start] = 0.0
    st.sums[1, 2, start] = 9.0
    sp = A.specialists(st, k=4)
    assert set(sp) == {"most_focused", "start_specialist", "stop_specialist", "self_attention", "sink"}
    assert [(l, h) for l, h, _ in sp["most_focused"]] == [(0, 3), (2, 1), (1, 0), (0, 0)]   # ties in (layer, head) order
    assert sp["most_focused"][0][2] == pytest.approx(0.1)
    assert sp["start_specialist"][0] == (1, 2, pytest.approx(0.9))
    assert [(l, h) for l, h, _ in sp["start_specialist"][1:]] == [(0, 0), (0, 1), (0, 2)]
    vals = [v for _, _, v in sp["sink"]]
    assert vals == sorted(vals, reverse=True) and len(vals) == 4
    assert len(A.specialists(st, k=100)["sink"]) == 12 and A.specialists(st, k=0)["sink"] == []
    assert A.HeadStats(np.zeros((1, 1, 14)), 0).means.sum() == 0       # no rows: no division by zero


def test_triple_from_sums_matches_the_restatement():
    from codonlm_amd import attention as A
    T = 64
    idx, P = AR.golden_case(T)
    m = AR.attention_mask(idx, AR.GOLDEN_B, T, sep_id=AR.SEP)
    rows = AR.stats_from_probs(P[0], m, idx=idx, pad_id=-1, tok_class=CLS)["rows"]
    got = A.triple_from_sums(rows[1].sum(1), idx[1], CLS)
    assert np.abs(got - AR.reference_triple(rows[1], idx[1], CLS)).max() <= 1e-14
    no_start = np.where(CLS[idx[1]] == 1, 9, idx[1])
    assert (A.triple_from_sums(rows[1].sum(1), no_start, CLS)[:, 1] == 0).all()


def test_writers_and_cli_argument_errors(tmp_path):
    from codonlm_amd import analyze_attention as C
    A, st = _fabricated()
    rows = C.csv_rows(st)
    assert rows[0] == ["layer", "head"] + list(A.STATS) and len(rows) == 1 + 3 * 4
    assert rows[6][:2] == [1, 1] and rows[6][2] == f"{st.means[1, 1, 0]:.6f}"
    text = C.report_markdown(st, k=3)
    assert text.startswith("# Attention Head Analysis\n") and text.count("## ") == 5
    assert "## most_focused (mean entropy)" in text and text.count("\n| 1 | ") == 5 and "\n| 4 | " not in text
    out = C.write_outputs(tmp_path / "run", st, np.zeros((3, 4, 3)))
    with out["csv"].open(newline="") as f:
        assert list(csv.reader(f)) == [[str(c) for c in r] for r in rows]
    with np.load(out["npz"]) as z:
        assert set(z.files) == {"sums", "n_rows", "means", "stats", "reference_row0"}
        assert np.array_equal(z["sums"], st.sums) and int(z["n_rows"]) == 10 and z["reference_row0"].shape == (3, 4, 3)
    assert out["report"].read_text() == C.report_markdown(st)
    parse = C.build_parser().parse_args
    for bad in (["--n_seqs", "0"], ["--batch", "0"], ["--window", "0"], ["--maps", "-1"], ["--max_tokens", "0"]):
        with pytest.raises(ValueError):
            C.check_args(parse(["--run_dir", "r"] + bad))
    C.check_args(parse(["--run_dir", "r", "--maps", "2", "--window", "8", "--dtype", "bf16"]))
    with pytest.raises(SystemExit):
        parse(["--run_dir", "r", "--dtype", "fp16"])
    with pytest.raises(FileNotFoundError):
        C.load_inputs(tmp_path, None, None)
    np.savez(tmp_path / "x.npz", Y=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="'X'"):
        C.load_inputs(tmp_path, tmp_path / "x.npz", None)
    np.savez(tmp_path / "artifacts.npz", val_inputs=np.arange(12).reshape(4, 3))
    assert C.load_inputs(tmp_path, None, 2).tolist() == [[0, 1, 2], [3, 4, 5]]
