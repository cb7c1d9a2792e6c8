"""Host side of input attribution (cg_attr_seed, cg_attr_reduce, cg_model_input_grad and
codonlm_amd.attribution): the ABI additions, the argument checks that return before any launch,
and the batching / ordering / padding logic of the library against a stub model.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch


def test_symbols_and_struct_mirror():
    from codonlm_amd import _lib as L
    for name in ("cg_attr_seed", "cg_attr_reduce", "cg_model_input_grad"):
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert L.lib.cg_struct_bytes(b"cg_attr_desc") == ctypes.sizeof(L.AttrDesc) > 0
    assert (L.ATTR_LOGPROB, L.ATTR_LOGIT) == (0, 1)
    assert L.lib.cg_version().decode() == "codonlm_hip 0.6 gfx950"  # additions only


FAKE = 4096  # a non-NULL pointer value: every call below returns before anything reads it


def test_attr_reduce_argument_checks():
    from codonlm_amd import _lib as L
    f = L.lib.cg_attr_reduce
    ok = dict(g=FAKE, ldg=8, idx=FAKE, tok=FAKE, lde=8, V=68, x0=FAKE, ldx=8, rows=4, d=8, gxt=FAKE, gxi=FAKE,
              gnorm=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["g"], a["ldg"], a["idx"], a["tok"], a["lde"], a["V"], a["x0"], a["ldx"], a["rows"], a["d"],
                 a["gxt"], a["gxi"], a["gnorm"], None)
    assert call(g=None) == L.CG_EINVAL
    assert call(idx=None) == L.CG_EINVAL
    assert call(tok=None) == L.CG_EINVAL  # gxt asked for without the table
    assert call(x0=None) == L.CG_EINVAL   # gxi asked for without the embedding output
    assert call(ldg=7) == L.CG_EINVAL and call(lde=4) == L.CG_EINVAL and call(ldx=0) == L.CG_EINVAL
    assert call(rows=-1) == L.CG_EINVAL and call(d=0) == L.CG_EINVAL
    # rows == 0 is fine and touches nothing, whatever the pointers are
    assert call(rows=0) == L.CG_OK
    assert call(rows=0, g=None, idx=None, tok=None, x0=None) == L.CG_OK
    # nothing asked for: nothing to launch
    assert call(gxt=None, gxi=None, gnorm=None, tok=None, x0=None) == L.CG_OK


def test_attr_seed_argument_checks():
    from codonlm_amd import _lib as L
    f = L.lib.cg_attr_seed

    def call(logits=FAKE, ldl=80, y=FAKE, w=None, rows=4, V=68, mode=L.ATTR_LOGPROB, dt=L.CG_F32, d=FAKE, ldd=80):
        return f(logits, ldl, y, w, rows, V, mode, dt, d, ldd, None)
    assert call(y=None) == L.CG_EINVAL and call(d=None) == L.CG_EINVAL
    assert call(logits=None) == L.CG_EINVAL  # the softmax needs the logits
    assert call(mode=2) == L.CG_EINVAL and call(mode=-1) == L.CG_EINVAL
    assert call(ldl=67) == L.CG_EINVAL and call(ldd=67) == L.CG_EINVAL
    assert call(dt=L.CG_BF16X2, ldd=135) == L.CG_EINVAL  # odd: no two halves
    assert call(dt=L.CG_BF16X2, ldd=134) == L.CG_EINVAL  # halves narrower than V
    assert call(dt=L.CG_BF16) == L.CG_EUNSUPPORTED
    assert call(rows=-1) == L.CG_EINVAL and call(V=0) == L.CG_EINVAL
    assert call(rows=0) == L.CG_OK and call(rows=0, logits=None, y=None, d=None) == L.CG_OK


def test_model_input_grad_argument_checks():
    from codonlm_amd import _lib as L
    from codonlm_amd.engine import EngineConfig
    f = L.lib.cg_model_input_grad
    a = L.AttrDesc()
    assert f(None, ctypes.byref(a), None) == L.CG_EINVAL
    m = L.Model()
    m.cfg = EngineConfig(vocab_size=68, block_size=64, n_layer=2, n_head=2, n_embd=128).to_c()
    assert f(ctypes.byref(m), None, None) == L.CG_EINVAL
    assert f(ctypes.byref(m), ctypes.byref(a), None) == L.CG_EINVAL  # no forward has run
    m.idx, m.B, m.T = FAKE, 2, 8
    m.training = 1
    a.y = FAKE
    assert f(ctypes.byref(m), ctypes.byref(a), None) == L.CG_EINVAL  # a training forward
    m.training = 0
    a.y = None
    assert f(ctypes.byref(m), ctypes.byref(a), None) == L.CG_EINVAL  # the loss seed needs the forward's targets
    a.y, a.mode = FAKE, 2
    assert f(ctypes.byref(m), ctypes.byref(a), None) == L.CG_EINVAL  # unknown mode
    a.mode, a.dx0, a.ld_dx0 = L.ATTR_LOGIT, FAKE, 64
    assert f(ctypes.byref(m), ctypes.byref(a), None) == L.CG_EINVAL  # dx0 rows narrower than n_embd
    # the backward state of the model is not touched by a refused call
    assert (m.head_dw_pending, m.dw_done_layer, m.reduce_pending.n) == (0, 0, 0)


# ------------------------------------------------------------------ the library against a stub model
class StubEngine:
    """Records every forward / input_grad and answers with values that encode (token, position):
    gxt = 100 token + position, gxi = the seeded class (or -1), gnorm = the row's index in its batch."""

    def __init__(self):
        self.calls = []

    def forward(self, x, targets, *, training):
        assert training is False and x.dtype == torch.int64 and x.dim() == 2
        self.x, self.targets = x, targets
        return None, None

    def input_grad(self, y=None, w=None, mode="logprob", want=("gxt", "gxi", "gnorm"), dx0=False):
        from codonlm_amd import ops
        B, T = self.x.shape
        if y is not None:
            assert y.shape == (B, T) and y.dtype == torch.int64
        self.calls.append({"x": self.x.clone(), "targets": self.targets, "y": None if y is None else y.clone(),
                           "mode": mode, "want": tuple(want)})
        r = ops.AttrResult()
        pos = torch.arange(T, dtype=torch.float32)[None].expand(B, T)
        vals = {"gxt": self.x.float() * 100 + pos,
                "gxi": (y if y is not None else torch.full((B, T), -1)).float(),
                "gnorm": torch.arange(B, dtype=torch.float32)[:, None].expand(B, T).clone()}
        for k in want:
            setattr(r, k, vals[k])
        return r


class StubModel:
    block_size = 16

    def __init__(self):
        self.engine = StubEngine()
        self._flat = torch.zeros(1)

    def flat_parameters(self):
        return self._flat


def _seqs():
    rng = np.random.default_rng(4)
    return [[1] + rng.integers(4, 68, size=n - 2).tolist() + [2] for n in (5, 2, 17, 9, 9, 3, 12)]


def test_plan_batches_pads_inputs_with_pad_and_targets_with_minus_one():
    from codonlm_amd import attribution as A
    from codonlm_amd import score as S
    seqs = _seqs()
    for bs in (1, 3, 32):
        plan = A.plan_batches(seqs, bs, 17)
        assert [b for b, _, _ in plan] == [list(b) for b in S.batch_order([len(s) for s in seqs], bs)]
        assert sorted(i for b, _, _ in plan for i in b) == list(range(len(seqs)))
        for b, x, y in plan:
            T = max(len(seqs[i]) for i in b) - 1
            assert x.shape == y.shape == (len(b), T) and x.dtype == y.dtype == np.int64 and len(b) <= bs
            for j, i in enumerate(b):
                n = len(seqs[i]) - 1
                assert x[j, :n].tolist() == seqs[i][:-1] and y[j, :n].tolist() == seqs[i][1:]
                assert (x[j, n:] == 0).all() and (y[j, n:] == -1).all()
    with pytest.raises(ValueError, match="block_size"):
        A.plan_batches(seqs, 4, 16)  # the 17-token sequence needs block_size 16
    with pytest.raises(ValueError, match="two tokens"):
        A.plan_batches([[1]], 4, 17)


def test_saliency_scatters_batches_back_to_input_order():
    from codonlm_amd import attribution as A
    seqs = _seqs()
    for bs in (1, 3, 32):
        m = StubModel()
        res = A.saliency(m, seqs, batch_size=bs)
        assert len(res) == len(seqs)
        for ids, r in zip(seqs, res):
            n = len(ids) - 1
            assert sorted(r) == ["gnorm", "gxi", "gxt"] and all(r[k].shape == (n,) for k in r)
            assert r["gxt"].tolist() == [100.0 * t + i for i, t in enumerate(ids[:-1])]
            assert r["gxi"].tolist() == [float(t) for t in ids[1:]]  # every real target seeded with its own class
        for c in m.engine.calls:
            assert c["mode"] == "logprob" and c["targets"] is None
            assert ((c["y"] == -1) == (c["x"] == 0)).all()  # the pad rows, and only they, seed nothing
    assert A.saliency(StubModel(), []) == []
    with pytest.raises(ValueError, match="objective"):
        A.saliency(StubModel(), seqs, objective="nll")
    with pytest.raises(ValueError, match="block_size"):
        A.saliency(StubModel(), [[1] + [5] * 16 + [2]])
    with pytest.raises(ValueError, match="block_size"):
        A.saliency(StubModel(), [[1] + [5] * 16 + [2]], objective="loss")


def test_loss_objective_runs_every_sequence_as_its_own_batch():
    from codonlm_amd import attribution as A
    seqs = _seqs()[:4]
    m = StubModel()
    res = A.saliency(m, seqs, objective="loss")
    assert len(m.engine.calls) == len(seqs)
    for ids, c, r in zip(seqs, m.engine.calls, res):
        assert c["y"] is None  # the forward's own loss is the seed
        assert c["x"].tolist() == [ids[:-1]] and c["targets"].tolist() == [ids[1:]]
        assert r["gxt"].tolist() == [100.0 * t + i for i, t in enumerate(ids[:-1])]
    with pytest.raises(ValueError, match="one target per input"):
        A.loss_saliency(m, [1, 5, 6], [5, 6])


def test_target_attribution_replicates_the_sequence_with_one_seed_per_row():
    from codonlm_amd import attribution as A
    ids = _seqs()[6]  # 12 tokens: 11 input positions
    m = StubModel()
    pos, cls = [7, 0, 10, 3, 3], [9, 8, 7, 6, 67]
    out = A.target_attribution(m, ids, pos, cls, mode="logit", batch_size=2)
    assert out.shape == (5, 11) and out.dtype == np.float32
    chunks = [(pos[s:s + 2], cls[s:s + 2]) for s in (0, 2, 4)]
    assert len(m.engine.calls) == 3
    row = 0
    for (p, c), call in zip(chunks, m.engine.calls):
        T = max(p) + 1  # the forward stops at the chunk's last seeded position
        assert call["mode"] == "logit" and call["want"] == ("gxt",)
        assert call["x"].tolist() == [ids[:T]] * len(p)
        y = np.full((len(p), T), -1)
        y[np.arange(len(p)), p] = c
        assert call["y"].tolist() == y.tolist()
        for _ in p:
            assert out[row, :T].tolist() == [100.0 * t + i for i, t in enumerate(ids[:T])]
            assert (out[row, T:] == 0).all()
            row += 1
    # the default class is the actual next token
    m = StubModel()
    A.target_attribution(m, ids, [4, 9])
    y = m.engine.calls[0]["y"]
    assert y[0, 4] == ids[5] and y[1, 9] == ids[10] and int((y != -1).sum()) == 2
    assert A.target_attribution(StubModel(), ids, []).shape == (0, 11)
    for bad in ([11], [-1]):
        with pytest.raises(ValueError, match="target positions"):
            A.target_attribution(StubModel(), ids, bad)
    with pytest.raises(ValueError, match="one class per"):
        A.target_attribution(StubModel(), ids, [1, 2], [5])
    with pytest.raises(ValueError, match="mode"):
        A.target_attribution(StubModel(), ids, [1], mode="prob")
    with pytest.raises(ValueError, match="block_size"):
        A.target_attribution(StubModel(), [1] + [5] * 16 + [2], [1])


def test_dependency_map_seeds_every_target_once():
    from codonlm_amd import attribution as A
    ids = _seqs()[3]  # 9 tokens: 8 targets
    for bs in (3, 1, 32):
        m = StubModel()
        dep = A.dependency_map(m, ids, value="gxi", batch_size=bs)
        assert dep.shape == (8, 8)
        assert len(m.engine.calls) == -(-8 // bs)
        # gxi of the stub = the seed matrix itself: class ids[t + 1] at (t, t), -1 inside the forward
        for t in range(8):
            assert dep[t, t] == ids[t + 1]
        assert all(c["want"] == ("gxi",) and c["mode"] == "logprob" for c in m.engine.calls)
    with pytest.raises(ValueError, match="value"):
        A.dependency_map(StubModel(), ids, value="grad")
    with pytest.raises(ValueError, match="two tokens"):
        A.dependency_map(StubModel(), [1])


def test_csv_rows_layout():
    from codonlm_amd import analyze_saliency as C
    from codonlm_amd import score as S
    rows = C.csv_rows([1, 4, 67, 70], S.DEFAULT_VOCAB, np.array([0.1234567, -2.0, 1e-7, 3.5], np.float32))
    assert rows[0] == ["position", "token", "saliency"]
    assert rows[1:] == [[0, "<BOS_CDS>", "0.123457"], [1, "AAA", "-2.000000"], [2, "TTT", "0.000000"],
                        [3, "tok_70", "3.500000"]]
    ap = C.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args([])  # --run_dir is required
    a = ap.parse_args(["--run_dir", "r"])
    assert a.dna is None and a.map is None and a.dtype == "fp32"


def test_run_sequence_reads_the_first_validation_row(tmp_path):
    from codonlm_amd import analyze_saliency as C
    X = np.arange(12, dtype=np.int32).reshape(2, 6)
    np.savez(tmp_path / "artifacts.npz", val_inputs=X)
    x, y = C.run_sequence(tmp_path)
    assert x.tolist() == [0, 1, 2, 3, 4, 5] and y.tolist() == [1, 2, 3, 4, 5, 0] and x.dtype == np.int64
    np.savez(tmp_path / "artifacts.npz", val_inputs=X, val_targets=X + 1)
    assert C.run_sequence(tmp_path)[1].tolist() == [1, 2, 3, 4, 5, 6]
    np.savez(tmp_path / "artifacts.npz", other=X)
    with pytest.raises(ValueError, match="validation inputs"):
        C.run_sequence(tmp_path)
    with pytest.raises(FileNotFoundError):
        C.run_sequence(tmp_path / "none")
