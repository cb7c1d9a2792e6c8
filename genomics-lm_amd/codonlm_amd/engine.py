"""Host side of the whole-model engine (cg_model_* in include/codonlm_hip.h).

Owns the device buffers of one TinyGPT instance:
  * ``flat``   -- fp32 master parameters in the library's flat layout
                  (cg_model_param_layout); nn.Parameters are views into it,
  * ``grads``  -- fp32 gradients, same layout (param.grad views),
  * ``shadow`` -- bf16 copy of ``flat`` read by the bf16 MFMA GEMMs,
  * ``workspace`` -- activations saved for backward + backward scratch, sized per (B, T).
The per-step sequence of kernels is issued by the native engine (engine.cpp); Python
only makes one call per phase.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib as L


@dataclass(frozen=True)
class EngineConfig:
    vocab_size: int
    block_size: int
    n_layer: int
    n_head: int
    n_embd: int
    n_kv_head: int | None = None
    use_swiglu: bool = False
    use_rope: bool = False
    sep_id: int | None = 3
    tie_embeddings: bool = True
    termination_aux: bool = False
    termination_n_classes: int = 5
    multi_offset_targets: tuple = ()
    dropout: float = 0.0
    label_smoothing: float = 0.0
    ln_eps: float = 1e-5
    dtype: str = "fp32"  # "fp32" (parity) | "bf16" (throughput)
    # cg_model_opts fields as ((name, value), ...): measured engine alternatives (tests, A/B runs)
    opts: tuple = ()

    @property
    def head_dim(self) -> int:
        return self.n_embd // self.n_head

    def to_c(self) -> L.ModelCfg:
        c = L.ModelCfg()
        c.vocab_size = self.vocab_size
        c.block_size = self.block_size
        c.n_layer = self.n_layer
        c.n_head = self.n_head
        kv = self.n_kv_head
        c.n_kv_head = kv if (kv is not None and 0 < kv <= self.n_head) else 0
        c.n_embd = self.n_embd
        c.use_swiglu = int(self.use_swiglu)
        c.use_rope = int(self.use_rope)
        c.sep_id = -1 if self.sep_id is None else int(self.sep_id)
        c.tie_embeddings = int(self.tie_embeddings)
        c.termination_aux = int(self.termination_aux)
        c.termination_n_classes = int(self.termination_n_classes)
        offs = list(self.multi_offset_targets)[:8]
        c.n_offsets = len(offs)
        for i, o in enumerate(offs):
            c.offsets[i] = int(o)
        c.dropout = float(self.dropout)
        c.label_smoothing = float(self.label_smoothing)
        c.ln_eps = float(self.ln_eps)
        c.dtype = L.CG_BF16 if self.dtype == "bf16" else L.CG_F32
        known = {f for f, _ in L.ModelOpts._fields_}
        for k, v in self.opts:
            if k not in known:
                raise ValueError(f"unknown engine option {k!r} (cg_model_opts: {sorted(known)})")
            setattr(c.opts, k, int(v))
        return c


def param_layout(cfg: EngineConfig):
    """[(kind, layer, offset, rows, cols, ld)], total elements -- from the native layout."""
    ccfg = cfg.to_c()
    total = C.c_longlong(0)
    n = L.lib.cg_model_param_layout(C.byref(ccfg), None, 0, C.byref(total))
    if n < 0:
        L.check(n, "cg_model_param_layout")
    arr = (L.ParamEntry * n)()
    L.lib.cg_model_param_layout(C.byref(ccfg), arr, n, C.byref(total))
    return [(e.kind, e.layer, e.offset, e.rows, e.cols, e.ld) for e in arr], int(total.value)


def rope_tables(block_size: int, head_dim: int):
    """cos/sin [T][hd/2] built like RotaryEmbedding._set_cos_sin_cache (model_tiny_gpt.py:15-25)."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    t = torch.arange(block_size, dtype=inv_freq.dtype)
    freqs = torch.outer(t, inv_freq)
    return freqs.cos().contiguous(), freqs.sin().contiguous()


class Engine:
    def __init__(self, cfg: EngineConfig, flat: torch.Tensor, grads: torch.Tensor,
                 loss_weights: torch.Tensor | None = None):
        self.cfg = cfg
        self.flat = flat
        self.grads = grads
        self.shadow = None
        self.loss_weights = loss_weights
        self.model = L.Model()
        self.model.cfg = cfg.to_c()
        self.workspace = None
        self._ws_key = None
        self.rope_cos = self.rope_sin = None
        self._shadow_stale = True
        self._rebind()

    # -- buffers --------------------------------------------------------------------
    def _rebind(self):
        dev = self.flat.device
        if self.cfg.use_rope:
            c, s = rope_tables(self.cfg.block_size, self.cfg.head_dim)
            self.rope_cos, self.rope_sin = c.to(dev), s.to(dev)
            self.model.rope_cos = self.rope_cos.data_ptr()
            self.model.rope_sin = self.rope_sin.data_ptr()
        self.model.params = self.flat.data_ptr()
        self.model.grads = self.grads.data_ptr()
        if self.cfg.dtype == "bf16":
            if self.shadow is None or self.shadow.device != dev or self.shadow.numel() != self.flat.numel():
                self.shadow = torch.empty(self.flat.numel(), dtype=torch.bfloat16, device=dev)
            self.model.shadow = self.shadow.data_ptr()
            self._shadow_stale = True
        lw = self.loss_weights
        self.model.loss_weights = lw.data_ptr() if lw is not None else None

    def set_buffers(self, flat, grads, loss_weights=None):
        self.flat, self.grads, self.loss_weights = flat, grads, loss_weights
        self.workspace = None
        self._ws_key = None
        self._rebind()

    def mark_params_changed(self):
        """Call after writing master params outside cg_adamw (load_state_dict, init)."""
        self._shadow_stale = True

    def sync_shadow(self, stream=None):
        if self.cfg.dtype != "bf16" or not self._shadow_stale:
            return
        s = stream if stream is not None else L.stream_ptr(self.flat.device)
        L.check(L.lib.cg_cast_f32_to_bf16(self.flat.data_ptr(), self.shadow.data_ptr(), self.flat.numel(), s),
                "cg_cast_f32_to_bf16")
        self._shadow_stale = False

    def _ensure_workspace(self, B: int, T: int):
        need = int(L.lib.cg_model_workspace_bytes(C.byref(self.model.cfg), B, T))
        if need <= 0:
            raise ValueError("invalid model configuration for workspace sizing")
        if self.workspace is None or self.workspace.numel() < need or self._ws_key != (B, T):
            if self.workspace is None or self.workspace.numel() < need:
                self.workspace = torch.empty(need, dtype=torch.uint8, device=self.flat.device)
            self._ws_key = (B, T)
        self.model.workspace = self.workspace.data_ptr()
        self.model.workspace_bytes = self.workspace.numel()

    # -- compute ----------------------------------------------------------------------
    def forward(self, idx: torch.Tensor, targets: torch.Tensor | None, *, training: bool, seed: int = 0,
                window: int | None = None, logits: torch.Tensor | None = None,
                loss: torch.Tensor | None = None, head: bool = True):
        """``head=False``: the trunk alone (cg_model_forward_trunk) -- through ln_f, no head product,
        no logits, no loss; returns (None, None).  The aux heads, term_loss, hidden and the backward
        work after it."""
        L.require_device(idx, "TinyGPT.forward")
        if not head and targets is not None:
            raise ValueError("head=False computes no next-codon loss: targets must be None")
        if idx.dim() != 2:
            raise ValueError("idx must be (B, T)")
        B, T = idx.shape
        if T > self.cfg.block_size:
            raise ValueError(f"sequence length {T} exceeds block_size {self.cfg.block_size}")
        if window is not None and int(window) < 1:
            raise ValueError("attention_window must be at least 1")
        dev = self.flat.device
        idx = idx.to(device=dev, dtype=torch.int64).contiguous()
        if targets is not None:
            targets = targets.to(device=dev, dtype=torch.int64).contiguous()
            if targets.shape != idx.shape:
                raise ValueError("targets must have the same shape as idx")
        self._ensure_workspace(B, T)
        self.sync_shadow()
        self._term_keep = None
        if not head:
            self._idx, self._targets = idx, None
            self._dlogits_seeded = False
            L.check(L.lib.cg_model_forward_trunk(C.byref(self.model), idx.data_ptr(), B, T, int(bool(training)),
                                                 int(seed) & 0xFFFFFFFF, int(window) if window is not None else 0,
                                                 L.stream_ptr(dev)), "cg_model_forward_trunk")
            return None, None
        if logits is None:
            logits = torch.empty(B, T, self.cfg.vocab_size, dtype=torch.float32, device=dev)
        if targets is not None and loss is None:
            loss = torch.empty((), dtype=torch.float32, device=dev)
        self._idx, self._targets = idx, targets  # keep alive for backward
        self._dlogits_seeded = False  # the fused cross-entropy's dlogits are the loss's again
        st = L.stream_ptr(dev)
        L.check(L.lib.cg_model_forward(C.byref(self.model), idx.data_ptr(),
                                       targets.data_ptr() if targets is not None else None,
                                       B, T, int(bool(training)), int(seed) & 0xFFFFFFFF,
                                       int(window) if window is not None else 0,
                                       logits.data_ptr(), loss.data_ptr() if loss is not None else None, st),
                "cg_model_forward")
        return logits, loss

    @torch.no_grad()
    def score(self, idx: torch.Tensor, targets: torch.Tensor | None = None, *, window: int | None = None, **kw):
        """Eval forward of idx (B, T) without a loss, then cg_score_rows over the engine's own
        logits buffer, in place: an ops.ScoreResult whose rows are the B*T positions (``T`` rows
        per sequence).  ``kw``: the keywords of ops.score_rows (ignore_index, smoothing, sel, acc,
        want).  The logits stay in ``score_logits`` (B, T, V) until the next score call."""
        from . import ops
        B, T = idx.shape
        V = self.cfg.vocab_size
        buf = getattr(self, "_score_buf", None)
        if buf is None or buf.numel() < B * T * V or buf.device != self.flat.device:
            buf = self._score_buf = torch.empty(B * T * V, dtype=torch.float32, device=self.flat.device)
        self.score_logits = buf[:B * T * V].view(B, T, V)
        self.forward(idx, None, training=False, window=window, logits=self.score_logits)
        wsb = getattr(self, "_score_ws", None)
        if wsb is None or ops._nbytes(wsb) < int(L.lib.cg_score_workspace(B * T)) or wsb.device != buf.device:
            wsb = self._score_ws = ops.score_workspace(B * T, buf.device)
        return ops.score_rows(self.score_logits.view(B * T, V), targets, T=T, workspace=wsb, **kw)

    def term_loss(self, labels: torch.Tensor, class_weights: torch.Tensor | None = None) -> torch.Tensor:
        """termination_aux_loss (objectives.py:94-105) of the last forward's ln_f output through the
        fused kernel (cg_model_term_loss): a 0-d fp32 device tensor, no logits.  labels int64 with
        one entry per position (-100 = ignored), class_weights fp32 (n_classes) or None.  The
        next backward takes the head's gradients from the fused path, scaled by set_term_grad."""
        m = self.model
        dev = self.flat.device
        if not self.cfg.termination_aux:
            raise ValueError("term_loss: the model has no termination head")
        if m.B <= 0 or labels.numel() != m.B * m.T:
            raise ValueError("term_loss: labels need one entry per position of the last forward")
        L.require_device(labels, "term_loss")
        lab = labels.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        cw = None
        if class_weights is not None:
            cw = class_weights.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
            if cw.numel() != self.cfg.termination_n_classes:
                raise ValueError("term_loss: class_weights need one entry per termination class")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        self._term_keep = (lab, cw)  # read again by the backward
        L.check(L.lib.cg_model_term_loss(C.byref(m), lab.data_ptr(), cw.data_ptr() if cw is not None else None,
                                         loss.data_ptr(), L.stream_ptr(dev)), "cg_model_term_loss")
        return loss

    def set_term_grad(self, scale: float, scale_dev=None):
        """d(objective)/d(termination loss) of the fused path: a host float times an optional
        one-element device tensor (read in the kernel, no host sync), as set_head_grads' scale."""
        m = self.model
        m.term_scale = float(scale)
        m.term_scale_dev = None
        self._term_scale_keep = None
        if scale_dev is not None:
            sd = scale_dev.detach().reshape(1).to(torch.float32).contiguous()
            self._term_scale_keep = sd
            m.term_scale_dev = sd.data_ptr()

    def backward_heads(self, accumulate: bool = False):
        """cg_model_backward_heads: the aux parameters' gradients alone (a frozen backbone)."""
        L.check(L.lib.cg_model_backward_heads(C.byref(self.model), int(bool(accumulate)),
                                              L.stream_ptr(self.flat.device)), "cg_model_backward_heads")

    def aux_forward(self, term: bool = True):
        """Aux heads of the last forward (model_tiny_gpt.py:329-337): termination logits
        fp32 (M, n_classes) or None, and [offset logits fp32 (M, V)] in offset order.  ``term=False``
        (after term_loss only): the offset heads alone, no termination logits."""
        cfg = self.cfg
        dev = self.flat.device
        M = self.model.B * self.model.T
        want_term, term = term, None
        if not want_term and not self.model.term_fused:
            raise ValueError("aux_forward(term=False) needs term_loss first")
        if cfg.termination_aux and want_term:
            term = torch.empty(M, cfg.termination_n_classes, dtype=torch.float32, device=dev)
        # rows padded to a multiple of 16 columns (the GEMM then takes the vector tiles); the
        # callers see [:, :V] views
        Vp = (cfg.vocab_size + 15) // 16 * 16
        offs = [torch.empty(M, Vp, dtype=torch.float32, device=dev) for _ in cfg.multi_offset_targets]
        arr = (C.c_void_p * len(offs))(*[o.data_ptr() for o in offs]) if offs else None
        L.check(L.lib.cg_model_aux_forward(C.byref(self.model), term.data_ptr() if term is not None else None,
                                           term.stride(0) if term is not None else 0, arr, Vp, L.stream_ptr(dev)),
                "cg_model_aux_forward")
        return term, [o[:, :cfg.vocab_size] for o in offs]

    def set_head_grads(self, scale: float, d_term=None, d_offsets=None, scale_dev=None):
        """Gradients phase 0 consumes: the next-codon loss scale (host float, times the device
        float ``scale_dev`` when given -- the autograd output gradient, read in-kernel so the
        backward needs no host sync) and the aux-head logit gradients (fp32, flattened to
        (M, cols)); None = that head is unused."""
        m = self.model
        m.head_grad_scale = float(scale)
        keep = []
        m.head_grad_scale_dev = None
        if scale_dev is not None:
            sd = scale_dev.detach().reshape(1).to(torch.float32).contiguous()
            keep.append(sd)
            m.head_grad_scale_dev = sd.data_ptr()
        m.d_term_logits, m.ld_d_term = None, 0
        if d_term is not None:
            t = d_term.reshape(-1, d_term.shape[-1]).to(torch.float32).contiguous()
            keep.append(t)
            m.d_term_logits, m.ld_d_term = t.data_ptr(), t.stride(0)
        for i in range(8):
            m.d_offset_logits[i] = None
        for i, g in enumerate(d_offsets or []):
            if g is None:
                continue
            t = g.reshape(-1, g.shape[-1]).to(torch.float32).contiguous()
            keep.append(t)
            m.d_offset_logits[i] = t.data_ptr()
        self._grad_keep = keep  # alive until the backward kernels are enqueued

    # -- incremental decoding (KV cache) -------------------------------------------------
    def new_kv_cache(self, B: int, Tmax: int | None = None) -> "KVCache":
        return KVCache(self, B, Tmax or self.cfg.block_size)

    def new_ragged_kv_cache(self, B: int, Tmax: int | None = None, xf_history: bool = False) -> "RaggedKVCache":
        return RaggedKVCache(self, B, Tmax or self.cfg.block_size, xf_history=xf_history)

    def offset_prior(self, weights) -> L.OffsetPrior:
        """The cg_offset_prior of an ordered {offset: weight}: heads in the dict's order; a zero
        weight and an offset the model has no head for are left out (they contribute nothing)."""
        offs = [int(o) for o in self.cfg.multi_offset_targets][:8]
        p = L.OffsetPrior()
        for k, w in (weights or {}).items():
            if float(w) == 0.0 or int(k) not in offs:
                continue
            if p.n >= 8:
                raise ValueError("at most 8 offset priors")
            p.head[p.n], p.weight[p.n] = offs.index(int(k)), float(w)
            p.n += 1
        return p

    def backward_phase(self, phase: int, layer: int = 0, accumulate: bool = False):
        st = L.stream_ptr(self.flat.device)
        L.check(L.lib.cg_model_backward(C.byref(self.model), phase, layer, int(bool(accumulate)), st),
                f"cg_model_backward(phase={phase}, layer={layer})")

    def backward(self, accumulate: bool = False, bucket_hook=None):
        """Full backward; ``bucket_hook(name)`` runs as soon as a bucket's gradients are final
        (the DDP overlap point): "head" after phase 0, block l once its dW group has been
        issued (cg_model.dw_done_layer), "embed" after phase 2."""
        self.backward_phase(0, 0, accumulate)
        if bucket_hook:
            bucket_hook("head")
        done = self.cfg.n_layer
        for layer in range(self.cfg.n_layer - 1, -1, -1):
            self.backward_phase(1, layer, accumulate)
            if bucket_hook:
                for b in range(done - 1, self.model.dw_done_layer - 1, -1):
                    bucket_hook(b)
            done = min(done, self.model.dw_done_layer)
        self.backward_phase(2, 0, accumulate)
        if bucket_hook:
            bucket_hook("embed")

    @torch.no_grad()
    def input_grad(self, y=None, w=None, mode: str = "logprob", want=("gxt", "gxi", "gnorm"), dx0: bool = False):
        """cg_model_input_grad of the last forward, which must have been an eval forward: the
        gradient of a seeded objective at the embedding output and its per-token reductions, as an
        ops.AttrResult of (B, T) tensors (``dx0`` (B, T, d) when asked for).  ``y`` int64 (B, T):
        the objective is sum w log p(y) over the positions with 0 <= y < V (``mode`` "logprob";
        "logit": the weighted logits), ``w`` fp32 (B, T) or None = 1.  ``y`` None: the loss of the
        forward itself (it must have had targets) -- its mean cross-entropy with the model's
        smoothing and class weights.  Writes no parameter gradient."""
        from . import ops
        m = self.model
        B, T, d = m.B, m.T, self.cfg.n_embd
        if B <= 0 or T <= 0:
            raise ValueError("input_grad: no forward has run")
        if mode not in ops.ATTR_MODES:
            raise ValueError(f"input_grad: mode is one of {sorted(ops.ATTR_MODES)}")
        ops._check_want("input_grad", want, ops.ATTR_OUTPUTS)
        dev = self.flat.device
        a = L.AttrDesc()
        a.mode = ops.ATTR_MODES[mode]
        keep = []
        if y is None:
            if w is not None:
                raise ValueError("input_grad: w needs y")
            if getattr(self, "_dlogits_seeded", False):
                raise ValueError("input_grad: a seeded call replaced the forward's loss gradient; run the forward again")
        else:
            for name, t, dt in (("y", y, torch.int64), ("w", w, torch.float32)):
                if t is not None:  # one entry per position of the forward
                    keep.append(ops._per_row(t, "input_grad", name, dt, B * T))
                    setattr(a, name, keep[-1].data_ptr())
        res = ops.AttrResult()
        ops._alloc_outputs(a, res, want, dev, [(name, (B, T), torch.float32) for name in ops.ATTR_OUTPUTS])
        if dx0:
            res.dx0 = torch.empty(B, T, d, dtype=torch.float32, device=dev)
            a.dx0, a.ld_dx0 = res.dx0.data_ptr(), d
        L.check(L.lib.cg_model_input_grad(C.byref(m), C.byref(a), L.stream_ptr(dev)), "cg_model_input_grad")
        if y is not None:
            self._dlogits_seeded = True  # until the next forward
        return res

    def attn_probs(self, layer: int) -> torch.Tensor:
        """Attention probabilities of block `layer` of the last forward: fp32 (B, H, T, T)."""
        B, T, H = self.model.B, self.model.T, self.cfg.n_head
        dev = self.flat.device
        out = torch.empty(B, H, T, T, dtype=torch.float32, device=dev)
        L.check(L.lib.cg_model_attn_probs(C.byref(self.model), int(layer), out.data_ptr(), L.stream_ptr(dev)),
                "cg_model_attn_probs")
        return out

    def attn_stats(self, layer: int, *, pad_id: int = -1, tok_class=None, row_keep=None,
                   want=("rows", "nvis", "received"), head_acc=None, n_rows=None, workspace=None):
        """cg_attn_stats on block `layer` of the last forward (any forward; nothing T x T is written):
        an ops.AttnStatsResult.  The layer's qkv rows, SEP mask, window and token ids are the
        forward's; the keywords are those of ops.attn_stats."""
        from . import ops
        B, T, H = self.model.B, self.model.T, self.cfg.n_head
        if getattr(self, "_idx", None) is None or B <= 0:
            raise ValueError("attn_stats: run a forward first")
        dev = self.flat.device
        d = L.AttnStatsDesc()
        res = ops.AttnStatsResult()
        keep = ops.attn_stats_fill(d, res, B, T, H, dev, pad_id=pad_id, tok_class=tok_class, row_keep=row_keep,
                                   want=want, head_acc=head_acc, n_rows=n_rows, workspace=workspace)
        L.check(L.lib.cg_model_attn_stats(C.byref(self.model), int(layer), C.byref(d), L.stream_ptr(dev)),
                "cg_model_attn_stats")
        del keep
        return res

    def hidden(self, which: int) -> torch.Tensor:
        dt = C.c_int(0)
        ld = C.c_longlong(0)
        ptr = L.lib.cg_model_hidden(C.byref(self.model), which, C.byref(dt), C.byref(ld))
        if not ptr:
            raise ValueError(f"no hidden state {which}")
        B, T, d = self.model.B, self.model.T, self.cfg.n_embd
        base = self.workspace.data_ptr()
        off = ptr - base
        if dt.value == L.CG_F32:
            t = self.workspace[off: off + B * T * d * 4].view(torch.float32)
        else:
            t = self.workspace[off: off + B * T * d * 2].view(torch.bfloat16)
        return t.view(B, T, d)


class KVCache:
    """Per-sequence K/V rows of every layer for incremental decoding (cg_model_prefill /
    cg_model_decode): one prefill of the prompt, then one native call per generated token
    instead of the reference's full re-forward of the prefix (query_model.py:160-214).
    Valid while the sequence fits ``Tmax`` <= block_size."""

    def __init__(self, engine: Engine, B: int, Tmax: int):
        cfg = engine.cfg
        if Tmax > cfg.block_size:
            raise ValueError("Tmax exceeds block_size")
        self.eng, self.B, self.Tmax = engine, int(B), int(Tmax)
        dev = engine.flat.device
        nbytes = int(L.lib.cg_kv_cache_bytes(C.byref(engine.model.cfg), self.B, self.Tmax))
        self.cache = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        self.seg = torch.zeros(self.B, dtype=torch.int32, device=dev)
        wsb = int(L.lib.cg_decode_workspace_bytes(C.byref(engine.model.cfg), self.B))
        self.ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        self.pos = 0

    @torch.no_grad()
    def prefill(self, idx: torch.Tensor, window: int | None = None) -> torch.Tensor:
        """Eval forward of the prompt (B, T); returns fp32 logits (B, T, V)."""
        eng = self.eng
        L.require_device(idx, "KVCache.prefill")
        B, T = idx.shape
        if B != self.B or T > self.Tmax:
            raise ValueError(f"prompt {tuple(idx.shape)} does not fit the cache (B={self.B}, Tmax={self.Tmax})")
        idx = idx.to(torch.int64).contiguous()
        eng._ensure_workspace(B, T)
        eng.sync_shadow()
        logits = torch.empty(B, T, eng.cfg.vocab_size, dtype=torch.float32, device=idx.device)
        eng._idx, eng._targets = idx, None
        L.check(L.lib.cg_model_prefill(C.byref(eng.model), idx.data_ptr(), B, T, int(window or 0),
                                       self.cache.data_ptr(), self.Tmax, self.seg.data_ptr(), logits.data_ptr(),
                                       L.stream_ptr(idx.device)), "cg_model_prefill")
        self.pos = T
        return logits

    @torch.no_grad()
    def decode(self, tok: torch.Tensor) -> torch.Tensor:
        """Append one token per sequence (B,) at the current position; returns logits (B, V)."""
        eng = self.eng
        if self.pos >= self.Tmax:
            raise ValueError("KV cache is full (the context reached Tmax)")
        tok = tok.reshape(self.B).to(device=self.cache.device, dtype=torch.int64).contiguous()
        eng.sync_shadow()
        logits = torch.empty(self.B, eng.cfg.vocab_size, dtype=torch.float32, device=tok.device)
        L.check(L.lib.cg_model_decode(C.byref(eng.model), tok.data_ptr(), self.B, self.pos, self.cache.data_ptr(),
                                      self.Tmax, self.seg.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                      logits.data_ptr(), L.stream_ptr(tok.device)), "cg_model_decode")
        self._tok = tok
        self.pos += 1
        return logits


class RaggedKVCache:
    """The KV cache of a batch whose sequences sit at different positions (cg_model_prefill_ragged /
    cg_model_decode_ragged): one prefill of right-padded prompts, then one native call per step
    with the positions in a device int32 tensor.  A row whose position is negative (or >= Tmax)
    is inactive in that step: its cache rows, ``logits`` row and ``term`` row stay as they are.
    ``logits`` (B, V) and ``term`` (B, n_classes; models with a termination head) are fixed
    buffers every step writes in place, so a generation loop holds no per-step allocations.

    With ``xf_history`` the cache also keeps the ln_f output of every cached row (``hist``,
    (B, Tmax, d) in the model dtype: cg_model_prefill_hist / cg_model_decode_ragged_hist), which is
    what ``add_offset_priors`` (cg_offset_prior_add) reads."""

    def __init__(self, engine: Engine, B: int, Tmax: int, xf_history: bool = False):
        cfg = engine.cfg
        if Tmax > cfg.block_size:
            raise ValueError("Tmax exceeds block_size")
        self.eng, self.B, self.Tmax = engine, int(B), int(Tmax)
        dev = engine.flat.device
        nbytes = int(L.lib.cg_kv_cache_bytes(C.byref(engine.model.cfg), self.B, self.Tmax))
        self.cache = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        self.seg = torch.zeros(self.B, dtype=torch.int32, device=dev)
        wsb = int(L.lib.cg_decode_ragged_workspace_bytes(C.byref(engine.model.cfg), self.B))
        self.ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        self.logits = torch.zeros(self.B, cfg.vocab_size, dtype=torch.float32, device=dev)
        self.term = (torch.zeros(self.B, cfg.termination_n_classes, dtype=torch.float32, device=dev)
                     if cfg.termination_aux else None)
        self.hist = self.prior_ws = None
        if xf_history:
            ccfg = engine.model.cfg
            hb = int(L.lib.cg_xf_hist_bytes(C.byref(ccfg), self.B, self.Tmax))
            hist = torch.zeros(max(hb, 1), dtype=torch.uint8, device=dev)
            self.hist = hist[:hb].view(torch.bfloat16 if cfg.dtype == "bf16" else torch.float32).view(
                self.B, self.Tmax, cfg.n_embd)
            self.prior_ws = torch.zeros(max(int(L.lib.cg_offset_prior_workspace(C.byref(ccfg), self.B)), 1),
                                        dtype=torch.uint8, device=dev)

    @torch.no_grad()
    def prefill(self, idx: torch.Tensor, lens: torch.Tensor, window: int | None = None, *,
                want_term: bool = False) -> torch.Tensor:
        """Eval forward of the right-padded prompts (B, T) with lengths ``lens`` (B,) in 1..T;
        returns ``logits``: row b holds the logits after prompt b's last token.  ``want_term``
        also fills ``term`` with the termination head at that row."""
        eng = self.eng
        L.require_device(idx, "RaggedKVCache.prefill")
        B, T = idx.shape
        if B != self.B or T > self.Tmax:
            raise ValueError(f"prompts {tuple(idx.shape)} do not fit the cache (B={self.B}, Tmax={self.Tmax})")
        dev = self.cache.device
        idx = idx.to(device=dev, dtype=torch.int64).contiguous()
        lens = lens.reshape(B).to(device=dev, dtype=torch.int32).contiguous()
        eng._ensure_workspace(B, T)
        eng.sync_shadow()
        eng._idx, eng._targets = idx, None
        L.check(L.lib.cg_model_prefill_ragged(C.byref(eng.model), idx.data_ptr(), lens.data_ptr(), B, T,
                                              int(window or 0), self.cache.data_ptr(), self.Tmax,
                                              self.seg.data_ptr(), self.logits.data_ptr(), L.stream_ptr(dev)),
                "cg_model_prefill_ragged")
        if self.hist is not None:
            L.check(L.lib.cg_model_prefill_hist(C.byref(eng.model), lens.data_ptr(), B, T, self.hist.data_ptr(),
                                                self.Tmax, L.stream_ptr(dev)), "cg_model_prefill_hist")
        if want_term:
            if self.term is None:
                raise ValueError("the model has no termination head")
            term, _ = eng.aux_forward()
            rows = torch.arange(B, device=dev) * T + (lens.to(torch.int64) - 1)
            self.term.copy_(term[rows])
        return self.logits

    @torch.no_grad()
    def decode(self, tok: torch.Tensor, pos: torch.Tensor, *, want_term: bool = False) -> torch.Tensor:
        """Token tok[b] (int64, device) enters at cache row pos[b] (int32, device); returns
        ``logits``, updated in the active rows."""
        eng = self.eng
        if tok.dtype != torch.int64 or pos.dtype != torch.int32 or tok.numel() != self.B or pos.numel() != self.B:
            raise ValueError("tok must be int64 (B,) and pos int32 (B,)")
        if not (tok.is_contiguous() and pos.is_contiguous()):
            raise ValueError("tok and pos must be contiguous")
        L.require_device(tok, "RaggedKVCache.decode")
        L.require_device(pos, "RaggedKVCache.decode")
        if want_term and self.term is None:
            raise ValueError("the model has no termination head")
        eng.sync_shadow()
        args = (C.byref(eng.model), tok.data_ptr(), pos.data_ptr(), self.B, self.cache.data_ptr(), self.Tmax,
                self.seg.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.logits.data_ptr(),
                self.term.data_ptr() if want_term else None, self.term.stride(0) if want_term else 0)
        if self.hist is not None:
            L.check(L.lib.cg_model_decode_ragged_hist(*args, self.hist.data_ptr(), L.stream_ptr(self.cache.device)),
                    "cg_model_decode_ragged_hist")
        else:
            L.check(L.lib.cg_model_decode_ragged(*args, L.stream_ptr(self.cache.device)), "cg_model_decode_ragged")
        return self.logits

    def offset_prior(self, weights) -> L.OffsetPrior:
        return self.eng.offset_prior(weights)

    @torch.no_grad()
    def add_offset_priors(self, pos: torch.Tensor, weights) -> torch.Tensor:
        """``logits[b] += sum_k w_k * offset_logits[k][pos[b] + 1 - k]`` on the active rows, for the
        heads of the ordered ``weights`` {offset: weight} (or a prepared cg_offset_prior) whose row
        exists; ``pos[b]`` (int32, device) is sequence b's last cached row.  Returns ``logits``."""
        if self.hist is None:
            raise ValueError("the cache was built without xf_history")
        if pos.dtype != torch.int32 or pos.numel() != self.B or not pos.is_contiguous():
            raise ValueError("pos must be a contiguous int32 (B,)")
        L.require_device(pos, "RaggedKVCache.add_offset_priors")
        p = weights if isinstance(weights, L.OffsetPrior) else self.offset_prior(weights)
        if p.n == 0:
            return self.logits
        self.eng.sync_shadow()
        L.check(L.lib.cg_offset_prior_add(C.byref(self.eng.model), C.byref(p), self.hist.data_ptr(), self.Tmax,
                                          pos.data_ptr(), self.B, self.logits.data_ptr(), self.logits.stride(0),
                                          self.prior_ws.data_ptr(), self.prior_ws.numel(),
                                          L.stream_ptr(self.cache.device)), "cg_offset_prior_add")
        return self.logits
