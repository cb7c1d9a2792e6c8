"""Batched, ragged, guided CDS generation on the MI355X (mirrors src/codonlm/generate.py).

``generate_batch`` runs any number of prompts of different lengths as one batch that stays on
the device from prompt to finished sequence: one ragged prefill (cg_model_prefill_ragged), then
per generated token one fused sampler / stop-rule launch (cg_sample_step: termination-head bias,
CDS mask, temperature, top-k, the draw and the reference's stop rules) and one ragged KV-cached
decode step (cg_model_decode_ragged).  The host reads four bytes (the number of sequences still
running) every ``poll_every`` steps and nothing else until the end.

The draws come from a counter-based generator keyed by (seed, stream, token index), so a
sequence's tokens do not depend on what else is in its batch or on ``poll_every``.  The rules
are stated in include/codonlm_hip.h (cg_sample_step).

``generate_model_raw``, ``generate_cds_constrained``, ``generate_cds_red`` and
``batch_red_sampler`` take the reference's arguments (plus ``seed`` / ``stream``) and return the
reference's ``info`` records.  The batched path does not slide the context window: prompt +
token cap must fit block_size (``query_model.generate`` keeps the sliding loop).  The
critic-guided generator is not part of it.

Multi-offset priors (``multi_offset_prior_enabled`` / ``multi_offset_prior_weights``, the
reference's ``_apply_multi_offset_priors``): the cache keeps the ln_f output of every cached row
(``new_ragged_kv_cache(..., xf_history=True)``) and, after the prefill and after every decode
step, cg_offset_prior_add adds ``w_k * offset_logits[k][ctx_len - k]`` to the next-token logits
in three launches for any number of heads; the sampler's termination bias, mask and temperature
then act on the adjusted logits, as in the reference.  A model without offset heads raises
NotImplementedError (the reference does nothing in that case).

``generate_cds_synonymous`` writes a CDS that translates to a given protein: with ``token_sets``
and ``plans``, ``generate_batch`` goes through cg_sample_step_plan, where every generated token
of every sequence has its own allowed set, a sequence ends when its plan is used up, and the
sampler returns the log-probability of what it drew (``with_logp``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

STOP_CODONS = {"TAA", "TAG", "TGA"}
INT_MAX = L.INT_MAX

# the standard genetic code over the codons in ACGT order, stop written as "_"
_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV_Y_YSSSS_CWCLFLF"
CODON_TABLE: Dict[str, str] = {a + b + c: _CODE[16 * i + 4 * j + k] for i, a in enumerate("ACGT")
                               for j, b in enumerate("ACGT") for k, c in enumerate("ACGT")}
AA_TO_CODONS: Dict[str, List[str]] = {}
for _codon, _aa in CODON_TABLE.items():
    AA_TO_CODONS.setdefault(_aa, []).append(_codon)


def _is_codon(tok: str) -> bool:
    return len(tok) == 3 and set(tok) <= set("ACGT")


def token_classes(itos: Sequence[str], stoi: Dict[str, int]) -> np.ndarray:
    """uint8 [V] of TOK_CODON / TOK_STOP / TOK_EOS bits (generate.py:84-92, :232-251)."""
    cls = np.zeros(len(itos), dtype=np.uint8)
    for i, tok in enumerate(itos):
        if _is_codon(tok):
            cls[i] |= L.TOK_CODON
            if tok in STOP_CODONS:
                cls[i] |= L.TOK_STOP
    eos = stoi.get("<EOS_CDS>")
    if eos is not None and 0 <= eos < len(itos):
        cls[eos] |= L.TOK_EOS
    return cls


def cds_mask(itos: Sequence[str]) -> np.ndarray:
    """uint8 [V]: 1 on the codon tokens (_cds_token_ids, generate.py:34-39)."""
    return np.array([1 if _is_codon(t) else 0 for t in itos], dtype=np.uint8)


def state_record(row) -> Dict[str, int]:
    """One cg_gen_state (8 int32 columns) as a dict."""
    rec = {k: int(v) for k, v in zip(L.GEN_STATE_FIELDS, row)}
    rec["stream"] &= 0xFFFFFFFF
    return rec


def round_seed(seed: int, round_idx: int) -> int:
    """The seed of round ``round_idx`` (1-based) of batch_red_sampler / attempt of generate_cds_red."""
    return (int(seed) + 0x9E3779B9 * int(round_idx)) & 0xFFFFFFFF


def _check_fit(model, contexts, max_tokens: int) -> None:
    if not contexts or any(len(c) < 1 for c in contexts):
        raise ValueError("every context needs at least one token")
    if int(max_tokens) < 1:
        raise ValueError("max_tokens must be at least 1")
    longest = max(len(c) for c in contexts)
    if longest + int(max_tokens) > int(model.block_size):
        raise ValueError(f"prompt ({longest} tokens) + token cap ({int(max_tokens)}) exceeds block_size "
                         f"{int(model.block_size)}: the batched path does not slide the context window "
                         "(query_model.generate does)")


def _check_fit_plans(model, contexts, plans) -> None:
    """The fit check of a batch that ends with its plans: per row, prompt + plan <= block_size."""
    if not contexts or any(len(c) < 1 for c in contexts):
        raise ValueError("every context needs at least one token")
    for b, (c, pl) in enumerate(zip(contexts, plans)):
        if len(pl) < 1:
            raise ValueError(f"end_with_plan: sequence {b} has an empty plan and would never end")
        if len(c) + len(pl) > int(model.block_size):
            raise ValueError(f"prompt ({len(c)} tokens) + plan ({len(pl)} tokens) of sequence {b} exceeds "
                             f"block_size {int(model.block_size)}: the batched path does not slide the context "
                             "window")


class TokenSets:
    """The set table of a planned batch: uint8 rows over the model's V tokens, equal sets stored
    once.  ``residue`` / ``stop`` / ``token`` return the index of a set, for use in a plan."""

    def __init__(self, stoi: Dict[str, int], itos: Sequence[str], V: int):
        self.stoi, self.itos, self.V = stoi, itos, int(V)
        self.rows: List[np.ndarray] = []
        self._index: Dict[bytes, int] = {}

    def add(self, ids) -> int:
        row = np.zeros(self.V, dtype=np.uint8)
        ids = [int(i) for i in ids]
        if any(i < 0 or i >= self.V for i in ids):
            raise ValueError(f"token id outside the model's vocabulary of {self.V}")
        row[ids] = 1
        key = row.tobytes()
        if key not in self._index:
            self._index[key] = len(self.rows)
            self.rows.append(row)
        return self._index[key]

    def codon_ids(self, aa: str) -> List[int]:
        """The ids of the codons of amino acid ``aa`` (any case) that the vocabulary has."""
        return [self.stoi[c] for c in AA_TO_CODONS.get(aa.upper(), []) if c in self.stoi]

    def residue(self, aa: str, *, strict: bool = False) -> int:
        """The synonymous set of one residue.  A residue without a codon in the vocabulary (and,
        when ``strict``, the stop "_") is a ValueError when ``strict``, else the set of all codon
        tokens (generate.py:673-676)."""
        ids = self.codon_ids(aa)
        if not ids or (strict and aa == "_"):
            if strict:
                raise ValueError(f"unknown residue {aa!r}: no codon of the vocabulary translates to it")
            ids = np.nonzero(cds_mask(self.itos))[0]
        return self.add(ids)

    def stop(self) -> int:
        return self.add(self.codon_ids("_"))

    def token(self, tok: int) -> int:
        return self.add([tok])

    def array(self) -> np.ndarray:
        return np.stack(self.rows) if self.rows else np.zeros((0, self.V), dtype=np.uint8)


def synonymous_plan(sets: TokenSets, protein: str, *, strict: bool = False) -> List[int]:
    """One synonymous set per residue of ``protein``, then the stop-codon set."""
    return [sets.residue(aa, strict=strict) for aa in protein] + [sets.stop()]


def translate(codons: Sequence[str]) -> str:
    """The protein of a codon list, stop as "_"; "?" for a token that is no codon."""
    return "".join(CODON_TABLE.get(c, "?") for c in codons)


@torch.no_grad()
def generate_batch(model, contexts: List[List[int]], stoi: Dict[str, int], itos: List[str], *, seed: int,
                   streams: Sequence[int] | None = None, poll_every: int = 16, max_tokens: int,
                   temperature: float = 1.0, topk: int = 0, target_codons: int = INT_MAX,
                   max_codons: int = INT_MAX, require_terminal_stop: bool = False, stop_on_eos: bool = True,
                   stop_on_bio_stop: bool = True, cds_only: bool = False, termination_bias_enabled: bool = False,
                   termination_stop_bias: float = 0.0, termination_trigger_class_max: int = 0,
                   termination_bias_window: int = 0, multi_offset_prior_enabled: bool = False,
                   attention_window: int | None = None, token_sets=None, plans: Sequence[Sequence[int]] | None = None,
                   end_with_plan: bool = False, with_logp: bool = False,
                   multi_offset_prior_weights: Dict[int, float] | None = None
                   ) -> List[Tuple[List[int], Dict[str, int]]]:
    """All contexts as one batch; returns [(ids, state)] in context order: ``ids`` = context +
    generated tokens, ``state`` = the sequence's final cg_gen_state as a dict (state_record).

    ``token_sets`` (uint8 [n_sets][V]) and ``plans`` (per context, the set index of every generated
    token; -1 or past the end = no set) give each step of each sequence its own allowed set; with
    ``end_with_plan`` a sequence ends when its plan is used up (flag GEN_PLAN_END), and the batch
    runs min(max_tokens, longest plan) steps.  ``with_logp`` adds ``logp_model`` (the sum of the
    model's own log-probabilities of the drawn tokens) and ``logp_draw`` (under the distribution
    drawn from) to every state dict.  Any of the four selects cg_sample_step_plan.

    ``multi_offset_prior_enabled`` with ``multi_offset_prior_weights`` (an ordered {offset: weight})
    adds the weighted offset-head logits to every step's logits before the sampler sees them."""
    if multi_offset_prior_enabled and not getattr(model, "multi_offset_targets", None):
        raise NotImplementedError("multi-offset priors need a model with offset heads (multi_offset_targets)")
    if multi_offset_prior_enabled and with_logp:
        raise ValueError("with_logp reports the model's own log-probability; it cannot be combined with "
                         "multi-offset priors")
    planned = token_sets is not None or plans is not None or bool(end_with_plan) or bool(with_logp)
    if planned:
        plans = [[] for _ in contexts] if plans is None else [[int(s) for s in pl] for pl in plans]
        if len(plans) != len(contexts):
            raise ValueError("one plan per context")
        if any(plans) and token_sets is None:
            raise ValueError("plans need token_sets")
        V = int(model.vocab_size)
        sets = np.zeros((0, V), dtype=np.uint8) if token_sets is None else np.asarray(token_sets)
        if sets.ndim != 2 or sets.dtype != np.uint8 or sets.shape[1] > V:
            raise ValueError(f"token_sets is uint8 [n_sets][V <= {V}]")
    if int(max_tokens) < 1:
        raise ValueError("max_tokens must be at least 1")
    if end_with_plan:
        _check_fit_plans(model, contexts, plans)
        steps = min(int(max_tokens), max(len(pl) for pl in plans))
    else:
        _check_fit(model, contexts, max_tokens)
        steps = int(max_tokens)
    V = int(model.vocab_size)
    if len(itos) > V:
        raise ValueError(f"vocabulary of {len(itos)} tokens exceeds the model's {V}")
    eng = model.engine
    dev = eng.flat.device
    B = len(contexts)
    streams = list(range(B)) if streams is None else [int(s) for s in streams]
    if len(streams) != B:
        raise ValueError("one stream per context")
    max_tokens = int(max_tokens)
    lens = [len(c) for c in contexts]
    T = max(lens)
    sep = model.sep_id
    pad = 0 if sep != 0 else 1
    idx = np.full((B, T), pad, dtype=np.int64)
    for b, c in enumerate(contexts):
        idx[b, :len(c)] = c
    cls = np.zeros(V, dtype=np.uint8)
    cls[:len(itos)] = token_classes(itos, stoi)
    tok_class = torch.from_numpy(cls).to(dev)
    allowed = None
    if cds_only:
        a = np.zeros(V, dtype=np.uint8)
        a[:len(itos)] = cds_mask(itos)
        if a.any():  # (_mask_to_allowed_tokens leaves the logits alone without codon tokens)
            allowed = torch.from_numpy(a).to(dev)
    use_term = bool(termination_bias_enabled and float(termination_stop_bias) > 0.0 and model.termination_aux
                    and (cls & L.TOK_STOP).any())

    st = np.zeros((B, 8), dtype=np.int32)
    st[:, 0] = lens
    st[:, 1] = lens
    st[:, 6] = -1
    st[:, 7] = np.array(streams, dtype=np.uint64).astype(np.uint32).view(np.int32)
    state = torch.from_numpy(st).to(dev)
    out_ids = torch.zeros(B, steps, dtype=torch.int64, device=dev)
    next_tok = torch.zeros(B, dtype=torch.int64, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    n_active = torch.zeros(1, dtype=torch.int32, device=dev)

    prior = eng.offset_prior(multi_offset_prior_weights) if multi_offset_prior_enabled else None
    if prior is not None and prior.n == 0:  # no weights, zero weights, offsets without a head: nothing to add
        prior = None
    cache = eng.new_ragged_kv_cache(B, int(model.block_size), xf_history=prior is not None)
    P = L.SampleParams()
    P.V = V
    P.tok_class = tok_class.data_ptr()
    P.allowed = allowed.data_ptr() if allowed is not None else None
    P.temperature = float(temperature)
    P.topk = int(topk or 0)
    P.target_codons = min(int(target_codons), INT_MAX)
    P.max_codons = min(int(max_codons), INT_MAX)
    P.max_tokens = min(max_tokens, INT_MAX)
    P.require_terminal_stop = int(bool(require_terminal_stop))
    P.stop_on_eos = int(bool(stop_on_eos))
    P.stop_on_bio_stop = int(bool(stop_on_bio_stop))
    P.stop_bias = float(termination_stop_bias) if use_term else 0.0
    P.trigger_class_max = int(termination_trigger_class_max)
    P.bias_window = int(termination_bias_window)
    P.n_term_classes = int(eng.cfg.termination_n_classes) if use_term else 0
    P.seed = int(seed) & 0xFFFFFFFF
    P.Tmax = cache.Tmax
    if planned:
        sets_full = np.zeros((sets.shape[0], V), dtype=np.uint8)
        sets_full[:, :sets.shape[1]] = sets
        plan_np = np.full((B, max(1, max(len(pl) for pl in plans))), -1, dtype=np.int32)
        for b, pl in enumerate(plans):
            plan_np[b, :len(pl)] = pl
        sets_dev = torch.from_numpy(sets_full).to(dev)
        plan_dev = torch.from_numpy(plan_np).to(dev)
        plan_len = torch.tensor([len(pl) for pl in plans], dtype=torch.int32, device=dev)
        logp = torch.zeros(B, 2, dtype=torch.float64, device=dev) if with_logp else None
        PL = L.SamplePlan()
        PL.n_sets = sets_full.shape[0]
        if PL.n_sets:
            PL.sets, PL.ld_sets = sets_dev.data_ptr(), sets_dev.stride(0)
            PL.plan, PL.ld_plan = plan_dev.data_ptr(), plan_dev.stride(0)
        PL.plan_len = plan_len.data_ptr()
        PL.end_with_plan = int(bool(end_with_plan))
        PL.logp = logp.data_ptr() if with_logp else None

    logits = cache.prefill(torch.from_numpy(idx).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev),
                           window=attention_window, want_term=use_term)
    if prior is not None:
        pos.copy_(state[:, 1] - 1)  # the last prompt row
        cache.add_offset_priors(pos, prior)
    term_ptr = cache.term.data_ptr() if use_term else None
    ld_term = cache.term.stride(0) if use_term else 0
    stream = L.stream_ptr(dev)
    poll_every = max(1, int(poll_every))
    for step in range(1, steps + 1):
        if planned:
            L.check(L.lib.cg_sample_step_plan(C.byref(P), C.byref(PL), logits.data_ptr(), logits.stride(0), term_ptr,
                                              ld_term, state.data_ptr(), next_tok.data_ptr(), out_ids.data_ptr(),
                                              out_ids.stride(0), n_active.data_ptr(), B, stream),
                    "cg_sample_step_plan")
        else:
            L.check(L.lib.cg_sample_step(C.byref(P), logits.data_ptr(), logits.stride(0), term_ptr, ld_term,
                                         state.data_ptr(), next_tok.data_ptr(), out_ids.data_ptr(),
                                         out_ids.stride(0), n_active.data_ptr(), B, stream), "cg_sample_step")
        if step == steps:  # the token cap, or the longest plan, has ended every sequence
            break
        if step % poll_every == 0 and int(n_active.item()) == 0:
            break
        pos.copy_(state[:, 1])
        cache.decode(next_tok, pos, want_term=use_term)
        if prior is not None:
            cache.add_offset_priors(pos, prior)
    st = state.cpu().numpy()
    out = out_ids.cpu().numpy()
    lp = logp.cpu().numpy() if planned and with_logp else None
    res = []
    for b, c in enumerate(contexts):
        rec = state_record(st[b])
        if lp is not None:
            rec["logp_model"], rec["logp_draw"] = float(lp[b, 0]), float(lp[b, 1])
        res.append((list(c) + [int(t) for t in out[b, :rec["n_tokens"]]], rec))
    return res


# ---------------------------------------------------------------------------
# the reference's info records from a final cg_gen_state
# ---------------------------------------------------------------------------
def raw_info(rec: Dict[str, int], max_new_tokens: int) -> Dict[str, object]:
    """generate_model_raw's info (generate.py:95-108)."""
    f = rec["flags"]
    stop_reason = ("biological_stop" if f & L.GEN_TERMINAL_STOP else "eos" if f & L.GEN_EOS else "max_new_tokens")
    return {
        "protocol": "raw_model",
        "cds_only": False,
        "require_terminal_stop": False,
        "guidance_components": [],
        "had_terminal_stop": bool(f & L.GEN_TERMINAL_STOP),
        "early_stop": False,
        "hit_hard_cap": stop_reason == "max_new_tokens",
        "generated_codons": rec["n_codons"],
        "generated_tokens": rec["n_tokens"],
        "max_new_tokens": int(max_new_tokens),
        "stop_reason": stop_reason,
    }


def constrained_info(rec: Dict[str, int], *, target_codons: int, hard_cap: int, require_terminal_stop: bool,
                     termination_bias_enabled: bool, termination_bias_window: int, cds_only: bool,
                     multi_offset_prior_enabled: bool = False) -> Dict[str, object]:
    """generate_cds_constrained's info (generate.py:262-290)."""
    f = rec["flags"]
    components = []
    if termination_bias_enabled:
        components.append("termination_bias")
    if multi_offset_prior_enabled:
        components.append("multi_offset_prior")
    if require_terminal_stop:
        components.append("forced_terminal_stop")
    if not cds_only:
        components.append("non_cds_tokens")
    return {
        "protocol": "guided" if components else "cds_constrained",
        "guidance_components": components,
        "had_terminal_stop": bool(f & L.GEN_TERMINAL_STOP),
        "early_stop": bool(f & L.GEN_EARLY_STOP),
        "hit_hard_cap": rec["n_codons"] >= int(hard_cap),
        "target_codons": int(target_codons),
        "generated_codons": rec["n_codons"],
        "termination_bias_enabled": bool(termination_bias_enabled),
        "termination_bias_steps": rec["bias_steps"],
        "termination_bias_window": int(termination_bias_window),
        "last_termination_class": rec["last_term_class"] if rec["last_term_class"] >= 0 else None,
        "cds_only": bool(cds_only),
        "require_terminal_stop": bool(require_terminal_stop),
        "generated_tokens": rec["n_tokens"],
    }


def _constrained_batch(model, contexts, stoi, itos, target_codons, hard_cap, *, require_terminal_stop, temperature,
                       topk, termination_bias_enabled, termination_stop_bias, termination_trigger_class_max,
                       termination_bias_window, cds_only, seed, streams, poll_every=16,
                       multi_offset_prior_enabled=False, multi_offset_prior_weights=None):
    """generate_cds_constrained over a batch: the loop bound of generate.py:193 is the codon cap
    hard_cap and the token cap 3 * hard_cap."""
    res = generate_batch(model, contexts, stoi, itos, seed=seed, streams=streams, poll_every=poll_every,
                         max_tokens=3 * int(hard_cap), temperature=temperature, topk=topk,
                         target_codons=int(target_codons), max_codons=int(hard_cap),
                         require_terminal_stop=require_terminal_stop, stop_on_eos=True, stop_on_bio_stop=True,
                         cds_only=cds_only, termination_bias_enabled=termination_bias_enabled,
                         termination_stop_bias=termination_stop_bias,
                         termination_trigger_class_max=termination_trigger_class_max,
                         termination_bias_window=termination_bias_window,
                         multi_offset_prior_enabled=multi_offset_prior_enabled,
                         multi_offset_prior_weights=multi_offset_prior_weights)
    return [(ids, constrained_info(rec, target_codons=target_codons, hard_cap=hard_cap,
                                   require_terminal_stop=require_terminal_stop,
                                   termination_bias_enabled=termination_bias_enabled,
                                   termination_bias_window=termination_bias_window, cds_only=cds_only,
                                   multi_offset_prior_enabled=multi_offset_prior_enabled))
            for ids, rec in res]


# ---------------------------------------------------------------------------
# drop-in functions (the reference's names and arguments)
# ---------------------------------------------------------------------------
def generate_model_raw(model, device, ctx_ids: List[int], stoi: Dict[str, int], itos: List[str],
                       max_new_tokens: int, temperature: float = 1.0, topk: int = 0, *, seed: int = 0,
                       stream: int = 0) -> Tuple[List[int], Dict[str, object]]:
    """Sample the model vocabulary without CDS masking or forced termination (generate.py:62-108)."""
    (ids, rec), = generate_batch(model, [list(ctx_ids)], stoi, itos, seed=seed, streams=[stream],
                                 max_tokens=int(max_new_tokens), temperature=temperature, topk=topk)
    return ids, raw_info(rec, max_new_tokens)


def generate_cds_constrained(model, device, ctx_ids: List[int], stoi: Dict[str, int], itos: List[str],
                             target_codons: int, hard_cap: int, require_terminal_stop: bool = False,
                             temperature: float = 1.0, topk: int = 0, termination_bias_enabled: bool = False,
                             termination_stop_bias: float = 0.0, termination_trigger_class_max: int = 0,
                             termination_bias_window: int = 0, cds_only: bool = True,
                             multi_offset_prior_enabled: bool = False,
                             multi_offset_prior_weights: Dict[int, float] | None = None, *, seed: int = 0,
                             stream: int = 0) -> Tuple[List[int], Dict[str, object]]:
    """Generate codons up to the constraints and return (ids, info) (generate.py:153-290)."""
    if multi_offset_prior_enabled and not getattr(model, "multi_offset_targets", None):
        raise NotImplementedError("multi-offset priors need a model with offset heads (multi_offset_targets)")
    (ids, info), = _constrained_batch(
        model, [list(ctx_ids)], stoi, itos, target_codons, hard_cap, require_terminal_stop=require_terminal_stop,
        temperature=temperature, topk=topk, termination_bias_enabled=termination_bias_enabled,
        termination_stop_bias=termination_stop_bias, termination_trigger_class_max=termination_trigger_class_max,
        termination_bias_window=termination_bias_window, cds_only=cds_only, seed=seed, streams=[stream],
        multi_offset_prior_enabled=multi_offset_prior_enabled, multi_offset_prior_weights=multi_offset_prior_weights)
    return ids, info


def generate_cds_red(model, device, ctx_ids: List[int], stoi: Dict[str, int], itos: List[str], target_codons: int,
                     hard_cap: int, max_attempts: int = 5, temperature: float = 1.0, topk: int = 0,
                     termination_bias_enabled: bool = False, termination_stop_bias: float = 0.0,
                     termination_trigger_class_max: int = 0, termination_bias_window: int = 0,
                     cds_only: bool = True, *, seed: int = 0,
                     stream: int = 0) -> Tuple[List[int], Dict[str, object]]:
    """Reset-and-discard for one prefix: retry until a terminal stop or max_attempts
    (generate.py:293-334); attempt i draws with round_seed(seed, i)."""
    total = 0
    last_ids: List[int] = []
    last_info: Dict[str, object] = {}
    for i in range(int(max_attempts)):
        last_ids, last_info = generate_cds_constrained(
            model, device, ctx_ids, stoi, itos, target_codons, hard_cap, require_terminal_stop=True,
            temperature=temperature, topk=topk, termination_bias_enabled=termination_bias_enabled,
            termination_stop_bias=termination_stop_bias,
            termination_trigger_class_max=termination_trigger_class_max,
            termination_bias_window=termination_bias_window, cds_only=cds_only, seed=round_seed(seed, i + 1),
            stream=stream)
        total += last_info["generated_codons"]
        if last_info["had_terminal_stop"]:
            last_info["attempts"] = i + 1
            last_info["total_tokens_red"] = total
            return last_ids, last_info
    last_info["attempts"] = int(max_attempts)
    last_info["total_tokens_red"] = total
    return last_ids, last_info


def batch_red_sampler(model, device, contexts: List[List[int]], stoi: Dict[str, int], itos: List[str],
                      target_codons: int, hard_cap: int, global_token_budget: int, temperature: float = 1.0,
                      topk: int = 0, termination_bias_enabled: bool = False, termination_stop_bias: float = 0.0,
                      termination_trigger_class_max: int = 0, termination_bias_window: int = 0,
                      cds_only: bool = True, *, seed: int = 0):
    """Reset-and-discard across prefixes (generate.py:337-397): returns (solved {index: (ids, info)},
    remaining [index], total_tokens).  Each round is ONE batch of all unsolved prefixes (stream =
    original index, seed = round_seed(seed, round)); the budget is then applied in original-index
    order over the round's generated_codons, and prefixes past the point where it is reached count
    as not attempted -- the outcome of the reference's sequential loop given the same draws."""
    active = list(range(len(contexts)))
    solved: Dict[int, Tuple[List[int], Dict[str, object]]] = {}
    total = 0
    round_idx = 0
    while active and total < global_token_budget:
        round_idx += 1
        res = _constrained_batch(
            model, [list(contexts[i]) for i in active], stoi, itos, target_codons, hard_cap,
            require_terminal_stop=True, temperature=temperature, topk=topk,
            termination_bias_enabled=termination_bias_enabled, termination_stop_bias=termination_stop_bias,
            termination_trigger_class_max=termination_trigger_class_max,
            termination_bias_window=termination_bias_window, cds_only=cds_only,
            seed=round_seed(seed, round_idx), streams=active)
        nxt = []
        for i, (ids, info) in zip(active, res):
            if total >= global_token_budget:
                nxt.append(i)
                continue
            total += info["generated_codons"]
            if info["had_terminal_stop"]:
                info["round"] = round_idx
                solved[i] = (ids, info)
            else:
                nxt.append(i)
        active = nxt
    return solved, active, total


def synonymous_info(ctx_len: int, ids: Sequence[int], target_protein: str, *, critic: bool = False,
                    ebm: bool = False) -> Dict[str, object]:
    """generate_cds_synonymous's info (generate.py:738-752)."""
    return {
        "protocol": "guided",
        "guidance_components": ["synonymous_template", *(["ebm" if ebm else "critic"] if critic or ebm else [])],
        "had_terminal_stop": True,
        "early_stop": False,
        "hit_hard_cap": False,
        "target_codons": len(target_protein) + 1,
        "generated_codons": len(target_protein) + 1,
        "cds_only": True,
        "require_terminal_stop": True,
        "generated_tokens": len(ids) - int(ctx_len),
    }


def generate_cds_synonymous(model, critic_model, c_tokenizer, device, ctx_ids: List[int], stoi: Dict[str, int],
                            itos: List[str], target_protein: str, alpha: float = 0.5, guide_top_k: int = 5,
                            target_task: str = "stability", target_class_idx: int | None = None, ebm_model=None,
                            temperature: float = 1.0, *, seed: int = 0,
                            stream: int = 0) -> Tuple[List[int], Dict[str, object]]:
    """A CDS that translates exactly to ``target_protein`` (generate.py:642-753): one draw per
    residue among its synonymous codons (upper-cased; a residue without a codon in the vocabulary
    draws among all codon tokens), then one among the stop codons, then <EOS_CDS> when the
    vocabulary has it.  The stop rules are off; the sequence ends with its plan.  The temperature
    applies to every draw, the stop codon's included.  Critic / EBM blending (alpha != 0 with a
    critic or EBM model) needs the second model in the loop and is not part of the batched
    generator."""
    if (critic_model is not None or ebm_model is not None) and alpha != 0.0:
        raise NotImplementedError("critic / EBM guided synonymous generation is outside the batched generator")
    sets = TokenSets(stoi, itos, int(model.vocab_size))
    plan = synonymous_plan(sets, target_protein)
    (ids, _), = generate_batch(model, [list(ctx_ids)], stoi, itos, seed=seed, streams=[stream], max_tokens=INT_MAX,
                               temperature=temperature, stop_on_eos=False, stop_on_bio_stop=False,
                               token_sets=sets.array(), plans=[plan], end_with_plan=True)
    eos = stoi.get("<EOS_CDS>")
    if eos is not None:
        ids = ids + [eos]
    return ids, synonymous_info(len(ctx_ids), ids, target_protein, critic=critic_model is not None,
                                ebm=ebm_model is not None)


__all__ = ["generate_batch", "generate_model_raw", "generate_cds_constrained", "generate_cds_red",
           "batch_red_sampler", "generate_cds_synonymous", "STOP_CODONS", "CODON_TABLE", "AA_TO_CODONS",
           "TokenSets", "synonymous_plan", "synonymous_info", "translate", "token_classes", "cds_mask", "raw_info",
           "constrained_info", "state_record", "round_seed"]
