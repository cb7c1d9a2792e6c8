"""Prefix-generation benchmark on the MI355X (mirrors scripts/eval_generation_prefix.py).

Real CDS prefixes of k codons are continued under paired protocols -- ``raw_model`` (the whole
vocabulary, no forced end), ``cds_constrained`` (codon tokens only) and, when a guidance flag is set,
``guided`` -- and every continuation gets the reference's GQS components and a memorization audit
against the training set.

Two things differ from the reference, neither in what is computed:

* the reference runs one full-recompute generator per (gene, k, sample, protocol); here every
  (gene, k, sample) of a protocol is one row of a ``generate.generate_batch`` call, ``batch_size`` rows
  at a time.  A row's tokens depend only on (seed, stream) with seed = ``--seed`` and stream =
  ``sample_seed(seed, gene, k, sample)``, the reference's sha256 rule, so the three protocols of a row
  share their draws and batching does not change a row;
* ``train_overlap_10`` / ``train_overlap_20`` come from ``memorization.TrainIndex`` (an exact window
  index in device memory) instead of a Python set of tuples.

The metric functions below restate ``score_protocol`` (:985-1057) and the closures of ``main`` it
calls, argument for argument; tests/test_gen_prefix_cpu.py holds them to the reference's own returns.
"""
from __future__ import annotations

import csv
import hashlib
import json
import statistics
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

PRESETS = {
    "quick": {"max_genes": 10, "samples": 2, "max_new": 100},
    "standard": {"max_genes": 20, "samples": 3, "max_new": 300},
    "full": {"max_genes": 50, "samples": 5, "max_new": 300},
}
PROTOCOLS = ("raw_model", "cds_constrained", "guided")
STOPS = {"TAA", "TAG", "TGA"}

# the reference's CODON_TO_AA (:381-448): the standard code with the stop codons named "Stop"
_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV_Y_YSSSS_CWCLFLF"
CODON_TO_AA: Dict[str, str] = {a + b + c: ("Stop" if _CODE[16 * i + 4 * j + k] == "_" else _CODE[16 * i + 4 * j + k])
                               for i, a in enumerate("ACGT") for j, b in enumerate("ACGT")
                               for k, c in enumerate("ACGT")}


# ------------------------------------------------------------------ metrics
def sample_seed(base_seed: int, gene_idx: int, k: int, sample_id: int) -> int:
    """sha256("base:gene:k:sample")[0:4], big-endian (_sample_seed :82-84)."""
    payload = f"{base_seed}:{gene_idx}:{k}:{sample_id}".encode()
    return int.from_bytes(hashlib.sha256(payload).digest()[:4], "big")


def bootstrap_interval(values: Sequence[float], *, statistic: str, seed: int, n_resamples: int) -> Tuple[float, float]:
    """The 95% percentile bootstrap of the mean or the median (_bootstrap_interval :87-104)."""
    array = np.asarray(values, dtype=np.float64)
    if array.size == 0:
        return float("nan"), float("nan")
    if array.size == 1 or n_resamples <= 0:
        value = float(np.median(array) if statistic == "median" else np.mean(array))
        return value, value
    rng = np.random.default_rng(seed)
    sampled = array[rng.integers(0, array.size, size=(int(n_resamples), array.size))]
    estimates = np.median(sampled, axis=1) if statistic == "median" else np.mean(sampled, axis=1)
    low, high = np.quantile(estimates, [0.025, 0.975])
    return float(low), float(high)


def codon_to_aa(codon: str) -> str:
    return CODON_TO_AA.get(codon, "?")


def aa_seq(codons: Sequence[str]) -> List[str]:
    return [codon_to_aa(c) for c in codons if len(c) == 3]


def is_codon(tok: str) -> bool:
    return len(tok) == 3 and set(tok) <= set("ACGT")


def ngram_repeat_ratio(tokens: Sequence[str], n: int = 3) -> float:
    """The fraction of repeated n-grams over non-overlapping windows (_ngram_repeat_ratio :459-469)."""
    if len(tokens) < n:
        return 0.0
    grams = [tuple(tokens[i:i + n]) for i in range(0, len(tokens) - n + 1, n)]
    total = len(grams)
    return 1.0 - (len(set(grams)) / total) if total else 0.0


def score_stop_behavior(gen_codons: Sequence[str], truth_len_codons: int) -> Tuple[float, bool, bool]:
    """(stop_score, valid_end, early_stop) (_score_stop_behavior :485-508): 1 for a terminal stop codon,
    0.5 when a stop also occurs before 90% of the truth length; without a terminal stop the score
    decays with the length error, reaching 0 at 20%."""
    valid_end = len(gen_codons) > 0 and gen_codons[-1] in STOPS
    early = False
    cutoff = max(1, int(0.9 * truth_len_codons))
    for i, c in enumerate(gen_codons[:-1]):
        if c in STOPS and i < cutoff:
            early = True
            break
    if valid_end:
        stop_score = 1.0 if not early else 0.5
    else:
        tau = abs(len(gen_codons) - truth_len_codons) / max(1, truth_len_codons)
        stop_score = max(0.0, 1.0 - tau / 0.2)
    return float(stop_score), bool(valid_end), bool(early)


def aa_identity(truth: Sequence[str], gen: Sequence[str]) -> float:
    """Position-wise identity over the shorter of the two (:901-905)."""
    n = min(len(truth), len(gen))
    if n == 0:
        return 0.0
    return float(sum(1 for i in range(n) if truth[i] == gen[i])) / n


def syn_rate(truth_cod: Sequence[str], gen_cod: Sequence[str]) -> float:
    """The fraction of positions whose codons code the same residue, stops excluded (:907-916)."""
    n = min(len(truth_cod), len(gen_cod))
    if n == 0:
        return 0.0
    cnt = 0
    for i in range(n):
        a, b = codon_to_aa(truth_cod[i]), codon_to_aa(gen_cod[i])
        if a != "Stop" and b != "Stop" and a == b:
            cnt += 1
    return float(cnt) / n


def ppl_stability_from_losses(n_ids: int, losses) -> float:
    """ppl_stability (:918-938) given the per-token losses of the id list (``n_ids`` ids, n_ids - 1
    losses, 0 where the target id is 0): exp(-max(0, last - first) / 0.02) over the means of the first
    and last w = min(10, (n_ids - 1) // 4) losses, in float32 as the reference's tensor means are; 1.0 for
    fewer than 22 ids."""
    if n_ids < 22:
        return 1.0
    loss = np.asarray(losses, dtype=np.float32).reshape(-1)
    if loss.size != n_ids - 1:
        raise ValueError(f"{n_ids} ids have {n_ids - 1} losses, not {loss.size}")
    w = min(10, loss.size // 4)
    first = float(loss[:w].mean(dtype=np.float32))
    last = float(loss[-w:].mean(dtype=np.float32))
    return float(np.exp(-max(0.0, last - first) / 0.02))


class UsageReference:
    """The codon unigram of the CDS file over the vocabulary (:866-889) and ``usage_agree`` against it."""

    def __init__(self, itos: Sequence[str], unigram: np.ndarray):
        self.codon_mask = np.array([1 if is_codon(t) else 0 for t in itos], dtype=np.int32)
        unigram = np.asarray(unigram, dtype=np.float64).copy()
        if unigram.sum() == 0:
            unigram[:] = 1.0
        cod = unigram * self.codon_mask
        self.unigram = unigram
        self.unigram_cod = cod / max(1e-9, cod.sum())

    @classmethod
    def from_lines(cls, lines, itos: Sequence[str], stoi: Dict[str, int], max_lines: int = 10000) -> "UsageReference":
        unigram = np.zeros(len(itos), dtype=np.float64)
        for n, line in enumerate(lines):
            if n >= max_lines:
                break
            seq = line.strip().upper().replace("U", "T")
            for i in range(0, len(seq) // 3 * 3, 3):
                j = stoi.get(seq[i:i + 3])
                if j is not None:
                    unigram[j] += 1
        return cls(itos, unigram)

    def usage_agree(self, gen_ids: Sequence[int]) -> float:
        return usage_agree(gen_ids, self.unigram_cod, self.codon_mask)


def usage_agree(gen_ids: Sequence[int], unigram_cod: np.ndarray, codon_mask: np.ndarray) -> float:
    """1 - min(1, KL(generated codon usage || reference usage) / KL0), KL0 = 0.5 (:940-952)."""
    counts = np.zeros_like(np.asarray(unigram_cod, dtype=np.float64))
    for j in gen_ids:
        counts[int(j)] += 1
    p = counts * codon_mask
    s = p.sum()
    if s <= 0:
        return 0.0
    p = p / s
    kl = float((p * (np.log((p + 1e-12) / (unigram_cod + 1e-12)))).sum())
    return float(max(0.0, 1.0 - min(1.0, kl / 0.5)))


def frame_integrity(gen_codons: Sequence[str]) -> float:
    return 1.0 if all(is_codon(c) for c in gen_codons) else 0.0


def gqs(stop_score, aaid, syn, stab, norep, usage, frame) -> float:
    """The generation quality score (:958-967)."""
    return 100.0 * (0.30 * stop_score + 0.20 * aaid + 0.15 * syn + 0.10 * stab + 0.10 * norep + 0.10 * usage
                    + 0.05 * frame)


# ------------------------------------------------------------------ records (the reference's columns, in order)
@dataclass
class SampleResult:
    run_id: str
    gene_idx: int
    k: int
    sample_id: int
    aa_identity: float
    syn_rate: float
    stop_score: float
    frame_integrity: float
    ppl_stability: float
    no_repeat: float
    usage_agree: float
    gqs: float
    gen_len: int
    valid_end: bool
    early_stop: bool
    gen_len_codons: int
    had_terminal_stop: bool
    hit_hard_cap: bool
    target_codons: int
    termination_bias_steps: int
    last_termination_class: object
    critic_stability: float = 0.0
    critic_family_prob: float = 0.0
    critic_function_prob: Optional[float] = None
    raw_gqs: float = 0.0
    raw_gen_len: int = 0
    raw_had_terminal_stop: bool = False
    raw_hit_hard_cap: bool = False
    raw_valid_end: bool = False
    train_overlap_10: float = 0.0
    train_overlap_20: float = 0.0


@dataclass
class ProtocolResult:
    run_id: str
    gene_idx: int
    k: int
    sample_id: int
    protocol: str
    sample_seed: int
    cds_only: bool
    require_terminal_stop: bool
    guidance_components: str
    temperature: float
    topk: int
    target_codons: int
    max_new_tokens: int
    generated_tokens: int
    aa_identity: float
    syn_rate: float
    stop_score: float
    frame_integrity: float
    ppl_stability: float
    no_repeat: float
    usage_agree: float
    gqs: float
    gen_len_codons: int
    valid_end: bool
    early_stop: bool
    had_terminal_stop: bool
    hit_hard_cap: bool
    stop_reason: str
    train_overlap_10: float
    train_overlap_20: float


SAMPLE_COLUMNS = tuple(SampleResult.__annotations__)
PROTOCOL_COLUMNS = tuple(ProtocolResult.__annotations__)
SUMMARY_COLUMNS = ("k", "termination_rate", "early_stop_rate", "median_gqs", "mean_aa_identity", "best_aa_identity",
                   "mean_aa_len", "median_aa_len", "terminal_stop_rate", "hard_cap_rate", "raw_termination_rate",
                   "raw_median_gqs", "raw_mean_aa_len", "raw_median_aa_len", "raw_terminal_stop_rate",
                   "raw_hard_cap_rate", "train_overlap_10", "train_overlap_20", "n")
PROTOCOL_SUMMARY_COLUMNS = ("k", "protocol", "n", "median_gqs", "median_gqs_ci_low", "median_gqs_ci_high",
                            "mean_aa_len", "mean_aa_len_ci_low", "mean_aa_len_ci_high", "terminal_stop_rate",
                            "terminal_stop_rate_ci_low", "terminal_stop_rate_ci_high", "hard_cap_rate",
                            "hard_cap_rate_ci_low", "hard_cap_rate_ci_high", "mean_train_overlap_10",
                            "mean_train_overlap_20")


@dataclass
class Settings:
    """The decoding and length settings of a benchmark run (the reference's flags and defaults)."""
    run_id: str = "run"
    k_list: Tuple[int, ...] = (1, 3, 5, 10)
    samples: int = 5
    max_new: int = 300
    temperature: float = 0.8
    topk: int = 5
    seed: int = 1337
    ci_resamples: int = 1000
    min_aa_len: int = 100
    target_aa_len: int = 256
    max_aa_len: int = 400
    require_terminal_stop: bool = False
    special_margin: int = 6
    termination_bias: bool = False
    termination_stop_bias: float = 0.0
    termination_trigger_class_max: int = 0
    termination_bias_window: int = 0
    allow_non_cds_tokens: bool = False
    multi_offset_prior: bool = False
    multi_offset_prior_weights: Optional[Dict[int, float]] = None
    gqs_normalize: str = "none"
    memorization_audit: bool = True
    batch_size: int = 256
    guide_top_k: int = 5

    def guidance(self) -> List[str]:
        """The guidance components the flags select, in the reference's order (:1091-1098)."""
        out = []
        if self.termination_bias:
            out.append("termination_bias")
        if self.multi_offset_prior:
            out.append("multi_offset_prior")
        if self.require_terminal_stop:
            out.append("forced_terminal_stop")
        if self.allow_non_cds_tokens:
            out.append("non_cds_tokens")
        return out


def length_plan(block_size: int, k: int, s: Settings) -> Tuple[int, int]:
    """(hard_cap, target_codons) of a prefix of k codons (:1077-1082)."""
    max_window_codons = int(block_size) - int(k) - int(s.special_margin)
    if max_window_codons < s.min_aa_len:
        raise ValueError("block_size too small for requested lengths and k")
    hard_cap = int(min(max_window_codons, s.max_aa_len, s.max_new))
    target_codons = int(min(s.target_aa_len, hard_cap))
    return hard_cap, int(max(target_codons, s.min_aa_len))


def truth_of(dna: str) -> Tuple[List[str], List[str]]:
    codons = [dna[i:i + 3] for i in range(0, (len(dna) // 3) * 3, 3)]
    return codons, aa_seq(codons)


@dataclass
class Row:
    """One (gene, k, sample) of the benchmark."""
    gene_idx: int
    k: int
    sample_id: int
    seed: int
    ctx_ids: List[int]
    hard_cap: int
    target_codons: int


def plan_rows(cds: Sequence[str], stoi: Dict[str, int], block_size: int, s: Settings) -> List[Row]:
    """Every (gene, k, sample) in the reference's loop order (:1068-1083)."""
    from .query_model import dna_prefix_to_ids
    rows = []
    for gene_idx, dna in enumerate(cds):
        n_truth = len(dna) // 3
        for k in s.k_list:
            ctx = dna_prefix_to_ids(dna[:3 * min(k, n_truth)], stoi)
            for sidx in range(s.samples):
                hard_cap, target = length_plan(block_size, k, s)
                rows.append(Row(gene_idx, int(k), sidx, sample_seed(s.seed, gene_idx, k, sidx), ctx, hard_cap, target))
    return rows


def _groups(rows: Sequence[Row], batch_size: int):
    """Chunks of rows that share (hard_cap, target_codons), which are sampler parameters of a batch."""
    by_key: Dict[Tuple[int, int], List[int]] = {}
    for i, r in enumerate(rows):
        by_key.setdefault((r.hard_cap, r.target_codons), []).append(i)
    for (hard_cap, target), idx in by_key.items():
        for a in range(0, len(idx), max(1, int(batch_size))):
            yield hard_cap, target, idx[a:a + max(1, int(batch_size))]


def generate_protocol(model, rows: Sequence[Row], stoi, itos, s: Settings, protocol: str):
    """[(ids, info)] per row for one protocol: ``generate_batch`` over chunks of ``batch_size`` rows,
    stream = the row's sample seed.  The calls are those of generate_model_raw /
    generate_cds_constrained with the same arguments, so a row equals the single call."""
    from . import generate as G
    out: List = [None] * len(rows)
    for hard_cap, target, idx in _groups(rows, s.batch_size):
        ctxs = [list(rows[i].ctx_ids) for i in idx]
        streams = [rows[i].seed for i in idx]
        topk = int(s.topk) if s.topk > 0 else 0
        if protocol == "raw_model":
            res = G.generate_batch(model, ctxs, stoi, itos, seed=s.seed, streams=streams, max_tokens=hard_cap,
                                   temperature=float(s.temperature), topk=topk)
            res = [(ids, G.raw_info(rec, hard_cap)) for ids, rec in res]
        else:
            guided = protocol == "guided"
            res = G._constrained_batch(
                model, ctxs, stoi, itos, target, hard_cap,
                require_terminal_stop=bool(s.require_terminal_stop) if guided else False,
                temperature=float(s.temperature), topk=topk,
                termination_bias_enabled=bool(s.termination_bias) if guided else False,
                termination_stop_bias=float(s.termination_stop_bias) if guided else 0.0,
                termination_trigger_class_max=int(s.termination_trigger_class_max) if guided else 0,
                termination_bias_window=int(s.termination_bias_window) if guided else 0,
                cds_only=(not bool(s.allow_non_cds_tokens)) if guided else True, seed=s.seed, streams=streams,
                multi_offset_prior_enabled=bool(s.multi_offset_prior) if guided else False,
                multi_offset_prior_weights=s.multi_offset_prior_weights if guided else None)
        for i, r in zip(idx, res):
            out[i] = r
    return out


def codons_of(generated_ids: Sequence[int], itos: Sequence[str]) -> List[str]:
    from .query_model import ids_to_codons
    return [tok for tok in ids_to_codons(list(generated_ids), itos) if is_codon(tok)]


def stability_losses(model, id_lists: Sequence[Sequence[int]], batch_size: int = 256) -> List[Optional[np.ndarray]]:
    """The per-token losses ppl_stability needs, for the id lists of at least 22 ids (None for the
    others): one batched scoring pass (score.token_logprobs_batch), loss = -log p, 0 where the target
    id is 0."""
    from . import score
    need = [i for i, ids in enumerate(id_lists) if len(ids) >= 22]
    out: List[Optional[np.ndarray]] = [None] * len(id_lists)
    if need:
        for i, lp in zip(need, score.token_logprobs_batch(model, [list(id_lists[i]) for i in need],
                                                          batch_size=batch_size)):
            out[i] = -lp
    return out


def score_rows(model, rows: Sequence[Row], results, protocol: str, cds: Sequence[str], stoi, itos, s: Settings,
               usage: UsageReference, train_indices: Dict[int, object], guidance: Sequence[str]):
    """score_protocol (:969-1057) over all rows of one protocol: (ProtocolResult list, metrics list)."""
    from . import memorization as M
    codon_lists = [codons_of(ids, itos) for ids, _ in results]
    stab_ids = [[stoi.get(c, 0) for c in codons] for codons in codon_lists]
    losses = stability_losses(model, stab_ids, s.batch_size)
    full_ids = [[stoi[c] for c in codons if c in stoi] for codons in codon_lists]
    overlaps = {}
    for n in (10, 20):
        index = train_indices.get(n)
        if index is not None and index.n_unique > 0:
            overlaps[n] = M.training_match_coverage(index, full_ids)
    out, metrics = [], []
    truths = {}
    for j, (row, (gen_ids, info), codons) in enumerate(zip(rows, results, codon_lists)):
        if row.gene_idx not in truths:
            truths[row.gene_idx] = truth_of(cds[row.gene_idx])
        truth_codons, truth_aa = truths[row.gene_idx]
        k = row.k
        continuation = codons[min(k, len(codons)):]
        continuation_ids = [stoi[c] for c in continuation if c in stoi]
        aaid = aa_identity(truth_aa[k:], aa_seq(continuation))
        syn = syn_rate(truth_codons[k:], continuation)
        stop_score, valid_end, early = score_stop_behavior(codons, truth_len_codons=len(truth_codons))
        stab = ppl_stability_from_losses(len(stab_ids[j]), losses[j]) if losses[j] is not None else 1.0
        no_repeat = 1.0 - ngram_repeat_ratio(codons, n=3)
        use = usage.usage_agree(continuation_ids)
        frame = frame_integrity(codons)
        score = gqs(stop_score, aaid, syn, stab, no_repeat, use, frame)
        o10 = float(overlaps[10][j]) if 10 in overlaps and len(full_ids[j]) >= 10 else 0.0
        o20 = float(overlaps[20][j]) if 20 in overlaps and len(full_ids[j]) >= 20 else 0.0
        out.append(ProtocolResult(
            run_id=s.run_id, gene_idx=row.gene_idx, k=k, sample_id=row.sample_id, protocol=protocol,
            sample_seed=row.seed, cds_only=bool(info.get("cds_only", protocol != "raw_model")),
            require_terminal_stop=bool(info.get("require_terminal_stop", False)),
            guidance_components=json.dumps(sorted(guidance)), temperature=float(s.temperature), topk=int(s.topk),
            target_codons=int(row.target_codons), max_new_tokens=int(row.hard_cap),
            generated_tokens=int(info.get("generated_tokens", max(0, len(gen_ids) - (k + 1)))),
            aa_identity=aaid, syn_rate=syn, stop_score=stop_score, frame_integrity=frame, ppl_stability=stab,
            no_repeat=no_repeat, usage_agree=use, gqs=score, gen_len_codons=len(codons), valid_end=valid_end,
            early_stop=early, had_terminal_stop=bool(info.get("had_terminal_stop", False)),
            hit_hard_cap=bool(info.get("hit_hard_cap", False)), stop_reason=str(info.get("stop_reason", "unspecified")),
            train_overlap_10=o10, train_overlap_20=o20))
        metrics.append({"codons": codons, "info": info})
    return out, metrics


def run_benchmark(model, cds: Sequence[str], stoi, itos, s: Settings, usage: UsageReference,
                  train_indices: Optional[Dict[int, object]] = None):
    """The whole measurement: (SampleResult rows, ProtocolResult rows in the reference's order,
    [(fasta id, sequence)], the guidance components).  ``train_indices`` maps a window length (10, 20)
    to a memorization.TrainIndex; None or a missing length leaves that overlap column 0."""
    train_indices = dict(train_indices or {}) if s.memorization_audit else {}
    guidance = s.guidance()
    is_guided = bool(guidance)
    rows = plan_rows(cds, stoi, int(model.block_size), s)
    scored = {}
    for protocol in ("raw_model", "cds_constrained") + (("guided",) if is_guided else ()):
        res = generate_protocol(model, rows, stoi, itos, s, protocol)
        scored[protocol] = score_rows(model, rows, res, protocol, cds, stoi, itos, s, usage, train_indices,
                                      guidance if protocol == "guided" else [])
    selected = "guided" if is_guided else "cds_constrained"
    samples, protocol_rows, sequences = [], [], []
    for j, row in enumerate(rows):
        raw, con, sel = scored["raw_model"][0][j], scored["cds_constrained"][0][j], scored[selected][0][j]
        protocol_rows.extend([raw, con])
        key = f"gene{row.gene_idx}_k{row.k}_sample{row.sample_id}_seed{row.seed}"
        sequences.append((f"raw_model_{key}", "".join(scored["raw_model"][1][j]["codons"])))
        sequences.append((f"cds_constrained_{key}", "".join(scored["cds_constrained"][1][j]["codons"])))
        if is_guided:
            protocol_rows.append(sel)
            sequences.append((f"guided_{key}", "".join(scored["guided"][1][j]["codons"])))
        info = scored[selected][1][j]["info"]
        samples.append(SampleResult(
            s.run_id, row.gene_idx, row.k, row.sample_id, sel.aa_identity, sel.syn_rate, sel.stop_score,
            sel.frame_integrity, sel.ppl_stability, sel.no_repeat, sel.usage_agree, sel.gqs, sel.gen_len_codons,
            sel.valid_end, sel.early_stop, gen_len_codons=sel.gen_len_codons,
            had_terminal_stop=bool(info.get("had_terminal_stop", False)), hit_hard_cap=bool(info.get("hit_hard_cap", False)),
            target_codons=int(row.target_codons), termination_bias_steps=int(info.get("termination_bias_steps", 0)),
            last_termination_class=info.get("last_termination_class"), critic_stability=0.0, critic_family_prob=0.0,
            critic_function_prob=0.0, raw_gqs=raw.gqs, raw_gen_len=raw.gen_len_codons,
            raw_had_terminal_stop=raw.had_terminal_stop, raw_hit_hard_cap=raw.hit_hard_cap, raw_valid_end=raw.valid_end,
            train_overlap_10=sel.train_overlap_10, train_overlap_20=sel.train_overlap_20))
    return samples, protocol_rows, sequences, guidance


# ------------------------------------------------------------------ summaries and files
def protocol_summary(protocol_rows: Sequence[ProtocolResult], s: Settings) -> List[dict]:
    """Per (k, protocol) the medians / means and their bootstrap intervals (:1368-1420)."""
    out = []
    for k in s.k_list:
        for protocol_index, protocol in enumerate(PROTOCOLS):
            sel = [r for r in protocol_rows if r.k == k and r.protocol == protocol]
            if not sel:
                continue
            ci_seed = sample_seed(s.seed, protocol_index, k, len(sel))
            columns = (("median_gqs", "median", [r.gqs for r in sel]),
                       ("mean_aa_len", "mean", [float(r.gen_len_codons) for r in sel]),
                       ("terminal_stop_rate", "mean", [float(r.had_terminal_stop) for r in sel]),
                       ("hard_cap_rate", "mean", [float(r.hit_hard_cap) for r in sel]))
            rec = {"k": k, "protocol": protocol, "n": len(sel)}
            for j, (name, stat, values) in enumerate(columns):
                low, high = bootstrap_interval(values, statistic=stat, seed=ci_seed + j, n_resamples=s.ci_resamples)
                rec[name] = float(np.median(values) if stat == "median" else np.mean(values))
                rec[name + "_ci_low"], rec[name + "_ci_high"] = low, high
            rec["mean_train_overlap_10"] = float(np.mean([r.train_overlap_10 for r in sel]))
            rec["mean_train_overlap_20"] = float(np.mean([r.train_overlap_20 for r in sel]))
            out.append({c: rec[c] for c in PROTOCOL_SUMMARY_COLUMNS})
    return out


def summary(samples: Sequence[SampleResult], s: Settings) -> List[dict]:
    """Per k the rates, medians and means of the selected protocol and the raw baseline (:1478-1563)."""
    out = []
    for k in s.k_list:
        rks = [r for r in samples if r.k == k]
        if not rks:
            continue
        n = len(rks)
        audit = s.memorization_audit
        rec = {
            "k": k,
            "termination_rate": sum(1 for r in rks if r.valid_end) / n,
            "early_stop_rate": sum(1 for r in rks if r.early_stop) / n,
            "median_gqs": float(statistics.median([r.gqs for r in rks])),
            "mean_aa_identity": float(sum(r.aa_identity for r in rks) / n),
            "best_aa_identity": float(max(r.aa_identity for r in rks)),
            "mean_aa_len": float(sum(r.gen_len_codons for r in rks) / n),
            "median_aa_len": float(statistics.median([r.gen_len_codons for r in rks])),
            "terminal_stop_rate": sum(1 for r in rks if r.had_terminal_stop) / n,
            "hard_cap_rate": sum(1 for r in rks if r.hit_hard_cap) / n,
            "raw_termination_rate": sum(1 for r in rks if r.raw_valid_end) / n,
            "raw_median_gqs": float(statistics.median([r.raw_gqs for r in rks])),
            "raw_mean_aa_len": float(sum(r.raw_gen_len for r in rks) / n),
            "raw_median_aa_len": float(statistics.median([r.raw_gen_len for r in rks])),
            "raw_terminal_stop_rate": sum(1 for r in rks if r.raw_had_terminal_stop) / n,
            "raw_hard_cap_rate": sum(1 for r in rks if r.raw_hit_hard_cap) / n,
            "train_overlap_10": float(sum(r.train_overlap_10 for r in rks) / n) if audit else 0.0,
            "train_overlap_20": float(sum(r.train_overlap_20 for r in rks) / n) if audit else 0.0,
        }
        if s.gqs_normalize == "len":
            norms = [r.gqs / float(max(1, r.target_codons or r.gen_len_codons)) for r in rks]
            rec["mean_gqs_norm"] = float(sum(norms) / len(norms))
            rec["median_gqs_norm"] = float(statistics.median(norms))
        rec["n"] = n
        out.append(rec)
    return out


def manifest(s: Settings, checkpoint: str, source_provenance: dict, guidance: Sequence[str], has_guided: bool) -> dict:
    """protocol_manifest.json (:1429-1470)."""
    protocols = {"raw_model": {"full_vocabulary": True, "forced_terminal_stop": False, "guidance_components": []},
                 "cds_constrained": {"full_vocabulary": False, "forced_terminal_stop": False, "guidance_components": []}}
    if has_guided:
        protocols["guided"] = {"full_vocabulary": bool(s.allow_non_cds_tokens),
                               "forced_terminal_stop": bool(s.require_terminal_stop),
                               "guidance_components": list(guidance)}
    return {"schema_version": 1, "run_id": s.run_id, "checkpoint": checkpoint, "source_data": source_provenance,
            "base_seed": int(s.seed), "sample_seed_derivation": "sha256(base_seed:gene_idx:k:sample_id)[0:4]",
            "confidence_interval": {"method": "percentile_bootstrap", "level": 0.95, "resamples": int(s.ci_resamples)},
            "decoding": {"temperature": float(s.temperature), "topk": int(s.topk), "guide_top_k": int(s.guide_top_k),
                         "max_new": int(s.max_new)},
            "protocols": protocols}


def write_outputs(out_dir: Path, samples, protocol_rows, sequences, s: Settings, manifest_record: dict) -> Dict[str, Path]:
    """The six files of the reference, with its column names and order."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = {name: out_dir / name for name in ("samples.csv", "protocol_samples.csv", "generated_protocols.fasta",
                                               "protocol_summary.csv", "protocol_manifest.json", "summary.csv")}
    for name, columns, records in (("samples.csv", SAMPLE_COLUMNS, samples),
                                   ("protocol_samples.csv", PROTOCOL_COLUMNS, protocol_rows)):
        with paths[name].open("w", newline="") as f:
            w = csv.writer(f)
            w.writerow(columns)
            for r in records:
                w.writerow([getattr(r, c) for c in columns])
    with paths["generated_protocols.fasta"].open("w") as f:
        for record_id, sequence in sequences:
            if sequence:
                f.write(f">{record_id}\n{sequence}\n")
    with paths["protocol_summary.csv"].open("w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(PROTOCOL_SUMMARY_COLUMNS))
        w.writeheader()
        w.writerows(protocol_summary(protocol_rows, s))
    paths["protocol_manifest.json"].write_text(json.dumps(manifest_record, indent=2, sort_keys=True) + "\n")
    rows = summary(samples, s)
    extra = ["mean_gqs_norm", "median_gqs_norm"] if any("mean_gqs_norm" in r for r in rows) else []
    with paths["summary.csv"].open("w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(SUMMARY_COLUMNS) + extra)
        w.writeheader()
        w.writerows(rows)
    return paths


__all__ = ["PRESETS", "PROTOCOLS", "CODON_TO_AA", "sample_seed", "bootstrap_interval", "codon_to_aa", "aa_seq",
           "ngram_repeat_ratio", "score_stop_behavior", "aa_identity", "syn_rate", "ppl_stability_from_losses",
           "UsageReference", "usage_agree", "frame_integrity", "gqs", "SampleResult", "ProtocolResult", "Settings",
           "length_plan", "plan_rows", "generate_protocol", "score_rows", "run_benchmark", "protocol_summary",
           "summary", "manifest", "write_outputs", "SAMPLE_COLUMNS", "PROTOCOL_COLUMNS", "SUMMARY_COLUMNS",
           "PROTOCOL_SUMMARY_COLUMNS", "stability_losses", "codons_of", "truth_of"]
