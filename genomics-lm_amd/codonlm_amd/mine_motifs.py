#!/usr/bin/env python3
"""Motif mining from a trained codon LM on the MI355X (mirrors scripts/mine_motifs.py).

    python -m codonlm_amd.mine_motifs --run_dir runs/<ID> --data_npz data.npz \
        [--n_samples 100] [--window_size 9] [--stride 3] [--n_clusters 10] [--pca 50] [--layer -1]

Same flags, special-token exclusion (canonical and legacy names looked up in the run's token list),
trimming to block_size, ``<run>/motif_mining/clusters.npz`` keys (``labels, centers, window_size,
stride, layer, method``) and ``motif_report.md`` layout (clusters by size descending, consensus,
first five examples) as the reference.  Added: ``--run_dir``, ``--seed``, ``--batch_size``,
``--dtype`` and the ``inertia, n_iter, seed`` keys.  The forwards, the window pooling and the
k-means steps run on the native engine (codonlm_amd.motifs); ``--method hdbscan`` is refused.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import motifs as M

SPECIAL_TOKENS = ("<pad>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>", "<bos>", "<eos>", "<eog>", "<PAD>")


def special_ids(tokens: Sequence[str]) -> List[int]:
    """Ids of the special tokens the run's token list holds (scripts/mine_motifs.py:77-87)."""
    stoi = {t: i for i, t in enumerate(tokens)}
    return [stoi[s] for s in SPECIAL_TOKENS if s in stoi]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Cluster sliding-window hidden-state embeddings into motifs.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--run_id", help="run under runs/")
    src.add_argument("--run_dir", help="run directory: checkpoints/best.pt and itos.txt")
    ap.add_argument("--data_npz", required=True, help="npz holding 'X' (token ids)")
    ap.add_argument("--n_samples", type=int, default=100)
    ap.add_argument("--window_size", type=int, default=9, help="sliding window size (in codons)")
    ap.add_argument("--stride", type=int, default=3)
    ap.add_argument("--n_clusters", type=int, default=10)
    ap.add_argument("--method", default="kmeans", choices=["kmeans", "hdbscan"])
    ap.add_argument("--pca", type=int, default=50, help="PCA components before clustering (0 = off)")
    ap.add_argument("--layer", type=int, default=-1, help="block to read (-1 is the last)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.method == "hdbscan":
        ap.error("--method hdbscan is not on the MI355X path: only kmeans runs on the native engine")
    from .score_mutations import load_model, load_vocab
    run_dir = Path(args.run_dir) if args.run_dir else Path("runs") / args.run_id
    run_id = args.run_id or run_dir.name
    print(f"[*] Loading model from {run_dir}...")
    model, _ = load_model(None, run_dir, args.dtype)
    tokens = load_vocab(None, run_dir)
    print(f"[*] Loading data from {args.data_npz}...")
    with np.load(args.data_npz, allow_pickle=False) as data:
        X_raw = data["X"][: args.n_samples]
    if X_raw.shape[1] > model.block_size:
        print(f"[!] Trimming sequences from {X_raw.shape[1]} to {model.block_size}")
        X_raw = X_raw[:, : model.block_size]
    X_raw = X_raw.astype(np.int64)
    print(f"[*] Extracting embeddings for {len(X_raw)} sequences (window={args.window_size}, stride={args.stride})...")
    res = M.mine(model, X_raw, window=args.window_size, stride=args.stride, n_clusters=args.n_clusters, pca=args.pca,
                 layer=args.layer, exclude_ids=special_ids(tokens), seed=args.seed, batch_size=args.batch_size,
                 method=args.method)
    if res is None:
        print("[!] No windows kept after filtering special tokens. Try a smaller window or check data.")
        return None
    print(f"[*] Extracted {len(res['labels'])} clean windows (filtered out special tokens).")
    print("[*] Generating motif report...")
    out_dir = run_dir / "motif_mining"
    out_dir.mkdir(parents=True, exist_ok=True)
    windows = M.window_tokens(X_raw, res["meta"], tokens)
    (out_dir / "motif_report.md").write_text(
        M.build_report(run_id, len(X_raw), res["labels"], windows, tokens, args.method, args.layer))
    out_path = out_dir / "clusters.npz"
    np.savez(out_path, labels=res["labels"], centers=res["centers"], window_size=args.window_size,
             stride=args.stride, layer=args.layer, method=args.method, inertia=res["inertia"],
             n_iter=res["n_iter"], seed=args.seed)
    print(f"[success] Motif mining complete. Results saved to {out_path}")
    return out_path


if __name__ == "__main__":
    main()
