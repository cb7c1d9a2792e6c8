#!/usr/bin/env python3
"""Golden vectors of the attention head statistics, made by running the REAL reference (build
container only, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attention.py

attention_heads.npz  for T in attention_restatement.GOLDEN_SHAPES (L = 2, B = 2, H = 3): the tokens,
                     the fp32 attention tensor (L, B, H, T, T) the restatement's SEP-masked softmax
                     gives -- the layout collect_artifacts_yaml.py captures -- and what the
                     reference's scripts/conference_attention._head_stats returns for it, once per
                     batch row (the function reads batch item 0: row b is passed as attn[:, b:b+1]).
Inputs and outputs only, never reference code.
"""
from __future__ import annotations

import sys

import numpy as np

import make_golden as MG  # noqa: E402  (sets up the reference import path)
from scripts import conference_attention as RA  # noqa: E402  (reference)

sys.path.insert(0, str(MG.HERE.parent))
import attention_restatement as AR  # noqa: E402  (the shared synthetic inputs)


def main():
    out = {}
    for T in AR.GOLDEN_SHAPES:
        idx, P = AR.golden_case(T)
        attn = P.astype(np.float32)
        stats = np.stack([RA._head_stats(attn[:, b:b + 1], [AR.ITOS[i] for i in idx[b]])
                          for b in range(idx.shape[0])])
        out[f"T{T}/tokens"], out[f"T{T}/attn"], out[f"T{T}/head_stats"] = idx, attn, stats
    path = MG.HERE / "attention_heads.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
