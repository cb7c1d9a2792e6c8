#!/usr/bin/env python3
"""Golden vectors of the termination-head replay workflow, made by running the REAL reference
(build container only, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_replay.py

replay_dataset.npz   what the reference GeneratedTerminationReplayDataset (src/codonlm/replay.py)
                     returns for the hand-written replay_fixture.jsonl at block sizes 8 and 16, and
                     the outputs of _replay_labels (scripts/build_generated_prefix_replay.py) for a
                     handful of (len, prefix, window, edges) cases.
replay_objective.npz one replay microbatch as loop.py:1075-1142 runs it, on the aux_objective
                     geometry, parameters and main batch (aux_objective.npz): objective(main) +
                     w * termination_aux_loss(replay batch, sparse labels, class weights) through the
                     reference TinyGPT (dropout 0) and every parameter gradient.
Inputs and outputs only, never reference code.
"""
from __future__ import annotations

import importlib.util
import json
import sys

import numpy as np
import torch

import make_golden as MG  # noqa: E402  (sets up the reference import path)
from src.codonlm.replay import GeneratedTerminationReplayDataset  # noqa: E402  (reference)

HERE = MG.HERE

LABEL_CASES = [  # (len(ids), prefix_tokens, window, bucket_edges)
    (40, 10, 31, (0, 3, 10, 30)), (40, 35, 31, (0, 3, 10, 30)), (12, 12, 31, (0, 3, 10, 30)),
    (12, 20, 5, (0, 3, 10, 30)), (100, 1, 31, (0, 3, 10, 30)), (50, 4, 0, (0, 3, 10, 30)),
    (50, 4, -3, (0, 3, 10, 30)), (64, 8, 40, (0, 1, 2, 5, 8)), (9, 0, 100, (2,)), (30, 3, 12, ()),
]
REPLAY_WEIGHT = 0.7
REPLAY_CLASS_WEIGHTS = [2.0, 1.5, 1.0, 0.5, 0.25]


def dataset_case():
    out = {}
    for bs in (8, 16):
        ds = GeneratedTerminationReplayDataset(HERE / "replay_fixture.jsonl", bs)
        xs, ys = zip(*(ds[i] for i in range(len(ds))))
        out[f"x_{bs}"] = torch.stack(xs).numpy()
        out[f"y_{bs}"] = torch.stack(ys).numpy()
    spec = importlib.util.spec_from_file_location("ref_build_replay",
                                                  f"{MG.REF}/scripts/build_generated_prefix_replay.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_build_replay"] = mod
    spec.loader.exec_module(mod)
    out["label_cases"] = np.array(json.dumps([[n, p, w, list(e)] for n, p, w, e in LABEL_CASES]))
    for i, (n, p, w, e) in enumerate(LABEL_CASES):
        lab = mod._replay_labels(list(range(n)), prefix_tokens=p, window=w, bucket_edges=e)
        out[f"labels_{i}"] = np.array([[d["pos"], d["class"]] for d in lab], dtype=np.int64).reshape(-1, 2)
    np.savez_compressed(HERE / "replay_dataset.npz", **out)
    print("[golden] replay_dataset:", {k: v.shape for k, v in out.items() if k[0] in "xy"})


def objective_case():
    z = np.load(HERE / "aux_objective.npz", allow_pickle=False)
    cfgd = json.loads(str(z["config"]))
    cfg = MG.OracleConfig(**cfgd)
    params = {k[6:]: z[k] for k in z.files if k.startswith("param/")}
    A = MG.AUX_OBJECTIVE
    model = MG.build_ref(cfg, params)
    model.train()
    x, y = torch.from_numpy(z["idx"]), torch.from_numpy(z["targets"])
    _, loss, aux = model(x, y, return_aux=True)
    lw = model.loss_weights if not torch.all(model.loss_weights == 1.0).item() else None
    off_total, _ = MG.ref_obj.multi_offset_lm_loss(aux["offset_logits"], y, A["offset_weights"],
                                                   label_smoothing=cfg.label_smoothing, loss_weights=lw)
    labels = MG.ref_obj.termination_distance_bucket_labels(y, stop_ids=A["stop_ids"], bucket_edges=A["bucket_edges"])
    term = MG.ref_obj.termination_aux_loss(aux["termination_logits"], labels,
                                           class_weights=torch.tensor(A["term_class_weights"]))
    main = loss + off_total + A["term_weight"] * term
    # the replay batch: three rows, PAD tails as the dataset leaves them, sparse labels on the last states
    rng = np.random.default_rng(99)
    T = cfg.block_size
    rx = np.zeros((3, T), np.int64)
    ry = np.full((3, T), -100, np.int64)
    for b, n in enumerate((T, 41, 17)):
        rx[b, :n] = rng.integers(4, 68, size=n)
        rx[b, 0] = 1
        first = max(3, n - 1 - (31, 9, 4)[b])
        for pos in range(first, n):
            ry[b, pos] = sum((n - 1 - pos) > e for e in (0, 3, 10, 30))
    _, none_loss, raux = model(torch.from_numpy(rx), return_aux=True)
    assert none_loss is None
    replay = MG.ref_obj.termination_aux_loss(raux["termination_logits"], torch.from_numpy(ry),
                                             class_weights=torch.tensor(REPLAY_CLASS_WEIGHTS))
    total = main + REPLAY_WEIGHT * replay
    total.backward()
    out = {"config": np.array(json.dumps(cfgd)), "replay_idx": rx, "replay_labels": ry,
           "replay_weight": np.array(REPLAY_WEIGHT), "replay_class_weights": np.array(REPLAY_CLASS_WEIGHTS, np.float32),
           "main": np.array(main.item()), "replay_loss": np.array(replay.item()), "total": np.array(total.item())}
    for k, p in model.named_parameters():
        out[f"grad/{k}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
    np.savez_compressed(HERE / "replay_objective.npz", **out)
    print(f"[golden] replay_objective: main={main.item():.6f} replay={replay.item():.6f} total={total.item():.6f}")


if __name__ == "__main__":
    torch.manual_seed(0)
    dataset_case()
    objective_case()
