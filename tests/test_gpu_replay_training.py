"""`run_training` with the termination-head correction stages (training/loop.py): the replay loss
(schedule, data order, clipping, class weights, run files), a frozen-backbone run and its resume,
and a world-2 run with replay on.  fp32 engine, dropout 0, the tiny setup of test_gpu_trainer_ddp.

Tolerance of a loss against the oracle: 1e-5 relative (test_gpu_aux.py).
"""
import csv
import json
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from oracle import tinygpt_oracle as O

pytestmark = pytest.mark.gpu

T = 32
REPLAY_CW = [2.0, 1.5, 1.0, 0.5, 0.25]


def _setup(root, **over):
    rng = np.random.default_rng(3)
    seq = rng.integers(4, 68, size=(26, T + 1)).astype(np.int32)
    seq[:, 10] = 3
    cfg = {"vocab_size": 68, "block_size": T, "n_layer": 2, "n_head": 2, "n_embd": 64, "dropout": 0.0,
           "batch_size": 2, "grad_accum_steps": 2, "max_nonfinite_accumulation_groups": 3, "lr": 3e-3,
           "min_lr": 1e-4, "weight_decay": 0.05, "warmup_steps": 1, "epochs": 2, "optimizer": "adamw",
           "scheduler": "cosine", "early_stop_patience": 5, "seed": 42, "compute_dtype": "fp32",
           "label_smoothing": 0.05}
    cfg.update(over)
    itos = root / "itos.txt"
    itos.write_text("\n".join(f"token_{i}" for i in range(68)) + "\n")
    cfg["itos_path"] = str(itos)
    # 20 train rows -> 10 batches of 2; 6 val rows -> 3 batches
    np.savez(root / "train.npz", X=seq[:20, :-1], Y=seq[:20, 1:])
    np.savez(root / "val.npz", X=seq[20:, :-1], Y=seq[20:, 1:])
    cp = root / "config.yaml"
    cp.write_text(yaml.safe_dump(cfg))
    return cfg, cp


def _args(root, cp, run_id, resume=None):
    return SimpleNamespace(config=str(cp), run_id=run_id, resume=resume, transfer_from=None,
                           train_npz=[str(root / "train.npz")], val_npz=[str(root / "val.npz")],
                           test_npz=[str(root / "val.npz")])


def _replay_file(root):
    """5 records: one longer than the block (clipped on the left), windows of different lengths"""
    from codonlm_amd.replay import replay_labels
    rng = np.random.default_rng(9)
    path = root / "replay.jsonl"
    with path.open("w") as f:
        for n, prefix, window in ((20, 6, 31), (T, 4, 9), (T + 13, 20, 31), (12, 3, 2), (27, 1, 5)):
            ids = [1] + [int(t) for t in rng.integers(4, 68, size=n - 1)]
            f.write(json.dumps({"ids": ids, "labels": replay_labels(n, prefix, window, (0, 3, 10, 30))}) + "\n")
    return path


REPLAY = {"replay_loss_enabled": True, "replay_every_microbatches": 2, "replay_batch_size": 2,
          "replay_loss_weight": 0.3, "replay_class_weights": REPLAY_CW, "replay_data": "replay.jsonl"}


_ORIG = {}


def _train(monkeypatch, root, cfg, cp, run_id, resume=None):
    """run_training in this process; returns what _finish saw and the model as build_model left it"""
    import codonlm_amd.training.loop as loop_mod
    monkeypatch.chdir(root)
    got = {}
    # the module's own functions, also on a second call within one test (the first call's patches
    # are still in place then, and chaining to them would overwrite the first call's record)
    orig_finish, orig_build = _ORIG.setdefault("fns", (loop_mod._finish, loop_mod.build_model))

    def finish(is_main, ckpt_dir, scores_dir, run_id_, t_wall0, st, health, model, history, status):
        got.update(step=st.step, status=status, history=[dict(h) for h in history],
                   named={k: v.detach().cpu().clone() for k, v in model.named_parameters()})
        return orig_finish(is_main, ckpt_dir, scores_dir, run_id_, t_wall0, st, health, model, history, status)

    def build(cfg_, device):
        m = orig_build(cfg_, device)
        got["initial"] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        got["cfg"] = cfg_
        return m
    monkeypatch.setattr(loop_mod, "_finish", finish)
    monkeypatch.setattr(loop_mod, "build_model", build)
    loop_mod.run_training(dict(cfg), _args(root, cp, run_id, resume))
    return got


def test_replay_schedule_data_order_and_run_files(tmp_path, monkeypatch, capsys):
    """lr 1e-30: the parameters stay at their initial values, so epoch 1's logged replay loss is the
    mean of the oracle's loss over exactly the replay batches the reference's DataLoader (seed + 17,
    shuffled, restarted when exhausted) yields at microbatches 2, 4, 6, 8, 10."""
    from torch.utils.data import DataLoader
    from codonlm_amd.replay import GeneratedTerminationReplayDataset
    _replay_file(tmp_path)
    cfg, cp = _setup(tmp_path, lr=1e-30, lr_embedding=1e-30, min_lr=1e-30, epochs=1, **REPLAY)
    got = _train(monkeypatch, tmp_path, cfg, cp, "replay-schedule")
    out = capsys.readouterr().out
    assert "[loss] replay_termination weight=0.3" in out and "[replay] loaded 5 generated-state records" in out
    ocfg = O.OracleConfig(vocab_size=68, block_size=T, n_layer=2, n_head=2, n_embd=64, sep_id=3, label_smoothing=0.05,
                          termination_aux=True)
    params = {k: v.numpy() for k, v in got["initial"].items() if k in O.param_shapes(ocfg)}
    ds = GeneratedTerminationReplayDataset(tmp_path / "replay.jsonl", T)
    gen = torch.Generator()
    gen.manual_seed(42 + 17)
    loader = DataLoader(ds, batch_size=2, shuffle=True, num_workers=0, drop_last=False, generator=gen)
    losses, it = [], iter(loader)
    cw = torch.tensor(REPLAY_CW)
    for _ in range(5):
        try:
            rx, ry = next(it)
        except StopIteration:
            it = iter(loader)
            rx, ry = next(it)
        with torch.no_grad():
            o = O.forward(ocfg, O._to_t(params, False), rx.numpy())
            losses.append(float(O.termination_loss(o["aux"]["termination_logits"], ry.numpy(), cw)))
    want = float(np.mean(losses))
    h = got["history"][0]
    print("replay losses", losses, "mean", want, "logged", h["train_replay_term_loss"])
    assert abs(h["train_replay_term_loss"] - want) <= 1e-5 * max(1.0, abs(want))
    # run files
    run = tmp_path / "runs/replay-schedule"
    rows = list(csv.reader((run / "scores/curves.csv").open()))
    assert rows[0][-1] == "train_replay_term_loss" and abs(float(rows[1][-1]) - want) <= 1e-4
    metrics = json.loads((run / "scores/metrics.json").read_text())
    assert abs(metrics["last_train_replay_term_loss"] - want) <= 1e-5 * max(1.0, abs(want))
    ck = torch.load(run / "checkpoints/last.pt", map_location="cpu", weights_only=True)
    assert abs(ck["train_replay_term_loss"] - want) <= 1e-5 * max(1.0, abs(want))
    assert ck["cfg"]["replay_examples"] == 5 and ck["cfg"]["replay_data"].endswith("replay.jsonl")


def test_zero_replay_weight_equals_replay_disabled(tmp_path, monkeypatch):
    _replay_file(tmp_path)
    cfg0, cp0 = _setup(tmp_path, termination_loss_enabled=True, epochs=1)
    ref = _train(monkeypatch, tmp_path, cfg0, cp0, "replay-off")
    cfg1, cp1 = _setup(tmp_path, termination_loss_enabled=True, epochs=1, **dict(REPLAY, replay_loss_weight=0.0))
    got = _train(monkeypatch, tmp_path, cfg1, cp1, "replay-zero")
    assert got["step"] == ref["step"] == 5
    assert got["history"][0]["train_replay_term_loss"] > 0 and ref["history"][0]["train_replay_term_loss"] is None
    moved = 0
    for k, v in ref["named"].items():
        assert bool((got["named"][k] == v).all()), k
        moved += int(not torch.equal(v, ref["initial"][k]))
    assert moved > 0


def test_frozen_backbone_run_and_resume(tmp_path, monkeypatch, capsys):
    over = dict(freeze_backbone=True, termination_loss_enabled=True, multi_offset_loss_enabled=True,
                multi_offset_targets=[2, 4], lr_embedding=5e-3)
    cfg, cp = _setup(tmp_path, **over)
    got = _train(monkeypatch, tmp_path, cfg, cp, "frozen")
    assert "[freeze] Backbone frozen:" in capsys.readouterr().out
    assert got["status"] == "completed" and got["step"] == 10
    for h in got["history"]:
        assert all(np.isfinite(h[k]) for k in ("train_loss", "val_loss", "train_next_loss", "train_term_loss"))
    ck = torch.load(tmp_path / "runs/frozen/checkpoints/best.pt", map_location="cpu", weights_only=True)
    heads = 0
    for k, v in got["initial"].items():
        if k.startswith(("termination_head", "offset_projs")):
            assert not torch.equal(ck["model"][k], v), k
            heads += 1
        else:
            assert torch.equal(ck["model"][k], v), k
    assert heads == 10
    # the checkpoint resumes: one more epoch, the backbone still untouched
    cfg3 = dict(cfg, epochs=3)
    cp3 = tmp_path / "resume.yaml"
    cp3.write_text(yaml.safe_dump(cfg3))
    again = _train(monkeypatch, tmp_path, cfg3, cp3, "frozen", resume=str(tmp_path / "runs/frozen/checkpoints/last.pt"))
    assert again["status"] == "completed" and again["step"] == 15
    for k, v in got["initial"].items():
        if not k.startswith(("termination_head", "offset_projs")) and k in again["named"]:
            assert torch.equal(again["named"][k], v), k


def test_frozen_backbone_needs_an_aux_head(tmp_path, monkeypatch):
    cfg, cp = _setup(tmp_path, freeze_backbone=True)
    with pytest.raises(ValueError, match="nothing to train"):
        _train(monkeypatch, tmp_path, cfg, cp, "frozen-empty")


# ------------------------------------------------------------------ world = 2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, root, cfg, cp, run_id, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank))
    os.chdir(root)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from codonlm_amd.training import loop
        captured = {}
        orig_finish = loop._finish

        def finish(is_main, ckpt_dir, scores_dir, run_id_, t_wall0, st, health, model, history, status):
            captured.update(step=st.step, status=status, history=[dict(h) for h in history],
                            flat=model.flat_parameters().detach().cpu().clone())
            return orig_finish(is_main, ckpt_dir, scores_dir, run_id_, t_wall0, st, health, model, history, status)
        loop._finish = finish
        loop.run_training(dict(cfg), _args(root, cp, run_id))
        dist.barrier()
        out[rank] = captured
    finally:
        dist.destroy_process_group()


def test_world2_with_replay(tmp_path):
    """Both ranks run the replay microbatches, all-reduce at the end of the group and finish with
    identical weights; a rank out of collective step is killed at its timeout instead of hanging."""
    _replay_file(tmp_path)
    cfg, cp = _setup(tmp_path, termination_loss_enabled=True, **REPLAY)
    out = mp.Manager().dict()
    ctx = mp.start_processes(_worker, args=(2, _free_port(), tmp_path, cfg, cp, "ddp-replay", out), nprocs=2,
                             join=False, start_method="spawn")
    waited = 0
    while not ctx.join(timeout=5):
        waited += 5
        if waited >= 240:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail("world-2 run_training with replay did not finish: ranks out of collective step")
    r0, r1 = out[0], out[1]
    assert r0["status"] == r1["status"] == "completed"
    assert r0["step"] == r1["step"] == 6
    assert torch.equal(r0["flat"], r1["flat"]), "ranks diverged"
    for r in (r0, r1):
        for h in r["history"]:
            for k in ("train_loss", "val_loss", "train_next_loss", "val_next_loss", "train_term_loss",
                      "val_term_loss", "train_replay_term_loss"):
                assert np.isfinite(h[k]), (k, h[k])
