"""The termination-head correction steps on the engine: a replay microbatch (trunk-only forward,
fused termination loss, accumulating backward), the fused loss on an ordinary forward, the heads-only
backward of a frozen backbone and the frozen FusedAdamW step.

Geometry, parameters and main batch: the aux_objective golden.  Tolerances: the ones test_gpu_aux.py
uses against the oracle -- loss 1e-5 relative, gradients 2e-4 * max(1e-3, max|ref|); bf16 against the
dense path: loss 2e-2 relative, cosine similarity above 0.98 (test_aux_objective_bf16_close_and_trains).
replay_objective.npz holds the reference's own numbers for objective(main) + w * replay loss
(tests/golden/make_golden_replay.py).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import tinygpt_oracle as O
from test_gpu_model import DEV, make_model, _idx
from test_oracle_golden import aux_objective_args

pytestmark = pytest.mark.gpu


def _setup(dtype="fp32"):
    cfgd, g = load_golden("aux_objective")
    m, cfg, params = make_model(cfgd, dict(g, param_seed=np.array(0)), dtype=dtype)
    m.train()
    x, y = _idx(g)
    return m, cfg, params, g, x, y, aux_objective_args(g)


def _objective(m, x, y, cfg, args, fused):
    """the trainer's objective (loop.py:1075-1112); fused: the termination loss from the fused kernel"""
    from codonlm_amd.training import objectives as obj
    labels = obj.termination_distance_bucket_labels(y, stop_ids=args["stop_ids"], bucket_edges=args["bucket_edges"])
    cw = torch.tensor(args["term_class_weights"], device=DEV)
    if fused:
        logits, loss, aux = m(x, y, return_aux=True, termination_labels=labels, termination_class_weights=cw)
        assert "termination_logits" not in aux
        term = aux["termination_loss"]
    else:
        logits, loss, aux = m(x, y, return_aux=True)
        term = obj.termination_aux_loss(aux["termination_logits"], labels, class_weights=cw)
    lw = m.loss_weights if not torch.all(m.loss_weights == 1.0).item() else None
    off_total, _ = obj.multi_offset_lm_loss(aux["offset_logits"], y, args["offset_weights"],
                                            label_smoothing=cfg.label_smoothing, loss_weights=lw)
    return loss + off_total + args["term_weight"] * term, term


def _assert_grads(named, ref, what):
    for k, p in named:
        r = ref[k]
        r = r.numpy() if isinstance(r, torch.Tensor) else r
        s = max(1e-3, float(np.abs(r).max()))
        err = float(np.abs(p.grad.detach().cpu().numpy() - r).max())
        print(what, k, f"err {err:.3e} scale {s:.3e}")
        assert err <= 2e-4 * s, (what, k, err, s)


def _freeze_backbone(m):
    for k, p in m.named_parameters():
        if not k.startswith(("termination_head", "offset_projs")):
            p.requires_grad_(False)
    m.zero_grad()


def test_replay_microbatch_matches_reference_golden():
    """main forward + backward, then a trunk-only forward on the replay batch, the fused loss with the
    replay class weights and an accumulating backward: the reference's total, replay loss and every
    parameter gradient of objective(main) + w * replay_loss."""
    m, cfg, _, _, x, y, args = _setup()
    _, r = load_golden("replay_objective")
    w = float(r["replay_weight"])
    main, _ = _objective(m, x, y, cfg, args, fused=False)
    main.backward()
    rx, ry = torch.from_numpy(r["replay_idx"]).to(DEV), torch.from_numpy(r["replay_labels"]).to(DEV)
    logits, none_loss, aux = m(rx, return_aux=True, termination_labels=ry,
                               termination_class_weights=torch.from_numpy(r["replay_class_weights"]).to(DEV),
                               head=False)
    assert logits is None and none_loss is None and set(aux) == {"termination_loss"}
    replay = aux["termination_loss"]
    (w * replay).backward()
    total = main.item() + w * replay.item()
    print("replay", replay.item(), float(r["replay_loss"]), "total", total, float(r["total"]))
    assert abs(replay.item() - float(r["replay_loss"])) <= 1e-5 * max(1.0, abs(float(r["replay_loss"])))
    assert abs(total - float(r["total"])) <= 1e-5 * max(1.0, abs(float(r["total"])))
    _assert_grads(m.named_parameters(), {k[5:]: v for k, v in r.items() if k.startswith("grad/")}, "replay")


def test_fused_loss_on_an_ordinary_forward_matches_oracle():
    """dense distance-bucket labels through the fused path against the oracle's autograd"""
    m, cfg, params, g, x, y, args = _setup()
    total, term = _objective(m, x, y, cfg, args, fused=True)
    total.backward()
    parts, grads = O.objective_backward(cfg, params, g["idx"], g["targets"], **args)
    for got, ref in ((total, parts["total"]), (term, parts["term_loss"])):
        assert abs(got.item() - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (got.item(), float(ref))
    _assert_grads(m.named_parameters(), grads, "fused")


def test_bf16_fused_agrees_with_its_dense_path():
    res = []
    for fused in (False, True):
        m, cfg, _, _, x, y, args = _setup("bf16")
        total, _ = _objective(m, x, y, cfg, args, fused=fused)
        total.backward()
        res.append((total.item(), {k: p.grad.detach().float().flatten().clone() for k, p in m.named_parameters()}))
    (t_dense, g_dense), (t_fused, g_fused) = res
    print("bf16 dense", t_dense, "fused", t_fused)
    assert abs(t_fused - t_dense) <= 2e-2 * abs(t_dense)
    # "non-negligible" as test_aux_objective_bf16_close_and_trains decides it: by the fp32 engine's
    # gradient (the key biases' exact gradient is 0 -- softmax shift invariance -- and a bf16 run
    # holds rounding noise there)
    m32, cfg, _, _, x, y, args = _setup()
    _objective(m32, x, y, cfg, args, fused=False)[0].backward()
    checked = 0
    for k, q in m32.named_parameters():
        if float(q.grad.detach().float().norm()) < 1e-6:
            continue
        cos = float(torch.nn.functional.cosine_similarity(g_fused[k], g_dense[k], dim=0))
        print("bf16", k, "cos", cos)
        assert cos > 0.98, (k, cos)
        checked += 1
    assert checked >= len(g_dense) - cfg.n_layer


def test_heads_only_backward_touches_the_aux_tail_alone():
    m, cfg, params, g, x, y, args = _setup()
    _freeze_backbone(m)
    flat_g = m.flat_grads()
    sentinel = torch.tensor([0x7FC0BEEF], dtype=torch.int32, device=DEV)
    flat_g.view(torch.int32).copy_(sentinel.expand(flat_g.numel()))
    total, _ = _objective(m, x, y, cfg, args, fused=True)
    total.backward()
    aux = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    assert aux and all(k.startswith(("termination_head", "offset_projs")) for k, _ in aux)
    base = m.flat_parameters().data_ptr()
    tail = min((p.data_ptr() - base) // 4 for _, p in aux)
    assert 0 < tail < flat_g.numel()
    assert bool((flat_g.view(torch.int32)[:tail] == sentinel).all())
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
    _, grads = O.objective_backward(cfg, params, g["idx"], g["targets"], **args)
    _assert_grads(aux, grads, "heads-only")
    # an accumulating second backward doubles the tail and still leaves the rest alone
    first = {k: p.grad.detach().clone() for k, p in aux}
    total, _ = _objective(m, x, y, cfg, args, fused=True)
    total.backward()
    assert bool((flat_g.view(torch.int32)[:tail] == sentinel).all())
    for k, p in aux:
        torch.testing.assert_close(p.grad, 2 * first[k], rtol=1e-5, atol=1e-7 * float(first[k].abs().max()) + 1e-12)


def test_frozen_adamw_moves_the_heads_alone():
    from codonlm_amd.optim import FusedAdamW
    m, cfg, _, _, x, y, args = _setup()
    _freeze_backbone(m)
    lr, lr_emb, wd = 2e-3, 7e-3, 0.05
    opt = FusedAdamW(m, lr=lr, weight_decay=wd, lr_embedding=lr_emb)
    assert len(opt.param_groups) == 1 and all(p.requires_grad for p in opt.param_groups[0]["params"])
    init = {k: p.detach().clone() for k, p in m.named_parameters()}
    P = {k: p.detach().cpu().clone() for k, p in m.named_parameters() if p.requires_grad}
    mo = {k: torch.zeros_like(v) for k, v in P.items()}
    vo = {k: torch.zeros_like(v) for k, v in P.items()}
    for step in (1, 2):
        opt.zero_grad()
        _objective(m, x, y, cfg, args, fused=True)[0].backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.requires_grad}
        opt.step()
        for k in P:
            O.adamw_step(P[k], grads[k], mo[k], vo[k], step, lr_emb, 0.0)
    moved = 0
    for k, p in m.named_parameters():
        if k in P:
            np.testing.assert_allclose(p.detach().cpu().numpy(), P[k].numpy(), rtol=1e-5, atol=2e-6, err_msg=k)
            moved += int(not torch.equal(p.detach(), init[k]))
        else:
            assert torch.equal(p.detach(), init[k]), k
    assert moved > 0
    sd = opt.state_dict()
    assert len(sd["state"]) == len(P) == sum(len(g_["params"]) for g_ in sd["param_groups"])


def test_trunk_only_forward():
    m, cfg, _, _, x, y, _ = _setup()
    m.eval()
    with torch.no_grad():
        m(x, y)
        full = m.engine.hidden(cfg.n_layer + 1).clone()
        logits, loss = m(x, head=False)
        assert logits is None and loss is None
        assert torch.equal(m.engine.hidden(cfg.n_layer + 1), full)
        logits, loss, aux = m(x, return_aux=True, head=False)
        assert logits is None and loss is None and "termination_logits" in aux
        with pytest.raises(ValueError):
            m(x, y, head=False)
        with pytest.raises(ValueError):
            m.engine.forward(x, y, training=False, head=False)
