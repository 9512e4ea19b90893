"""The flat AdamW path on the device: Bf16Compute.flat_adamw + clip_grad_norm_ against torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_ (five steps, each compared on its own), what is refused, and a tiny detector trained for two steps
through engine.det_engine.build_optimizers_schedulers / train_step.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests.flat_adamw_common import five_step_comparison, norm64, ulps
from tests.helpers import GOLDEN, deterministic_fill_, disable_drop_path, t

import det_draws as D  # tests/golden, put on the path by tests.helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_five_steps_against_torch_adamw():
    five_step_comparison(DEV)


def _toy():
    from grit_amd.amp import Bf16Compute
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(13, 7), nn.LayerNorm(7), nn.Linear(7, 5)).to(DEV)
    wrapped = Bf16Compute(net)
    assert wrapped.flat_optimizer
    return wrapped, [m for _, m in wrapped.named_master_parameters()]


def test_clip_and_step_do_not_synchronise_the_host():
    wrapped, masters = _toy()
    opt = wrapped.flat_adamw(masters, lr=1e-3)
    for b in wrapped.ddp.buckets:
        b.flat.normal_()
    wrapped.clip_grad_norm_(0.1)  # first call: library load, workspaces, pinned tables
    opt.step()
    wrapped.after_optimizer_step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        norm = wrapped.clip_grad_norm_(0.1)
        opt.step()
        wrapped.after_optimizer_step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert norm.is_cuda and norm.dim() == 0 and float(norm) > 0.1


def test_flat_adam_refuses_a_pending_clip():
    wrapped, masters = _toy()
    adam = wrapped.flat_adam(masters, lr=1e-3)
    before = [m.detach().clone() for m in masters]
    wrapped.clip_grad_norm_(0.1)
    with pytest.raises(RuntimeError, match="clip"):
        adam.step()
    assert all(torch.equal(m.detach(), b) for m, b in zip(masters, before))
    wrapped.after_optimizer_step()
    adam.step()  # a step without a clip call is taken as before


def test_sharded_optimizer_refuses_to_clip():
    from grit_amd.amp import Bf16Compute
    stub = Bf16Compute.__new__(Bf16Compute)
    nn.Module.__init__(stub)
    stub.shard_optimizer, stub.flat_optimizer = True, True
    with pytest.raises(NotImplementedError):
        stub.clip_grad_norm_(0.1)


def test_tiny_detector_trains_on_the_flat_path():
    """Fixture G19's end-to-end configuration (224 x 224, B 2, 30 queries, 11 classes, pre_trained='none'); lr and weight_decay are
    raised so that 1 - lr * wd is not absorbed by fp32 (at the recipe's 1e-5 * 1e-4 it rounds to 1, in torch as here)."""
    from engine.det_engine import build_optimizers_schedulers, train_step
    from grit_amd.amp import Bf16Compute
    from grit_amd.config import detection_config
    from grit_amd.utils.misc import NestedTensor
    from models.detection.detector import build_detector
    e = json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))['e2e']
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
                              'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model'],
                              'model.det_module.dropout': 0.0, 'optimizer.lr': 1e-3, 'optimizer.lr_backbone': 2e-3,
                              'optimizer.weight_decay': 0.1})
    model, criterion, _ = build_detector(cfg)
    deterministic_fill_(model)
    model.to(DEV).train()
    disable_drop_path(model)
    images, tg = D.end_to_end_batch(e['seed'], num_classes=e['num_classes'], counts=tuple(e['counts']))
    targets = [{'labels': t(l, device=DEV), 'boxes': t(b, device=DEV)} for l, b in tg]
    images = t(images, device=DEV)
    samples = NestedTensor(images, torch.zeros(images.shape[0], 224, 224, dtype=torch.bool, device=DEV))
    wrapped = Bf16Compute(model)
    optimizers, _ = build_optimizers_schedulers(wrapped, cfg)
    masters = dict(wrapped.named_master_parameters())
    group_of = {id(p): g for o in optimizers for g in o.param_groups for p in g['params']}
    assert len(group_of) == len(masters)

    # a step on exactly zero gradients (the buckets are zero before the first backward, the moments too): parameters of the
    # no-decay groups are unchanged, those of the decay groups are multiplied by 1 - lr * wd, rounded once
    before = {n: m.detach().clone() for n, m in masters.items()}
    for o in optimizers:
        o.step()
    wrapped.after_optimizer_step()
    kinds = set()
    for n, m in masters.items():
        g = group_of[id(m)]
        if g['weight_decay'] == 0:
            assert torch.equal(m.detach(), before[n]), n
        else:
            factor = torch.tensor(1.0 - g['lr'] * g['weight_decay'], dtype=torch.float32, device=DEV)
            assert float(factor) < 1.0
            assert torch.equal(m.detach(), before[n] * factor), n
            assert not torch.equal(m.detach(), before[n]), n
        kinds.add(g['weight_decay'] == 0)
    assert kinds == {True, False}

    total, losses = train_step(wrapped, criterion, optimizers, samples, targets, max_norm=0.1)
    assert np.isfinite(float(total)) and all(np.isfinite(float(v)) for v in losses.values())
    before = {n: m.detach().clone() for n, m in masters.items()}
    total, losses = train_step(wrapped, criterion, optimizers, samples, targets, max_norm=0.1)
    assert np.isfinite(float(total)) and all(np.isfinite(float(v)) for v in losses.values())
    assert wrapped._clip is None
    dead = wrapped.ddp._dead
    live = [(n, wrapped.ddp._view_of[wrapped._compute_of[n]]) for n in masters if wrapped._compute_of[n] not in dead]
    with_grad = [n for n, g in live if float(g.float().abs().max()) > 0]
    assert len(with_grad) > len(masters) // 2
    still = [n for n in with_grad if torch.equal(masters[n].detach(), before[n])]
    assert not still, still
    for n, m in masters.items():
        assert torch.isfinite(m).all(), n
        assert torch.equal(wrapped._compute_of[n].detach(), m.detach().bfloat16()), n
    # the norm of the second step's gradients, as they still lie in the buckets
    got = wrapped.clip_grad_norm_(0.1)
    want = norm64([g for _, g in live])
    wrapped.after_optimizer_step()
    print("tiny detector: total norm %r (float64: %r), %d of %d masters live" % (float(got), want, len(live), len(masters)))
    assert want > 0 and ulps(got, want) <= 2, (float(got), want)
