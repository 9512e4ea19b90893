"""Host logic of the flat AdamW path (grit_amd.amp.FlatAdamW, Bf16Compute.clip_grad_norm_, engine.det_engine) on CPU tensors:
Bf16Compute(flat_optimizer=True) with torch restatements of the two kernels injected through use_reference_ops.  The kernels
themselves are covered on the GPU (tests/test_adamw_kernels_gpu.py, tests/test_flat_adamw_gpu.py)."""
import io
import math

import pytest
import torch
from torch import nn

from tests.flat_adamw_common import five_step_comparison
from tests.helpers import use_reference_ops


class _Ops(object):
    """oracle.torch_ref plus the restatements of grit_adamw_flat_dev and grit_grad_norm_flat."""

    def __getattr__(self, name):
        from oracle import torch_ref
        return getattr(torch_ref, name)

    @staticmethod
    def adamw_flat(master, grad, mom, var, compute, b1, b2, eps, grad_scale, hyper, clip_scale):
        scale = torch.tensor(grad_scale, dtype=torch.float32) if clip_scale is None else clip_scale
        g = grad.float() * scale
        master.mul_(hyper[2])
        mom.add_((g - mom) * (1.0 - b1))
        var.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (var.sqrt() * hyper[1]).add_(eps)
        master.sub_(hyper[0] * (mom / denom))
        compute.copy_(master)

    @staticmethod
    def grad_norm_flat(ranges, grad_scale, max_norm, out):
        s = sum((r.double() ** 2).sum() for r in ranges)
        total = (grad_scale * s.sqrt()).float()
        coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (total + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
        out[0], out[1], out[2] = total, torch.tensor(grad_scale, dtype=torch.float32) * coef, coef


def ops():
    return use_reference_ops(_Ops())


class Net(nn.Module):
    """`det` leaves the live set while `cached` is set (the phase change of the caption recipe)."""

    def __init__(self):
        super().__init__()
        self.det = nn.Linear(8, 8)
        self.head = nn.Linear(8, 4)
        self.cached = False

    def forward(self, x):
        if not self.cached:
            x = torch.tanh(self.det(x))
        return self.head(x)


def _wrapped_net(seed=0):
    from grit_amd.amp import Bf16Compute
    torch.manual_seed(seed)
    model = Net()
    wrapped = Bf16Compute(model, bucket_mb=0.0002, flat_optimizer=True)
    return model, wrapped, dict(wrapped.named_master_parameters())


def _groups(masters):
    return [{'params': [m for m in masters.values() if m.dim() > 1], 'lr': 1e-2, 'weight_decay': 0.05},
            {'params': [m for m in masters.values() if m.dim() == 1], 'lr': 5e-3, 'weight_decay': 0.0}]


def _step(wrapped, opt, x, y, max_norm=0.1):
    loss = ((wrapped(x).float() - y) ** 2).mean()
    loss.backward()
    wrapped.finish_gradient_sync()
    wrapped.clip_grad_norm_(max_norm)
    opt.step()
    wrapped.after_optimizer_step()


def test_five_steps_against_torch_adamw_on_the_host():
    with ops():
        five_step_comparison("cpu")


def test_state_dict_has_torch_adamw_layout_and_loads_both_ways():
    _, wrapped, masters = _wrapped_net()
    opt = wrapped.flat_adamw(_groups(masters), lr=1e-2)
    x, y = torch.randn(4, 8).bfloat16(), torch.randn(4, 4)
    with ops():
        _step(wrapped, opt, x, y)
    clones = {n: m.detach().clone().requires_grad_() for n, m in masters.items()}
    ref = torch.optim.AdamW(_groups(clones), lr=1e-2)
    for p in clones.values():
        p.grad = torch.randn_like(p)
    ref.step()
    ours, theirs = opt.state_dict(), ref.state_dict()
    assert set(ours) == set(theirs)
    assert [sorted(g) for g in ours['param_groups']] == [sorted(g) for g in theirs['param_groups']]
    assert [g['params'] for g in ours['param_groups']] == [g['params'] for g in theirs['param_groups']]
    assert set(ours['state']) == set(theirs['state'])
    for k, st in theirs['state'].items():
        assert set(ours['state'][k]) == set(st)
        assert all(ours['state'][k][f].shape == st[f].shape for f in st)
    # torch.optim.AdamW -> FlatAdamW: moments land in the flat buffers, the step counts in the books
    opt.load_state_dict(theirs)
    for n, m in masters.items():
        assert torch.equal(opt.state[m]['exp_avg'], ref.state[clones[n]]['exp_avg'])
        assert torch.equal(wrapped._moment_views[m][1], ref.state[clones[n]]['exp_avg_sq'])
        assert opt._steps[m] == 1
    # ... and the reverse
    ref2 = torch.optim.AdamW(_groups(clones), lr=1e-2)
    ref2.load_state_dict(opt.state_dict())
    for n, m in masters.items():
        assert torch.equal(ref2.state[clones[n]]['exp_avg_sq'], opt.state[m]['exp_avg_sq'])
        assert float(ref2.state[clones[n]]['step']) == 1.0


def test_save_load_step_continues_like_an_uninterrupted_run():
    """Two identical wrappers take the same six steps (`det` sits out steps 1-3 and rejoins); one of them is handed to a NEW
    optimizer through a saved state dict after step 3.  Masters, moments and per-parameter step counts stay equal bit for bit."""
    x, y = torch.randn(4, 8, generator=torch.Generator().manual_seed(5)).bfloat16(), torch.randn(4, 4, generator=torch.Generator().manual_seed(6))
    runs = []
    with ops():
        for interrupted in (False, True):
            model, wrapped, masters = _wrapped_net()
            opt = wrapped.flat_adamw(_groups(masters), lr=1e-2)
            for k in range(6):
                model.cached = 1 <= k <= 3
                if interrupted and k == 4:
                    blob = io.BytesIO()
                    torch.save(opt.state_dict(), blob)
                    blob.seek(0)
                    ages = {n: opt._steps[m] for n, m in masters.items()}
                    assert ages['det.weight'] < ages['head.weight'] == 4, ages
                    opt = wrapped.flat_adamw(_groups(masters), lr=1e-2)  # (zeroes the moments: the load must restore them)
                    opt.load_state_dict(torch.load(blob))
                    assert {n: opt._steps[m] for n, m in masters.items()} == ages
                _step(wrapped, opt, x, y)
            runs.append(({n: m.detach().clone() for n, m in masters.items()},
                         {n: [t.clone() for t in wrapped._moment_views[m]] for n, m in masters.items()},
                         {n: opt._steps[m] for n, m in masters.items()},
                         {n: int(float(opt.state[m]['step'])) for n, m in masters.items()}))
    (pa, ma, sa, ta), (pb, mb, sb, tb) = runs
    assert sa == sb == ta == tb and sa['head.weight'] == 6 and sa['det.weight'] < 6, (sa, sb, ta, tb)
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
        assert torch.equal(ma[n][0], mb[n][0]) and torch.equal(ma[n][1], mb[n][1]), n


def test_groups_that_differ_in_betas_are_refused():
    _, wrapped, masters = _wrapped_net()
    groups = _groups(masters)
    groups[1]['betas'] = (0.8, 0.999)
    opt = wrapped.flat_adamw(groups, lr=1e-2)
    with pytest.raises(NotImplementedError):
        with ops():
            opt.step()
    groups = _groups(masters)
    groups[0]['eps'] = 1e-6
    with pytest.raises(NotImplementedError):
        wrapped.flat_adamw(groups, lr=1e-2).prepare_replay()


def test_replay_rows_follow_groups_ages_and_the_scheduler():
    _, wrapped, masters = _wrapped_net()
    opt = wrapped.flat_adamw(_groups(masters), lr=1e-2)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [1], gamma=0.1)
    x, y = torch.randn(4, 8).bfloat16(), torch.randn(4, 4)
    with ops():
        _step(wrapped, opt, x, y)
    b1, b2 = opt.param_groups[0]['betas']

    def check():
        opt.prepare_replay()
        assert opt._hyper_dev.shape[1] == 4 and len(opt._runs) == len(opt._run_group) >= 2
        seen = set()
        for i, ((_, _, _, _, _, start, end), params, age) in enumerate(opt._runs):
            g = opt.param_groups[opt._run_group[i]]
            assert all(any(p is q for q in g['params']) for p in params)  # a run never mixes groups
            seen.add(opt._run_group[i])
            t = age + 1
            want = torch.tensor([g['lr'] / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t), 1 - g['lr'] * g['weight_decay'], 0.0])
            assert torch.equal(opt._hyper_dev[i], want), (i, opt._hyper_dev[i], want)
        assert seen == {0, 1}

    check()
    sched.step()
    assert abs(opt.param_groups[0]['lr'] - 1e-3) < 1e-15
    check()


def test_flat_adam_refuses_a_pending_clip_and_sharding_refuses_to_clip():
    from grit_amd.amp import Bf16Compute
    from tests.helpers import oracle_ops
    _, wrapped, masters = _wrapped_net()
    adam = wrapped.flat_adam(list(masters.values()), lr=1e-2)
    with ops():
        norm = wrapped.clip_grad_norm_(0.1)
        assert float(norm) == 0.0 and wrapped._clip is not None  # (no gradient yet: the buckets are zero)
        with pytest.raises(RuntimeError, match="clip"):
            adam.step()
        wrapped.after_optimizer_step()
        adam.step()  # unclipped: as before
    stub = Bf16Compute.__new__(Bf16Compute)
    nn.Module.__init__(stub)
    stub.shard_optimizer, stub.flat_optimizer = True, True
    with pytest.raises(NotImplementedError):
        stub.clip_grad_norm_(0.1)


def test_clip_on_the_torch_route_is_torchs_clip():
    """flat_optimizer=False (the CPU / gloo route): torch.nn.utils.clip_grad_norm_ on the masters' fp32 .grad."""
    from grit_amd.amp import Bf16Compute
    torch.manual_seed(0)
    wrapped = Bf16Compute(Net(), bucket_mb=0.0002)
    assert not wrapped.flat_optimizer
    masters = [m for _, m in wrapped.named_master_parameters()]
    x, y = torch.randn(4, 8).bfloat16(), torch.randn(4, 4)
    ((wrapped(x).float() - y) ** 2).mean().backward()
    wrapped.finish_gradient_sync()
    before = torch.sqrt(sum((m.grad.double() ** 2).sum() for m in masters))
    norm = wrapped.clip_grad_norm_(0.01)
    after = torch.sqrt(sum((m.grad.double() ** 2).sum() for m in masters))
    assert abs(float(norm) - float(before)) < 1e-5 * float(before) and float(before) > 0.01
    assert abs(float(after) - 0.01) < 1e-4 * 0.01


# ------------------------------------------------------------------------------------------------ engine.det_engine

def _tiny_config(**over):
    from grit_amd.config import detection_config
    return detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': 11,
                               'model.det_module.num_queries': 30, 'optimizer.lr_drop_epochs': [2], 'optimizer.sp_lr_drop_epochs': [1],
                               **over})


@pytest.fixture(scope="module")
def tiny_detectors():
    from grit_amd.amp import Bf16Compute
    from models.detection.detector import build_detector
    plain = build_detector(_tiny_config())[0]
    names = [n for n, p in plain.named_parameters() if p.requires_grad]
    wrapped = Bf16Compute(build_detector(_tiny_config())[0], flat_optimizer=True)
    return plain, wrapped, names


@pytest.mark.parametrize("sp_names", [[], ['query_embed']])
@pytest.mark.parametrize("kind", ["plain", "wrapped"])
def test_build_optimizers_schedulers(tiny_detectors, kind, sp_names):
    from engine.det_engine import build_optimizers_schedulers
    from grit_amd.amp import FlatAdamW
    plain, wrapped, names = tiny_detectors
    cfg = _tiny_config(**{'optimizer.sp_names': sp_names})
    o = cfg.optimizer
    assert (o.sp_lr, o.lr, o.lr_backbone, o.weight_decay) == (1e-4, 1e-5, 2e-5, 1e-4)
    model = plain if kind == "plain" else wrapped
    named = dict(plain.named_parameters()) if kind == "plain" else dict(wrapped.named_master_parameters())
    assert sorted(named) == sorted(names) or kind == "plain"
    optimizers, schedulers = build_optimizers_schedulers(model, cfg)
    assert len(optimizers) == len(schedulers) == (2 if sp_names else 1)
    assert all(isinstance(x, FlatAdamW if kind == "wrapped" else torch.optim.AdamW) for x in optimizers)
    assert all(g['params'] for x in optimizers for g in x.param_groups)  # empty groups are dropped
    where = {}
    for oi, opt in enumerate(optimizers):
        for g in opt.param_groups:
            for p in g['params']:
                assert id(p) not in where  # exactly one group of exactly one optimizer
                where[id(p)] = (oi, g)
    assert len(where) == len(names)
    skip = ['query_embed']  # (the Swin backbone of this build has no no_weight_decay())
    seen = set()
    for n in names:
        oi, g = where[id(named[n])]
        p = named[n]
        if any(s in n for s in sp_names):
            assert oi == 1 and g['lr'] == o.sp_lr and g['weight_decay'] == o.weight_decay, n
            seen.add('sp')
            continue
        assert oi == 0, n
        no_decay = p.dim() == 1 or n.endswith('.bias') or n.split('.')[-1] in skip
        assert g['weight_decay'] == (0.0 if no_decay else o.weight_decay), n
        assert g['lr'] == (o.lr_backbone if 'backbone' in n else o.lr), n
        seen.add(('backbone' in n, no_decay))
    assert seen == {(False, False), (False, True), (True, False), (True, True)} | ({'sp'} if sp_names else set())
    # the schedulers drop at the configured epochs: [2] for the main optimizer, [1] for the second
    lrs = []
    for _ in range(3):
        lrs.append([[g['lr'] for g in x.param_groups] for x in optimizers])
        for s in schedulers:
            s.step()
    main = [l[0] for l in lrs]
    assert main[0] == main[1] and all(abs(b - a * o.decay_rate) < 1e-12 for a, b in zip(main[1], main[2]))
    if sp_names:
        sp = [l[1][0] for l in lrs]
        assert sp[0] == o.sp_lr and abs(sp[1] - o.sp_lr * o.decay_rate) < 1e-12 and sp[2] == sp[1]


class _ToyCriterion(nn.Module):
    weight_dict = {'loss_a': 2.0, 'loss_b': 0.5}

    def forward(self, outputs, targets):
        return {'loss_a': ((outputs - targets) ** 2).mean(), 'loss_b': outputs.abs().mean(), 'unweighted': outputs.sum()}


def test_train_step_on_a_plain_module_is_unchanged():
    """One torch optimizer, a plain module: the same updated weights as the five lines train_step has always been; a list of
    optimizers is accepted as well."""
    from engine.det_engine import train_step
    x, y = torch.randn(6, 8, generator=torch.Generator().manual_seed(1)), torch.randn(6, 4, generator=torch.Generator().manual_seed(2))
    results = []
    for how in ("train_step", "literal", "list"):
        torch.manual_seed(0)
        model, criterion = nn.Linear(8, 4), _ToyCriterion()
        optimizer = torch.optim.AdamW(model.parameters(), lr=1e-2)
        for _ in range(3):
            if how == "literal":
                model.train()
                criterion.train()
                loss_dict = criterion(model(x), y)
                total = sum(loss_dict[k] * criterion.weight_dict[k] for k in loss_dict if k in criterion.weight_dict)
                optimizer.zero_grad(set_to_none=True)
                total.backward()
                torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], 0.1)
                optimizer.step()
                total, losses = total.detach(), {k: v.detach() for k, v in loss_dict.items()}
            else:
                total, losses = train_step(model, criterion, [optimizer] if how == "list" else optimizer, x, y, max_norm=0.1)
        assert set(losses) == {'loss_a', 'loss_b', 'unweighted'} and not total.requires_grad
        results.append((model.weight.detach().clone(), model.bias.detach().clone(), total))
    for w, b, total in results[1:]:
        assert torch.equal(w, results[0][0]) and torch.equal(b, results[0][1]) and torch.equal(total, results[0][2])
