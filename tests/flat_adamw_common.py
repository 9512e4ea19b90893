"""What tests/test_flat_adamw_cpu.py and tests/test_flat_adamw_gpu.py share: the five-step comparison of Bf16Compute.flat_adamw +
clip_grad_norm_ with torch.optim.AdamW + torch.nn.utils.clip_grad_norm_, and the helpers it needs."""
import numpy as np
import torch
from torch import nn
from torch.optim.lr_scheduler import MultiStepLR

RTOL, ATOL = 2e-6, 2e-7  # the project's bound for the flat Adam kernel (tests/test_stream_numerics_gpu.py)
MAX_NORM = 0.1


def ulps(a, b):
    """Distance of two fp32 values in units in the last place (same sign, finite)."""
    ia, ib = (int(np.float32(float(x)).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def norm64(tensors, grad_scale=1.0):
    """float(grad_scale * sqrt(sum g^2)) with squares and sums in float64, rounded to fp32."""
    s = sum(float((x.detach().double().cpu() ** 2).sum()) for x in tensors)
    return float(np.float32(grad_scale * np.sqrt(s)))


def padding_is_zero(wrapped):
    """Every element of the flat buffers (gradient bucket, compute copy, master, moments) outside the slots' numel() is zero."""
    for bi, (b, compute, master, _, mom, var) in enumerate(wrapped._pairs):
        inside = torch.zeros(b.flat.numel(), dtype=torch.bool, device=b.flat.device)
        for m, i, off, _, _ in wrapped._slots:
            if i == bi:
                inside[off:off + m.numel()] = True
        if bool(inside.all()):
            return False  # (the check would be vacuous)
        for buf in (b.flat, compute, master, mom, var):
            if bool((buf[~inside] != 0).any()):
                return False
    return True


def five_step_comparison(dev):
    """Linear(13, 7) -> LayerNorm(7) -> Linear(7, 5): no parameter size is a multiple of SLOT_ALIGN, so the padding is in play.  Two
    groups (weights; biases and norms) that differ in lr and weight_decay, MultiStepLR dropping at step 3.  In every step seeded
    bf16 gradients are written straight into the bucket views; the reference is torch.optim.AdamW on fp32 clones (on the host) with
    the same gradients and torch's clip, re-synchronised to the wrapper's pre-step masters and moments.  Step 1 has a norm below
    max_norm (the unclipped branch), step 2 has no clip call at all."""
    from grit_amd.amp import Bf16Compute, FlatAdamW, SLOT_ALIGN
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(13, 7), nn.LayerNorm(7), nn.Linear(7, 5)).to(dev)
    assert all(p.numel() % SLOT_ALIGN for p in net.parameters())
    wrapped = Bf16Compute(net, flat_optimizer=True)
    masters = dict(wrapped.named_master_parameters())

    def groups(of):
        return [{'params': [of[n] for n in masters if masters[n].dim() > 1], 'lr': 1e-2, 'weight_decay': 0.1},
                {'params': [of[n] for n in masters if masters[n].dim() == 1], 'lr': 3e-3, 'weight_decay': 0.0}]

    opt = wrapped.flat_adamw(groups(masters), lr=1e-2)
    assert isinstance(opt, FlatAdamW) and len(opt._runs) >= 2
    sched = MultiStepLR(opt, [3], gamma=0.1)
    ref = {n: m.detach().cpu().clone().requires_grad_() for n, m in masters.items()}
    ref_opt = torch.optim.AdamW(groups(ref), lr=1e-2)
    ref_sched = MultiStepLR(ref_opt, [3], gamma=0.1)
    gen = torch.Generator().manual_seed(1234)
    for k in range(5):
        scale, clip = {1: (1e-3, True), 2: (0.1, False)}.get(k, (0.1, True))
        grads = {n: (scale * torch.randn(m.shape, generator=gen)).bfloat16() for n, m in masters.items()}
        for n, g in grads.items():
            wrapped.ddp._view_of[wrapped._compute_of[n]].copy_(g)
        for n, m in masters.items():  # every step is compared on its own
            ref[n].data.copy_(m.detach())
            ref[n].grad = grads[n].float()
            ref_opt.state[ref[n]] = {'step': torch.tensor(float(k)), 'exp_avg': opt.state[m]['exp_avg'].detach().cpu().clone(),
                                     'exp_avg_sq': opt.state[m]['exp_avg_sq'].detach().cpu().clone()}
        want_norm = norm64(grads.values())
        assert (want_norm < MAX_NORM) == (k == 1)
        if clip:
            torch.nn.utils.clip_grad_norm_(list(ref.values()), MAX_NORM)
            got_norm = wrapped.clip_grad_norm_(MAX_NORM)
            assert got_norm.dim() == 0 and got_norm.dtype == torch.float32
            assert ulps(got_norm, want_norm) <= 2, (k, float(got_norm), want_norm)
            coef = float(wrapped._clip[2])
            assert (coef == 1.0) if k == 1 else (coef < 1.0)
        ref_opt.step()
        opt.step()
        wrapped.after_optimizer_step()
        assert wrapped._clip is None
        for n, m in masters.items():
            assert int(float(opt.state[m]['step'])) == k + 1
            pairs = (("master", m.detach(), ref[n].detach()), ("exp_avg", opt.state[m]['exp_avg'], ref_opt.state[ref[n]]['exp_avg']),
                     ("exp_avg_sq", opt.state[m]['exp_avg_sq'], ref_opt.state[ref[n]]['exp_avg_sq']))
            for what, got, want in pairs:
                np.testing.assert_allclose(got.cpu().double().numpy(), want.double().numpy(), rtol=RTOL, atol=ATOL,
                                           err_msg="%s of %s, step %d" % (what, n, k))
            assert torch.equal(wrapped._compute_of[n].detach(), m.detach().bfloat16()), (n, k)
        assert padding_is_zero(wrapped), k
        sched.step()
        ref_sched.step()
    assert abs(opt.param_groups[0]['lr'] - 1e-3) < 1e-12 and abs(opt.param_groups[1]['lr'] - 3e-4) < 1e-12
