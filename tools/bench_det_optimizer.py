"""The optimizer side of a detector pre-training step, flat path against torch: one JSON line per item.

    python tools/bench_det_optimizer.py [--iters 20] [--out FILE]

The state is the full detector's (build_detector with the default detection configuration, pre_trained='none'): its trainable
parameters in the reference's four AdamW groups (engine.det_engine.build_optimizers_schedulers), seeded random gradients.  Timed with
HIP events after warm-up, the legs alternating in one process (three legs each; `spread` is max - min of a kind's legs):
  * flat    Bf16Compute.clip_grad_norm_ + FlatAdamW.step() + after_optimizer_step(): grit_grad_norm_flat over the bf16 buckets
            (2 B per parameter), one grit_adamw_flat_dev per run (28 B per parameter)
  * torch   torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(...).step(), fused or foreach as torch picks, on fp32 parameters of
            the same shapes with fp32 .grad
  * norm    grit_grad_norm_flat alone (clip_grad_norm_ + after_optimizer_step)
It asserts nothing about speed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_optimizer: needs a HIP device (a CPU timing says nothing about the kernels)")
    import models  # noqa: F401  (the reference's import paths)
    from engine.det_engine import build_optimizers_schedulers
    from grit_amd.amp import Bf16Compute
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    dev = torch.device('cuda')
    config = detection_config(**{'model.backbone.pre_trained': 'none'})
    max_norm = config.optimizer.clip_max_norm
    torch.manual_seed(0)
    model = build_detector(config)[0].to(dev)
    plain = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters() if p.requires_grad]
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    wrapped = Bf16Compute(model)
    flat_opts, _ = build_optimizers_schedulers(wrapped, config)
    for b in wrapped.ddp.buckets:  # gradients ~ N(0, 1e-3) in every live slot; the padding between slots stays zero
        for view in b.views:
            view.normal_(0.0, 1e-3)

    class Named(torch.nn.Module):  # the same names over the fp32 copies: the same four groups
        def __init__(self):
            super().__init__()
            self.backbone = None
            self._named = list(zip(names, plain))

        def named_parameters(self, *a, **k):
            return iter(self._named)

    torch_opts, _ = build_optimizers_schedulers(Named(), config)
    for p in plain:
        p.grad = torch.randn_like(p) * 1e-3

    def flat_step():
        wrapped.clip_grad_norm_(max_norm)
        for o in flat_opts:
            o.step()
        wrapped.after_optimizer_step()

    def torch_step():
        torch.nn.utils.clip_grad_norm_(plain, max_norm)
        for o in torch_opts:
            o.step()

    def norm_only():
        wrapped.clip_grad_norm_(max_norm)
        wrapped.after_optimizer_step()

    def timed(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters

    kinds = [('flat', flat_step), ('torch', torch_step), ('norm', norm_only)]
    for _, fn in kinds:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    legs = {name: [] for name, _ in kinds}
    for _ in range(3):
        for name, fn in kinds:
            legs[name].append(timed(fn, args.iters))
    n_params = sum(p.numel() for p in plain)
    shape = dict(parameters=n_params, tensors=len(plain), runs=sum(len(o._runs) for o in flat_opts), buckets=len(wrapped.ddp.buckets),
                 groups=sum(len(o.param_groups) for o in flat_opts), device=torch.cuda.get_device_name(0))
    lines = []
    for name, _ in kinds:
        ms = legs[name]
        lines.append(dict(item=name, ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms], spread=round(max(ms) - min(ms), 4),
                          iters=args.iters, **shape))
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
