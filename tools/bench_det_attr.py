"""The detector's attribute head, device path against the torch composition of the same maths (the host forms of
grit_amd/ops/det_attr.py run on the device): one JSON line per item.

    python tools/bench_det_attr.py [--batch 32] [--queries 150] [--classes 1849] [--attrs 400] [--width 256] [--max-targets 60]
                                   [--iters 50] [--step-batch 4] [--step-size 384] [--step-iters 5] [--bf16] [--out FILE]
    python tools/bench_det_attr.py --trace-steps 6 [--attr] [--bf16]      (a run for rocprofv3 --hip-trace --memory-copy-trace)
    python tools/bench_det_attr.py --summarise DIR_WITH DIR_WITHOUT      (the copies and synchronisations of two such traces)

Seeded inputs.  Timed with HIP events after warm-up, device and torch alternating in one process (three legs each; `spread` is
max - min of a kind's legs):
  * front   grit_attr_embed_cat (label, embedding row, concatenation: one launch) | argmax(sigmoid) + embedding + cat
  * embed   grit_attr_embed_grad (no atomics, row order)                          | zeros + index_add_ (atomics)
  * loss    grit_det_attr_{fwd,bwd}_f32 through their autograd node               | attr_loss_host + autograd
  * step    engine.det_engine.train_step of train_detector.py --synthetic with the head and attributes | the same step without
It asserts nothing about speed.  `--trace-steps` runs that many steps after two warm-up steps and reads nothing back until one final
synchronisation, so that a trace of it with the head and one without differ only by what the head adds.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def alternate(pairs, iters, shape):
    """pairs: [(item, {'device': fn, 'torch': fn})] -> JSON-able lines, the two kinds of an item alternating."""
    lines = []
    for item, kinds in pairs:
        for fn in kinds.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        legs = {k: [] for k in kinds}
        for _ in range(3):
            for k, fn in kinds.items():
                legs[k].append(timed(fn, iters))
        for k, ms in legs.items():
            lines.append(dict(item=item, kind=k, ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms],
                              spread=round(max(ms) - min(ms), 4), iters=iters, **shape))
    return lines


def step_setup(attr, bf16, batch, size, max_targets):
    import train_detector as T
    from engine.det_engine import build_optimizers_schedulers, train_step
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    over = {'model.backbone.pre_trained': 'none'}
    if attr:
        over.update({'model.has_attr_head': True, 'model.det_module.loss.attr_loss_coef': 1.0, 'optimizer.sp_names': ['attr_head']})
    config = detection_config(**over)
    torch.manual_seed(config.exp.seed)
    dev = torch.device('cuda')
    model, criterion, _ = build_detector(config)
    model.to(dev)
    if bf16:
        from grit_amd.amp import Bf16Compute
        model = Bf16Compute(model)
    optimizers, _ = build_optimizers_schedulers(model, config)
    g = torch.Generator().manual_seed(config.exp.seed)
    samples, targets = T.synthetic_batch(g, batch, size, config.model.det_module.num_classes, max_targets, dev)
    if attr:
        T.add_synthetic_attributes(g, targets, config.model.num_attr_classes, dev)

    def step():
        return train_step(model, criterion, optimizers, samples, targets, config.optimizer.clip_max_norm)

    return step


def summarise(directory):
    """Counts of a rocprofv3 csv trace: copies by direction, and the HIP calls that wait for the device or copy."""
    out = {'copies': {}, 'calls': {}}
    for path in glob.glob(os.path.join(directory, '**', '*memory_copy_trace.csv'), recursive=True):
        for row in csv.DictReader(open(path)):
            d = row.get('Direction') or row.get('Kind') or '?'
            out['copies'][d] = out['copies'].get(d, 0) + 1
    for path in glob.glob(os.path.join(directory, '**', '*hip_api_trace.csv'), recursive=True):
        for row in csv.DictReader(open(path)):
            f = row.get('Function') or '?'
            if 'Synchronize' in f or 'Memcpy' in f or 'Wait' in f:
                out['calls'][f] = out['calls'].get(f, 0) + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--queries', type=int, default=150)
    ap.add_argument('--classes', type=int, default=1849)
    ap.add_argument('--attrs', type=int, default=400)
    ap.add_argument('--width', type=int, default=256)
    ap.add_argument('--max-targets', type=int, default=60)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--step-batch', type=int, default=4)
    ap.add_argument('--step-size', type=int, default=384)
    ap.add_argument('--step-iters', type=int, default=5)
    ap.add_argument('--bf16', action='store_true')
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--trace-steps', type=int, default=0)
    ap.add_argument('--attr', action='store_true')
    ap.add_argument('--summarise', nargs=2, default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.summarise:
        a, b = (summarise(d) for d in args.summarise)
        extra = {kind: {k: a[kind].get(k, 0) - b[kind].get(k, 0) for k in sorted(set(a[kind]) | set(b[kind]))
                        if a[kind].get(k, 0) != b[kind].get(k, 0)} for kind in ('copies', 'calls')}
        text = json.dumps(dict(item='trace', with_head=a, without_head=b, with_minus_without=extra))
        print(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text + '\n')
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_attr: needs a HIP device (a CPU timing says nothing about the kernels)")
    import models  # noqa: F401  (the reference's import paths)
    if args.trace_steps:
        step = step_setup(args.attr, args.bf16, args.step_batch, args.step_size, 30)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        for _ in range(args.trace_steps):
            total, _ = step()
        torch.cuda.synchronize()
        print(json.dumps(dict(item='trace-run', attr=args.attr, bf16=args.bf16, steps=args.trace_steps, total=float(total))))
        return
    from grit_amd.ops import det_attr, det_loss
    dev = torch.device('cuda')
    B, Q, K, A, d = args.batch, args.queries, args.classes, args.attrs, args.width
    rng = np.random.default_rng(0)
    dtype = torch.bfloat16 if args.bf16 else torch.float32
    obj_h = torch.from_numpy(rng.standard_normal((B * Q, d)).astype(np.float32)).to(dev).to(dtype)
    logits = torch.from_numpy((2 * rng.standard_normal((B * Q, K)) - 2).astype(np.float32)).to(dev).to(dtype)
    weight = torch.from_numpy(rng.standard_normal((K, d)).astype(np.float32)).to(dev).to(dtype)
    dcat = torch.from_numpy(rng.standard_normal((B * Q, 2 * d)).astype(np.float32)).to(dev).to(dtype)
    _, labels = det_attr.embed_cat(obj_h, logits, weight)
    assert torch.equal(labels.long(), det_attr.attr_labels_host(logits))
    targets, pairs = [], []
    for b in range(B):
        n = int(rng.integers(1, args.max_targets + 1))
        targets.append({'labels': torch.from_numpy(rng.integers(0, K, n)).to(dev), 'boxes': torch.full((n, 4), 0.5, device=dev),
                        'attributes': torch.from_numpy((rng.random((n, A)) < 0.02).astype(np.uint8)).to(dev), 'has_attr': b % 2 == 0})
        m = np.full(Q, -1, np.int32)
        m[rng.permutation(Q)[:n]] = rng.permutation(n)
        pairs.append(m)
    packed = det_loss.pack_targets(targets, num_attr=A)
    match_t = torch.from_numpy(np.stack(pairs)).to(dev)
    x = torch.from_numpy((2 * rng.standard_normal((B, Q, A))).astype(np.float32)).to(dev).requires_grad_(True)

    def loss_device():
        det_attr.attr_loss(x, match_t, packed).backward()
        x.grad = None

    def loss_torch():
        det_attr.attr_loss_host(x, packed.attributes, packed.offsets, packed.has_attr, match_t).backward()
        x.grad = None

    shape = dict(batch=B, queries=Q, classes=K, attrs=A, width=d, dtype=str(dtype), targets=sum(packed.counts),
                 device=torch.cuda.get_device_name(0))
    lines = alternate([
        ('front', {'device': lambda: det_attr.embed_cat(obj_h, logits, weight), 'torch': lambda: det_attr.attr_embed_cat_host(obj_h, logits, weight)}),
        ('embed', {'device': lambda: det_attr.embed_grad(dcat, labels, K), 'torch': lambda: det_attr.attr_embed_grad_host(dcat, labels, K)}),
        ('loss', {'device': loss_device, 'torch': loss_torch}),
    ], args.iters, shape)
    a = float(det_attr.attr_loss(x.detach(), match_t, packed))
    b = float(det_attr.attr_loss_host(x.detach(), packed.attributes, packed.offsets, packed.has_attr, match_t))
    lines.append(dict(item='parity', device_loss=a, torch_loss=b, relative_difference=abs(a - b) / abs(b)))
    if not args.no_step:
        steps = {'with_head': step_setup(True, args.bf16, args.step_batch, args.step_size, 30),
                 'without_head': step_setup(False, args.bf16, args.step_batch, args.step_size, 30)}
        lines += alternate([('step', steps)], args.step_iters,
                           dict(batch=args.step_batch, size=args.step_size, bf16=args.bf16, device=torch.cuda.get_device_name(0)))
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
