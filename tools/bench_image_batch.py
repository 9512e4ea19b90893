"""Device image pipeline: time per batch (HIP events) and bytes moved, COCO-like sizes -> 384x640 (maxwh) or a fixed
640x640 batch.  `python tools/bench_image_batch.py [--batch 32] [--iters 50]`

`--augment`: the RandAugment path instead -- batch of 480 x 640 sources -> (384, 512), `image_batch` with and without
plans (drawn once with a fixed seed), same process, alternating rounds, HIP-event time per batch, launches and bytes.

`--detector`: the detector's input pipeline -- batch of 500 x 375 sources, plans drawn once under a fixed seed from
make_transforms('train', 'train'), `image_batch_geo` next to the plain bicubic `image_batch` to the same target sizes, device-resident
input, alternating rounds in one process, HIP-event time per batch; where Pillow is importable also the host chain (flip, resize,
crop, resize; one core) per batch."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grit_amd.datasets.caption.transforms import MaxWHResize, RandAugment  # noqa: E402
from grit_amd.ops.image_batch import image_batch, image_batch_geo, plan_augment, plan_geo, tmp_pitch  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) / iters * 1e3


def augmented(a):
    rng = np.random.default_rng(0)
    shapes, sizes = [(480, 640)] * a.batch, [(384, 512)] * a.batch
    host = [torch.from_numpy(rng.integers(0, 256, s + (3,), dtype=np.uint8)) for s in shapes]
    dev = [h.cuda() for h in host]
    random.seed(0)
    draw = RandAugment()
    plans = [draw.draw() for _ in shapes]
    _, _, n_stages, work = plan_augment(sizes, plans)
    src = sum(3 * h * w for h, w in shapes)
    tmp = sum(h * tmp_pitch(s[1]) for (h, w), s in zip(shapes, sizes))
    out = a.batch * 384 * 512 * 13
    plain_bytes = src + 2 * tmp + out  # rows: src -> tmp; columns: tmp -> floats + mask
    aug_bytes = src + 2 * tmp + 2 * work + 2 * n_stages * work + out  # columns -> uint8, n stages, uint8 -> floats + mask
    for feed, label in ((dev, 'device-resident'), (host, 'host, pageable (staged)')):
        runs = {'plain': lambda: image_batch(feed, sizes, device='cuda'),
                'augmented': lambda: image_batch(feed, sizes, device='cuda', augment=plans)}
        for fn in runs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        best = {k: (float('inf'), float('inf')) for k in runs}
        for _ in range(a.rounds):  # alternate, keep the fastest round of each
            for k, fn in runs.items():
                best[k] = min(best[k], timed(fn, a.iters))
        for k, nbytes, launches in (('plain', plain_bytes, 2), ('augmented', aug_bytes, 3 + n_stages)):
            print(json.dumps({'case': '480x640->(384,512) ' + k, 'input': label, 'batch': a.batch, 'launches': launches,
                              'ms_per_batch': round(best[k][0], 3),
                              'wall_ms_per_batch': round(best[k][1], 3), 'moved_MB': round(nbytes / 1e6, 1),
                              'GB_per_s': round(nbytes / best[k][0] / 1e6, 1)}))


def pillow_chain_ms(host, plans):
    """The same plans as a PIL chain on this core, milliseconds per batch; None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    pil = [Image.fromarray(h.numpy(), 'RGB') for h in host]
    t0 = time.perf_counter()
    for im, plan in zip(pil, plans):
        for op in plan:
            if op[0] == 'hflip':
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            elif op[0] == 'crop':
                im = im.crop((op[2], op[1], op[2] + op[4], op[1] + op[3]))
            else:
                im = im.resize((op[2], op[1]), Image.BILINEAR)
        im.load()
    return (time.perf_counter() - t0) * 1e3


def detector(a):
    from grit_amd.datasets.detection import make_transforms
    rng = np.random.default_rng(0)
    host = [torch.from_numpy(rng.integers(0, 256, (375, 500, 3), dtype=np.uint8)) for _ in range(a.batch)]
    dev = [h.cuda() for h in host]
    random.seed(0)
    torch.manual_seed(0)
    recipe = make_transforms('train', 'train')
    plans = [recipe(h.numpy(), {})[0].plan for h in host]
    g = plan_geo([(375, 500)] * a.batch, plans)
    H, W = max(s[0] for s in g.sizes), max(s[1] for s in g.sizes)
    two = int((g.geo[:, 0] == 2).sum())
    src = a.batch * 375 * 500 * 3
    geo_bytes = src + 2 * g.tmp_bytes + 2 * g.work_bytes + a.batch * H * W * 13  # a two-resize image reads the source once, the work buffer once
    runs = {'bicubic image_batch': lambda: image_batch(dev, g.sizes, device='cuda'),
            'detector image_batch_geo': lambda: image_batch_geo(dev, plans, device='cuda')}
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    best = {k: (float('inf'), float('inf')) for k in runs}
    for _ in range(a.rounds):  # alternate, keep the fastest round of each
        for k, fn in runs.items():
            best[k] = min(best[k], timed(fn, a.iters))
    for k in runs:
        line = {'case': '500x375 train recipe, ' + k, 'input': 'device-resident', 'batch': a.batch, 'out': [H, W], 'two_resize_images': two,
                'ms_per_batch': round(best[k][0], 3), 'wall_ms_per_batch': round(best[k][1], 3)}
        if 'geo' in k:
            line.update(launches=4 if two else 2, moved_MB=round(geo_bytes / 1e6, 1), GB_per_s=round(geo_bytes / best[k][0] / 1e6, 1))
        print(json.dumps(line))
    ms = pillow_chain_ms(host, plans)
    print(json.dumps({'case': '500x375 train recipe, Pillow chain on one host core (no ToTensor / Normalize / padding)', 'batch': a.batch,
                      'ms_per_batch': None if ms is None else round(ms, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--augment', action='store_true', help="time the RandAugment path next to the plain one")
    ap.add_argument('--detector', action='store_true', help="time the detector's input pipeline next to the plain bicubic one")
    ap.add_argument('--rounds', type=int, default=5, help="alternating rounds of --iters batches each (--augment, --detector)")
    a = ap.parse_args()
    if a.augment:
        return augmented(a)
    if a.detector:
        return detector(a)
    rng = np.random.default_rng(0)
    coco = [(480, 640), (427, 640), (640, 480), (333, 500), (375, 500), (500, 375), (640, 428), (480, 640)]
    for name, shapes, policy in (('coco->maxwh(384,640)', [coco[i % 8] for i in range(a.batch)], MaxWHResize((384, 640))),
                                 ('1280x1280->640x640', [(1280, 1280)] * a.batch, MaxWHResize((640, 640)))):
        host = [torch.from_numpy(rng.integers(0, 256, s + (3,), dtype=np.uint8)) for s in shapes]
        dev = [h.cuda() for h in host]
        sizes = [policy.output_size(*s) for s in shapes]
        H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
        src = sum(3 * h * w for h, w in shapes)
        tmp = sum(3 * h * s[1] for (h, w), s in zip(shapes, sizes))
        algo = src + a.batch * H * W * 13
        pinned = [h.pin_memory() for h in host]
        for feed, label in ((dev, 'device-resident'), (pinned, 'host, pinned by the producer'), (host, 'host, pageable (staged)')):
            for _ in range(3):
                image_batch(feed, sizes, device='cuda')
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.iters):
                image_batch(feed, sizes, device='cuda')
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / a.iters
            ms = e0.elapsed_time(e1) / a.iters
            print(json.dumps({'case': name, 'input': label, 'batch': a.batch, 'out': [H, W], 'ms_per_batch': round(ms, 3),
                              'wall_ms_per_batch': round(wall * 1e3, 3), 'images_per_s': round(a.batch / wall),
                              'algorithmic_MB': round(algo / 1e6, 1), 'scratch_MB': round(2 * tmp / 1e6, 1),
                              'GB_per_s_algorithmic': round(algo / ms / 1e6, 1)}))


if __name__ == '__main__':
    main()
