"""Detector evaluation: PostProcess on grit_det_topk_f32 against the plain-torch composition it replaced, the per-image evaluation
launch, and the host's accumulation.  One JSON line per item.

    python tools/bench_det_eval.py [--batch 32] [--queries 150] [--classes 1849] [--gts 30] [--iters 50] [--images 5000] [--out FILE]

Seeded inputs: logits ~ N(-4, 1) (the best scores then lie around 0.5, where no two fp32 sigmoids of an image's best 101 coincide,
so the composition's order among equal scores, which torch leaves unspecified, does not enter the parity check), boxes inside the
unit square, image sizes in [300, 700).  HIP events after warm-up, the two PostProcess legs alternating in one process (three legs
each; `spread` is max - min of a kind's legs):
  * device      models.detection.od_losses.PostProcess (two launches + the sigmoid of the [B, 100] selected logits)
  * torch       PostProcess.forward as it was before: sigmoid over [B, Q, K], topk over Q * K, gather, scale (kept verbatim below)
  * parity      scores, labels and boxes of the two, compared bit for bit in the same run
  * eval_img    the grit_det_eval_img launch alone on the device leg's detections, `--gts` annotations per image (a third of them
                jittered copies of detections); an absolute time, the composition has no counterpart
  * accumulate  CocoEvaluator's accumulation (numpy, host wall time) of `--images` x 100 seeded records over `--classes` categories
It asserts nothing about speed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_post_process(outputs, target_sizes):
    """PostProcess.forward before grit_det_topk_f32, verbatim: the baseline leg."""
    from grit_amd.utils import box_ops
    logits, boxes = outputs['pred_logits'], outputs['pred_boxes']
    B, Q, K = logits.shape
    scores, flat = logits.sigmoid().reshape(B, Q * K).topk(min(100, Q * K), dim=1)
    query, labels = flat // K, flat % K
    corners = box_ops.box_cxcywh_to_xyxy(boxes).gather(1, query[..., None].expand(-1, -1, 4))
    height, width = target_sizes.unbind(1)
    corners = corners * torch.stack([width, height, width, height], 1)[:, None, :]
    return [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, corners)]


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def seeded_records(rng, images, n_det, classes, gts):
    """A split of `images` images with `gts` annotations each and n_det random records each, as numpy arrays."""
    from grit_amd.ops.det_eval import PackedGroundTruth
    G = images * gts
    wh = np.exp(rng.uniform(np.log(6.0), np.log(320.0), (G, 2)))
    box = np.concatenate([rng.uniform(0, 320, (G, 2)), wh], 1)
    cat = np.sort(rng.integers(0, classes, (images, gts)), 1).reshape(-1).astype(np.int32)
    gt = PackedGroundTruth(np.arange(images), np.arange(classes), (np.arange(images + 1) * gts).astype(np.int32), box, wh.prod(1),
                           cat, (rng.random(G) < 0.05).astype(np.uint8), np.repeat(np.arange(images), gts).astype(np.int32),
                           np.arange(1, G + 1))
    label = rng.integers(0, classes, (images, n_det)).astype(np.int32)
    score = np.sort(rng.random((images, n_det)).astype(np.float32), 1)[:, ::-1]
    rank = np.zeros((images, n_det), np.int32)
    for n in range(1, n_det):
        rank[:, n] = (label[:, :n] == label[:, n:n + 1]).sum(1)
    matched = (rng.random((images * n_det, 4, 1)) < np.linspace(0.6, 0.1, 10)).astype(np.uint32)
    ignored = (rng.random((images * n_det, 4, 10)) < 0.05).astype(np.uint32)
    weights = (1 << np.arange(10)).astype(np.uint32)
    flags = (matched * weights).sum(-1).astype(np.uint32) | ((ignored * weights).sum(-1).astype(np.uint32) << 16)
    return gt, flags, rank.reshape(-1), score.reshape(-1).copy(), label.reshape(-1), np.ones(images, np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--queries', type=int, default=150)
    ap.add_argument('--classes', type=int, default=1849)
    ap.add_argument('--gts', type=int, default=30)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_eval: needs a HIP device (a CPU timing says nothing about the kernels)")
    import datasets  # noqa: F401  (the reference's import paths)
    import models  # noqa: F401
    from datasets.detection.metrics import AnnotationIndex, CocoEvaluator, Params, accumulate_records
    from models.detection.od_losses import PostProcess
    dev = torch.device('cuda')
    B, Q, K = args.batch, args.queries, args.classes
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((rng.standard_normal((B, Q, K)) - 4.0).astype(np.float32)).to(dev)
    wh = 0.05 + 0.4 * rng.random((B, Q, 2))
    boxes = torch.from_numpy(np.concatenate([wh / 2 + (1 - wh) * rng.random((B, Q, 2)), wh], -1).astype(np.float32)).to(dev)
    sizes = torch.from_numpy(rng.integers(300, 700, (B, 2))).to(dev)
    outputs = {'pred_logits': logits, 'pred_boxes': boxes}
    post = PostProcess()
    kinds = [('device', lambda: post(outputs, sizes)), ('torch', lambda: torch_post_process(outputs, sizes))]
    results = {}
    for name, fn in kinds:
        for _ in range(3):
            results[name] = fn()
    torch.cuda.synchronize()
    legs = {name: [] for name, _ in kinds}
    for _ in range(3):
        for name, fn in kinds:
            legs[name].append(timed(fn, args.iters))
    shape = dict(batch=B, queries=Q, classes=K, device=torch.cuda.get_device_name(0))
    lines = []
    for name, _ in kinds:
        ms = legs[name]
        lines.append(dict(item=name, ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms], spread=round(max(ms) - min(ms), 4),
                          iters=args.iters, **shape))
    equal = {key: all(torch.equal(a[key], b[key]) and a[key].dtype == b[key].dtype for a, b in zip(results['device'], results['torch']))
             for key in ('scores', 'labels', 'boxes')}
    lines.append(dict(item='parity', bit_equal=equal, images=B, detections=int(results['device'][0]['scores'].numel())))

    # the per-image evaluation launch alone
    det = [{k: v.cpu().numpy() for k, v in r.items()} for r in results['device']]
    anns = []
    for b in range(B):
        for j in range(args.gts):
            if j % 3 == 0:
                x0, y0, x1, y1 = det[b]['boxes'][j].astype(np.float64)
                jit = rng.normal(0, 0.05, 4) * np.array([x1 - x0, y1 - y0, x1 - x0, y1 - y0])
                bbox, cat = [x0 + jit[0], y0 + jit[1], x1 - x0 + jit[2], y1 - y0 + jit[3]], int(det[b]['labels'][j])
            else:
                w, h = np.exp(rng.uniform(np.log(6.0), np.log(250.0), 2))
                bbox, cat = [float(rng.uniform(0, 300)), float(rng.uniform(0, 300)), w, h], int(rng.integers(0, K))
            anns.append({'id': len(anns) + 1, 'image_id': b, 'category_id': cat, 'bbox': [float(v) for v in bbox],
                         'area': float(bbox[2] * bbox[3] * rng.uniform(0.5, 1.0)), 'iscrowd': int(rng.random() < 0.05)})
    dataset = {'images': [{'id': b} for b in range(B)], 'categories': [{'id': c} for c in range(K)], 'annotations': anns}
    evaluator = CocoEvaluator(AnnotationIndex(dataset), ('bbox',))
    from grit_amd.ops import det_eval
    scores = torch.stack([r['scores'] for r in results['device']])
    labels = torch.stack([r['labels'] for r in results['device']])
    corners = torch.stack([r['boxes'] for r in results['device']])
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    evaluator.update(results['device'], list(range(B)))
    launch = lambda: det_eval.eval_images(scores, labels, corners, slots, evaluator.gt, evaluator.iou_thr, evaluator.area_rng, evaluator.records)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ms = [timed(launch, args.iters) for _ in range(3)]
    evaluator.accumulate()
    evaluator.summarize()
    lines.append(dict(item='eval_img', ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms], spread=round(max(ms) - min(ms), 4),
                      iters=args.iters, gts_per_image=args.gts, bbox_map=float(evaluator.coco_eval['bbox'].stats[0]), **shape))

    # the accumulation on the host
    gt, flags, rank, score, label, seen = seeded_records(rng, args.images, 100, K, args.gts)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        accumulate_records(gt, flags, rank, score, label, seen, Params())
        walls.append(time.perf_counter() - t0)
    lines.append(dict(item='accumulate', host_s=round(float(np.median(walls)), 4), legs=[round(x, 4) for x in walls], images=args.images,
                      records=args.images * 100, classes=K, annotations=int(gt.img_off[-1])))
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
