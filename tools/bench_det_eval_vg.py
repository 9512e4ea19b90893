"""Visual Genome evaluation: the matching launch (grit_det_voc_img) against the two host-side forms of the same matching, and the
two post-processes.  One JSON line per item.

    python tools/bench_det_eval_vg.py [--batch 32] [--queries 150] [--classes 1849] [--attrs 400] [--objects 30]
                                      [--attrs-per-object 3] [--iters 50] [--out FILE]

Seeded inputs: logits and attribute logits ~ N(-4, 1), boxes inside the unit square, image sizes in [300, 700); per image `--objects`
objects (a third of them jittered copies of object detections with their labels, a third jittered copies of attribute detections),
each with about `--attrs-per-object` attributes, so the attribute split has about objects x attrs-per-object rows per image.
HIP events after warm-up, three legs of `--iters` calls each, the median leg reported; `spread` is max - min of the legs.
  * post_obj / post_attr      models.detection.od_losses.PostProcess / PostProcessAttr (two launches + the sigmoid of [B, 100])
  * post_attr_torch           the torch composition PostProcessAttr stands for (sigmoid, topk over Q x A, gather, scale)
  * voc_img_obj / _attr       the grit_det_voc_img launch alone on those detections, 20 x `--iters` calls a leg: back-to-back launches,
                              so the figure is bounded below by the host's enqueue rate
  * torch_match_obj / _attr   the same matching as a vectorised torch composition on the device: a padded [B, N, G] float64 overlap
                              table, masked maximum, first argmax, first occurrence by an [N, N] comparison; its equality with the
                              kernel's records is reported (`equal`), not assumed
  * numpy_match_obj / _attr   the same matching in numpy on host copies of the detections, vectorised per image (host wall time; the
                              copy to the host is timed separately as `to_host_ms`)
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


def torch_post_process_attr(outputs, target_sizes):
    from grit_amd.utils import box_ops
    logits, boxes = outputs['attr_logits'], outputs['pred_boxes']
    B, Q, A = logits.shape
    scores, flat = logits.sigmoid().reshape(B, Q * A).topk(min(100, Q * A), dim=1)
    query, labels = flat // A, flat % A
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


def legs(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = [timed(fn, iters) for _ in range(3)]
    return dict(ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms], spread=round(max(ms) - min(ms), 4), iters=iters)


class PaddedGroundTruth(object):
    """The split as [I, G] tables on the device for the torch composition: corners float64, class (-1 in the padding)."""

    def __init__(self, packed, device):
        G = max(packed.max_per_img, 1)
        corners, cat = np.zeros((packed.n_img, G, 4)), np.full((packed.n_img, G), -1, np.int64)
        for i in range(packed.n_img):
            lo, hi = packed.img_off[i], packed.img_off[i + 1]
            b = packed.box[lo:hi]
            corners[i, :hi - lo] = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)
            cat[i, :hi - lo] = packed.cat[lo:hi]
        self.corners, self.cat = torch.from_numpy(corners).to(device), torch.from_numpy(cat).to(device)
        self.valid = torch.from_numpy(packed.cat_valid.astype(bool)).to(device)
        self.index = torch.arange(G, device=device)


def torch_match(labels, boxes, slots, table, thr):
    """(flag uint8, jmax int32, ovmax float64), each [B, N], for images whose slots are all inside the split."""
    g, cat = table.corners[slots.long()], table.cat[slots.long()]  # [B, G, 4], [B, G]
    n_cat = table.valid.shape[0]
    inside = (labels >= 0) & (labels < n_cat)
    takes_part = inside & table.valid[labels.clamp(0, n_cat - 1)]
    bb = boxes.double()[:, :, None, :]
    gg = g[:, None, :, :]
    iw = (torch.minimum(gg[..., 2], bb[..., 2]) - torch.maximum(gg[..., 0], bb[..., 0]) + 1.0).clamp_(min=0.0)
    ih = (torch.minimum(gg[..., 3], bb[..., 3]) - torch.maximum(gg[..., 1], bb[..., 1]) + 1.0).clamp_(min=0.0)
    inters = iw * ih
    uni = (bb[..., 2] - bb[..., 0] + 1.0) * (bb[..., 3] - bb[..., 1] + 1.0) + (gg[..., 2] - gg[..., 0] + 1.0) * (gg[..., 3] - gg[..., 1] + 1.0) - inters
    mine = (cat[:, None, :] == labels[:, :, None]) & takes_part[:, :, None]
    ov = torch.where(mine, inters / uni, torch.full_like(inters, float('-inf')))
    ovmax = ov.amax(2)
    G = cat.shape[1]
    jmax = torch.where(mine & (ov == ovmax[:, :, None]), table.index, torch.full_like(table.index, G)).amin(2)
    jmax = torch.where(jmax == G, torch.full_like(jmax, -1), jmax)
    above = ovmax > thr
    N = labels.shape[1]
    earlier = torch.ones(N, N, dtype=torch.bool, device=labels.device).tril(-1)  # [n, m]: m < n
    same = (labels[:, :, None] == labels[:, None, :]) & (jmax[:, :, None] == jmax[:, None, :]) & above[:, None, :] & earlier
    flag = torch.where(above, torch.where(same.any(2), 3, 1), 2)
    flag = torch.where(takes_part, flag, torch.zeros_like(flag))
    return flag.to(torch.uint8), jmax.to(torch.int32), ovmax


def numpy_match(labels, boxes, slots, packed, thr):
    """The same on the host, vectorised per image: labels [B, N], boxes [B, N, 4] fp32 (numpy)."""
    B, N = labels.shape
    flag, row, iou = np.zeros((B, N), np.uint8), np.full((B, N), -1, np.int32), np.full((B, N), -np.inf)
    earlier = np.tri(N, N, -1, dtype=bool)
    for b in range(B):
        lo, hi = packed.img_off[slots[b]], packed.img_off[slots[b] + 1]
        lab = labels[b]
        part = (lab >= 0) & (lab < packed.n_cat)
        part &= packed.cat_valid[np.clip(lab, 0, packed.n_cat - 1)] != 0
        if hi > lo:
            g = packed.box[lo:hi]
            g0, g1, g2, g3 = g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
            bb = boxes[b].astype(np.float64)[:, :, None]
            iw = np.maximum(np.minimum(g2, bb[:, 2]) - np.maximum(g0, bb[:, 0]) + 1.0, 0.0)
            ih = np.maximum(np.minimum(g3, bb[:, 3]) - np.maximum(g1, bb[:, 1]) + 1.0, 0.0)
            inters = iw * ih
            uni = (bb[:, 2] - bb[:, 0] + 1.0) * (bb[:, 3] - bb[:, 1] + 1.0) + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - inters
            mine = (packed.cat[lo:hi][None, :] == lab[:, None]) & part[:, None]
            ov = np.where(mine, inters / uni, -np.inf)
            iou[b] = ov.max(1)
            row[b] = np.where(mine.any(1), ov.argmax(1), -1)
        above = iou[b] > thr
        same = (lab[:, None] == lab[None, :]) & (row[b][:, None] == row[b][None, :]) & above[None, :] & earlier
        flag[b] = np.where(part, np.where(above, np.where(same.any(1), 3, 1), 2), 0)
    return flag, row, iou


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--queries', type=int, default=150)
    ap.add_argument('--classes', type=int, default=1849)
    ap.add_argument('--attrs', type=int, default=400)
    ap.add_argument('--objects', type=int, default=30)
    ap.add_argument('--attrs-per-object', type=float, default=3.0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_eval_vg: needs a HIP device (a CPU timing says nothing about the kernels)")
    import datasets  # noqa: F401  (the reference's import paths)
    import models  # noqa: F401
    from datasets.detection.metrics import AnnotationIndex, VGEvaluator
    from grit_amd.ops import det_eval
    from models.detection.od_losses import PostProcess, PostProcessAttr
    dev = torch.device('cuda')
    B, Q, K, A = args.batch, args.queries, args.classes, args.attrs
    rng = np.random.default_rng(0)
    up = lambda a: torch.from_numpy(a).to(dev)
    wh = 0.05 + 0.4 * rng.random((B, Q, 2))
    outputs = {'pred_logits': up((rng.standard_normal((B, Q, K)) - 4.0).astype(np.float32)),
               'attr_logits': up((rng.standard_normal((B, Q, A)) - 4.0).astype(np.float32)),
               'pred_boxes': up(np.concatenate([wh / 2 + (1 - wh) * rng.random((B, Q, 2)), wh], -1).astype(np.float32))}
    sizes = up(rng.integers(300, 700, (B, 2)))
    post = {'obj': PostProcess(), 'attr': PostProcessAttr()}
    results = {kind: post[kind](outputs, sizes) for kind in post}
    shape = dict(batch=B, queries=Q, classes=K, attrs=A, device=torch.cuda.get_device_name(0))
    lines = [dict(item='post_obj', **legs(lambda: post['obj'](outputs, sizes), args.iters), **shape),
             dict(item='post_attr', **legs(lambda: post['attr'](outputs, sizes), args.iters), **shape),
             dict(item='post_attr_torch', **legs(lambda: torch_post_process_attr(outputs, sizes), args.iters), **shape)]
    composed = torch_post_process_attr(outputs, sizes)
    lines.append(dict(item='post_attr_parity', bit_equal={key: all(torch.equal(a[key], b[key]) for a, b in zip(results['attr'], composed))
                                                          for key in ('scores', 'labels', 'boxes')}))

    host = {kind: [{k: v.cpu().numpy() for k, v in r.items()} for r in res] for kind, res in results.items()}
    anns = []
    for b in range(B):
        for j in range(args.objects):
            kind = ('obj', 'attr', None)[j % 3]
            if kind is None:
                w, h = np.exp(rng.uniform(np.log(6.0), np.log(250.0), 2))
                bbox, cat, attributes = [float(rng.uniform(0, 300)), float(rng.uniform(0, 300)), w, h], int(rng.integers(0, K)), []
            else:
                x0, y0, x1, y1 = host[kind][b]['boxes'][j].astype(np.float64)
                jit = rng.normal(0, 0.05, 4) * np.array([x1 - x0, y1 - y0, x1 - x0, y1 - y0])
                bbox = [x0 + jit[0], y0 + jit[1], x1 - x0 + jit[2], y1 - y0 + jit[3]]
                cat = int(host['obj'][b]['labels'][j]) if kind == 'obj' else int(rng.integers(0, K))
                attributes = [int(host['attr'][b]['labels'][j])] if kind == 'attr' else []
            attributes += [int(a) for a in rng.integers(0, A, rng.poisson(max(args.attrs_per_object - len(attributes), 0)))]
            anns.append({'id': len(anns) + 1, 'image_id': b, 'category_id': cat, 'bbox': [float(v) for v in bbox], 'area': 1.0, 'iscrowd': 0,
                         'attributes': attributes})
    dataset = {'images': [{'id': b, 'has_attr': True} for b in range(B)], 'categories': [{'id': c} for c in range(K)], 'annotations': anns}
    ev = VGEvaluator(AnnotationIndex(dataset), ('obj', 'attr'), num_attr=A, device=dev)
    ev.update(results, list(range(B)))
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    for kind in ('obj', 'attr'):
        scores = torch.stack([r['scores'] for r in results[kind]])
        labels = torch.stack([r['labels'] for r in results[kind]])
        corners = torch.stack([r['boxes'] for r in results[kind]])
        gt, packed, records = ev.gt[kind], ev.packed[kind], ev.records[kind]
        rows = dict(rows_per_image=round(float(packed.img_off[-1]) / B, 1), max_rows=packed.max_per_img)
        launch = lambda: det_eval.voc_images(scores, labels, corners, slots, gt, 0.5, records)
        lines.append(dict(item='voc_img_' + kind, **legs(launch, 20 * args.iters), **rows, **shape))  # ~10 us a call: a longer window
        want = records.to_host()
        table = PaddedGroundTruth(packed, dev)
        composed = lambda: torch_match(labels, corners, slots, table, 0.5)
        flag, jmax, ovmax = (x.cpu().numpy().reshape(-1) for x in composed())
        equal = dict(flag=bool(np.array_equal(flag, want.flag)), gt=bool(np.array_equal(jmax, want.gt)),
                     iou_bits=bool(np.array_equal(ovmax.view(np.int64), want.iou.view(np.int64))))
        lines.append(dict(item='torch_match_' + kind, **legs(composed, args.iters), equal=equal, **rows, **shape))
        t0 = time.perf_counter()
        for _ in range(10):
            h_labels, h_boxes = labels.cpu().numpy(), corners.cpu().numpy()
        to_host = (time.perf_counter() - t0) / 10
        h_slots = slots.cpu().numpy()
        flag, jmax, ovmax = (x.reshape(-1) for x in numpy_match(h_labels, h_boxes, h_slots, packed, 0.5))
        equal = dict(flag=bool(np.array_equal(flag, want.flag)), gt=bool(np.array_equal(jmax, want.gt)),
                     iou_bits=bool(np.array_equal(ovmax.view(np.int64), want.iou.view(np.int64))))
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(5):
                numpy_match(h_labels, h_boxes, h_slots, packed, 0.5)
            walls.append((time.perf_counter() - t0) / 5 * 1e3)
        lines.append(dict(item='numpy_match_' + kind, host_ms=round(float(np.median(walls)), 4), legs=[round(x, 4) for x in walls],
                          to_host_ms=round(to_host * 1e3, 4), equal=equal, **rows, **shape))
    ev.accumulate()
    ev.summarize()
    lines.append(dict(item='summary', stats={k: {n: round(float(v), 6) for n, v in s.items()} for k, s in ev.stats.items()},
                      flags={k: np.bincount(ev.records[k].to_host().flag, minlength=4).tolist() for k in ev.kinds}))
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
