"""The detector's set criterion, device path against a plain-torch composition with a host assignment: one JSON line per item.

    python tools/bench_det_criterion.py [--batch 32] [--queries 150] [--classes 1849] [--layers 7] [--max-targets 60] [--iters 20] [--out FILE]

Seeded inputs: logits ~ N(-2, 2), boxes and targets inside the unit square, T ~ U{1..max-targets} per image.  Timed with HIP events
after warm-up, the two criteria alternating in one process (three legs each; `spread` is max - min of a kind's legs):
  * device   models.detection.od_losses.SetCriterion forward + weighted sum + backward (grit_det_match_f32, grit_det_loss_{fwd,bwd}_f32)
  * torch    the same losses composed from torch ops: per layer the cost matrix, a copy to the host, one
             scipy.optimize.linear_sum_assignment per image, a one-hot target, the focal / L1 / GIoU losses, backward.  When scipy
             is not importable this leg is reported as absent -- there is no host assignment to compare with.
  * match    the matching launch alone (cost + assignment of all layers * images)
It prints the relative difference of the two weighted totals as well; it asserts nothing about speed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COST = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
WEIGHT = {'loss_ce': 2.0, 'loss_bbox': 5.0, 'loss_giou': 2.0}


def draw_boxes(rng, n):
    wh = 0.05 + 0.4 * rng.random((n, 2))
    return np.concatenate([wh / 2 + (1 - wh) * rng.random((n, 2)), wh], 1).astype(np.float32)


def torch_criterion(logits, boxes, targets, lsa, alpha=0.25):
    """Plain-torch statement of the criterion (all layers), host assignment through `lsa`.  Returns the weighted total."""
    from utils.box_ops import box_cxcywh_to_xyxy, generalized_box_iou
    L, B, Q, K = logits.shape
    sizes = [len(t['labels']) for t in targets]
    labels = torch.cat([t['labels'] for t in targets])
    tboxes = torch.cat([t['boxes'] for t in targets])
    num_boxes = max(float(sum(sizes)), 1.0)
    total = 0
    for l in range(L):
        with torch.no_grad():
            p = logits[l].flatten(0, 1).sigmoid()
            b = boxes[l].flatten(0, 1)
            neg = 0.75 * p ** 2 * (-(1 - p + 1e-8).log())
            pos = 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log())
            C = (COST['cost_bbox'] * torch.cdist(b, tboxes, p=1) + COST['cost_class'] * (pos[:, labels] - neg[:, labels])
                 - COST['cost_giou'] * generalized_box_iou(box_cxcywh_to_xyxy(b), box_cxcywh_to_xyxy(tboxes)))
            C = C.view(B, Q, -1).cpu()
            pairs = [lsa(c[i]) for i, c in enumerate(C.split(sizes, -1))]
        bi = torch.cat([torch.full((len(i),), n, dtype=torch.int64) for n, (i, _) in enumerate(pairs)]).to(logits.device)
        qi = torch.cat([torch.as_tensor(i, dtype=torch.int64) for i, _ in pairs]).to(logits.device)
        ti = torch.cat([torch.as_tensor(j, dtype=torch.int64) + off for (_, j), off in zip(pairs, np.cumsum([0] + sizes[:-1]))]).to(logits.device)
        onehot = torch.zeros_like(logits[l])
        onehot[bi, qi, labels[ti]] = 1
        x = logits[l]
        prob = x.sigmoid()
        ce = torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction='none')
        p_t = prob * onehot + (1 - prob) * (1 - onehot)
        focal = (alpha * onehot + (1 - alpha) * (1 - onehot)) * ce * (1 - p_t) ** 2
        src, tgt = boxes[l][bi, qi], tboxes[ti]
        giou = torch.diag(generalized_box_iou(box_cxcywh_to_xyxy(src), box_cxcywh_to_xyxy(tgt)))
        total = total + (WEIGHT['loss_ce'] * focal.sum() + WEIGHT['loss_bbox'] * (src - tgt).abs().sum()
                         + WEIGHT['loss_giou'] * (1 - giou).sum()) / num_boxes
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--queries', type=int, default=150)
    ap.add_argument('--classes', type=int, default=1849)
    ap.add_argument('--layers', type=int, default=7)
    ap.add_argument('--max-targets', type=int, default=60)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_criterion: needs a HIP device (a CPU timing says nothing about the kernels)")
    import models  # noqa: F401  (the reference's import paths)
    import utils  # noqa: F401
    from models.detection.od_losses import HungarianMatcher, SetCriterion
    from grit_amd.ops import det_loss
    try:
        from scipy.optimize import linear_sum_assignment as lsa
    except ImportError:
        lsa = None
    dev = torch.device('cuda')
    L, B, Q, K = args.layers, args.batch, args.queries, args.classes
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((2 * rng.standard_normal((L, B, Q, K)) - 2).astype(np.float32)).to(dev).requires_grad_(True)
    boxes = torch.from_numpy(np.stack([draw_boxes(rng, B * Q).reshape(B, Q, 4) for _ in range(L)])).to(dev).requires_grad_(True)
    targets = []
    for _ in range(B):
        n = int(rng.integers(1, args.max_targets + 1))
        targets.append({'labels': torch.from_numpy(rng.integers(0, K, n)).to(dev), 'boxes': torch.from_numpy(draw_boxes(rng, n)).to(dev)})
    weight = dict(WEIGHT)
    for i in range(L - 1):
        weight.update({'%s_%d' % (k, i): v for k, v in WEIGHT.items()})
    matcher = HungarianMatcher(**COST)
    crit = SetCriterion(K, matcher, weight, ['labels', 'boxes', 'cardinality'])
    outputs = {'pred_logits': logits[-1], 'pred_boxes': boxes[-1],
               'aux_outputs': [{'pred_logits': logits[i], 'pred_boxes': boxes[i]} for i in range(L - 1)],
               'pred_logits_all': logits, 'pred_boxes_all': boxes}  # as DetectionModule.detection_head hands them out

    def device_step():
        losses = crit(outputs, targets)
        total = sum(losses[k] * weight[k] for k in losses if k in weight)
        total.backward()
        logits.grad = boxes.grad = None
        return total

    def torch_step():
        total = torch_criterion(logits, boxes, targets, lsa)
        total.backward()
        logits.grad = boxes.grad = None
        return total

    packed = det_loss.pack_targets(targets)

    def match_only():
        return matcher.match_layers(logits, boxes, packed)

    def timed(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters

    lines = []
    kinds = [('device', device_step, args.iters), ('match', match_only, args.iters)]
    if lsa is not None:
        kinds.insert(1, ('torch', torch_step, max(2, args.iters // 5)))
    totals = {}
    for name, fn, _ in kinds:
        for _ in range(3):
            r = fn()
        totals[name] = r
    torch.cuda.synchronize()
    legs = {name: [] for name, _, _ in kinds}
    for _ in range(3):
        for name, fn, iters in kinds:
            legs[name].append(timed(fn, iters))
    shape = dict(layers=L, batch=B, queries=Q, classes=K, targets=sum(len(t['labels']) for t in targets), device=torch.cuda.get_device_name(0))
    for name, _, iters in kinds:
        ms = legs[name]
        lines.append(dict(item=name, ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms], spread=round(max(ms) - min(ms), 4),
                          iters=iters, **shape))
    if lsa is None:
        lines.append(dict(item='torch', absent='scipy is not importable here: no host assignment to compare with', **shape))
    else:
        a, b = float(totals['device']), float(totals['torch'])
        lines.append(dict(item='parity', device_total=a, torch_total=b, relative_difference=abs(a - b) / abs(b)))
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
