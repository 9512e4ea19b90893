"""Fixture G19, tests/golden/det_loss_g19.npz + .json: the reference's HungarianMatcher, SetCriterion, detection heads and Detector
(imported behind the stubs of make_golden.py plus one for torchvision.ops.boxes.box_area) on seeded inputs.  A generator, not a test:

    python tests/golden/make_det_loss_golden.py /path/to/the/reference/checkout [--skip-e2e]

Only data is written, split over det_loss_g19.npz, det_loss_g19.1.npz, ... so that no file exceeds 1 MiB (det_draws.load_shards
reads them back as one dictionary).  Inputs are NOT stored: generator and tests repeat them from tests/golden/det_draws.py and the seeds kept here.

  match/*   per (layer, Q, T) problem of det_draws.MATCH_CASES (K = 37) and of the one K = 1849 case: the seed, scipy's pairs, the
            optimum (float64 sum over the fp32 cost matrix), the uniqueness margin and the fp32 cost matrix the reference handed
            to scipy -- for every problem.
  crit/*    L = 3, B = 3, Q = 150, T = (0, 5, 40), K in (37, 1849): every loss key in fp32 and from the same code run in float64, and
            of the float64 run's weighted total the gradients: dboxes at the matched rows (it is zero elsewhere), dlogits at the matched
            rows (whole rows), every 97th element of the flat map, and the float64 sum of |dlogits|.  Plus an all-empty batch.
  head/*    DetectionModule.detection_head in train and eval mode, 4-d and 2-d references, deterministic fill.
  e2e/*     a 224 x 224, B = 2 detector step: Detector.forward (train mode, dropout 0) -> SetCriterion, every loss key.
  json      the Detector's state-dict keys, the seeds and the margins.

Uniqueness margin of a problem: for each matched pair in turn, forbid it and solve again; the margin is the smallest increase of the
optimum.  A problem's seed is redrawn until the margin is >= 1e-2, so that index equality with scipy is a fair demand on a solver
that sees costs differing by fp32 rounding.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import det_draws as D  # noqa: E402

MARGIN = 1e-2


def import_reference(ref):
    import types
    import make_golden
    make_golden.REF = ref
    make_golden.import_reference()
    tv = sys.modules["torchvision"]
    ops = types.ModuleType("torchvision.ops")
    bx = types.ModuleType("torchvision.ops.boxes")
    bx.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    ops.boxes, tv.ops = bx, ops
    sys.modules.update({"torchvision.ops": ops, "torchvision.ops.boxes": bx})


def solve(C):
    from scipy.optimize import linear_sum_assignment
    i, j = linear_sum_assignment(C)
    return i, j, float(C.astype(np.float64)[i, j].sum())


def margin_of(C):
    """Smallest increase of the optimum when one matched pair is forbidden (inf when nothing is matched)."""
    i, j, opt = solve(C)
    best = np.inf
    for a, b in zip(i, j):
        Cf = C.astype(np.float64).copy()
        Cf[a, b] = 1e6
        ii, jj = solve(Cf)[:2]
        alt = float(Cf[ii, jj].sum())
        if alt < 1e5:
            best = min(best, alt - opt)
    return best


class Capture(object):
    """Stands in for scipy's solver inside the reference module: records every cost matrix it is handed."""

    def __init__(self):
        self.costs = []

    def __call__(self, c):
        from scipy.optimize import linear_sum_assignment
        c = np.asarray(c)
        self.costs.append(c.copy())
        return linear_sum_assignment(c)


def ref_costs(od, logits, boxes, tg):
    """The fp32 cost matrices the reference matcher builds for one layer: logits [B, Q, K], boxes [B, Q, 4], tg = [(labels, boxes)]."""
    cap = Capture()
    od.linear_sum_assignment = cap
    matcher = od.HungarianMatcher(D.COST_WEIGHTS['class'], D.COST_WEIGHTS['bbox'], D.COST_WEIGHTS['giou'])
    matcher({'pred_logits': torch.from_numpy(logits), 'pred_boxes': torch.from_numpy(boxes)},
            [{'labels': torch.from_numpy(l), 'boxes': torch.from_numpy(b)} for l, b in tg])
    return cap.costs


def draw_problem(od, base_seed, Q, K, tg):
    """Redraw the predictions of one problem until its margin is large enough -> (seed, cost, margin)."""
    for attempt in range(200):
        seed = base_seed * 1000 + attempt
        logits, boxes = D.predictions(seed, Q, K)
        C = ref_costs(od, logits[None], boxes[None], [tg])[0].astype(np.float32)
        m = margin_of(C) if min(C.shape) > 0 else np.inf
        if m >= MARGIN:
            return seed, C, m
    raise RuntimeError("no draw with margin >= %g for Q %d T %d" % (MARGIN, Q, len(tg[0])))


def make_match(od, out, meta):
    problems = []
    for ci, (Q, T) in enumerate(D.MATCH_CASES):
        tg = D.targets(7000 + ci, T, D.MATCH_K)
        for layer in range(D.MATCH_LAYERS):
            seed, C, m = draw_problem(od, 100 + ci * 10 + layer, Q, D.MATCH_K, tg)
            i, j, opt = solve(C)
            key = 'match/%d/%d' % (ci, layer)
            out[key + '/i'], out[key + '/j'] = i.astype(np.int32), j.astype(np.int32)
            out[key + '/cost'] = C
            problems.append({'case': ci, 'layer': layer, 'Q': Q, 'T': T, 'seed': seed, 'target_seed': 7000 + ci, 'optimum': opt,
                             'margin': None if np.isinf(m) else m})
            print('match Q %3d T %3d layer %d seed %d optimum %.6f margin %s' % (Q, T, layer, seed, opt, m))
    meta['match'] = problems
    big = []
    for b, T in enumerate(D.BIG_CASE_T):
        tg = D.targets(7100 + b, T, D.BIG_K)
        for layer in range(2):
            seed, C, m = draw_problem(od, 300 + b * 10 + layer, 150, D.BIG_K, tg)
            i, j, opt = solve(C)
            key = 'bigmatch/%d/%d' % (b, layer)
            out[key + '/i'], out[key + '/j'], out[key + '/cost'] = i.astype(np.int32), j.astype(np.int32), C
            big.append({'image': b, 'layer': layer, 'Q': 150, 'T': T, 'seed': seed, 'target_seed': 7100 + b, 'optimum': opt, 'margin': m})
            print('bigmatch T %d layer %d seed %d margin %s' % (T, layer, seed, m))
    meta['bigmatch'] = big


def run_criterion(od, logits, boxes, tg, K, dtype):
    """The reference criterion on logits [L, B, Q, K] / boxes (numpy fp32) in `dtype`: losses, and the gradients of the weighted total."""
    od.linear_sum_assignment = Capture()
    L = logits.shape[0]
    weight = dict(D.LOSS_WEIGHTS)
    for i in range(L - 1):
        weight.update({'%s_%d' % (k, i): v for k, v in D.LOSS_WEIGHTS.items()})
    matcher = od.HungarianMatcher(D.COST_WEIGHTS['class'], D.COST_WEIGHTS['bbox'], D.COST_WEIGHTS['giou'])
    crit = od.SetCriterion(K, matcher, weight, ['labels', 'boxes', 'cardinality'], focal_alpha=0.25)
    lg = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    bx = torch.from_numpy(boxes).to(dtype).requires_grad_(True)
    outputs = {'pred_logits': lg[-1], 'pred_boxes': bx[-1],
               'aux_outputs': [{'pred_logits': lg[i], 'pred_boxes': bx[i]} for i in range(L - 1)]}
    targets = [{'labels': torch.from_numpy(l), 'boxes': torch.from_numpy(b).to(dtype)} for l, b in tg]
    losses = crit(outputs, targets)
    total = sum(losses[k] * weight[k] for k in losses if k in weight)
    total.backward()
    return {k: float(v) for k, v in losses.items()}, float(total), lg.grad.numpy(), bx.grad.numpy(), od.linear_sum_assignment.costs


def make_criterion(od, out, meta):
    meta['crit'] = {}
    L, B, Q = D.CRIT_L, D.CRIT_B, D.CRIT_Q
    for K in D.CRIT_KS:
        tg = [D.targets(8000 + K + b, T, K) for b, T in enumerate(D.CRIT_T)]
        seeds = np.zeros((L, B), np.int64)
        margins = np.zeros((L, B))
        logits = np.zeros((L, B, Q, K), np.float32)
        boxes = np.zeros((L, B, Q, 4), np.float32)
        for l in range(L):
            for b in range(B):
                seed, _, m = draw_problem(od, 500 + (K % 100) * 100 + l * 10 + b, Q, K, tg[b])
                seeds[l, b], margins[l, b] = seed, (m if np.isfinite(m) else -1)
                logits[l, b], boxes[l, b] = D.predictions(seed, Q, K)
        l32, t32, _, _, _ = run_criterion(od, logits, boxes, tg, K, torch.float32)
        l64, t64, dlogits, dboxes, costs = run_criterion(od, logits, boxes, tg, K, torch.float64)
        # the matching of the run: layers in the criterion's order (last first, then the auxiliary ones)
        order = [L - 1] + list(range(L - 1))
        rows, vals, brow = [], [], []
        for n, C in enumerate(costs):
            l, b = order[n // B], n % B
            i, j = solve(C)[:2]
            for q, t in zip(i, j):
                rows.append((l, b, q, t))
                vals.append(dlogits[l, b, q])
                brow.append(dboxes[l, b, q])
        mask = np.ones((L, B, Q), bool)
        for l, b, q, _ in rows:
            mask[l, b, q] = False
        assert not dboxes[mask].any()
        key = 'crit/%d' % K
        out[key + '/rows'] = np.asarray(rows, np.int32).reshape(-1, 4)
        for first in range(0, len(vals), 15):  # pieces small enough to be spread over the shards
            out[key + '/row_values/%03d' % first] = np.stack(vals[first:first + 15])
        out[key + '/dboxes'] = np.asarray(brow, np.float64).reshape(-1, 4)
        out[key + '/sample'] = dlogits.reshape(-1)[::D.SAMPLE_STRIDE].copy()
        out[key + '/abs_sum'] = np.array(np.abs(dlogits).sum())
        out[key + '/dlogits_max'] = np.array(np.abs(dlogits).max())
        out[key + '/dboxes_max'] = np.array(np.abs(dboxes).max())
        meta['crit'][str(K)] = {'seeds': seeds.tolist(), 'margins': margins.tolist(), 'target_seeds': [8000 + K + b for b in range(B)],
                                'losses32': l32, 'losses64': l64, 'total32': t32, 'total64': t64}
        print('crit K %d total %.8f / %.8f margins min %.4f |dlogits| %.6f' % (K, t32, t64, margins[margins >= 0].min(), np.abs(dlogits).sum()))
    # all-empty batch: num_boxes clamps to 1
    K = 37
    tg = [D.targets(0, 0, K) for _ in range(2)]
    logits = np.stack([np.stack([D.predictions(900 + l * 2 + b, 20, K)[0] for b in range(2)]) for l in range(2)])
    boxes = np.stack([np.stack([D.predictions(900 + l * 2 + b, 20, K)[1] for b in range(2)]) for l in range(2)])
    l64, t64, dlogits, dboxes, _ = run_criterion(od, logits, boxes, tg, K, torch.float64)
    out['empty/abs_sum'] = np.array(np.abs(dlogits).sum())
    meta['empty'] = {'losses64': l64, 'total64': t64, 'L': 2, 'B': 2, 'Q': 20, 'K': K, 'seed0': 900}


def make_heads(out, meta):
    from models.detection.det_module import DetectionModule
    from fill import deterministic_fill_
    cfg = dict(d_model=32, nhead=4, num_decoder_layers=2, dim_feedforward=64, dropout=0.0, num_classes=5, num_queries=6,
               aux_loss=True, with_box_refine=True, num_feature_levels=4, dec_n_points=4)
    mod = deterministic_fill_(DetectionModule(**cfg), 'g19.head.')
    rng = np.random.default_rng(19)
    hs = rng.standard_normal((3, 2, 6, 32)).astype(np.float32)
    refs = (0.05 + 0.9 * rng.random((3, 2, 6, 4))).astype(np.float32)
    out['head/hs'], out['head/refs'] = hs, refs
    for dim in (4, 2):
        inter = torch.from_numpy(refs[..., :dim].copy())
        init = inter[0].clone()  # inter_references[0] is the initial reference in the decoder's own output
        for mode in ('train', 'eval'):
            mod.train(mode == 'train')
            with torch.no_grad():
                o = mod.detection_head(torch.from_numpy(hs), init, inter)
            key = 'head/%s%d' % (mode, dim)
            out[key + '/logits'], out[key + '/boxes'] = o['pred_logits'].numpy(), o['pred_boxes'].numpy()
            if mode == 'train':
                out[key + '/aux_logits'] = np.stack([a['pred_logits'].numpy() for a in o['aux_outputs']])
                out[key + '/aux_boxes'] = np.stack([a['pred_boxes'].numpy() for a in o['aux_outputs']])
    meta['head'] = cfg


E2E = dict(num_classes=11, num_queries=30, d_model=512, counts=(3, 6))


def _ref_detector():
    from types import SimpleNamespace
    from models.common.swin_model import swin_base_win7_384
    from models.detection.det_module import build_det_module_with_config
    from models.detection.detector import Detector
    from fill import deterministic_fill_
    cfg = SimpleNamespace(d_model=E2E['d_model'], num_heads=8, num_layers=6, dim_feedforward=1024, dropout=0.0, activation='relu',
                          num_classes=E2E['num_classes'], num_levels=4, num_points=4, num_queries=E2E['num_queries'],
                          return_intermediate=True, aux_loss=True, with_box_refine=True)
    backbone, _ = swin_base_win7_384(pretrained=None)
    return deterministic_fill_(Detector(backbone, build_det_module_with_config(cfg), hidden_dim=E2E['d_model']))


def make_keys(meta):
    meta['state_dict_keys'] = sorted(_ref_detector().state_dict().keys())


def make_e2e(od, out, meta):
    from engine.utils import NestedTensor
    model = _ref_detector().train()
    weight = dict(D.LOSS_WEIGHTS)
    for i in range(6):
        weight.update({'%s_%d' % (k, i): v for k, v in D.LOSS_WEIGHTS.items()})
    for seed in range(1900, 1940):
        images, tg = D.end_to_end_batch(seed, num_classes=E2E['num_classes'], counts=E2E['counts'])
        od.linear_sum_assignment = Capture()
        matcher = od.HungarianMatcher(D.COST_WEIGHTS['class'], D.COST_WEIGHTS['bbox'], D.COST_WEIGHTS['giou'])
        crit = od.SetCriterion(E2E['num_classes'], matcher, weight, ['labels', 'boxes', 'cardinality'], focal_alpha=0.25)
        with torch.no_grad():
            outputs = model(NestedTensor(torch.from_numpy(images), torch.zeros(2, 224, 224, dtype=torch.bool)))
            losses = crit(outputs, [{'labels': torch.from_numpy(l), 'boxes': torch.from_numpy(b)} for l, b in tg])
        margins = [margin_of(C.astype(np.float32)) for C in od.linear_sum_assignment.costs]
        print('e2e seed %d min margin %.5f' % (seed, min(margins)))
        if len(margins) == 14 and min(margins) >= MARGIN:
            break
    else:
        raise RuntimeError("no end-to-end draw with every margin >= %g" % MARGIN)
    total = sum(float(losses[k]) * weight[k] for k in losses if k in weight)
    meta['e2e'] = dict(E2E, seed=seed, margins=margins, losses={k: float(v) for k, v in losses.items()}, total=total)
    print('e2e total', total)


def main(ref, skip_e2e=False):
    import_reference(ref)
    import models.detection.od_losses as od
    out, meta = {}, {}
    path = os.path.join(HERE, 'det_loss_g19')
    make_match(od, out, meta)
    make_criterion(od, out, meta)
    make_heads(out, meta)
    make_keys(meta)
    if skip_e2e:
        if os.path.exists(path + '.json'):
            old = json.load(open(path + '.json'))
            if 'e2e' in old:
                meta['e2e'] = old['e2e']
    else:
        make_e2e(od, out, meta)
    import glob
    for old in glob.glob(path + '*.npz'):
        os.remove(old)
    shards, size = [{}], 0
    for k in sorted(out):
        a = np.asarray(out[k])
        if size and size + a.nbytes > D.SHARD_BYTES:
            shards.append({})
            size = 0
        shards[-1][k] = a
        size += a.nbytes + 200
    for n, shard in enumerate(shards):
        np.savez_compressed(path + ('.%d' % n if n else '') + '.npz', **shard)
    with open(path + '.json', 'w') as f:
        json.dump(meta, f)
    print('g19: npz shards of %s bytes, %d bytes json' % ([os.path.getsize(p) for p in sorted(glob.glob(path + '*.npz'))], os.path.getsize(path + '.json')))


if __name__ == '__main__':
    main(sys.argv[1], '--skip-e2e' in sys.argv)
