"""Fixture G21, tests/golden/det_eval_g21_<case>.npz + det_eval_g21.json: the reference's COCOeval (its
datasets/detection/metrics/cocoeval.py, loaded by path) on the seeded cases of tests/golden/det_eval_draws.py.  A generator, not a test:

    python tests/golden/make_det_eval_golden.py /path/to/the/reference/checkout

The reference module imports pycocotools.mask for one function, the IoU of two lists of boxes.  pycocotools is no dependency of this
project, so that ONE function is stood in for by the published box IoU of the COCO API written out in float64 (bb_iou below, the formula of
include/grit_hip.h); `np.float`, which the module still uses, is set to `float`.  Everything else -- evaluateImg, accumulate,
summarize -- is the reference's own code.  Parity is therefore with the reference's cocoeval.py over that formula, not with the
pycocotools C library.

Only data is written.  Inputs are NOT stored: generator and tests redraw them from det_eval_draws.py.  Per case a-d:
  flags [I * N, A] uint32, rank [I * N] int32   the reference's evalImgs in the record layout of grit_det_eval_img: bit t of
                                                flags[row, a] = dtMatches[t] != 0, bit 16 + t = dtIgnore[t]; rank = the detection's
                                                position in its (image, category) list, -1 when it is in none; row = slot * N + n
  gt_ignore                                     gtIgnore of every (category, area range, image) entry in evalImgs order, concatenated
  precision, recall, scores, stats              COCOeval.eval / .stats;  result_text in the json
Case e (from logits, K = 37 and 1849): the seed, stats and result_text; its seed is advanced until det_eval_draws.fair holds.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import det_eval_draws as D  # noqa: E402


def bb_iou(dt, gt, iscrowd):
    """maskUtils.iou for boxes: [D, G] float64, boxes (x, y, w, h)."""
    if len(dt) == 0 or len(gt) == 0:
        return []
    out = np.zeros((len(dt), len(gt)))
    for a, d in enumerate(dt):
        for b, g in enumerate(gt):
            w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
            if w <= 0:
                w = 0
            h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
            if h <= 0:
                h = 0
            i = w * h
            u = d[2] * d[3] if iscrowd[b] else d[2] * d[3] + g[2] * g[3] - i
            out[a, b] = i / u
    return out


def load_cocoeval(ref):
    mask = types.ModuleType('pycocotools.mask')
    mask.iou = bb_iou
    pkg = types.ModuleType('pycocotools')
    pkg.mask = mask
    sys.modules.update({'pycocotools': pkg, 'pycocotools.mask': mask})
    np.float = float
    spec = importlib.util.spec_from_file_location('reference_cocoeval', os.path.join(ref, 'datasets', 'detection', 'metrics', 'cocoeval.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def run(cocoeval, dataset, seen, dets, n_det):
    """The reference on one case -> the fixture's arrays and the text."""
    slot = {i: n for n, i in enumerate(sorted(im['id'] for im in dataset['images']))}
    results = []
    for i in seen:
        scores, labels, boxes = dets[i]
        for n, box in enumerate(D.xywh(boxes).tolist()):
            results.append({'id': slot[i] * n_det + n + 1, 'image_id': i, 'category_id': int(labels[n]), 'bbox': box,
                            'score': float(scores[n]), 'area': box[2] * box[3], 'iscrowd': 0})
    E = cocoeval.COCOeval(D.Index(dataset), D.Index(dict(dataset, annotations=results)), iouType='bbox')
    E.params.imgIds = list(seen)
    E.evaluate()
    E.accumulate()
    E.summarize()
    A, T = len(E.params.areaRng), len(E.params.iouThrs)
    ranges = [tuple(r) for r in E.params.areaRng]
    flags = np.zeros((len(slot) * n_det, A), np.uint32)
    rank = np.full(len(slot) * n_det, -1, np.int32)
    gt_ignore = []
    for e in E.evalImgs:
        if e is None:
            continue
        a = ranges.index(tuple(e['aRng']))
        gt_ignore.append(np.asarray(e['gtIgnore'], np.uint8).reshape(-1))
        for pos, dt_id in enumerate(e['dtIds']):
            rank[dt_id - 1] = pos
            for t in range(T):
                flags[dt_id - 1, a] |= np.uint32((1 << t) * bool(e['dtMatches'][t, pos] != 0) | (1 << (16 + t)) * bool(e['dtIgnore'][t, pos]))
    arrays = {'flags': flags, 'rank': rank, 'gt_ignore': np.concatenate(gt_ignore) if gt_ignore else np.zeros(0, np.uint8),
              'precision': E.eval['precision'], 'recall': E.eval['recall'], 'scores': E.eval['scores'], 'stats': np.asarray(E.stats)}
    return arrays, E.result_text


def main(ref):
    cocoeval = load_cocoeval(ref)
    meta = {'text': {}, 'e2e': {}}
    for name in D.CASES:
        c = D.case(name)
        arrays, text = run(cocoeval, c['dataset'], c['seen'], c['dets'], c['n_det'])
        path = os.path.join(HERE, 'det_eval_g21_%s.npz' % name)
        np.savez_compressed(path, **arrays)
        meta['text'][name] = text
        print('case %s: %d bytes, stats %s' % (name, os.path.getsize(path), np.round(arrays['stats'], 4).tolist()))
    for K in D.E2E_KS:
        for seed in range(2150 + K, 2250 + K):
            logits, boxes, sizes, dataset, image_ids = D.end_to_end(K, seed)
            if D.fair(logits):
                break
        else:
            raise RuntimeError("no fair draw for K %d" % K)
        top_logit, top_index, corners = D.select(logits, boxes, sizes)
        dets = {i: (D.sigmoid32(top_logit[b]), (top_index[b] % K).astype(np.int64), corners[b]) for b, i in enumerate(image_ids)}
        arrays, text = run(cocoeval, dataset, image_ids, dets, top_logit.shape[1])
        meta['e2e'][str(K)] = {'seed': seed, 'stats': arrays['stats'].tolist(), 'text': text}
        print('case e K %d: seed %d, stats %s' % (K, seed, np.round(arrays['stats'], 4).tolist()))
    with open(os.path.join(HERE, 'det_eval_g21.json'), 'w') as f:
        json.dump(meta, f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1])
