"""COCO-style box evaluation of the detector (the reference's datasets/detection/metrics/coco_eval.py CocoEvaluator over its
cocoeval.py COCOeval, iouType 'bbox'): the per-image matching runs on the device (grit_amd/ops/det_eval.py, grit_det_eval_img) and
leaves per-detection records there; `accumulate` copies them to the host ONCE per evaluation and does what cocoeval.py:336-456
does, vectorised per category, in the same IEEE float64 operations in the same order; `summarize` gives the 12 stats and the text.

Parity is with the reference's cocoeval.py over the published box IoU of the COCO API written out as a formula
(include/grit_hip.h), not with the pycocotools C library.  'segm' and 'keypoints' are not implemented.  One rank: the records
of several ranks are not gathered.
"""
import numpy as np

from grit_amd.ops import det_eval as _ev


class Params(object):
    """Params.setDetParams of the reference: the thresholds are numpy.linspace's numbers and are handed to the device as they are."""

    def __init__(self):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = 'bbox'


class AnnotationIndex(object):
    """The four calls of the COCO API that the evaluation needs, over a dataset dictionary {'images': [{'id'}], 'categories':
    [{'id'}], 'annotations': [{'id', 'image_id', 'category_id', 'bbox', 'area', 'iscrowd'}]}.  Further keys -- an annotation's
    'attributes', an image's 'has_attr' -- pass through untouched."""

    def __init__(self, dataset):
        self.dataset = dataset
        self.anns = {a['id']: a for a in dataset['annotations']}
        self.img_to_anns = {}
        for a in dataset['annotations']:
            self.img_to_anns.setdefault(a['image_id'], []).append(a)

    def getImgIds(self):
        return [i['id'] for i in self.dataset['images']]

    def getCatIds(self):
        return [c['id'] for c in self.dataset['categories']]

    def getAnnIds(self, imgIds=(), catIds=()):
        anns = [a for i in imgIds for a in self.img_to_anns.get(i, [])] if len(imgIds) else list(self.dataset['annotations'])
        cats = set(catIds)
        return [a['id'] for a in anns if not cats or a['category_id'] in cats]

    def loadAnns(self, ids=()):
        return [self.anns[i] for i in ids]

    def loadImgs(self, ids=()):
        """The image dictionaries as given ('has_attr' included), for the Visual Genome protocol's attribute split (vg_eval.py)."""
        images = {i['id']: i for i in self.dataset['images']}
        return [images[i] for i in ids]


def accumulate_records(gt, rec_flags, rec_rank, rec_score, rec_label, seen, params):
    """cocoeval.py:336-456 from the records of grit_det_eval_img (numpy; gt: PackedGroundTruth) -> {'precision' [T, R, K, A, M],
    'recall' [T, K, A, M], 'scores' [T, R, K, A, M], 'counts'}; K runs over gt.cat_ids.  -1 where a category has no regular
    ground truth in the seen images."""
    T, R, K, A, M = len(params.iouThrs), len(params.recThrs), len(gt.cat_ids), len(params.areaRng), len(params.maxDets)
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    seen = np.asarray(seen).astype(bool)
    n_det = rec_rank.shape[0] // max(gt.n_img, 1)
    # regular ground truths per (category, area range), over the seen images only
    npig = np.zeros((gt.n_cat, A), np.int64)
    ann_seen = seen[gt.ann_img]
    for a, (lo, hi) in enumerate(params.areaRng):
        regular = ann_seen & (gt.crowd == 0) & ~((gt.area < lo) | (gt.area > hi))
        npig[:, a] = np.bincount(gt.cat[regular], minlength=gt.n_cat)
    # the detections that take part, images in slot order and in score order within an image; then ONE stable sort by
    # (category, -score): a category's slice of it is the reference's mergesort of that category's concatenation, and the slice
    # of a maxDets cut is a subsequence of it
    rows = np.nonzero(np.repeat(seen, n_det) & (rec_rank >= 0))[0]
    score64 = rec_score[rows].astype(np.float64)
    order = np.lexsort((-score64, rec_label[rows]))
    rows, score64 = rows[order], score64[order]
    label, rank, flags = rec_label[rows], rec_rank[rows], rec_flags[rows].astype(np.uint32)
    first = np.searchsorted(label, gt.cat_ids, 'left')
    end = np.searchsorted(label, gt.cat_ids, 'right')
    bits = np.arange(T, dtype=np.uint32)[:, None]
    eps = np.spacing(1)
    for k, cat in enumerate(gt.cat_ids):
        if not npig[cat].any():
            continue
        seg = slice(first[k], end[k])
        for m, max_det in enumerate(params.maxDets):
            keep = rank[seg] < max_det
            f, s = flags[seg][keep], score64[seg][keep]
            nd = len(s)
            for a in range(A):
                if npig[cat, a] == 0:
                    continue
                if nd == 0:
                    recall[:, k, a, m] = 0
                    precision[:, :, k, a, m] = 0
                    scores[:, :, k, a, m] = 0
                    continue
                matched = ((f[None, :, a] >> bits) & 1).astype(bool)
                ignored = ((f[None, :, a] >> (bits + 16)) & 1).astype(bool)
                tp = np.cumsum(matched & ~ignored, axis=1).astype(dtype=float)
                fp = np.cumsum(~matched & ~ignored, axis=1).astype(dtype=float)
                rc = tp / npig[cat, a]
                pr = tp / (fp + tp + eps)
                recall[:, k, a, m] = rc[:, -1]
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                for t in range(T):
                    inds = np.searchsorted(rc[t], params.recThrs, side='left')
                    ok = inds < nd  # the reference's loop stops at the first recall threshold that is not reached
                    q, ss = np.zeros(R), np.zeros(R)
                    q[ok], ss[ok] = pr[t, inds[ok]], s[inds[ok]]
                    precision[t, :, k, a, m], scores[t, :, k, a, m] = q, ss
    return {'params': params, 'counts': [T, R, K, A, M], 'precision': precision, 'recall': recall, 'scores': scores}


def summarize_eval(evaluation, params):
    """COCOeval.summarize for 'bbox' -> (stats [12], the twelve text lines)."""
    lines = []

    def one(ap=1, iouThr=None, areaRng='all', maxDets=100):
        template = '{:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        title, kind = ('Average Precision', '(AP)') if ap == 1 else ('Average Recall', '(AR)')
        iou = '{:0.2f}:{:0.2f}'.format(params.iouThrs[0], params.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        aind = [i for i, name in enumerate(params.areaRngLbl) if name == areaRng]
        mind = [i for i, m in enumerate(params.maxDets) if m == maxDets]
        s = evaluation['precision'] if ap == 1 else evaluation['recall']
        if iouThr is not None:
            s = s[np.where(iouThr == params.iouThrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        lines.append(template.format(title, kind, iou, areaRng, maxDets, mean))
        return mean

    top = params.maxDets[2]
    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iouThr=.5, maxDets=top)
    stats[2] = one(1, iouThr=.75, maxDets=top)
    for i, name in enumerate(('small', 'medium', 'large')):
        stats[3 + i] = one(1, areaRng=name, maxDets=top)
    for i in range(3):
        stats[6 + i] = one(0, maxDets=params.maxDets[i])
    for i, name in enumerate(('small', 'medium', 'large')):
        stats[9 + i] = one(0, areaRng=name, maxDets=top)
    return stats, ''.join(line + '\n' for line in lines)


class BoxEval(object):
    """What the reference keeps in CocoEvaluator.coco_eval['bbox']: params, eval, stats, result_text."""

    def __init__(self, gt):
        self.gt, self.params = gt, Params()
        self.eval, self.stats, self.result_text = {}, [], ""

    def accumulate(self, rec_flags, rec_rank, rec_score, rec_label, seen):
        self.eval = accumulate_records(self.gt, rec_flags, rec_rank, rec_score, rec_label, seen, self.params)

    def summarize(self):
        if not self.eval:
            raise Exception('Please run accumulate() first')
        self.stats, self.result_text = summarize_eval(self.eval, self.params)


class CocoEvaluator(object):
    """CocoEvaluator(coco_gt, iou_types): coco_gt is a COCO-API-like object (getImgIds / getCatIds / getAnnIds / loadAnns, e.g.
    AnnotationIndex) or a PackedGroundTruth.  `update` launches the matching of a batch and returns at once; `accumulate` makes
    the one device-to-host copy; `summarize` fills coco_eval['bbox'].stats and .result_text.  n_det: detections per image
    (PostProcess gives min(100, Q * K)); by default taken from the first update."""

    def __init__(self, coco_gt, iou_types=('bbox',), device='cuda', n_det=None):
        if not isinstance(iou_types, (list, tuple)):
            raise TypeError("CocoEvaluator: iou_types must be a list or a tuple")
        for kind in iou_types:
            if kind in ('segm', 'keypoints'):
                raise NotImplementedError("CocoEvaluator: %r evaluation is not implemented, only 'bbox'" % kind)
            if kind != 'bbox':
                raise ValueError("Unknown iou type {}".format(kind))
        import torch
        self.iou_types = tuple(iou_types)
        self.packed = coco_gt if isinstance(coco_gt, _ev.PackedGroundTruth) else _ev.pack_ground_truth(coco_gt)
        self.gt = _ev.DeviceGroundTruth(self.packed, device)
        self.coco_eval = {'bbox': BoxEval(self.packed)}
        params = self.coco_eval['bbox'].params
        self.iou_thr = torch.from_numpy(np.asarray(params.iouThrs, np.float64)).to(self.gt.device)
        self.area_rng = torch.from_numpy(np.asarray(params.areaRng, np.float64)).to(self.gt.device)
        self._slot_of = {int(i): n for n, i in enumerate(self.packed.img_ids)}
        self.records = None
        self.n_det = n_det
        self.reset()

    def reset(self):
        """Forget the detections seen so far (the reference builds a new evaluator after every epoch)."""
        self.records = _ev.EvalRecords(self.packed.n_img, self.n_det, len(self.area_rng), self.gt.device) if self.n_det else None

    def _slots(self, image_ids):
        import torch
        if isinstance(image_ids, torch.Tensor):
            return self.gt.slots_of(image_ids.to(self.gt.device))
        if all(isinstance(i, torch.Tensor) for i in image_ids):
            return self.gt.slots_of(torch.stack([i.reshape(()) for i in image_ids]).to(self.gt.device))
        host = torch.tensor([self._slot_of.get(int(i), -1) for i in image_ids], dtype=torch.int32)
        return host.pin_memory().to(self.gt.device, non_blocking=True)

    def update(self, results_or_outputs, targets=None):
        """results: PostProcess's list of {'scores', 'labels', 'boxes'} (one per image) with `targets` = the batch's target dicts
        (their 'image_id'), a tensor or a list of image ids; or the reference's {image_id: prediction} with targets None; or the
        model's outputs {'pred_logits', 'pred_boxes'}, which go through PostProcess with the targets' 'orig_size' first.  No host
        synchronisation when the image ids are device tensors."""
        import torch
        results = results_or_outputs
        if isinstance(results, dict) and 'pred_logits' in results:
            from grit_amd.models.detection.od_losses import PostProcess
            results = PostProcess()(results, torch.stack([t['orig_size'] for t in targets], dim=0))
        if isinstance(results, dict):
            targets, results = list(results.keys()), list(results.values())
        if targets is None or len(targets) != len(results):
            raise ValueError("CocoEvaluator.update: one target (or image id) per result")
        if len(results) == 0:
            return
        ids = [t['image_id'] for t in targets] if isinstance(targets, (list, tuple)) and isinstance(targets[0], dict) else targets
        scores = torch.stack([r['scores'] for r in results]).float()
        labels = torch.stack([r['labels'] for r in results]).to(torch.int64)
        boxes = torch.stack([r['boxes'] for r in results]).float()
        if self.records is None:
            self.n_det = scores.shape[1]
            self.reset()
        _ev.eval_images(scores, labels, boxes, self._slots(ids), self.gt, self.iou_thr, self.area_rng, self.records)

    def synchronize_between_processes(self):
        """One rank: nothing to gather."""

    def accumulate(self):
        if self.records is None:
            raise Exception('Please run update() first')
        self.coco_eval['bbox'].accumulate(*self.records.to_host())

    def summarize(self):
        self.coco_eval['bbox'].summarize()
