"""Visual Genome evaluation of the detector: object AP and attribute AP (the reference's datasets/detection/metrics/vg_eval.py and
the `_do_python_eval` part of weighted_eval.py).  PASCAL-VOC AP at IoU 0.5 per class, once over the object classes and once over
the attribute classes, where an object is ground truth for every attribute it carries; the mean AP, the mean weighted by the
number of positives, and the per-class score thresholds of the best F score.

As in the COCO evaluation next door, the per-image matching runs on the device (grit_amd/ops/det_eval.py, grit_det_voc_img) and
leaves per-detection records there; `accumulate` copies them to the host ONCE and does the rest in numpy float64.

The reference's two files are Python 2 and import a module that it does not ship, so they cannot be run: the protocol is pinned by
hand-worked cases and by an independent sequential model (tests/vg_eval_model.py), not by recorded outputs.  Deviations:
  * no text-file round trip: scores are not rounded to 3 decimals, boxes not to 1, and the `+ 1` of the writer is not applied on top
    of the `+ 1` of the overlap;
  * equal scores are ordered (score descending, image slot ascending, rank within the image ascending), stably -- the reference's
    numpy.argsort leaves them undefined;
  * a class with ground truth and no detections has threshold 0 (the reference would index a scalar), and without any non-zero
    threshold the mean threshold is 0, not NaN;
  * attribute detections are PostProcessAttr's (models/detection/od_losses.py): the reference never built any.
One rank: the records of several ranks are not gathered.
"""
import numpy as np

from grit_amd.ops import det_eval as _ev

IOU_THRESHOLD = 0.5
KIND_NAMES = {'obj': 'objects', 'attr': 'attributes'}


def voc_ap(rec, prec):
    """The VOC-2010 area under the precision / recall points `rec`, `prec` (float64, in detection order): the curve gets the ends
    (0, 0) and (1, 0), precision is made non-increasing from the right, and the area is summed where recall changes."""
    mrec = np.concatenate(([0.], np.asarray(rec, np.float64), [1.]))
    mpre = np.concatenate(([0.], np.asarray(prec, np.float64), [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def accumulate_voc(packed_gt, records, class_ids):
    """packed_gt: PackedGroundTruth of the split; records: (flag, gt, iou, score, label, seen) as VocRecords.to_host() gives them;
    class_ids: the evaluated classes, in the order of the result.  Per class: npos = its ground-truth rows over ALL the split's
    images; its detections (flag 1: true positive, 2 / 3: false positive) from the seen images in the order (score descending,
    slot, rank); tp and fp cumulative, rec = tp / npos, prec = tp / max(tp + fp, eps); AP = voc_ap, 0 with npos 0 or no detection;
    threshold = the score at the first maximum of nan_to_num(prec rec / (prec + rec)) when npos > 1 and there is a detection,
    else 0.  -> {'class_ids', 'ap' [C], 'npos' [C], 'threshold' [C] (zeros replaced by the mean of the others), 'map' (plain mean,
    classes with AP 0 included), 'wmap' (weights npos / sum npos; 0 without any positive), 'mean_threshold'}."""
    flag, _, _, score, label, seen = records
    class_ids = np.asarray(class_ids, np.int64)
    if len(class_ids) == 0:
        raise ValueError("accumulate_voc: no class to evaluate")
    n_det = len(flag) // max(packed_gt.n_img, 1)
    n_cls = max(packed_gt.n_cat, int(class_ids.max()) + 1)
    npos_all = np.bincount(packed_gt.cat, minlength=n_cls)
    # rows in (slot, rank) order, then ONE stable sort by (class, -score): a class's slice is its detections in the stated order
    rows = np.nonzero(np.repeat(np.asarray(seen).astype(bool), n_det) & (flag > 0))[0]
    score64 = score[rows].astype(np.float64)
    order = np.lexsort((-score64, label[rows]))
    rows, score64 = rows[order], score64[order]
    label, is_tp = label[rows], flag[rows] == 1
    first, end = np.searchsorted(label, class_ids, 'left'), np.searchsorted(label, class_ids, 'right')
    eps = np.finfo(np.float64).eps
    ap, npos, threshold = np.zeros(len(class_ids)), np.zeros(len(class_ids)), np.zeros(len(class_ids))
    for k, c in enumerate(class_ids):
        npos[k] = npos_all[c]
        if npos[k] == 0 or first[k] == end[k]:
            continue
        hit = is_tp[first[k]:end[k]]
        tp, fp = np.cumsum(hit).astype(np.float64), np.cumsum(~hit).astype(np.float64)
        rec = tp / npos[k]
        prec = tp / np.maximum(tp + fp, eps)
        ap[k] = voc_ap(rec, prec)
        if npos[k] > 1:
            with np.errstate(invalid='ignore', divide='ignore'):
                f = np.nan_to_num((prec * rec) / (prec + rec))
            threshold[k] = score64[first[k]:end[k]][np.argmax(f)]
    nonzero = threshold != 0
    mean_threshold = float(np.mean(threshold[nonzero])) if nonzero.any() else 0.0
    threshold[~nonzero] = mean_threshold
    total = npos.sum()
    return {'class_ids': class_ids, 'ap': ap, 'npos': npos, 'threshold': threshold, 'map': float(np.mean(ap)),
            'wmap': float(np.average(ap, weights=npos / total)) if total > 0 else 0.0, 'mean_threshold': mean_threshold}


def summary_text(kind, evaluation):
    """The three summary lines of the reference's printout for one kind ('obj' / 'attr')."""
    name = KIND_NAMES.get(kind, kind)
    return ('%s: Mean AP = %.4f\n%s: Weighted Mean AP = %.4f\n%s: Mean Detection Threshold = %.3f\n'
            % (name, evaluation['map'], name, evaluation['wmap'], name, evaluation['mean_threshold']))


class VGEvaluator(object):
    """VGEvaluator(index, kinds=('obj',) or ('obj', 'attr'), num_attr=...): `index` is a COCO-API-like object (AnnotationIndex:
    getImgIds / getCatIds / getAnnIds / loadAnns, and loadImgs for 'attr') whose annotations carry 'attributes' (attribute ids) and
    whose images carry 'has_attr'; or a dictionary kind -> PackedGroundTruth.  `update` launches the matching of a batch per kind
    and returns at once; `accumulate` makes the one device-to-host copy per kind; `summarize` fills `stats` and `result_text`."""

    def __init__(self, index, kinds=('obj',), num_attr=None, device='cuda', iou_thr=IOU_THRESHOLD):
        if not isinstance(kinds, (list, tuple)) or not kinds:
            raise TypeError("VGEvaluator: kinds must be a non-empty list or tuple")
        for kind in kinds:
            if kind not in KIND_NAMES:
                raise ValueError("Unknown kind {}".format(kind))
        if 'attr' in kinds and not isinstance(index, dict) and not num_attr:
            raise ValueError("VGEvaluator: kind 'attr' needs num_attr")
        self.kinds, self.iou_thr = tuple(kinds), float(iou_thr)
        self.packed, self.gt = {}, {}
        for kind in self.kinds:
            if isinstance(index, dict):
                packed = index[kind]
            else:
                packed = _ev.pack_ground_truth(index) if kind == 'obj' else _ev.pack_ground_truth_attr(index, num_attr)
            self.packed[kind] = packed
            self.gt[kind] = _ev.DeviceGroundTruth(packed, device)
        self.reset()

    def reset(self):
        """Forget the detections seen so far."""
        self.records, self.eval, self.stats, self.result_text = {}, {}, {}, ""

    def update(self, results, targets):
        """results: {'obj': PostProcess's list, 'attr': PostProcessAttr's list} -- per image {'scores', 'labels', 'boxes'} -- with
        an entry for every kind of the evaluator; targets: the batch's target dicts (their 'image_id'), a tensor or a list of
        image ids.  No host synchronisation when the image ids are device tensors."""
        import torch
        for kind in self.kinds:  # before the first launch
            if kind not in results:
                raise ValueError("VGEvaluator.update: no results of kind %r" % kind)
            if targets is None or len(targets) != len(results[kind]):
                raise ValueError("VGEvaluator.update: one target (or image id) per result")
        for kind in self.kinds:
            res = results[kind]
            if len(res) == 0:
                continue
            ids = [t['image_id'] for t in targets] if isinstance(targets, (list, tuple)) and isinstance(targets[0], dict) else targets
            scores = torch.stack([r['scores'] for r in res]).float()
            labels = torch.stack([r['labels'] for r in res]).to(torch.int64)
            boxes = torch.stack([r['boxes'] for r in res]).float()
            if kind not in self.records:
                self.records[kind] = _ev.VocRecords(self.packed[kind].n_img, scores.shape[1], self.gt[kind].device)
            _ev.voc_images(scores, labels, boxes, self.gt[kind].slots_for(ids), self.gt[kind], self.iou_thr, self.records[kind])

    def synchronize_between_processes(self):
        """One rank: nothing to gather."""

    def accumulate(self):
        if not all(kind in self.records for kind in self.kinds):
            raise Exception('Please run update() first')
        for kind in self.kinds:
            self.eval[kind] = accumulate_voc(self.packed[kind], self.records[kind].to_host(), self.packed[kind].cat_ids)

    def summarize(self):
        if not all(kind in self.eval for kind in self.kinds):
            raise Exception('Please run accumulate() first')
        self.stats = {kind: {k: self.eval[kind][k] for k in ('map', 'wmap', 'mean_threshold')} for kind in self.kinds}
        self.result_text = ''.join(summary_text(kind, self.eval[kind]) for kind in self.kinds)
