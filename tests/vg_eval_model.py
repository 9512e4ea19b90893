"""The per-image matching of the Visual Genome protocol (include/grit_hip.h, grit_det_voc_img) as a numpy model in the plainest
form, written from the protocol's statement: a sequential walk over an image's detections in score order with one `det` flag per
ground-truth row.  The kernel decides "true positive or duplicate" by a first-occurrence test over the detections instead, so the
two check each other.  Also the inputs that both the CPU and the GPU tests use: the hand-built images and the seeded draws."""
import collections

import numpy as np

Records = collections.namedtuple("Records", "flag gt iou score label seen")  # the fields of VocRecords.to_host(), in its order


def empty_records(n_img, n_det):
    """What grit_amd.ops.det_eval.VocRecords holds before the first launch."""
    return Records(np.zeros(n_img * n_det, np.uint8), np.full(n_img * n_det, -1, np.int32), np.full(n_img * n_det, -np.inf, np.float64),
                   np.zeros(n_img * n_det, np.float32), np.full(n_img * n_det, -1, np.int32), np.zeros(n_img, np.uint8))


def overlaps(bb, rows):
    """bb: a detection's corners (float64 [4]); rows: ground truth (x, y, w, h) float64 [G, 4] -> the protocol's overlap [G], one
    IEEE operation at a time."""
    g0, g1 = rows[:, 0], rows[:, 1]
    g2, g3 = rows[:, 0] + rows[:, 2], rows[:, 1] + rows[:, 3]
    iw = np.maximum(np.minimum(g2, bb[2]) - np.maximum(g0, bb[0]) + 1.0, 0.0)
    ih = np.maximum(np.minimum(g3, bb[3]) - np.maximum(g1, bb[1]) + 1.0, 0.0)
    inters = iw * ih
    uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - inters
    return inters / uni


def match_images(scores, labels, boxes, slots, gt, thr=0.5, records=None):
    """scores [B, N] fp32, labels [B, N] int64, boxes [B, N, 4] fp32 corners in score order, slots [B]; gt: PackedGroundTruth ->
    Records over the split (`records` is updated in place when given)."""
    B, N = scores.shape
    rec = empty_records(gt.n_img, N) if records is None else records
    for b in range(B):
        img = int(slots[b])
        if img < 0 or img >= gt.n_img:
            continue
        first, end = int(gt.img_off[img]), int(gt.img_off[img + 1])
        det = [False] * (end - first)
        for n in range(N):  # in score order: an earlier detection takes a row before a later one
            row = img * N + n
            label = int(labels[b, n])
            rec.score[row], rec.label[row] = scores[b, n], np.int32(label)
            rec.flag[row], rec.gt[row], rec.iou[row] = 0, -1, -np.inf
            if label < 0 or label >= gt.n_cat or not gt.cat_valid[label]:
                continue
            mine = [g for g in range(end - first) if gt.cat[first + g] == label]
            ovmax, jmax = -np.inf, -1
            if mine:
                ov = overlaps(boxes[b, n].astype(np.float64), gt.box[first:end][mine])
                ovmax, jmax = np.max(ov), mine[int(np.argmax(ov))]
            rec.gt[row], rec.iou[row] = jmax, ovmax
            if ovmax > thr:
                rec.flag[row] = 3 if det[jmax] else 1
                det[jmax] = True
            else:
                rec.flag[row] = 2
        rec.seen[img] = 1
    return rec


class Index(object):
    """getImgIds / getCatIds / getAnnIds / loadAnns / loadImgs over a dataset dictionary."""

    def __init__(self, dataset):
        self.dataset = dataset

    def getImgIds(self):
        return [i['id'] for i in self.dataset['images']]

    def getCatIds(self):
        return [c['id'] for c in self.dataset['categories']]

    def getAnnIds(self, imgIds=()):
        return [a['id'] for a in self.dataset['annotations'] if a['image_id'] in imgIds]

    def loadAnns(self, ids=()):
        by_id = {a['id']: a for a in self.dataset['annotations']}
        return [by_id[i] for i in ids]

    def loadImgs(self, ids=()):
        by_id = {i['id']: i for i in self.dataset['images']}
        return [by_id[i] for i in ids]


def dataset_of(image_ids, cat_ids, anns):
    """anns: (image_id, category, [x, y, w, h]) in annotation order; ids from 1."""
    return {'images': [{'id': i} for i in image_ids], 'categories': [{'id': c} for c in cat_ids],
            'annotations': [{'id': n + 1, 'image_id': i, 'category_id': c, 'bbox': [float(v) for v in b], 'area': float(b[2] * b[3]),
                             'iscrowd': 0} for n, (i, c, b) in enumerate(anns)]}


# ---- hand-built images: every expected record is worked out by hand -----------------------------------------------------------------

HAND_CATS = [0, 1, 2, 4]  # 3 is no category (cat_valid 0); n_cat = 5
HAND_IMAGES = [7, 3]  # in batch order; slots 1 and 0
HAND_N = 6
INF = float('inf')


def hand_built():
    """-> (dataset, scores [2, 6], labels, boxes, expected flag / gt / iou [2, 6] in batch order).

    Image 7 (rows after packing: 0 = class 0 (0, 0, 9, 4); 1 and 2 = class 1, twice (10, 10, 20, 20)):
      n0  label 0, (0, 0, 9, 9): areas 100 and 50, intersection 50, union 100, overlap exactly 0.5 -> no match (strict), row 0
      n1  label 0, (0, 0, 9, 5): area 60, intersection 50, union 60 -> 50 / 60, true positive on row 0
      n2  label 0, (0, 0, 9, 4): overlap 1 with row 0, which n1 holds -> duplicate
      n3  label 1, (10, 10, 30, 30): overlap 1 with rows 1 and 2 -> the first of the two, true positive
      n4  label 1, the same box: row 1 again (NOT the free row 2) -> duplicate
      n5  label 3: no category -> takes no part
    Image 3 (rows: 0 = class 0 (0, 0, 9, 9); 1 = class 0 (10, 0, 9, 9); 2 = class 4 (100, 100, 9, 9)):
      n0  label 0, (5, 0, 14, 9): 50 / 150 with both rows of class 0 -> row 0, no match
      n1  label 4, (0, 0, 9, 9): nothing in common with row 2 -> overlap 0 on row 2, no match
      n2  label 2: a category without rows in this image -> no match, row -1, overlap -inf
      n3  label 7: outside the table; n4 label -1; n5 label 5 = n_cat: take no part"""
    anns = [(7, 1, [10, 10, 20, 20]), (7, 0, [0, 0, 9, 4]), (7, 1, [10, 10, 20, 20]), (7, 3, [0, 0, 50, 50]),
            (3, 4, [100, 100, 9, 9]), (3, 0, [0, 0, 9, 9]), (3, 0, [10, 0, 9, 9])]
    dataset = dataset_of([7, 3], HAND_CATS, anns)
    labels = np.array([[0, 0, 0, 1, 1, 3], [0, 4, 2, 7, -1, 5]], np.int64)
    boxes = np.array([[[0, 0, 9, 9], [0, 0, 9, 5], [0, 0, 9, 4], [10, 10, 30, 30], [10, 10, 30, 30], [0, 0, 9, 4]],
                      [[5, 0, 14, 9], [0, 0, 9, 9], [0, 0, 9, 9], [0, 0, 9, 9], [0, 0, 9, 9], [0, 0, 9, 9]]], np.float32)
    scores = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4], [0.95, 0.85, 0.75, 0.65, 0.55, 0.45]], np.float32)
    flag = np.array([[2, 1, 3, 1, 3, 0], [2, 2, 2, 0, 0, 0]], np.uint8)
    row = np.array([[0, 0, 0, 1, 1, -1], [0, 2, -1, -1, -1, -1]], np.int32)
    iou = np.array([[0.5, 50.0 / 60.0, 1.0, 1.0, 1.0, -INF], [50.0 / 150.0, 0.0, -INF, -INF, -INF, -INF]], np.float64)
    return dataset, scores, labels, boxes, flag, row, iou


# ---- seeded draws --------------------------------------------------------------------------------------------------------------------

DRAW_CATS = [0, 1, 2, 3, 4, 6, 7]  # 5 is no category; n_cat = 8
DRAW_IMAGES = [11, 4, 23, 9, 15, 30]  # slots 2, 0, 4, 1, 3, 5
MAX_ROWS = 512  # GRIT_DET_MAX_SIDE
DRAW_SEEDS = {1: 3101, 63: 3102, 65: 3103, 100: 3104}  # per N; checked on the CPU (tests/test_vg_eval_cpu.py) before any device run


def _boxes_xywh(rng, n, extent=600.0):
    wh = np.exp(rng.uniform(np.log(8.0), np.log(250.0), (n, 2)))
    return np.concatenate([rng.uniform(0, extent - wh), wh], 1)


def draw_split(n_det, seed=None):
    """A split whose images have: 4 no ground truth; 9 one row; 11 rows of one class only (20 of class 2); 15 MAX_ROWS rows;
    23 thirty rows, ten of them of class 7, which none of its detections has; 30 thirty rows.  Detections: about half jittered
    copies of the image's rows (mostly with the row's label, drawn from a few rows so that several fall on one row), a tenth
    copies of the detection before, the rest boxes anywhere with labels from -1 .. 9 (5, 8, 9 and -1 take no part); scores
    descending with ties.  The batch has two more entries whose slots are -1 and past the split.
    -> (dataset, scores [8, N], labels, boxes, image ids in batch order with None for the two extra entries)."""
    rng = np.random.default_rng(DRAW_SEEDS[n_det] if seed is None else seed)
    anns = []
    counts = {4: 0, 9: 1, 11: 20, 15: MAX_ROWS, 23: 30, 30: 30}
    for image in DRAW_IMAGES:
        n = counts[image]
        cats = rng.choice([c for c in DRAW_CATS if c != 7], n)
        if image == 11:
            cats[:] = 2
        if image == 23:
            cats[:10] = 7
        anns += [(image, int(c), b) for c, b in zip(cats, _boxes_xywh(rng, n))]
    batch = [23, None, 11, 4, 30, 15, None, 9]
    scores, labels, boxes = [], [], []
    for image in batch:
        mine = [a for a in anns if a[0] == image and a[1] != 7]
        pool = mine if len(mine) <= 8 else [mine[int(j)] for j in rng.choice(len(mine), 8, replace=False)]
        lab, box = np.zeros(n_det, np.int64), np.zeros((n_det, 4))
        for n in range(n_det):
            r = rng.random()
            if pool and r < 0.5:
                _, c, (x, y, w, h) = pool[int(rng.integers(len(pool)))]
                j = rng.normal(0, 0.12, 4) * np.array([w, h, w, h])
                lab[n], box[n] = (c if rng.random() < 0.9 else int(rng.choice(DRAW_CATS[:-1]))), [x + j[0], y + j[1], x + w + j[2], y + h + j[3]]
            elif n and r < 0.6:
                lab[n], box[n] = lab[n - 1], box[n - 1]
            else:
                x, y, w, h = _boxes_xywh(rng, 1)[0]
                lab[n], box[n] = int(rng.integers(-1, 10)), [x, y, x + w, y + h]
            if lab[n] == 7:
                lab[n] = 6
        scores.append(np.sort(rng.integers(1, 4 * n_det + 2, n_det) / np.float32(4 * n_det + 2))[::-1])
        labels.append(lab)
        boxes.append(box)
    return (dataset_of(DRAW_IMAGES, DRAW_CATS, anns), np.stack(scores).astype(np.float32), np.stack(labels),
            np.stack(boxes).astype(np.float32), batch)


def draw_slots(batch, gt):
    """The batch's slots: the image's rank among the split's ids; -1 and n_img + 3 for the two extra entries."""
    extra = iter([-1, gt.n_img + 3])
    ids = [int(i) for i in gt.img_ids]
    return np.array([ids.index(i) if i is not None else next(extra) for i in batch], np.int32)
