"""Seeded inputs of fixture G21 (tests/golden/det_eval_g21*), shared by its generator and the tests: nothing drawn here is stored.

A case is {'dataset': a COCO dataset dictionary, 'seen': the image ids that get detections (in the order they are fed),
'dets': {image_id: (scores [N] fp32 descending, labels [N] int64, boxes [N, 4] fp32 absolute corners)}, 'n_det': N}.
Cases a-d feed the per-image evaluation directly; case e starts from logits (end_to_end).
"""
import numpy as np

CASES = ('a', 'b', 'c', 'd')
E2E_KS = (37, 1849)
E2E_B, E2E_Q = 3, 150
TOPK = 100


class Index(object):
    """getImgIds / getCatIds / getAnnIds / loadAnns over a dataset dictionary: all the reference's COCOeval asks of cocoGt and cocoDt."""

    def __init__(self, dataset):
        self.dataset = dataset
        self.anns = {a['id']: a for a in dataset['annotations']}

    def getImgIds(self):
        return [i['id'] for i in self.dataset['images']]

    def getCatIds(self):
        return [c['id'] for c in self.dataset['categories']]

    def getAnnIds(self, imgIds=(), catIds=()):
        imgs, cats = list(imgIds), set(catIds)
        by_img = {}
        for a in self.dataset['annotations']:
            by_img.setdefault(a['image_id'], []).append(a)
        anns = [a for i in imgs for a in by_img.get(i, [])] if imgs else list(self.dataset['annotations'])
        return [a['id'] for a in anns if not cats or a['category_id'] in cats]

    def loadAnns(self, ids=()):
        return [self.anns[i] for i in ids]


def _dataset(image_ids, cat_ids, anns):
    """anns: (image_id, category, [x, y, w, h], area, crowd) in annotation order; ids from 1."""
    return {'images': [{'id': i} for i in image_ids], 'categories': [{'id': c} for c in cat_ids],
            'annotations': [{'id': n + 1, 'image_id': i, 'category_id': c, 'bbox': [float(v) for v in b], 'area': float(s), 'iscrowd': int(w)}
                            for n, (i, c, b, s, w) in enumerate(anns)]}


def _side(rng, n):
    """Box sides, log-uniform in [6, 320): the areas straddle 32^2 and 96^2."""
    return np.exp(rng.uniform(np.log(6.0), np.log(320.0), n))


def _random_anns(rng, image_id, n, cats, crowd_p=0.15, width=640.0, height=480.0):
    out = []
    w, h = np.minimum(_side(rng, n), width - 1), np.minimum(_side(rng, n), height - 1)
    x, y = rng.uniform(0, width - w), rng.uniform(0, height - h)
    for j in range(n):
        area = w[j] * h[j] * rng.uniform(0.4, 1.0)  # a segmentation's area, not the box's
        out.append((image_id, int(rng.choice(cats)), [x[j], y[j], w[j], h[j]], area, rng.random() < crowd_p))
    return out


def _detections(rng, anns, n_det, labels_from, scores=None, width=640.0, height=480.0):
    """n_det detections of one image: about half of them jittered copies of its annotations (usually with the annotation's
    label), the rest anywhere.  Scores descending."""
    boxes, labels = np.zeros((n_det, 4)), np.zeros(n_det, np.int64)
    for n in range(n_det):
        if anns and rng.random() < 0.55:
            _, c, (x, y, w, h), _, _ = anns[int(rng.integers(len(anns)))]
            j = rng.normal(0, 0.08, 4) * np.array([w, h, w, h])
            boxes[n] = [x + j[0], y + j[1], x + w + j[2], y + h + j[3]]
            labels[n] = c if rng.random() < 0.85 else int(rng.choice(labels_from))
        else:
            w, h = min(_side(rng, 1)[0], width - 1), min(_side(rng, 1)[0], height - 1)
            x, y = rng.uniform(0, width - w), rng.uniform(0, height - h)
            boxes[n] = [x, y, x + w, y + h]
            labels[n] = int(rng.choice(labels_from))
    if scores is None:
        scores = rng.random(n_det)
    scores = np.sort(np.asarray(scores, np.float32))[::-1].copy()
    return scores, labels, boxes.astype(np.float32)


def case_a():
    """8 images (ids neither sorted nor contiguous), categories 0, 1, 2, 4, 5 (3 is no category: cat_valid 0), 40 detections each.
    Category 2 has detections and no ground truth anywhere; category 4 only crowd ground truths; image 17 has no ground truth;
    one annotation of the non-category 3 is left out by the packing; labels 3 and 6 (outside the table) take no part."""
    rng = np.random.default_rng(2101)
    image_ids, cats = [31, 5, 17, 8, 120, 64, 2, 77], [0, 1, 2, 4, 5]
    anns = []
    for i in image_ids:
        if i == 17:
            continue
        anns += _random_anns(rng, i, int(rng.integers(3, 13)), [0, 1, 5])
        if i in (5, 64, 2):
            anns += [(i, 4, b, s, True) for (_, _, b, s, _) in _random_anns(rng, i, 2, [4])]
    anns.append((8, 3, [10.0, 10.0, 50.0, 50.0], 2500.0, False))
    order = rng.permutation(len(anns))  # annotation order is not image order
    anns = [anns[j] for j in order]
    dets = {i: _detections(rng, [a for a in anns if a[0] == i and a[1] != 3], 40, [0, 1, 2, 3, 4, 5, 6]) for i in image_ids}
    return {'dataset': _dataset(image_ids, cats, anns), 'seen': list(image_ids), 'dets': dets, 'n_det': 40}


def case_b():
    """Equal scores inside an image and across images, 100 detections per image, 3 categories: far more than 10 of each."""
    rng = np.random.default_rng(2102)
    image_ids, cats = [1, 2, 3], [0, 1, 2]
    anns = [a for i in image_ids for a in _random_anns(rng, i, 25, cats)]
    dets = {i: _detections(rng, [a for a in anns if a[0] == i], 100, cats, scores=rng.integers(1, 9, 100) / 8.0) for i in image_ids}
    return {'dataset': _dataset(image_ids, cats, anns), 'seen': list(image_ids), 'dets': dets, 'n_det': 100}


def case_c(extra=0):
    """Image 1: 60 ground truths of one category.  Image 2: 512 ground truths (+ extra) over 4 categories."""
    rng = np.random.default_rng(2103)
    cats = [0, 1, 2, 3]
    anns = _random_anns(rng, 1, 60, [2]) + _random_anns(rng, 2, 512 + extra, cats)
    dets = {i: _detections(rng, [a for a in anns if a[0] == i], 100, cats) for i in (1, 2)}
    return {'dataset': _dataset([1, 2], cats, anns), 'seen': [1, 2], 'dets': dets, 'n_det': 100}


def case_d():
    """Boxes on small integers.  Image 1, by category:
      0  IoU exactly 1.0, 0.75 and 0.5 (a detection inside a 20 x 20 ground truth, of area 400, 300, 200)
      1  two ground truths of equal IoU 0.6 with the first detection -- the later one is taken, so the second detection, which only
         fits the later one, stays unmatched
      2  a regular ground truth (IoU 0.9) in front of a crowd one (IoU 1.0 over the detection's area): the walk stops at the
         regular one up to t = 0.9 and goes on to the crowd one at 0.95; the next detection can only take the crowd one again
      3  areas on the borders 32^2 and 96^2 themselves (neither < nor > holds), and a detection of area 32^2 without a partner
    Image 2 has ground truth and is never fed: its annotations must not count."""
    anns = [(1, 0, [10, 10, 20, 20], 400, False), (1, 0, [100, 100, 20, 20], 400, False), (1, 0, [200, 200, 20, 20], 400, False),
            (1, 1, [300, 300, 20, 20], 400, False), (1, 1, [310, 300, 20, 20], 400, False),
            (1, 2, [400, 100, 20, 20], 400, False), (1, 2, [400, 100, 18, 20], 360, True),
            (1, 3, [10, 300, 32, 32], 1024, False), (1, 3, [100, 300, 96, 96], 9216, False),
            (2, 0, [10, 10, 20, 20], 400, False), (2, 3, [50, 50, 40, 40], 1600, False)]
    boxes = np.array([[10, 10, 30, 30], [200, 200, 220, 215], [100, 100, 120, 110],
                      [305, 300, 325, 320], [312, 300, 332, 320],
                      [400, 100, 418, 120], [400, 104, 420, 116],
                      [10, 300, 42, 332], [100, 300, 196, 396], [500, 10, 532, 42]], np.float32)
    labels = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 3], np.int64)
    scores = np.linspace(0.95, 0.5, 10).astype(np.float32)
    return {'dataset': _dataset([1, 2], [0, 1, 2, 3], anns), 'seen': [1], 'dets': {1: (scores, labels, boxes)}, 'n_det': 10}


def case(name):
    return {'a': case_a, 'b': case_b, 'c': case_c, 'd': case_d}[name]()


def xywh(boxes):
    """convert_to_xywh(...).tolist() of the reference: the subtraction in fp32, then widened."""
    b = np.asarray(boxes, np.float32)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float64)


def sigmoid32(x):
    x = np.asarray(x, np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def select(logits, boxes, sizes):
    """PostProcess by its definition on logits [B, Q, K], boxes [B, Q, 4], sizes [B, 2] (fp32): per image the min(100, Q K) rows
    (logit descending, flat index ascending) -> top_logit, top_index, corners (fp32 arithmetic, one rounding per operation)."""
    B, Q, K = logits.shape
    N = min(TOPK, Q * K)
    flat = logits.reshape(B, Q * K)
    top_index = np.stack([np.lexsort((np.arange(Q * K), -flat[b].astype(np.float64)))[:N] for b in range(B)]).astype(np.int32)
    top_logit = np.take_along_axis(flat, top_index.astype(np.int64), 1)
    bx = np.take_along_axis(boxes, (top_index // K).astype(np.int64)[..., None], 1).astype(np.float32)
    half = np.float32(0.5)
    height, width = sizes[:, 0].astype(np.float32)[:, None], sizes[:, 1].astype(np.float32)[:, None]
    corners = np.stack([(bx[..., 0] - half * bx[..., 2]) * width, (bx[..., 1] - half * bx[..., 3]) * height,
                        (bx[..., 0] + half * bx[..., 2]) * width, (bx[..., 1] + half * bx[..., 3]) * height], -1).astype(np.float32)
    return top_logit, top_index, corners


def end_to_end(K, seed):
    """Case e: logits [3, 150, K] ~ N(-4, 1) (the best scores then lie around 0.5, where fp32 sigmoids are far apart), boxes and
    sizes; ground truth = jittered copies of some of each image's best detections, with their labels, plus annotations anywhere.
    -> (logits, boxes, sizes, dataset, image_ids in batch order)."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((E2E_B, E2E_Q, K)) - 4.0).astype(np.float32)
    wh = 0.05 + 0.4 * rng.random((E2E_B, E2E_Q, 2))
    boxes = np.concatenate([wh / 2 + (1 - wh) * rng.random((E2E_B, E2E_Q, 2)), wh], -1).astype(np.float32)
    sizes = np.array([[480, 640], [375, 500], [600, 400]], np.float32)
    image_ids = [9, 4, 6]
    _, top_index, corners = select(logits, boxes, sizes)
    anns = []
    for b, i in enumerate(image_ids):
        for n in rng.choice(TOPK, 12, replace=False):
            x0, y0, x1, y1 = corners[b, n].astype(np.float64)
            j = rng.normal(0, 0.05, 4) * np.array([x1 - x0, y1 - y0, x1 - x0, y1 - y0])
            w, h = x1 - x0 + j[2], y1 - y0 + j[3]
            anns.append((i, int(top_index[b, n] % K), [x0 + j[0], y0 + j[1], w, h], w * h * rng.uniform(0.5, 1.0), rng.random() < 0.1))
        anns += _random_anns(rng, i, 5, list(range(K)), width=float(sizes[b, 1]), height=float(sizes[b, 0]))
    return logits, boxes, sizes, _dataset(image_ids, list(range(K)), anns), image_ids


def fair(logits):
    """The condition of case e: each image's N + 1 largest sigmoid values are pairwise distinct as fp32 (the reference's topk order
    among equal scores is unspecified), and -- so that one ulp of another sigmoid implementation cannot reorder the accumulation's
    sort over all images -- all of them differ by more than 1e-6 relative."""
    B = logits.shape[0]
    flat = logits.reshape(B, -1)
    N = min(TOPK, flat.shape[1])
    best = np.sort(sigmoid32(np.sort(flat, 1)[:, ::-1][:, :N + 1]).astype(np.float64), 1)
    if any(len(np.unique(row.astype(np.float32))) != row.size for row in best):
        return False
    every = np.sort(best.reshape(-1))
    return bool((np.diff(every) > 1e-6 * every[1:]).all())
