"""A numpy model of the detector-evaluation kernels (grit_det_topk_f32, grit_det_eval_img; include/grit_hip.h), records and bit
layout included -- what tests/det_transforms_model.py is to the image pipeline.  It states what the kernels compute in the
plainest loops; it is checked against the reference's evalImgs (fixture G21) on the CPU and the kernels are checked against it
and the fixture on the GPU."""
import numpy as np

import det_eval_draws as D  # tests/golden, put on the path by tests.helpers


def topk(logits, boxes, sizes):
    """grit_det_topk_f32: the definition is the one of the draws (det_eval_draws.select)."""
    return D.select(np.asarray(logits, np.float32), np.asarray(boxes, np.float32), np.asarray(sizes, np.float32))


def iou(d, g, crowd):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    w = 0.0 if w <= 0 else w
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    h = 0.0 if h <= 0 else h
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


class Records(object):
    def __init__(self, n_img, n_det, n_rng):
        self.flags = np.zeros((n_img * n_det, n_rng), np.uint32)
        self.rank = np.full(n_img * n_det, -1, np.int32)
        self.score = np.zeros(n_img * n_det, np.float32)
        self.label = np.full(n_img * n_det, -1, np.int32)
        self.seen = np.zeros(n_img, np.uint8)


def eval_images(gt, scores, labels, boxes, slots, iou_thr, area_rng, rec):
    """grit_det_eval_img on numpy arrays: gt a PackedGroundTruth, scores / labels [B, N], boxes [B, N, 4] corners, slots [B]."""
    B, N = scores.shape
    for b in range(B):
        img = int(slots[b])
        if img < 0 or img >= gt.n_img:
            continue
        first, end = int(gt.img_off[img]), int(gt.img_off[img + 1])
        det = [[float(v) for v in row] for row in D.xywh(boxes[b])]
        valid = [0 <= int(l) < gt.n_cat and bool(gt.cat_valid[int(l)]) for l in labels[b]]
        for n in range(N):
            row = img * N + n
            rec.score[row], rec.label[row] = scores[b, n], labels[b, n]
            rec.rank[row] = sum(1 for m in range(n) if labels[b, m] == labels[b, n]) if valid[n] else -1
            rec.flags[row] = 0
        rec.seen[img] = 1
        for label in sorted(set(int(l) for l, v in zip(labels[b], valid) if v)):
            members = [n for n in range(N) if labels[b, n] == label]
            gts = [g for g in range(first, end) if gt.cat[g] == label]
            for a, (lo, hi) in enumerate(area_rng):
                ignored = {g: bool(gt.crowd[g]) or gt.area[g] < lo or gt.area[g] > hi for g in gts}
                walk = [g for g in gts if not ignored[g]] + [g for g in gts if ignored[g]]  # ignored last, stably
                for t, thr in enumerate(iou_thr):
                    taken = set()
                    for n in members:
                        best, match = min(thr, 1 - 1e-10), None
                        for g in walk:
                            if g in taken and not gt.crowd[g]:
                                continue
                            if match is not None and not ignored[match] and ignored[g]:
                                break
                            value = iou(det[n], gt.box[g], bool(gt.crowd[g]))
                            if value < best:
                                continue
                            best, match = value, g
                        row = img * N + n
                        if match is not None:
                            taken.add(match)
                            rec.flags[row, a] |= np.uint32(1 << t)
                            if ignored[match]:
                                rec.flags[row, a] |= np.uint32(1 << (16 + t))
                        else:
                            area = det[n][2] * det[n][3]
                            if area < lo or area > hi:
                                rec.flags[row, a] |= np.uint32(1 << (16 + t))


def gt_ignore(gt, seen_slots, area_rng):
    """gtIgnore of every (category, area range, image) entry the reference keeps, in its order, concatenated.  An entry exists when
    the image has ground truth of the category; an entry that exists only through detections has no ground truth to list."""
    out = []
    for cat in gt.cat_ids:
        for lo, hi in area_rng:
            for img in sorted(seen_slots):
                g = np.arange(gt.img_off[img], gt.img_off[img + 1])
                g = g[gt.cat[g] == cat]
                ig = (gt.crowd[g] != 0) | (gt.area[g] < lo) | (gt.area[g] > hi)
                out.append(np.sort(ig.astype(np.uint8), kind='stable'))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def run_case(case, pack, params):
    """A case of det_eval_draws through the model -> (PackedGroundTruth, Records)."""
    gt = pack(D.Index(case['dataset']))
    slot_of = {int(i): n for n, i in enumerate(gt.img_ids)}
    rec = Records(gt.n_img, case['n_det'], len(params.areaRng))
    ids = case['seen']
    scores = np.stack([case['dets'][i][0] for i in ids])
    labels = np.stack([case['dets'][i][1] for i in ids])
    boxes = np.stack([case['dets'][i][2] for i in ids])
    eval_images(gt, scores, labels, boxes, [slot_of[i] for i in ids], params.iouThrs, params.areaRng, rec)
    return gt, rec
