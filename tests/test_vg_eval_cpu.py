"""The Visual Genome protocol's evaluation, the parts that need no device: voc_ap on hand-worked curves, accumulate_voc against a
brute-force loop, the attribute packer, and the sequential model of the matching kernel (tests/vg_eval_model.py) on hand-built
images.  The reference's Python 2 files cannot be run, so nothing here is a recorded output: every expected number is worked out
by hand or by a second, plainer formulation."""
import numpy as np
import pytest

from tests import vg_eval_model as M

from grit_amd.datasets.detection.metrics import AnnotationIndex
from grit_amd.datasets.detection.metrics.vg_eval import accumulate_voc, summary_text, voc_ap
from grit_amd.ops.det_eval import MAX_PER_IMAGE, PackedGroundTruth, pack_ground_truth, pack_ground_truth_attr


def test_voc_ap_on_hand_worked_curves():
    assert voc_ap(np.array([0.25, 0.5, 0.75, 1.0]), np.ones(4)) == 1.0  # all true positives
    # TP, FP, TP with npos 2: recall 0.5, 0.5, 1; precision 1, 1/2, 2/3 -> from the right 1, 2/3, 2/3: 0.5 * 1 + 0.5 * 2/3
    got = voc_ap(np.array([0.5, 0.5, 1.0]), np.array([1.0, 0.5, 2.0 / 3.0]))
    assert got == 0.5 * 1.0 + 0.5 * (2.0 / 3.0)
    assert voc_ap(np.zeros(0), np.zeros(0)) == 0.0  # no detections
    # FP, TP with npos 4: recall 0, 0.25; precision 0, 0.5 -> 0.25 * 0.5; the rest of the recall axis has precision 0
    assert voc_ap(np.array([0.0, 0.25]), np.array([0.0, 0.5])) == 0.125


def _gt(n_img, cats, cat_ids):
    """A PackedGroundTruth with the rows `cats` = [(slot, class)]: the accumulation reads cat, n_img, n_cat only."""
    cats = sorted(cats)
    off = np.searchsorted([s for s, _ in cats], np.arange(n_img + 1)).astype(np.int32)
    G = len(cats)
    return PackedGroundTruth(np.arange(n_img) * 3 + 1, cat_ids, off, np.zeros((G, 4)), np.zeros(G), np.array([c for _, c in cats], np.int32),
                             np.zeros(G, np.uint8), np.array([s for s, _ in cats], np.int32), np.arange(1, G + 1))


def _brute_force(gt, rec, class_ids):
    """Per class, one detection at a time: the order (score descending, slot, rank) by a Python sort on tuples."""
    n_det = len(rec.flag) // gt.n_img
    aps, nposs, thr = [], [], []
    for c in class_ids:
        npos = int(sum(1 for x in gt.cat if x == c))
        dets = []
        for slot in range(gt.n_img):
            if not rec.seen[slot]:
                continue
            for n in range(n_det):
                row = slot * n_det + n
                if rec.flag[row] != 0 and rec.label[row] == c:
                    dets.append((-float(rec.score[row]), slot, n, int(rec.flag[row])))
        dets.sort()
        tp = fp = 0
        recs, precs, best_f, best_score = [], [], -1.0, 0.0
        for neg, _, _, flag in dets:
            tp, fp = tp + (flag == 1), fp + (flag != 1)
            r = tp / npos if npos else 0.0
            p = tp / max(tp + fp, np.finfo(np.float64).eps)
            recs.append(r)
            precs.append(p)
            f = (p * r) / (p + r) if p + r > 0 else 0.0
            if f > best_f:
                best_f, best_score = f, -neg
        aps.append(voc_ap(np.array(recs), np.array(precs)) if npos and dets else 0.0)
        nposs.append(float(npos))
        thr.append(best_score if npos > 1 and dets else 0.0)
    thr = np.array(thr)
    mean_thr = thr[thr != 0].mean() if (thr != 0).any() else 0.0
    thr[thr == 0] = mean_thr
    nposs = np.array(nposs)
    return np.array(aps), nposs, thr, float(np.mean(aps)), float(np.average(aps, weights=nposs / nposs.sum())), float(mean_thr)


def _records(n_img, n_det, rows, seen):
    """rows: {(slot, rank): (flag, label, score)}."""
    rec = M.empty_records(n_img, n_det)
    for (slot, n), (flag, label, score) in rows.items():
        rec.flag[slot * n_det + n], rec.label[slot * n_det + n], rec.score[slot * n_det + n] = flag, label, score
    rec.seen[list(seen)] = 1
    return rec


def test_accumulate_voc_equals_the_brute_force_loop():
    """Classes 0 .. 4 and 6.  0: tied scores within and across images, true and false positives mixed.  1: npos 0 with detections.
    2: ground truth and no detection.  3: npos 1 (no threshold of its own).  4: detections only in an image that was not seen.
    6: all false positives.  Image slot 2 is not seen: its records do not count, its ground truth does."""
    gt = _gt(4, [(0, 0), (0, 0), (1, 0), (3, 0), (2, 0), (0, 2), (1, 2), (1, 3), (2, 4), (3, 4), (0, 6), (3, 6)], [0, 1, 2, 3, 4, 6])
    rows = {(0, 0): (1, 0, 0.75), (0, 1): (2, 0, 0.75), (0, 2): (1, 0, 0.5), (0, 3): (3, 0, 0.5), (0, 4): (2, 1, 0.5),
            (1, 0): (2, 0, 0.75), (1, 1): (1, 0, 0.75), (1, 2): (1, 3, 0.625), (1, 3): (2, 3, 0.25), (1, 4): (0, 0, 0.9),
            (2, 0): (1, 4, 0.9), (2, 1): (1, 0, 0.99),
            (3, 0): (1, 0, 0.875), (3, 1): (2, 6, 0.5), (3, 2): (3, 6, 0.5), (3, 3): (2, 1, 0.25), (3, 4): (2, 0, 0.5)}
    rec = _records(4, 5, rows, seen=[0, 1, 3])
    class_ids = [0, 1, 2, 3, 4, 6]
    got = accumulate_voc(gt, rec, class_ids)
    ap, npos, thr, mean_ap, wmap, mean_thr = _brute_force(gt, rec, class_ids)
    assert np.array_equal(got['ap'], ap) and np.array_equal(got['npos'], npos) and np.array_equal(got['threshold'], thr)
    assert got['map'] == mean_ap and got['wmap'] == wmap and got['mean_threshold'] == mean_thr
    assert npos.tolist() == [5, 0, 2, 1, 2, 2]
    # class 0 by hand: order 0.875 TP (slot 3); 0.75: slot 0 TP, slot 0 FP, slot 1 FP, slot 1 TP; 0.5: slot 0 TP, slot 0 dup, slot 3 FP
    #   tp 1 2 2 2 3 4 4 4, precision 1 1 2/3 1/2 3/5 2/3 4/7 1/2 -> from the right 1 1 2/3 2/3 2/3 2/3 4/7 1/2; recall steps at
    #   detections 1, 2, 5, 6 of 0.2 each: 0.2 * (1 + 1 + 2/3 + 2/3)
    assert got['ap'][0] == pytest.approx(0.2 * (1 + 1 + 2 / 3 + 2 / 3), abs=1e-15)
    assert got['ap'][1:].tolist() == [0, 0, 1.0, 0, 0]  # npos 0; no detection; one TP first; unseen image only; false positives only
    # thresholds: class 0 has its best F at the sixth detection (score 0.5: p 2/3, r 0.8); the others get the mean of the non-zero ones
    assert got['threshold'][0] == 0.5 and got['mean_threshold'] == 0.5 and got['threshold'].tolist() == [0.5] * 6
    assert got['map'] == pytest.approx((got['ap'][0] + 1.0) / 6) and got['wmap'] == pytest.approx((5 * got['ap'][0] + 1.0) / 12)


def test_accumulate_voc_threshold_rules_and_no_positives():
    """Two classes with thresholds of their own and one without: the zero is replaced by the mean of the two.  Without any
    ground truth wmap is 0 and no threshold is NaN."""
    gt = _gt(2, [(0, 0), (1, 0), (0, 1), (1, 1), (1, 1), (0, 2)], [0, 1, 2])
    rows = {(0, 0): (1, 0, 0.875), (0, 1): (1, 1, 0.75), (0, 2): (2, 2, 0.5),
            (1, 0): (2, 1, 0.625), (1, 1): (1, 0, 0.25), (1, 2): (1, 1, 0.125)}
    got = accumulate_voc(gt, _records(2, 3, rows, seen=[0, 1]), [0, 1, 2])
    # class 0: TP 0.875 (p 1, r 1/2: F' 1/3), TP 0.25 (p 1, r 1: F' 1/2) -> 0.25.  class 1: TP 0.75 (1, 1/3: 1/4), FP, TP 0.125
    # (2/3, 2/3: 1/3) -> 0.125.  class 2: npos 1 -> 0 -> the mean 0.1875
    assert got['threshold'].tolist() == [0.25, 0.125, 0.1875] and got['mean_threshold'] == 0.1875
    ap, npos, thr, mean_ap, wmap, mean_thr = _brute_force(gt, _records(2, 3, rows, seen=[0, 1]), [0, 1, 2])
    assert np.array_equal(got['ap'], ap) and np.array_equal(got['threshold'], thr) and got['wmap'] == wmap
    empty = accumulate_voc(_gt(2, [], [0, 1]), _records(2, 3, {(0, 0): (2, 0, 0.5)}, seen=[0]), [0, 1])
    assert empty['ap'].tolist() == [0, 0] and empty['map'] == 0 and empty['wmap'] == 0 and empty['threshold'].tolist() == [0, 0]
    assert 'Mean AP = 0.0000' in summary_text('obj', empty) and summary_text('attr', empty).startswith('attributes: ')
    with pytest.raises(ValueError):
        accumulate_voc(gt, _records(2, 3, rows, seen=[0, 1]), [])


def _attr_dataset():
    images = [{'id': 8, 'has_attr': True}, {'id': 2, 'has_attr': False}, {'id': 5}]
    anns = [{'id': 1, 'image_id': 8, 'category_id': 3, 'bbox': [1, 2, 3, 4], 'area': 12., 'iscrowd': 0, 'attributes': [4, 1]},
            {'id': 2, 'image_id': 8, 'category_id': 0, 'bbox': [5, 6, 7, 8], 'area': 56., 'iscrowd': 0, 'attributes': [1, 1, 0]},
            {'id': 3, 'image_id': 8, 'category_id': 0, 'bbox': [9, 9, 9, 9], 'area': 81., 'iscrowd': 0},
            {'id': 4, 'image_id': 2, 'category_id': 1, 'bbox': [1, 1, 1, 1], 'area': 1., 'iscrowd': 0, 'attributes': [2]},
            {'id': 5, 'image_id': 5, 'category_id': 1, 'bbox': [2, 2, 2, 2.5], 'area': 5., 'iscrowd': 0, 'attributes': [5]}]
    return {'images': images, 'categories': [{'id': c} for c in range(4)], 'annotations': anns}


def test_attribute_packer_expands_orders_and_leaves_images_out():
    dataset = _attr_dataset()
    for index in (AnnotationIndex(dataset), M.Index(dataset)):
        gt = pack_ground_truth_attr(index, 6)
        assert gt.img_ids.tolist() == [5, 8]  # ascending; image 2 (has_attr False) is not part of the split; no key: True
        assert gt.cat_ids.tolist() == list(range(6)) and gt.n_cat == 6 and gt.cat_valid.tolist() == [1] * 6
        assert gt.img_off.tolist() == [0, 1, 5] and gt.max_per_img == 4
        # image 8: attribute 0 (object 2), attribute 1 (objects 1 and 2, in annotation order; listed twice counts once), attribute 4
        assert gt.cat.tolist() == [5, 0, 1, 1, 4] and gt.ann_id.tolist() == [5, 2, 1, 2, 1] and gt.ann_img.tolist() == [0, 1, 1, 1, 1]
        assert gt.box.tolist() == [[2, 2, 2, 2.5], [5, 6, 7, 8], [1, 2, 3, 4], [5, 6, 7, 8], [1, 2, 3, 4]]
        assert gt.area.tolist() == [5, 56, 12, 56, 12] and not gt.crowd.any() and gt.box.dtype == np.float64
    objects = pack_ground_truth(AnnotationIndex(dataset))  # the object split is what it was: the new keys pass through unread
    assert objects.img_ids.tolist() == [2, 5, 8] and objects.cat.tolist() == [1, 1, 0, 0, 3]
    with pytest.raises(ValueError, match="outside"):
        pack_ground_truth_attr(AnnotationIndex(dataset), 5)
    with pytest.raises(ValueError, match="no image"):
        pack_ground_truth_attr(AnnotationIndex({'images': [{'id': 1, 'has_attr': False}], 'categories': [], 'annotations': []}), 5)


def test_attribute_packer_row_bound():
    """The bound is on the expanded rows of an image, not on its objects."""
    def dataset(objects, per_object):
        anns = [{'id': n + 1, 'image_id': 1, 'category_id': 0, 'bbox': [0, 0, 5, 5], 'area': 25., 'iscrowd': 0,
                 'attributes': list(range(per_object))} for n in range(objects)]
        return AnnotationIndex({'images': [{'id': 1}], 'categories': [{'id': 0}], 'annotations': anns})
    assert MAX_PER_IMAGE == 512
    gt = pack_ground_truth_attr(dataset(128, 4), 4)
    assert gt.max_per_img == 512 and gt.cat.tolist() == [a for a in range(4) for _ in range(128)]
    with pytest.raises(ValueError, match="512"):
        pack_ground_truth_attr(dataset(103, 5), 5)  # 515 rows of 103 objects


def test_model_on_the_hand_built_images():
    dataset, scores, labels, boxes, flag, row, iou = M.hand_built()
    gt = pack_ground_truth(M.Index(dataset))
    assert gt.img_ids.tolist() == [3, 7] and gt.cat_valid.tolist() == [1, 1, 1, 0, 1]
    assert gt.cat.tolist() == [0, 0, 4, 0, 1, 1]  # the annotation of the non-category 3 is left out
    rec = M.match_images(scores, labels, boxes, np.array([1, 0], np.int32), gt)
    N = M.HAND_N
    for b, slot in enumerate([1, 0]):
        rows = slice(slot * N, slot * N + N)
        assert rec.flag[rows].tolist() == flag[b].tolist(), b
        assert rec.gt[rows].tolist() == row[b].tolist(), b
        assert np.array_equal(rec.iou[rows].view(np.int64), iou[b].view(np.int64)), b
        assert np.array_equal(rec.score[rows], scores[b]) and rec.label[rows].tolist() == labels[b].tolist()
    assert rec.seen.tolist() == [1, 1]
    assert rec.iou[N + 0] == 0.5 and rec.flag[N + 0] == 2  # overlap exactly at the threshold is no match
    assert rec.gt[N + 3] == 1 and rec.flag[N + 4] == 3 and rec.gt[N + 4] == 1  # first argmax; the duplicate does not move on to row 2
    assert rec.flag[N + 5] == 0 and labels[0, 5] == 3  # cat_valid 0
    # a lower threshold turns the 0.5 into the true positive and the two after it into duplicates
    low = M.match_images(scores, labels, boxes, np.array([1, 0], np.int32), gt, thr=0.4)
    assert low.flag[N:N + 3].tolist() == [1, 3, 3]


def test_model_leaves_images_outside_the_split_alone():
    dataset, scores, labels, boxes, *_ = M.hand_built()
    gt = pack_ground_truth(M.Index(dataset))
    rec = M.match_images(scores, labels, boxes, np.array([-1, 2], np.int32), gt)
    fresh = M.empty_records(2, M.HAND_N)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rec, fresh))


@pytest.mark.parametrize("n_det", sorted(M.DRAW_SEEDS))
def test_seeded_draws_hold_what_they_are_for(n_det):
    """The seeds of the device test, checked where no device is needed: every ground-truth shape is there, and at N = 100 the
    model's records hold at least 5 of every flag (so at least 5 duplicates)."""
    dataset, scores, labels, boxes, batch = M.draw_split(n_det)
    gt = pack_ground_truth(M.Index(dataset))
    per_image = dict(zip(gt.img_ids.tolist(), np.diff(gt.img_off).tolist()))
    assert per_image == {4: 0, 9: 1, 11: 20, 15: M.MAX_ROWS, 23: 30, 30: 30} and gt.max_per_img == MAX_PER_IMAGE
    slots = M.draw_slots(batch, gt)
    assert sorted(slots.tolist()) == [-1, 0, 1, 2, 3, 4, 5, gt.n_img + 3] and scores.shape == (8, n_det)
    assert (np.diff(scores, axis=1) <= 0).all()
    first = gt.img_off[list(gt.img_ids).index(11)]
    assert set(gt.cat[first:first + 20].tolist()) == {2}
    at = batch.index(23)
    assert 7 in gt.cat.tolist() and 7 not in labels[at].tolist()
    rec = M.match_images(scores, labels, boxes, slots, gt)
    counts = np.bincount(rec.flag, minlength=4)
    assert rec.seen.tolist() == [1] * 6
    if n_det == 100:
        assert (counts >= 5).all(), counts
    elif n_det > 1:
        assert (counts >= 1).all(), counts
