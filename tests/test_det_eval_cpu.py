"""Detector evaluation, the parts that need no device: the numpy model of the kernels (tests/det_eval_model.py) against the
reference's evalImgs, and the host's accumulate / summarize against the reference's COCOeval.eval and stats (fixture G21,
tests/golden/make_det_eval_golden.py).  Every comparison is exact: the operations are the same IEEE float64 ones in the same order."""
import json
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN  # puts tests/golden on the path

import det_eval_draws as D
from tests import det_eval_model as M

from grit_amd.datasets.detection.metrics import AnnotationIndex, CocoEvaluator, Params, accumulate_records, summarize_eval
from grit_amd.ops.det_eval import MAX_PER_IMAGE, pack_ground_truth


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLDEN, "det_eval_g21.json")))


@pytest.fixture(scope="module")
def modelled():
    """case -> (fixture arrays, packed ground truth, the model's records); computed once."""
    out = {}
    for name in D.CASES:
        with np.load(os.path.join(GOLDEN, "det_eval_g21_%s.npz" % name)) as z:
            fixture = {k: z[k] for k in z.files}
        out[name] = (fixture,) + M.run_case(D.case(name), pack_ground_truth, Params())
    return out


@pytest.mark.parametrize("name", D.CASES)
def test_model_records_equal_the_reference(modelled, name):
    fixture, gt, rec = modelled[name]
    assert np.array_equal(rec.rank, fixture['rank'])
    assert np.array_equal(rec.flags, fixture['flags'])
    seen = np.nonzero(rec.seen)[0]
    assert np.array_equal(M.gt_ignore(gt, seen, Params().areaRng), fixture['gt_ignore'])


@pytest.mark.parametrize("name", D.CASES)
def test_accumulate_and_summarize_equal_the_reference(modelled, meta, name):
    fixture, gt, rec = modelled[name]
    params = Params()
    ev = accumulate_records(gt, rec.flags, rec.rank, rec.score, rec.label, rec.seen, params)
    for key in ('precision', 'recall', 'scores'):
        assert ev[key].shape == fixture[key].shape
        assert np.array_equal(ev[key], fixture[key]), key
    stats, text = summarize_eval(ev, params)
    assert np.array_equal(stats, fixture['stats'])
    assert text == meta['text'][name] and len(text.splitlines()) == 12


def test_cases_hold_what_they_are_for(modelled):
    fixture, gt, rec = modelled['a']
    cats = list(gt.cat_ids)
    assert (gt.crowd != 0).any() and (np.abs(gt.area - gt.box[:, 2] * gt.box[:, 3]) > 1).any()
    assert (gt.area < 32 ** 2).any() and ((gt.area > 32 ** 2) & (gt.area < 96 ** 2)).any() and (gt.area > 96 ** 2).any()
    assert (np.diff(gt.img_off) == 0).any()  # an image without ground truth
    assert (rec.label == 2).any() and not (gt.cat == 2).any() and (fixture['precision'][:, :, cats.index(2)] == -1).all()
    assert (gt.cat == 4).any() and gt.crowd[gt.cat == 4].all() and (fixture['precision'][:, :, cats.index(4)] == -1).all()
    assert gt.cat_valid[3] == 0 and (rec.label == 3).any() and (rec.rank[rec.label == 3] == -1).all()
    assert (rec.rank[rec.label == 6] == -1).all() and (rec.label == 6).any()
    fixture, gt, rec = modelled['b']
    assert len(np.unique(rec.score)) < 10 and rec.rank.max() > 10
    m = fixture['recall']  # the maxDets slices differ
    assert not np.array_equal(m[..., 0], m[..., 1]) and not np.array_equal(m[..., 1], m[..., 2])
    fixture, gt, rec = modelled['c']
    assert sorted(np.diff(gt.img_off)) == [60, MAX_PER_IMAGE] and len(set(gt.cat[:60])) == 1
    fixture, gt, rec = modelled['d']
    t = lambda n, a=0: [int(rec.flags[n, a] >> i & 1) for i in range(10)]
    assert t(0) == [1] * 10 and t(1) == [1] * 6 + [0] * 4 and t(2) == [1] + [0] * 9  # IoU 1.0, 0.75, 0.5: >= at the threshold itself
    # equal IoU 0.6: the later ground truth is taken, so up to t = 0.6 the next detection (IoU 0.25 / 0.82) finds only the earlier one
    assert t(3) == [1, 1, 1] + [0] * 7 and t(4) == [0] * 3 + [1] * 4 + [0] * 3
    assert t(5) == [1] * 10 and rec.flags[5, 0] >> 16 == 1 << 9  # the crowd one only once the regular one is out of reach
    assert rec.flags[6, 0] >> 16 == rec.flags[6, 0] & 0xffff == (1 << 9) - 1
    assert rec.seen.tolist() == [1, 0]


def test_packing_order_and_refusals():
    case = D.case('a')
    gt = pack_ground_truth(D.Index(case['dataset']))
    assert gt.img_ids.tolist() == sorted(case['seen']) and gt.cat_ids.tolist() == [0, 1, 2, 4, 5] and gt.n_cat == 6
    assert gt.cat_valid.tolist() == [1, 1, 1, 0, 1, 1]
    by_id = {a['id']: a for a in case['dataset']['annotations']}
    assert len(gt.ann_id) == len(by_id) - 1 and 3 not in gt.cat  # the annotation of the non-category is left out
    for slot, img in enumerate(gt.img_ids):
        ids = gt.ann_id[gt.img_off[slot]:gt.img_off[slot + 1]]
        assert all(by_id[i]['image_id'] == img for i in ids)
        keys = [(by_id[i]['category_id'], i) for i in ids]  # ids grow in annotation order
        assert keys == sorted(keys)
        assert (gt.ann_img[gt.img_off[slot]:gt.img_off[slot + 1]] == slot).all()
    a = by_id[int(gt.ann_id[0])]
    assert gt.box[0].tolist() == a['bbox'] and gt.area[0] == a['area'] and gt.crowd[0] == a['iscrowd']
    same = pack_ground_truth(AnnotationIndex(case['dataset']))
    assert all(np.array_equal(getattr(gt, k), getattr(same, k)) for k in ('img_off', 'box', 'area', 'cat', 'crowd', 'ann_id'))
    zero = dict(case['dataset'], annotations=[dict(a, id=0 if a['id'] == 7 else a['id']) for a in case['dataset']['annotations']])
    with pytest.raises(ValueError, match="annotation id 0"):
        pack_ground_truth(D.Index(zero))
    assert pack_ground_truth(D.Index(D.case_c()['dataset'])).max_per_img == MAX_PER_IMAGE
    with pytest.raises(ValueError, match="513 annotations"):
        pack_ground_truth(D.Index(D.case_c(extra=1)['dataset']))


def test_model_selection_order():
    logits = np.zeros((1, 3, 4), np.float32)
    logits[0, 2, 1] = logits[0, 0, 3] = 1.0
    top_logit, top_index, corners = M.topk(logits, np.full((1, 3, 4), 0.5, np.float32), np.array([[100, 200]], np.float32))
    assert top_index[0].tolist() == [3, 9, 0, 1, 2, 4, 5, 6, 7, 8, 10, 11] and top_logit[0, :3].tolist() == [1, 1, 0]
    assert corners[0, 0].tolist() == [50, 25, 150, 75]


def test_other_iou_types_are_refused():
    for kind in ('segm', 'keypoints'):
        with pytest.raises(NotImplementedError):
            CocoEvaluator(None, (kind,))


def test_header_declares_the_entry_points():
    from grit_amd import abi
    a = abi.read()
    assert len(a.functions['grit_det_topk_f32'][1]) == 11 and len(a.functions['grit_det_eval_img'][1]) == 17
    assert [f for f, _ in a.structs['grit_det_gt']] == ['img_off', 'box', 'area', 'cat', 'crowd', 'cat_valid', 'n_img', 'n_cat', 'max_per_img']
    assert a.constants['GRIT_DET_TOPK'] == 100 and a.constants['GRIT_DET_TOPK_CHUNKS'] * 100 <= 4096
