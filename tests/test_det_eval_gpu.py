"""Detector evaluation on the device: grit_det_topk_f32 against its definition and, through PostProcess, against the plain-torch
composition it replaced; grit_det_eval_img against the numpy model (tests/det_eval_model.py) and the reference's evalImgs (fixture
G21); the evaluator, engine.det_engine.evaluate and train_detector.py --eval end to end.  Needs an MI355X.  Everything is exact."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, ROOT, deterministic_fill_, t

import det_draws
import det_eval_draws as D
from tests import det_eval_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _topk(logits, boxes=None, sizes=None):
    from grit_amd.ops.det_eval import det_topk
    B, Q, K = logits.shape
    rng = np.random.default_rng(B * 1000 + Q + K)
    boxes = det_draws.boxes(rng, B * Q).reshape(B, Q, 4) if boxes is None else boxes
    sizes = rng.integers(200, 700, (B, 2)).astype(np.float32) if sizes is None else sizes
    got = [x.cpu().numpy() for x in det_topk(t(logits, device=DEV), t(boxes, device=DEV), t(sizes, device=DEV))]
    return got, M.topk(logits, boxes, sizes)


def _same(got, want):
    for g, w, name in zip(got, want, ('logit', 'index', 'boxes')):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), name  # bit for bit


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Q,K", [(1, 1), (1, 37), (4, 25), (101, 1), (150, 1849)])
def test_topk_equals_its_definition(B, Q, K):
    logits = (2.0 * np.random.default_rng(Q * K + B).standard_normal((B, Q, K)) - 2.0).astype(np.float32)
    _same(*_topk(logits))


def _chunk_len(n):
    from grit_amd import lib
    chunks = min(lib.DET_TOPK_CHUNKS, -(-n // 8192))
    return -(-n // chunks), chunks


def test_topk_of_equal_logits_and_of_few_distinct_values():
    """All equal: the first 100 indices, i.e. the first chunk's.  Few distinct values: every chunk's threshold value has more
    equals than are wanted, so the in-order walk over the equal ones decides."""
    logits = np.full((2, 150, 1849), -1.5, np.float32)
    _same(*_topk(logits))
    rng = np.random.default_rng(5)
    logits = rng.integers(-3, 4, (2, 150, 1849)).astype(np.float32)
    logits[1] = rng.integers(0, 2, (150, 1849)) * 1e-3  # zeros and one positive value, and -0.0 below +0.0
    logits[1, 7, 11] = -0.0
    _same(*_topk(logits))


def test_topk_winners_on_the_chunk_borders():
    Q, K = 150, 1849
    n = Q * K
    length, chunks = _chunk_len(n)
    assert chunks > 2 and length * chunks >= n
    logits = (np.random.default_rng(9).standard_normal((2, n)) - 4.0).astype(np.float32)
    edges = np.array(sorted({min(c * length + d, n - 1) for c in range(chunks + 1) for d in (-2, -1, 0, 1) if c * length + d >= 0}))
    logits[0, edges] = 50.0 + np.arange(len(edges), dtype=np.float32) % 3  # winners (with ties) on both sides of every border
    logits[1, -120:] = 60.0  # all winners in the last, shorter chunk, all equal
    logits[1, :30] = 60.0
    got, want = _topk(logits.reshape(2, Q, K))
    _same(got, want)
    assert len(edges) > 100 and set(got[1][0].tolist()) <= set(edges.tolist())
    assert got[1][1].tolist() == list(range(30)) + list(range(n - 120, n - 50))


def test_topk_refuses_what_it_cannot_index():
    from grit_amd import lib
    L = lib.load()
    x = torch.zeros(8, device=DEV)
    p = lib.ptr
    assert L.grit_det_topk_f32(p(x), p(x), p(x), 1, 1 << 16, 1 << 15, p(x), p(x), p(x), p(x), lib.current_stream_ptr()) == lib.ERR_BAD_ARG
    with pytest.raises(lib.GritHipError):
        from grit_amd.ops.det_eval import det_topk
        det_topk(torch.zeros(1, 2, 3), torch.zeros(1, 2, 4), torch.zeros(1, 2))


def parent_post_process(outputs, target_sizes):
    """PostProcess.forward of the parent commit, verbatim."""
    from grit_amd.utils import box_ops
    logits, boxes = outputs['pred_logits'], outputs['pred_boxes']
    B, Q, K = logits.shape
    scores, flat = logits.sigmoid().reshape(B, Q * K).topk(min(100, Q * K), dim=1)
    query, labels = flat // K, flat % K
    corners = box_ops.box_cxcywh_to_xyxy(boxes).gather(1, query[..., None].expand(-1, -1, 4))
    height, width = target_sizes.unbind(1)
    corners = corners * torch.stack([width, height, width, height], 1)[:, None, :]
    return [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, corners)]


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLDEN, "det_eval_g21.json")))


@pytest.fixture(scope="module")
def case_e(meta):
    out = {}
    for K in D.E2E_KS:
        logits, boxes, sizes, dataset, image_ids = D.end_to_end(K, meta['e2e'][str(K)]['seed'])
        assert D.fair(logits)
        out[K] = (t(logits, device=DEV), t(boxes, device=DEV), t(sizes, device=DEV), dataset, image_ids)
    return out


@pytest.mark.parametrize("K", D.E2E_KS)
def test_post_process_equals_the_parent_composition(case_e, K):
    from models.detection.od_losses import PostProcess
    logits, boxes, sizes, _, _ = case_e[K]
    outputs = {'pred_logits': logits, 'pred_boxes': boxes}
    for size in (sizes, sizes.to(torch.int64)):  # orig_size is an integer tensor in the recipe
        got, want = PostProcess()(outputs, size), parent_post_process(outputs, size)
        assert len(got) == len(want) == D.E2E_B
        for g, w in zip(got, want):
            assert set(g) == set(w)
            for key in ('scores', 'labels', 'boxes'):
                assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape
                assert torch.equal(g[key], w[key]), key
            assert torch.equal(g['scores'].view(torch.int32), w['scores'].view(torch.int32))
    with pytest.raises(Exception, match="CPU"):
        PostProcess()({'pred_logits': logits.cpu(), 'pred_boxes': boxes.cpu()}, sizes.cpu())


@pytest.mark.parametrize("K", D.E2E_KS)
def test_case_e_through_post_process_and_evaluator(case_e, meta, K):
    from datasets.detection.metrics import AnnotationIndex, CocoEvaluator
    from models.detection.od_losses import PostProcess
    logits, boxes, sizes, dataset, image_ids = case_e[K]
    ev = CocoEvaluator(AnnotationIndex(dataset), ('bbox',))
    targets = [{'image_id': torch.tensor(i, device=DEV), 'orig_size': s} for i, s in zip(image_ids, sizes)]
    ev.update(PostProcess()({'pred_logits': logits, 'pred_boxes': boxes}, sizes), targets)
    ev.accumulate()
    ev.summarize()
    box = ev.coco_eval['bbox']
    assert np.array_equal(box.stats, np.asarray(meta['e2e'][str(K)]['stats']))
    assert box.result_text == meta['e2e'][str(K)]['text']


@pytest.fixture(scope="module")
def evaluated():
    """case -> (fixture, model records, evaluator fed in one batch); every case runs on the device once."""
    from datasets.detection.metrics import CocoEvaluator, Params
    from grit_amd.ops.det_eval import pack_ground_truth
    out = {}
    for name in D.CASES:
        case = D.case(name)
        with np.load(os.path.join(GOLDEN, "det_eval_g21_%s.npz" % name)) as z:
            fixture = {k: z[k] for k in z.files}
        gt, rec = M.run_case(case, pack_ground_truth, Params())
        ev = CocoEvaluator(gt, ('bbox',))
        _feed(ev, case, case['seen'])
        out[name] = (case, fixture, rec, ev)
    return out


def _feed(ev, case, ids):
    results = [{'scores': t(case['dets'][i][0], device=DEV), 'labels': t(case['dets'][i][1], device=DEV),
                'boxes': t(case['dets'][i][2], device=DEV)} for i in ids]
    ev.update(results, [{'image_id': torch.tensor(i, device=DEV)} for i in ids])


@pytest.mark.parametrize("name", D.CASES)
def test_records_equal_the_model_and_the_reference(evaluated, meta, name):
    case, fixture, rec, ev = evaluated[name]
    flags, rank, score, label, seen = ev.records.to_host()
    assert np.array_equal(rank, rec.rank) and np.array_equal(rank, fixture['rank'])
    assert np.array_equal(flags, rec.flags) and np.array_equal(flags, fixture['flags'])
    assert np.array_equal(seen, rec.seen) and np.array_equal(label, rec.label)
    assert np.array_equal(score.view(np.int32), rec.score.view(np.int32))
    ev.accumulate()
    ev.summarize()
    box = ev.coco_eval['bbox']
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(box.eval[key], fixture[key]), key
    assert np.array_equal(box.stats, fixture['stats']) and box.result_text == meta['text'][name]


def test_two_calls_give_identical_bytes_and_batching_does_not_matter(evaluated):
    from datasets.detection.metrics import CocoEvaluator
    for name in ('a', 'b'):
        case, _, _, ev = evaluated[name]
        first = ev.records.to_host()
        again = CocoEvaluator(ev.packed, ('bbox',))
        _feed(again, case, case['seen'])
        split = CocoEvaluator(ev.packed, ('bbox',))
        ids = case['seen']
        _feed(split, case, ids[-1:])  # two batches of different size, and not in order
        _feed(split, case, ids[:-1])
        for other in (again, split):
            for a, b in zip(first, other.records.to_host()):
                assert a.tobytes() == b.tobytes()
    logits = (np.random.default_rng(3).standard_normal((2, 150, 1849)) - 2.0).astype(np.float32)
    (a, _), (b, _) = _topk(logits), _topk(logits)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_more_annotations_than_the_bound_are_unsupported(evaluated):
    from grit_amd import lib
    from grit_amd.ops import det_eval as E
    ev = evaluated['c'][3]
    over = lib.DetGt.from_buffer_copy(ev.gt.struct)
    over.max_per_img = E.MAX_PER_IMAGE + 1
    r, p = ev.records, lib.ptr
    x = torch.zeros((1, 100, 4), device=DEV)
    args = lambda s: (p(x[0, :, 0]), p(torch.zeros((1, 100), dtype=torch.int64, device=DEV)), p(x), p(torch.zeros(1, dtype=torch.int32, device=DEV)),
                      1, 100, ctypes.c_void_p(ctypes.addressof(s)), p(ev.iou_thr), 10, p(ev.area_rng), 4, p(r.flags), p(r.rank), p(r.score),
                      p(r.label), p(r.seen), lib.current_stream_ptr())
    before = [a.copy() for a in r.to_host()]
    assert lib.load().grit_det_eval_img(*args(over)) == lib.ERR_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(before, r.to_host()))


def test_evaluate_on_the_tiny_detector():
    """engine.det_engine.evaluate on the 224 x 224 detector of G19's end-to-end case: the six keys, finite losses, twelve lines."""
    from datasets.detection.metrics import AnnotationIndex, CocoEvaluator
    from engine.det_engine import evaluate
    from grit_amd.config import detection_config
    from grit_amd.utils.misc import NestedTensor
    from models.detection.detector import build_detector
    e = json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))['e2e']
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
                              'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model'],
                              'model.det_module.dropout': 0.0})
    model, criterion, post = build_detector(cfg)
    deterministic_fill_(model)
    model.to(DEV)
    images, tg = det_draws.end_to_end_batch(e['seed'], num_classes=e['num_classes'], counts=tuple(e['counts']))
    targets, anns = [], []
    for n, (labels, boxes) in enumerate(tg):
        targets.append({'labels': t(labels, device=DEV), 'boxes': t(boxes, device=DEV), 'image_id': torch.tensor(40 - n, device=DEV),
                        'orig_size': torch.tensor([224, 224], device=DEV)})
        for label, (cx, cy, w, h) in zip(labels.tolist(), (boxes.astype(np.float64) * 224).tolist()):
            anns.append({'id': len(anns) + 1, 'image_id': 40 - n, 'category_id': label, 'bbox': [cx - w / 2, cy - h / 2, w, h],
                         'area': w * h, 'iscrowd': 0})
    dataset = {'images': [{'id': 40}, {'id': 39}], 'categories': [{'id': c} for c in range(e['num_classes'])], 'annotations': anns}
    samples = NestedTensor(t(images, device=DEV), torch.zeros(2, 224, 224, dtype=torch.bool, device=DEV))
    ev = CocoEvaluator(AnnotationIndex(dataset), ('bbox',))
    out = evaluate(model, criterion, post, [(samples, targets)], ev)
    keys = ['bbox_map', 'bbox_map50', 'bbox_map75', 'bbox_map_small', 'bbox_map_medium', 'bbox_map_large']
    assert all(k in out and -1.0 <= out[k] <= 1.0 for k in keys)
    losses = {k: v for k, v in out.items() if k not in keys and k != 'result_text'}
    assert 'losses' in losses and 'loss_ce' in losses and all(np.isfinite(v) for v in losses.values())
    assert len(out['result_text'].splitlines()) == 12 and not model.training
    assert ev.records.to_host()[4].tolist() == [1, 1] and (ev.records.to_host()[1] >= 0).all()


def test_train_detector_eval_in_a_child_process():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_detector.py"), "--synthetic", "--steps", "1", "--eval", "--batch-size", "2",
                        "--eval-batches", "1", "--max-targets", "5"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0, text[-3000:]
    assert "bbox_map" in text and text.count("Average Precision") == 6 and text.count("Average Recall") == 6
