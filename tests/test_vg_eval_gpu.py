"""The Visual Genome protocol on the device: grit_det_voc_img against the sequential model (tests/vg_eval_model.py), equal in every
record byte; PostProcessAttr against the torch composition; post-processes and VGEvaluator end to end against the model's records
through the same accumulation.  Needs an MI355X.  Everything is exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import t

import det_eval_draws as D
from tests import vg_eval_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_VALUES = (1, 63, 65, 100)


def _launch(gt, scores, labels, boxes, slots, records=None, thr=0.5):
    from grit_amd.ops import det_eval as E
    dgt = E.DeviceGroundTruth(gt, DEV)
    records = E.VocRecords(gt.n_img, scores.shape[1], DEV) if records is None else records
    E.voc_images(t(scores, device=DEV), t(labels, device=DEV), t(boxes, device=DEV), t(slots, device=DEV), dgt, thr, records)
    return records


def _same_bytes(got, want):
    for name, g, w in zip(M.Records._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), name  # rec_iou as bit patterns, -inf and all


@pytest.fixture(scope="module")
def drawn():
    """N -> (packed ground truth, inputs, slots, the model's records, the kernel's records): one launch per N."""
    from grit_amd.ops.det_eval import pack_ground_truth
    out = {}
    for n_det in N_VALUES:
        dataset, scores, labels, boxes, batch = M.draw_split(n_det)
        gt = pack_ground_truth(M.Index(dataset))
        slots = M.draw_slots(batch, gt)
        want = M.match_images(scores, labels, boxes, slots, gt)
        out[n_det] = (gt, (scores, labels, boxes), slots, want, _launch(gt, scores, labels, boxes, slots))
    return out


@pytest.mark.parametrize("n_det", N_VALUES)
def test_kernel_records_equal_the_model(drawn, n_det):
    """Images without ground truth, with one row, with rows of one class, with GRIT_DET_MAX_SIDE rows and with rows whose class has
    no detection; batch entries with slot -1 and a slot past the split."""
    from grit_amd.ops.det_eval import MAX_PER_IMAGE
    gt, _, slots, want, records = drawn[n_det]
    assert gt.max_per_img == MAX_PER_IMAGE == M.MAX_ROWS and 0 in np.diff(gt.img_off) and 1 in np.diff(gt.img_off)
    assert slots.min() == -1 and slots.max() >= gt.n_img
    counts = np.bincount(want.flag, minlength=4)
    if n_det == 100:
        assert (counts >= 5).all(), counts  # every flag value, so at least 5 duplicates
    elif n_det > 1:
        assert (counts >= 1).all(), counts
    got = records.to_host()
    _same_bytes(got, want)
    assert got.seen.tolist() == [1] * gt.n_img and got.iou.dtype == np.float64 and got.flag.dtype == np.uint8


def test_hand_built_images_through_the_kernel():
    from grit_amd.ops.det_eval import pack_ground_truth
    dataset, scores, labels, boxes, flag, row, iou = M.hand_built()
    gt = pack_ground_truth(M.Index(dataset))
    slots = np.array([1, 0], np.int32)
    got = _launch(gt, scores, labels, boxes, slots).to_host()
    _same_bytes(got, M.match_images(scores, labels, boxes, slots, gt))
    N = M.HAND_N
    for b, slot in enumerate([1, 0]):  # and the numbers worked out by hand
        rows = slice(slot * N, slot * N + N)
        assert got.flag[rows].tolist() == flag[b].tolist() and got.gt[rows].tolist() == row[b].tolist()
        assert np.array_equal(got.iou[rows].view(np.int64), iou[b].view(np.int64))
    low = _launch(gt, scores, labels, boxes, slots, thr=0.4).to_host()
    _same_bytes(low, M.match_images(scores, labels, boxes, slots, gt, thr=0.4))
    assert low.flag[N:N + 3].tolist() == [1, 3, 3]


def test_two_calls_give_identical_bytes_and_batching_does_not_matter(drawn):
    gt, (scores, labels, boxes), slots, want, records = drawn[100]
    first = records.to_host()
    again = _launch(gt, scores, labels, boxes, slots).to_host()
    split = _launch(gt, scores[5:], labels[5:], boxes[5:], slots[5:])
    split = _launch(gt, scores[:5], labels[:5], boxes[:5], slots[:5], records=split).to_host()
    for other in (again, split):
        for a, b in zip(first, other):
            assert a.tobytes() == b.tobytes()
    over = _launch(gt, scores, labels, boxes, slots, records=records).to_host()  # a second launch over filled records
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, over))


def test_attribute_rows_go_through_the_same_kernel():
    """The attribute split of a dataset whose image 2 has no attributes: its slot is -1 and its detections leave no record."""
    from grit_amd.ops import det_eval as E
    rng = np.random.default_rng(3201)
    A, n_det = 9, 65
    images = [{'id': 1, 'has_attr': True}, {'id': 2, 'has_attr': False}, {'id': 3, 'has_attr': True}]
    anns, boxes = [], M._boxes_xywh(rng, 24)
    for n, b in enumerate(boxes):
        anns.append({'id': n + 1, 'image_id': 1 + n % 3, 'category_id': 0, 'bbox': [float(v) for v in b], 'area': 1.0, 'iscrowd': 0,
                     'attributes': [int(a) for a in np.nonzero(rng.random(A) < 0.35)[0]]})
    gt = E.pack_ground_truth_attr(M.Index({'images': images, 'categories': [{'id': 0}], 'annotations': anns}), A)
    assert gt.img_ids.tolist() == [1, 3] and gt.img_off[-1] > 24
    ids = torch.tensor([3, 2, 1], device=DEV)
    dgt = E.DeviceGroundTruth(gt, DEV)
    slots = dgt.slots_of(ids).cpu().numpy()
    assert slots.tolist() == [1, -1, 0]
    assert all(dgt.slots_for(form).tolist() == [1, -1, 0] for form in (ids, list(ids), [3, 2, 1])) and dgt.slots_for([7, 0]).tolist() == [-1, -1]
    labels = rng.integers(0, A, (3, n_det))
    det = np.zeros((3, n_det, 4))
    for b, image in enumerate([3, 2, 1]):
        mine = [a for a in anns if a['image_id'] == image]
        for n in range(n_det):
            a = mine[int(rng.integers(len(mine)))]
            x, y, w, h = a['bbox']
            j = rng.normal(0, 0.1, 4) * np.array([w, h, w, h])
            det[b, n] = [x + j[0], y + j[1], x + w + j[2], y + h + j[3]]
            if a['attributes'] and rng.random() < 0.7:
                labels[b, n] = a['attributes'][int(rng.integers(len(a['attributes'])))]
    scores = np.sort(rng.random((3, n_det)).astype(np.float32), 1)[:, ::-1].copy()
    want = M.match_images(scores, labels, det.astype(np.float32), slots, gt)
    assert (np.bincount(want.flag, minlength=4)[1:] >= 3).all() and want.seen.tolist() == [1, 1]
    _same_bytes(_launch(gt, scores, labels, det.astype(np.float32), slots).to_host(), want)


def test_bounds_and_argument_checks(drawn):
    from grit_amd import lib
    from grit_amd.ops import det_eval as E
    gt, (scores, labels, boxes), slots, want, records = drawn[63]
    dgt = E.DeviceGroundTruth(gt, DEV)
    over = lib.DetGt.from_buffer_copy(dgt.struct)
    over.max_per_img = E.MAX_PER_IMAGE + 1
    p, r = lib.ptr, records
    dev = [t(x, device=DEV) for x in (scores, labels, boxes, slots)]
    args = lambda s, n, thr: (p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), 8, n, ctypes.c_void_p(ctypes.addressof(s)), thr, p(r.flag),
                              p(r.gt), p(r.iou), p(r.score), p(r.label), p(r.seen), lib.current_stream_ptr())
    before = records.to_host()
    L = lib.load()
    assert L.grit_det_voc_img(*args(over, 63, 0.5)) == lib.ERR_UNSUPPORTED
    assert L.grit_det_voc_img(*args(dgt.struct, E.TOPK + 1, 0.5)) == lib.ERR_BAD_ARG
    assert L.grit_det_voc_img(*args(dgt.struct, 63, float('nan'))) == lib.ERR_BAD_ARG
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, records.to_host()))
    with pytest.raises(lib.GritHipError, match="CPU"):
        E.voc_images(t(scores), t(labels), t(boxes), t(slots), dgt, 0.5, records)
    with pytest.raises(lib.GritHipError, match="CPU"):
        E.DeviceGroundTruth(gt, 'cpu')
    with pytest.raises(lib.GritHipError, match="detections per image"):
        E.voc_images(dev[0][:, :60].contiguous(), dev[1][:, :60].contiguous(), dev[2][:, :60].contiguous(), dev[3], dgt, 0.5, records)
    with pytest.raises(lib.GritHipError, match="int64"):
        E.voc_images(dev[0], dev[1].to(torch.int32), dev[2], dev[3], dgt, 0.5, records)
    with pytest.raises(lib.GritHipError, match="NaN"):
        E.voc_images(dev[0], dev[1], dev[2], dev[3], dgt, float('nan'), records)


def torch_post_process_attr(outputs, target_sizes):
    """The torch composition PostProcessAttr stands for: sigmoid -> topk over the flat [Q * A] map -> gather of the query's box."""
    from grit_amd.utils import box_ops
    logits, boxes = outputs['attr_logits'], outputs['pred_boxes']
    B, Q, A = logits.shape
    scores, flat = logits.sigmoid().reshape(B, Q * A).topk(min(100, Q * A), dim=1)
    query, labels = flat // A, flat % A
    corners = box_ops.box_cxcywh_to_xyxy(boxes).gather(1, query[..., None].expand(-1, -1, 4))
    height, width = target_sizes.unbind(1)
    corners = corners * torch.stack([width, height, width, height], 1)[:, None, :]
    return [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, corners)]


def _outputs(seed, B, Q, K, A):
    """Fixed random outputs: logits ~ N(-4, 1), where the best fp32 sigmoids of an image are pairwise distinct (checked)."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, Q, K)) - 4.0).astype(np.float32)
    attr = (rng.standard_normal((B, Q, A)) - 4.0).astype(np.float32)
    assert D.fair(logits) and D.fair(attr)
    wh = 0.05 + 0.4 * rng.random((B, Q, 2))
    boxes = np.concatenate([wh / 2 + (1 - wh) * rng.random((B, Q, 2)), wh], -1).astype(np.float32)
    sizes = rng.integers(300, 700, (B, 2)).astype(np.float32)
    return {'pred_logits': t(logits, device=DEV), 'pred_boxes': t(boxes, device=DEV), 'attr_logits': t(attr, device=DEV)}, t(sizes, device=DEV)


@pytest.mark.parametrize("Q,A,seed", [(7, 5, 3301), (150, 400, 3302)])
def test_post_process_attr_equals_the_torch_composition(Q, A, seed):
    from models.detection.od_losses import PostProcessAttr
    outputs, sizes = _outputs(seed, 3, Q, 4, A)
    for size in (sizes, sizes.to(torch.int64)):
        got, want = PostProcessAttr()(outputs, size), torch_post_process_attr(outputs, size)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert set(g) == set(w) and g['scores'].shape == (min(100, Q * A),)
            for key in ('scores', 'labels', 'boxes'):
                assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape
                assert torch.equal(g[key], w[key]), key
            assert torch.equal(g['scores'].view(torch.int32), w['scores'].view(torch.int32))
    with pytest.raises(ValueError, match="attr_logits"):
        PostProcessAttr()({'pred_boxes': outputs['pred_boxes']}, sizes)
    with pytest.raises(Exception, match="CPU"):
        PostProcessAttr()({k: v.cpu() for k, v in outputs.items()}, sizes.cpu())


def test_end_to_end_through_both_post_processes_and_the_evaluator():
    """Fixed outputs -> PostProcess / PostProcessAttr -> VGEvaluator; the same detections through the model and accumulate_voc: the
    APs, map and wmap are equal exactly (the same host code on equal records).  Ground truth: jittered copies of some of each
    image's detections with their labels, plus objects anywhere; image 6 has no attributes."""
    from datasets.detection.metrics import AnnotationIndex, VGEvaluator, accumulate_voc
    from models.detection.od_losses import PostProcess, PostProcessAttr
    B, Q, K, A = 4, 40, 12, 9
    outputs, sizes = _outputs(3303, B, Q, K, A)
    image_ids = [9, 4, 6, 12]
    results = {'obj': PostProcess()(outputs, sizes), 'attr': PostProcessAttr()(outputs, sizes)}
    host = {kind: [{k: v.cpu().numpy() for k, v in r.items()} for r in res] for kind, res in results.items()}
    rng = np.random.default_rng(3304)
    images = [{'id': i, 'has_attr': i != 6} for i in image_ids]
    anns = []

    def add(image, category, corners, attributes):
        x0, y0, x1, y1 = [float(v) for v in corners]
        j = rng.normal(0, 0.04, 4) * np.array([x1 - x0, y1 - y0, x1 - x0, y1 - y0])
        anns.append({'id': len(anns) + 1, 'image_id': image, 'category_id': category, 'iscrowd': 0, 'area': 1.0,
                     'bbox': [x0 + j[0], y0 + j[1], x1 - x0 + j[2], y1 - y0 + j[3]], 'attributes': attributes})

    for b, image in enumerate(image_ids):
        for n in rng.choice(100, 10, replace=False):  # objects on object detections
            add(image, int(host['obj'][b]['labels'][n]), host['obj'][b]['boxes'][n], [])
        for n in rng.choice(100, 10, replace=False):  # objects on attribute detections, carrying that attribute and another one
            a = int(host['attr'][b]['labels'][n])
            add(image, int(rng.integers(K)), host['attr'][b]['boxes'][n], [a, (a + 3) % A])
        for box in M._boxes_xywh(rng, 4, 300.0):
            add(image, int(rng.integers(K)), [box[0], box[1], box[0] + box[2], box[1] + box[3]], [int(rng.integers(A))])
    index = AnnotationIndex({'images': images, 'categories': [{'id': c} for c in range(K)], 'annotations': anns})
    ev = VGEvaluator(index, ('obj', 'attr'), num_attr=A, device=DEV)
    targets = [{'image_id': torch.tensor(i, device=DEV)} for i in image_ids]
    half = lambda lo, hi: {kind: res[lo:hi] for kind, res in results.items()}
    ev.update(half(0, 3), targets[:3])  # two batches of different size
    ev.update(half(3, 4), targets[3:])
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize()
    assert ev.packed['attr'].img_ids.tolist() == [4, 9, 12] and ev.packed['obj'].img_ids.tolist() == [4, 6, 9, 12]
    for kind in ('obj', 'attr'):
        gt = ev.packed[kind]
        ids = gt.img_ids.tolist()
        slots = np.array([ids.index(i) if i in ids else -1 for i in image_ids], np.int32)
        stack = lambda key: np.stack([r[key] for r in host[kind]])
        want = M.match_images(stack('scores'), stack('labels'), stack('boxes'), slots, gt)
        _same_bytes(ev.records[kind].to_host(), want)
        model = accumulate_voc(gt, want, gt.cat_ids)
        assert np.array_equal(ev.eval[kind]['ap'], model['ap']) and np.array_equal(ev.eval[kind]['npos'], model['npos'])
        assert ev.eval[kind]['map'] == model['map'] and ev.eval[kind]['wmap'] == model['wmap']
        assert ev.stats[kind]['map'] == model['map'] and 0.0 < model['map'] <= 1.0 and (want.flag == 1).sum() >= 5
    assert ev.result_text.count('Mean AP') == 4 and 'attributes: Weighted Mean AP' in ev.result_text
    with pytest.raises(ValueError, match="attr"):
        ev.update({'obj': results['obj']}, targets)


def test_evaluate_feeds_the_vg_evaluator_on_the_tiny_detector():
    """engine.det_engine.evaluate with vg_evaluator on a small detector with the attribute head: the new keys beside the old ones."""
    from datasets.detection.metrics import AnnotationIndex, CocoEvaluator, VGEvaluator
    from engine.det_engine import evaluate
    from grit_amd.config import detection_config
    from grit_amd.utils.misc import NestedTensor
    from models.detection.detector import build_detector
    from tests.helpers import deterministic_fill_
    K, A = 11, 7
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': K, 'model.det_module.num_queries': 30,
                              'model.det_module.reduced_dim': 512, 'model.det_module.dropout': 0.0, 'model.has_attr_head': True,
                              'model.num_attr_classes': A, 'model.det_module.loss.attr_loss_coef': 1.0})
    model, criterion, post = build_detector(cfg)
    assert set(post) == {'bbox', 'attr'}
    deterministic_fill_(model)
    model.to(DEV)
    rng = np.random.default_rng(3401)
    targets, anns, images = [], [], []
    for n, image in enumerate([40, 39]):
        wh = 0.1 + 0.3 * rng.random((3, 2))
        boxes = np.concatenate([wh / 2 + (1 - wh) * rng.random((3, 2)), wh], 1).astype(np.float32)
        labels, attributes = rng.integers(0, K, 3), (rng.random((3, A)) < 0.3).astype(np.uint8)
        target = {'labels': t(labels, device=DEV), 'boxes': t(boxes, device=DEV), 'image_id': torch.tensor(image, device=DEV),
                  'orig_size': torch.tensor([224, 224], device=DEV), 'has_attr': n == 0}
        if n == 0:
            target['attributes'] = t(attributes, device=DEV)
        targets.append(target)
        images.append({'id': image, 'has_attr': n == 0})
        for label, (cx, cy, w, h), row in zip(labels.tolist(), (boxes.astype(np.float64) * 224).tolist(), attributes.tolist()):
            anns.append({'id': len(anns) + 1, 'image_id': image, 'category_id': label, 'bbox': [cx - w / 2, cy - h / 2, w, h], 'area': w * h,
                         'iscrowd': 0, 'attributes': [a for a, on in enumerate(row) if on] if n == 0 else []})
    index = AnnotationIndex({'images': images, 'categories': [{'id': c} for c in range(K)], 'annotations': anns})
    samples = NestedTensor(torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV),
                           torch.zeros(2, 224, 224, dtype=torch.bool, device=DEV))
    vg = VGEvaluator(index, ('obj', 'attr'), num_attr=A, device=DEV)
    out = evaluate(model, criterion, post, [(samples, targets)], CocoEvaluator(index, ('bbox',)), vg_evaluator=vg)
    for key in ('bbox_map', 'vg_obj_map', 'vg_obj_wmap', 'vg_attr_map', 'vg_attr_wmap'):
        assert key in out and -1.0 <= out[key] <= 1.0, key
    assert 'loss_attr' in out and len(out['result_text'].splitlines()) == 12 and len(out['vg_text'].splitlines()) == 6
    assert vg.records['obj'].to_host().seen.tolist() == [1, 1] and vg.records['attr'].to_host().seen.tolist() == [1]
    plain = evaluate(model, criterion, post, [(samples, targets)], CocoEvaluator(index, ('bbox',)))
    assert not any(k.startswith('vg_') for k in plain) and plain['bbox_map'] == out['bbox_map']
    with pytest.raises(ValueError, match="attr"):
        evaluate(model, criterion, {'bbox': post['bbox']}, [(samples, targets)], CocoEvaluator(index, ('bbox',)), vg_evaluator=vg)
