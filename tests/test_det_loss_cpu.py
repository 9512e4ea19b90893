"""Detector pre-training pieces that need no GPU: box_ops on hand-computed boxes, the import paths and configuration of the
detector / criterion, the state-dict keys, the detection heads against fixture G19 (tests/golden/make_det_loss_golden.py) and the
refusal of CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, deterministic_fill_, t

import det_draws as D  # tests/golden, put on the path by tests.helpers


@pytest.fixture(scope="module")
def g19():
    return D.load_shards(GOLDEN), json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))


def test_box_ops_on_hand_computed_boxes():
    from utils.box_ops import box_cxcywh_to_xyxy, box_iou, box_xyxy_to_cxcywh, generalized_box_iou
    a = torch.tensor([[0., 0., 2., 2.]])
    others = torch.tensor([[3., 0., 5., 2.],    # disjoint: hull 5 x 2
                           [0.5, 0.5, 1.5, 1.5],  # nested
                           [0., 0., 2., 2.],    # identical
                           [2., 0., 4., 2.]])   # touching along an edge: hull 4 x 2
    iou, union = box_iou(a, others)
    assert torch.allclose(iou, torch.tensor([[0., 0.25, 1., 0.]]))
    assert torch.allclose(union, torch.tensor([[8., 4., 4., 8.]]))
    giou = generalized_box_iou(a, others)
    assert torch.allclose(giou, torch.tensor([[0. - (10. - 8.) / 10., 0.25, 1., 0.]]))
    assert generalized_box_iou(others, a).shape == (4, 1)
    c = torch.tensor([[0.5, 0.25, 0.2, 0.1]])
    assert torch.allclose(box_cxcywh_to_xyxy(c), torch.tensor([[0.4, 0.2, 0.6, 0.3]]))
    assert torch.allclose(box_xyxy_to_cxcywh(box_cxcywh_to_xyxy(c)), c)
    with pytest.raises(ValueError):
        generalized_box_iou(torch.tensor([[1., 0., 0., 1.]]), a)


def test_import_paths_and_weight_dict():
    from grit_amd.config import detection_config
    import models.detection.detector as det
    import models.detection.od_losses as od
    import grit_amd.models.detection.od_losses as own
    assert od is own and det.SetCriterion is od.SetCriterion
    assert {'HungarianMatcher', 'SetCriterion', 'PostProcess', 'build_matcher', 'sigmoid_focal_loss'} <= set(dir(od))
    cfg = detection_config().model.det_module
    weights = det.build_weight_dict(cfg)
    assert weights['loss_ce'] == 2. and weights['loss_bbox'] == 5. and weights['loss_giou'] == 2.
    for i in range(cfg.num_layers):
        for k in ('loss_ce', 'loss_bbox', 'loss_giou'):
            assert weights['%s_%d' % (k, i)] == weights[k]
    assert 'loss_ce_%d' % cfg.num_layers not in weights
    matcher = od.build_matcher(cfg.matcher)
    assert (matcher.cost_class, matcher.cost_bbox, matcher.cost_giou) == (2., 5., 2.)
    with pytest.raises(NotImplementedError):
        od.SetCriterion(5, matcher, weights, ['labels', 'masks'])
    crit = od.SetCriterion(5, matcher, weights, ['labels', 'boxes', 'cardinality'])
    with pytest.raises(NotImplementedError):
        crit({'pred_logits': torch.zeros(1, 2, 5), 'pred_boxes': torch.zeros(1, 2, 4), 'enc_outputs': {}}, [{}])
    with pytest.raises(NotImplementedError):
        det.Detector(None, None, has_attr_head=True)


def test_detector_state_dict_keys(g19):
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    e = g19[1]['e2e']
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
                              'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model']})
    model, criterion, post = build_detector(cfg)
    assert sorted(model.state_dict().keys()) == g19[1]['state_dict_keys']
    assert set(post) == {'bbox'}


def test_cpu_tensors_are_rejected():
    from models.detection.od_losses import HungarianMatcher, SetCriterion
    from grit_amd.ops import det_loss
    out = {'pred_logits': torch.zeros(1, 4, 5), 'pred_boxes': torch.full((1, 4, 4), 0.5)}
    tg = [{'labels': torch.zeros(2, dtype=torch.long), 'boxes': torch.full((2, 4), 0.5)}]
    matcher = HungarianMatcher(2, 5, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        matcher(out, tg)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        SetCriterion(5, matcher, {}, ['labels'])(out, tg)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        det_loss.linear_sum_assignment(torch.zeros(1, 4, 2), torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("dim", [4, 2])
def test_detection_head_matches_reference(g19, dim):
    """Train mode: level 0 starts from init_reference, level l from inter_references[l - 1] (levels 0 and 1 share the initial
    reference); eval mode: the last head alone, from inter_references[-2]."""
    from models.detection.det_module import DetectionModule
    g, meta = g19
    mod = deterministic_fill_(DetectionModule(**meta['head']), 'g19.head.')
    hs = t(g['head/hs'])
    inter = t(g['head/refs'][..., :dim].copy())
    init = inter[0].clone()
    mod.train()
    with torch.no_grad():
        out = mod.detection_head(hs, init, inter)
    key = 'head/train%d' % dim
    assert torch.allclose(out['pred_logits'], t(g[key + '/logits']), rtol=1e-5, atol=1e-6)
    assert torch.allclose(out['pred_boxes'], t(g[key + '/boxes']), rtol=1e-5, atol=1e-6)
    assert len(out['aux_outputs']) == hs.shape[0] - 1
    for i, aux in enumerate(out['aux_outputs']):
        assert torch.allclose(aux['pred_logits'], t(g[key + '/aux_logits'][i]), rtol=1e-5, atol=1e-6)
        assert torch.allclose(aux['pred_boxes'], t(g[key + '/aux_boxes'][i]), rtol=1e-5, atol=1e-6)
    # the quirk itself: feeding level 1 another reference than the initial one changes its boxes
    other = inter.clone()
    other[0] = 1 - other[0]
    with torch.no_grad():
        moved = mod.detection_head(hs, init, other)
    assert not torch.allclose(moved['aux_outputs'][1]['pred_boxes'], out['aux_outputs'][1]['pred_boxes'])
    assert torch.equal(moved['aux_outputs'][0]['pred_boxes'], out['aux_outputs'][0]['pred_boxes'])
    mod.eval()
    with torch.no_grad():
        out = mod.detection_head(hs, init, inter)
    key = 'head/eval%d' % dim
    assert 'aux_outputs' not in out
    assert torch.allclose(out['pred_logits'], t(g[key + '/logits']), rtol=1e-5, atol=1e-6)
    assert torch.allclose(out['pred_boxes'], t(g[key + '/boxes']), rtol=1e-5, atol=1e-6)


def test_sigmoid_focal_loss_against_a_scalar_statement():
    """Element by element with math.*: -alpha_t (1 - p_t)^gamma log(p_t), mean over dim 1, sum, / num_boxes."""
    import math
    from models.detection.od_losses import sigmoid_focal_loss
    g = torch.Generator().manual_seed(5)
    x = (4 * torch.randn(3, 4, 5, generator=g)).double()
    z = (torch.rand(3, 4, 5, generator=g) < 0.3).double()
    for alpha in (0.25, -1.0):
        want = 0.0
        for xv, zv in zip(x.flatten().tolist(), z.flatten().tolist()):
            p = 1.0 / (1.0 + math.exp(-xv))
            p_t = p if zv else 1.0 - p
            weight = 1.0 if alpha < 0 else (alpha if zv else 1.0 - alpha)
            want += -weight * (1.0 - p_t) ** 2 * math.log(p_t)
        want = want / 4 / 7.0
        got = float(sigmoid_focal_loss(x, z, 7.0, alpha=alpha, gamma=2))
        assert abs(got - want) < 1e-12 * abs(want)
    # the detection heads hand the stacks over explicitly
    from models.detection.det_module import DetectionModule
    mod = DetectionModule(d_model=32, nhead=4, num_decoder_layers=2, dim_feedforward=32, dropout=0., num_classes=3, num_queries=4, aux_loss=True).train()
    refs = torch.rand(3, 1, 4, 4)
    out = mod.detection_head(torch.randn(3, 1, 4, 32), refs[0], refs)
    assert out['pred_logits_all'].shape == (3, 1, 4, 3) and torch.equal(out['pred_logits_all'][-1], out['pred_logits'])
    assert torch.equal(out['pred_boxes_all'][0], out['aux_outputs'][0]['pred_boxes'])
