"""The device set criterion (grit_det_loss_{fwd,bwd}_f32 behind models.detection.od_losses.SetCriterion) against the reference's
criterion run in float64 (fixture G19, tests/golden/make_det_loss_golden.py), and a tiny end-to-end detector step.  Needs an MI355X.

Bounds.  Per quantity the bound is max(4 x the deviation measured on an MI355X, 4 x |ref32 - ref64| of the fixture), capped at 1e-5
relative for a loss and 1e-5 of the gradient's largest magnitude for a gradient: per-element fp32 evaluation with float64
accumulation justifies no more.  The measured deviations (relative to the same scales) are MEASURED below.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, deterministic_fill_, disable_drop_path, t

import det_draws as D  # tests/golden, put on the path by tests.helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 1e-5

# largest deviation from the float64 reference seen on an MI355X, relative to |reference| (losses) or to max |gradient|
MEASURED = {
    37: {'loss': 4.27e-8, 'dlogits': 2.96e-7, 'dboxes': 2.52e-8, 'abs_sum': 2.39e-8},
    1849: {'loss': 4.59e-8, 'dlogits': 4.09e-7, 'dboxes': 3.72e-8, 'abs_sum': 2.37e-8},
}


@pytest.fixture(scope="module")
def g19():
    return D.load_shards(GOLDEN), json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))


def _weights(L):
    w = dict(D.LOSS_WEIGHTS)
    for i in range(L - 1):
        w.update({'%s_%d' % (k, i): v for k, v in D.LOSS_WEIGHTS.items()})
    return w


def _criterion(K, L):
    from models.detection.od_losses import HungarianMatcher, SetCriterion
    c = D.COST_WEIGHTS
    return SetCriterion(K, HungarianMatcher(c['class'], c['bbox'], c['giou']), _weights(L), ['labels', 'boxes', 'cardinality'], 0.25)


def _outputs(logits, boxes):
    L = logits.shape[0]
    return {'pred_logits': logits[-1], 'pred_boxes': boxes[-1],
            'aux_outputs': [{'pred_logits': logits[i], 'pred_boxes': boxes[i]} for i in range(L - 1)]}


def _inputs(meta, K):
    L, B, Q = D.CRIT_L, D.CRIT_B, D.CRIT_Q
    logits = np.zeros((L, B, Q, K), np.float32)
    boxes = np.zeros((L, B, Q, 4), np.float32)
    for l in range(L):
        for b in range(B):
            logits[l, b], boxes[l, b] = D.predictions(meta['seeds'][l][b], Q, K)
    targets = []
    for b, T in enumerate(D.CRIT_T):
        labels, tb = D.targets(meta['target_seeds'][b], T, K)
        targets.append({'labels': t(labels, device=DEV), 'boxes': t(tb, device=DEV)})
    return t(logits, device=DEV).requires_grad_(True), t(boxes, device=DEV).requires_grad_(True), targets


@pytest.mark.parametrize("K", D.CRIT_KS)
def test_losses_and_gradients_against_float64_reference(g19, K):
    g, meta = g19
    meta = meta['crit'][str(K)]
    L = D.CRIT_L
    logits, boxes, targets = _inputs(meta, K)
    crit = _criterion(K, L)
    losses = crit(_outputs(logits, boxes), targets)
    assert set(losses) == set(meta['losses64'])
    total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict)
    total.backward()
    measured = MEASURED[K]
    seen = {'loss': 0.0, 'dlogits': 0.0, 'dboxes': 0.0, 'abs_sum': 0.0}
    failures = []
    for k, ref in sorted(meta['losses64'].items()):
        got = float(losses[k])
        scale = max(abs(ref), 1e-30)
        dev = abs(got - ref) / scale
        bound = min(CAP, max(4 * measured['loss'], 4 * abs(meta['losses32'][k] - ref) / scale))
        seen['loss'] = max(seen['loss'], dev)
        if ref == 0.0:
            bound, dev = 0.0, abs(got)
        if dev > bound:
            failures.append((k, got, ref, dev, bound))
    dl = logits.grad.double().cpu().numpy()
    db = boxes.grad.double().cpu().numpy()
    key = 'crit/%d' % K
    gmax, bmax = float(g[key + '/dlogits_max']), float(g[key + '/dboxes_max'])
    rows = g[key + '/rows']
    got_rows = dl[rows[:, 0], rows[:, 1], rows[:, 2]]  # whole rows
    ref_rows = np.concatenate([g[k] for k in sorted(g) if k.startswith(key + '/row_values/')])
    assert ref_rows.shape == got_rows.shape
    seen['dlogits'] = max(np.abs(got_rows - ref_rows).max(), np.abs(dl.reshape(-1)[::D.SAMPLE_STRIDE] - g[key + '/sample']).max()) / gmax
    seen['abs_sum'] = abs(np.abs(dl).sum() - float(g[key + '/abs_sum'])) / float(g[key + '/abs_sum'])
    mask = np.ones(db.shape[:3], bool)
    mask[rows[:, 0], rows[:, 1], rows[:, 2]] = False
    assert not db[mask].any(), "dboxes must be zero outside the matched queries"
    seen['dboxes'] = np.abs(db[rows[:, 0], rows[:, 1], rows[:, 2]] - g[key + '/dboxes']).max() / bmax
    print("det criterion K = %d: deviations %s" % (K, {k: float('%.3e' % v) for k, v in seen.items()}))
    for name in ('dlogits', 'dboxes', 'abs_sum'):
        bound = min(CAP, 4 * measured[name])
        if seen[name] > bound:
            failures.append((name, seen[name], bound))
    assert not failures, failures


def test_all_empty_targets(g19):
    g, meta = g19
    e = meta['empty']
    L, B, Q, K = e['L'], e['B'], e['Q'], e['K']
    logits = np.stack([np.stack([D.predictions(e['seed0'] + l * 2 + b, Q, K)[0] for b in range(B)]) for l in range(L)])
    boxes = np.stack([np.stack([D.predictions(e['seed0'] + l * 2 + b, Q, K)[1] for b in range(B)]) for l in range(L)])
    logits, boxes = t(logits, device=DEV).requires_grad_(True), t(boxes, device=DEV).requires_grad_(True)
    targets = [{'labels': torch.zeros(0, dtype=torch.int64, device=DEV), 'boxes': torch.zeros(0, 4, device=DEV)} for _ in range(B)]
    crit = _criterion(K, L)
    losses = crit(_outputs(logits, boxes), targets)
    for k, ref in e['losses64'].items():
        assert np.isfinite(float(losses[k]))
        assert abs(float(losses[k]) - ref) <= CAP * abs(ref), (k, float(losses[k]), ref)  # num_boxes clamped to 1
    sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict).backward()
    assert bool((logits.grad != 0).all()), "the focal loss reaches every logit"
    assert not bool(boxes.grad.any())
    ref = float(g['empty/abs_sum'])
    assert abs(float(logits.grad.double().abs().sum()) - ref) <= CAP * ref


def test_matcher_called_directly_returns_scipy_pairs(g19):
    from models.detection.od_losses import HungarianMatcher
    g, meta = g19
    problems = [p for p in meta['match'] if p['Q'] == 20 and p['layer'] == 0]  # T = 5 (T < Q) and T = 30 (T > Q)
    logits = np.stack([D.predictions(p['seed'], 20, D.MATCH_K)[0] for p in problems])
    boxes = np.stack([D.predictions(p['seed'], 20, D.MATCH_K)[1] for p in problems])
    targets = []
    for p in problems:
        labels, tb = D.targets(p['target_seed'], p['T'], D.MATCH_K)
        targets.append({'labels': t(labels, device=DEV), 'boxes': t(tb, device=DEV)})
    c = D.COST_WEIGHTS
    pairs = HungarianMatcher(c['class'], c['bbox'], c['giou'])({'pred_logits': t(logits, device=DEV), 'pred_boxes': t(boxes, device=DEV)}, targets)
    assert isinstance(pairs, list) and len(pairs) == 2
    for p, (i, j) in zip(problems, pairs):
        assert i.dtype == torch.int64 and j.dtype == torch.int64
        assert i.cpu().tolist() == g['match/%d/0/i' % p['case']].tolist()
        assert j.cpu().tolist() == g['match/%d/0/j' % p['case']].tolist()


def test_criterion_does_not_synchronise_the_host(g19):
    meta = g19[1]['crit']['37']
    logits, boxes, targets = _inputs(meta, 37)
    crit = _criterion(37, D.CRIT_L)
    crit(_outputs(logits, boxes), targets)['loss_ce'].backward()  # first call: library load, workspaces
    logits.grad = boxes.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = crit(_outputs(logits, boxes), targets)
        total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict)
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert np.isfinite(float(total)) and logits.grad is not None and boxes.grad is not None


@pytest.fixture(scope="module")
def tiny_detector(g19):
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    e = g19[1]['e2e']
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
                              'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model'],
                              'model.det_module.dropout': 0.0})
    model, criterion, _ = build_detector(cfg)
    deterministic_fill_(model)
    model.to(DEV).train()
    disable_drop_path(model)
    images, tg = D.end_to_end_batch(e['seed'], num_classes=e['num_classes'], counts=tuple(e['counts']))
    targets = [{'labels': t(l, device=DEV), 'boxes': t(b, device=DEV)} for l, b in tg]
    return model, criterion, t(images, device=DEV), targets


def test_end_to_end_losses_match_reference(g19, tiny_detector):
    from grit_amd.utils.misc import NestedTensor
    e = g19[1]['e2e']
    assert len(e['margins']) == 14 and min(e['margins']) >= 1e-2
    model, criterion, images, targets = tiny_detector
    with torch.no_grad():
        outputs = model(NestedTensor(images, torch.zeros(images.shape[0], 224, 224, dtype=torch.bool, device=DEV)))
        losses = criterion(outputs, targets)
    assert set(losses) == set(e['losses'])
    total = sum(float(losses[k]) * criterion.weight_dict[k] for k in losses if k in criterion.weight_dict)
    bad = {k: (float(losses[k]), ref) for k, ref in e['losses'].items() if abs(float(losses[k]) - ref) > 1e-4 * abs(ref)}
    print("det end to end: total %.6f (reference %.6f)" % (total, e['total']))
    assert not bad, bad
    assert abs(total - e['total']) <= 1e-4 * abs(e['total'])


def test_train_step_moves_the_heads(tiny_detector):
    from engine.det_engine import train_step
    from grit_amd.utils.misc import NestedTensor
    model, criterion, images, targets = tiny_detector
    heads = [model.det_module.class_embed[-1].weight, model.det_module.bbox_embed[-1].layers[-1].weight, model.det_module.class_embed[0].bias]
    before = [p.detach().clone() for p in heads]
    optimizer = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    samples = NestedTensor(images, torch.zeros(images.shape[0], 224, 224, dtype=torch.bool, device=DEV))
    total, losses = train_step(model, criterion, optimizer, samples, targets, max_norm=0.1)
    assert np.isfinite(float(total)) and all(np.isfinite(float(v)) for v in losses.values())
    for p, old in zip(heads, before):
        assert not torch.equal(p.detach(), old)
