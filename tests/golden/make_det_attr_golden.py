"""Fixture G23, tests/golden/det_attr_g23.npz + .json: the reference's AttrHead, SetCriterion.weighted_attr_loss and a Detector step
with the attribute head (imported behind the stubs of make_det_loss_golden.py) on seeded inputs.  A generator, not a test:

    python tests/golden/make_det_attr_golden.py /path/to/the/reference/checkout [--skip-e2e]

Only data is written, and no inputs: generator and tests repeat them from tests/golden/det_attr_draws.py and the seeds kept here.

  head/K/*  AttrHead(256, 400, K), deterministic fill 'g23.head.K.', B = 2, Q = 150, K in (37, 1849), run in fp32 and in float64: the
            labels, and of the float64 run attr_logits and the gradients of sum(attr_logits * w) -- d obj_h, d od_cls_embed.weight
            (the rows of the chosen classes; the others are zero) and the Linears' -- each as every 29th element of its flat form,
            with its largest magnitude and the largest |fp32 - float64| in the json.  The seed is redrawn until every row's gap
            between its best and second-best class logit is >= 1e-3.
  loss/*    weighted_attr_loss in fp32 and float64 on the given pairs of det_attr_draws.loss_case, for A in (37, 400), Q in (19, 150),
            T = (0, 5, 40) ((0, 5, Q + 21) for 'tq'), kinds: mixed has_attr, no image has attributes, all targets zero, all one,
            an image with T > Q.  Of the float64 run the gradient at the matched rows of the images with attributes (it is zero
            elsewhere), every 29th element, its largest magnitude and the float64 sum of |gradient|.
  e2e       the 224 x 224, B = 2 detector step of G19 with the head (A = 23): every loss key, the matcher margins and the label gap.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import det_attr_draws as A23  # noqa: E402
import det_draws as D  # noqa: E402
from make_det_loss_golden import E2E, MARGIN, Capture, import_reference, margin_of  # noqa: E402


def sample(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)[::A23.STRIDE])


def run_head(K, seed, dtype):
    from models.detection.heads import AttrHead
    from fill import deterministic_fill_
    head = deterministic_fill_(AttrHead(A23.HEAD_D, A23.HEAD_A, K), 'g23.head.%d.' % K).to(dtype)
    obj_h, logits, w = A23.head_inputs(seed, K)
    h = torch.from_numpy(obj_h).to(dtype).requires_grad_(True)
    lg = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    out = head(h, lg)['attr_logits']
    (out * torch.from_numpy(w).to(dtype)).sum().backward()
    assert lg.grad is None or not lg.grad.any()
    labels = torch.argmax(torch.sigmoid(lg.detach()), -1).numpy()
    grads = {'dobj_h': h.grad.numpy(), 'dembed': head.od_cls_embed.weight.grad.numpy()}
    for name in ('attr_linear1', 'attr_linear2'):
        grads['d%s_weight' % name] = getattr(head, name).weight.grad.numpy()
        grads['d%s_bias' % name] = getattr(head, name).bias.grad.numpy()
    return labels, out.detach().numpy(), grads


def make_head(out, meta):
    meta['head'] = {}
    for K in A23.HEAD_KS:
        for attempt in range(200):
            seed = 2300 + K * 1000 + attempt
            gap = A23.top_gap(A23.head_inputs(seed, K)[1])
            if gap >= A23.HEAD_MARGIN:
                break
        else:
            raise RuntimeError("no draw with a label gap >= %g for K %d" % (A23.HEAD_MARGIN, K))
        l32, o32, g32 = run_head(K, seed, torch.float32)
        l64, o64, g64 = run_head(K, seed, torch.float64)
        assert (l32 == l64).all()
        key = 'head/%d' % K
        out[key + '/labels'] = l64.astype(np.int32)
        chosen = np.unique(l64)
        rest = np.ones(K, bool)
        rest[chosen] = False
        assert not g64['dembed'][rest].any()
        g32['dembed'], g64['dembed'] = g32['dembed'][chosen], g64['dembed'][chosen]
        info = {'seed': seed, 'margin': gap, 'max': {}, 'dev32': {}}
        for name, a64, a32 in [('attr_logits', o64, o32)] + [(n, g64[n], g32[n]) for n in sorted(g64)]:
            out['%s/%s' % (key, name)] = sample(a64)
            info['max'][name] = float(np.abs(a64).max())
            info['dev32'][name] = float(np.abs(a32.astype(np.float64) - a64).max())
        meta['head'][str(K)] = info
        print('head K %d seed %d gap %.5f chosen %d dev32 %s' % (K, seed, gap, len(chosen), info['dev32']))


def run_loss(od, kind, A, Q, dtype):
    x, attrs, flags, pairs = A23.loss_case(kind, A, Q)
    crit = od.SetCriterion(5, None, {}, ['labels'])
    lg = torch.from_numpy(x).to(dtype).requires_grad_(True)
    targets = [{'attributes': torch.from_numpy(a), 'has_attr': torch.tensor(f)} for a, f in zip(attrs, flags)]
    indices = [(torch.from_numpy(q), torch.from_numpy(t)) for q, t in pairs]
    # the reference casts the gathered targets with .float(), after which BCEWithLogitsLoss computes in fp32 whatever the logits
    # are: for the float64 run that one cast goes to double
    as_float = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        loss = crit.weighted_attr_loss({'attr_logits': lg}, targets, indices)['loss_attr']
    finally:
        torch.Tensor.float = as_float
    assert loss.dtype == dtype
    loss.backward()
    return float(loss.detach()), lg.grad.numpy()


def matched_rows(grad, flags, pairs):
    rows = [grad[b, q] for b, (f, (q, _)) in enumerate(zip(flags, pairs)) if f and len(q)]
    return np.concatenate(rows) if rows else np.zeros((0, grad.shape[-1]))


def make_loss(od, out, meta):
    meta['loss'] = {}
    for kind in A23.LOSS_KINDS:
        for A in A23.LOSS_AS:
            for Q in A23.LOSS_QS:
                l32, _ = run_loss(od, kind, A, Q, torch.float32)
                l64, g64 = run_loss(od, kind, A, Q, torch.float64)
                _, _, flags, pairs = A23.loss_case(kind, A, Q)
                mask = np.ones(g64.shape[:2], bool)
                for b, (f, (q, _)) in enumerate(zip(flags, pairs)):
                    if f:
                        mask[b, q] = False
                assert not g64[mask].any()
                key = 'loss/%s/%d/%d' % (kind, A, Q)
                out[key + '/grad'] = sample(matched_rows(g64, flags, pairs))
                meta['loss']['%s/%d/%d' % (kind, A, Q)] = {'loss32': l32, 'loss64': l64, 'grad_max': float(np.abs(g64).max()),
                                                           'grad_abs_sum': float(np.abs(g64).sum())}
                print('loss %-5s A %3d Q %3d  %.9f / %.12f  |g| %.6f' % (kind, A, Q, l32, l64, np.abs(g64).sum()))


def make_e2e(od, meta, first_seed):
    from types import SimpleNamespace
    from engine.utils import NestedTensor
    from fill import deterministic_fill_
    from models.common.swin_model import swin_base_win7_384
    from models.detection.det_module import build_det_module_with_config
    from models.detection.detector import Detector
    cfg = SimpleNamespace(d_model=E2E['d_model'], num_heads=8, num_layers=6, dim_feedforward=1024, dropout=0.0, activation='relu',
                          num_classes=E2E['num_classes'], num_levels=4, num_points=4, num_queries=E2E['num_queries'],
                          return_intermediate=True, aux_loss=True, with_box_refine=True)
    backbone, _ = swin_base_win7_384(pretrained=None)
    model = deterministic_fill_(Detector(backbone, build_det_module_with_config(cfg), hidden_dim=E2E['d_model'], has_attr_head=True,
                                         num_attr_classes=A23.E2E_A, num_od_classes=E2E['num_classes'])).train()
    weight = dict(D.LOSS_WEIGHTS, loss_attr=1.0)
    for i in range(6):
        weight.update({'%s_%d' % (k, i): v for k, v in D.LOSS_WEIGHTS.items()})
    for seed in [first_seed] + list(range(1900, 1960)):
        images, tg = D.end_to_end_batch(seed, num_classes=E2E['num_classes'], counts=E2E['counts'])
        extra = A23.e2e_attributes(seed, E2E['counts'])
        od.linear_sum_assignment = Capture()
        matcher = od.HungarianMatcher(D.COST_WEIGHTS['class'], D.COST_WEIGHTS['bbox'], D.COST_WEIGHTS['giou'])
        crit = od.SetCriterion(E2E['num_classes'], matcher, weight, ['labels', 'boxes', 'cardinality'], focal_alpha=0.25)
        with torch.no_grad():
            outputs = model(NestedTensor(torch.from_numpy(images), torch.zeros(2, 224, 224, dtype=torch.bool)))
            losses = crit(outputs, [{'labels': torch.from_numpy(l), 'boxes': torch.from_numpy(b), 'attributes': torch.from_numpy(a),
                                     'has_attr': torch.tensor(f)} for (l, b), (a, f) in zip(tg, extra)])
        margins = [margin_of(C.astype(np.float32)) for C in od.linear_sum_assignment.costs]
        gap = A23.top_gap(outputs['pred_logits'].numpy())
        print('e2e seed %d min margin %.5f label gap %.5f' % (seed, min(margins), gap))
        if len(margins) == 14 and min(margins) >= MARGIN and gap >= A23.HEAD_MARGIN:
            break
    else:
        raise RuntimeError("no end-to-end draw with every margin >= %g and a label gap >= %g" % (MARGIN, A23.HEAD_MARGIN))
    total = sum(float(losses[k]) * weight[k] for k in losses if k in weight)
    meta['e2e'] = dict(E2E, num_attr_classes=A23.E2E_A, seed=seed, margins=margins, label_gap=gap,
                       losses={k: float(v) for k, v in losses.items()}, total=total,
                       state_dict_keys=sorted(model.state_dict().keys()))
    print('e2e total', total, 'loss_attr', float(losses['loss_attr']))


def main(ref, skip_e2e=False):
    import_reference(ref)
    import models.detection.od_losses as od
    out, meta = {}, {}
    path = os.path.join(HERE, 'det_attr_g23')
    make_head(out, meta)
    make_loss(od, out, meta)
    if skip_e2e:
        if os.path.exists(path + '.json'):
            old = json.load(open(path + '.json'))
            if 'e2e' in old:
                meta['e2e'] = old['e2e']
    else:
        make_e2e(od, meta, json.load(open(os.path.join(HERE, 'det_loss_g19.json')))['e2e']['seed'])
    np.savez_compressed(path + '.npz', **out)
    with open(path + '.json', 'w') as f:
        json.dump(meta, f)
    print('g23: %d bytes npz, %d bytes json' % (os.path.getsize(path + '.npz'), os.path.getsize(path + '.json')))


if __name__ == '__main__':
    main(sys.argv[1], '--skip-e2e' in sys.argv)
