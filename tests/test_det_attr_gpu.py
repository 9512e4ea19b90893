"""The attribute head on the device (grit_attr_embed_{cat,grad}, grit_det_attr_{fwd,bwd}_f32 behind models.detection.heads.AttrHead
and models.detection.od_losses.SetCriterion) against the host forms and the reference run in float64 (fixture G23,
tests/golden/make_det_attr_golden.py).  Needs an MI355X.

Labels and copies are exact.  The embedding gradient is an fp32 sum in row order: each element lies within (n - 1) 2^-24 sum|terms|
of the float64 sum of its n terms.  Loss and head follow the set criterion's rule (tests/test_det_criterion_gpu.py): per quantity the
bound is max(4 x the deviation measured on an MI355X, 4 x |ref32 - ref64| of the fixture), capped at 1e-5 relative for a loss and
1e-5 of the gradient's largest magnitude for a gradient.  The measured deviations (relative to the same scales) are MEASURED below.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, deterministic_fill_, disable_drop_path, t

import det_attr_draws as A23  # tests/golden, put on the path by tests.helpers
import det_draws as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 1e-5

# largest deviation from the float64 reference seen on an MI355X, relative to |reference| (loss) or to the largest magnitude of the
# quantity (everything else)
MEASURED = {
    'loss': 5.37e-8, 'dlogits': 1.50e-7, 'abs_sum': 5.41e-8,  # over the G23 cases and the Q x A grid below
    'head': {'attr_logits': 6.15e-7, 'dobj_h': 4.42e-7, 'dembed': 3.86e-7, 'dattr_linear1_weight': 3.53e-7, 'dattr_linear1_bias': 2.04e-7,
             'dattr_linear2_weight': 4.62e-7, 'dattr_linear2_bias': 7.31e-8},  # the larger of K = 37 and K = 1849
}


@pytest.fixture(scope="module")
def g23():
    with np.load(os.path.join(GOLDEN, "det_attr_g23.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    return arrays, json.load(open(os.path.join(GOLDEN, "det_attr_g23.json")))


# ---- kernel A ----------------------------------------------------------------------------------------------------------------------

def _lattice(rng, rows, K):
    """Per row K distinct multiples of 2^-7 in [-8, 8): neighbouring sigmoids are >= 44 fp32 ulps apart."""
    return np.stack([(rng.permutation(2048)[:K].astype(np.float32) - 1024.0) / 128.0 for _ in range(rows)])


def _front(obj_h, logits, weight):
    from grit_amd.ops.det_attr import embed_cat
    out, labels = embed_cat(obj_h, logits, weight)
    d = obj_h.shape[1]
    assert torch.equal(out[:, :d], obj_h), "left half: obj_h bit for bit"
    assert torch.equal(out[:, d:], weight[labels.long()]), "right half: the embedding rows bit for bit"
    return labels.cpu()


@pytest.mark.parametrize("K", [1, 37, 63, 64, 65, 1849])
def test_labels_exact_and_halves_bit_equal(K):
    from grit_amd.ops.det_attr import attr_labels_host
    rng = np.random.default_rng(230 + K)
    for rows in (1, 5, 300):
        for d in (64, 256):
            x = _lattice(rng, rows, K)
            obj_h = t(rng.standard_normal((rows, d)).astype(np.float32), device=DEV)
            weight = t(rng.standard_normal((K, d)).astype(np.float32), device=DEV)
            want = attr_labels_host(t(x))
            assert want.tolist() == x.argmax(1).tolist()  # distinct unsaturated values: sigmoid keeps the order
            assert _front(obj_h, t(x, device=DEV), weight).tolist() == want.tolist()
            if K >= 2:  # the maximum at two indices: the first wins
                dup, first = x.copy(), []
                for r in range(rows):
                    a = int(x[r].argmax())
                    b = int((a + 1 + rng.integers(0, K - 1)) % K)
                    dup[r, b] = x[r, a]
                    first.append(min(a, b))
                assert attr_labels_host(t(dup)).tolist() == first
                assert _front(obj_h, t(dup, device=DEV), weight).tolist() == first
            # bf16 logits: the fp32 rule on the stored values, ties among equal bf16 values to the first index
            xb = t(x).to(torch.bfloat16)
            want = torch.argmax(torch.sigmoid(xb.float()), -1)
            assert _front(obj_h, xb.to(DEV), weight).tolist() == want.tolist()
            # bf16 maps
            assert _front(obj_h.to(torch.bfloat16), t(x, device=DEV), weight.to(torch.bfloat16)).tolist() == attr_labels_host(t(x)).tolist()


def test_saturated_sigmoids_pick_the_first_index():
    """fp32 sigmoid is 1.0 from a logit of about 16.7: among several saturated logits the FIRST index is the label, although a
    later one is larger.  An argmax over the logits fails here."""
    from grit_amd.ops.det_attr import attr_labels_host
    rng = np.random.default_rng(2318)
    for K in (37, 65, 1849):
        rows = 40
        x = np.minimum(_lattice(rng, rows, K), 7.5) + 4.0  # everything <= 11.5
        want = []
        for r in range(rows):
            spots = np.sort(rng.permutation(K - 1)[:3] + 1)  # after at least one smaller index
            x[r, spots] = np.array([18.0, 25.0, 21.5], np.float32) + (r % 4)
            want.append(int(spots[0]))
        assert (x.argmax(1) != np.asarray(want)).all()
        assert attr_labels_host(t(x)).tolist() == want
        obj_h = t(rng.standard_normal((rows, 64)).astype(np.float32), device=DEV)
        weight = t(rng.standard_normal((K, 64)).astype(np.float32), device=DEV)
        assert _front(obj_h, t(x, device=DEV), weight).tolist() == want
    row = np.full((1, 12), -3.0, np.float32)
    row[0, 3], row[0, 9] = 19.0, 25.0
    assert _front(obj_h[:1], t(row, device=DEV), weight[:12]).tolist() == [3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_that_are_no_multiple_of_16_bytes(dtype):
    rng = np.random.default_rng(2306)
    for d in (6, 7, 70):
        obj_h = t(rng.standard_normal((9, d)).astype(np.float32), device=DEV).to(dtype)
        weight = t(rng.standard_normal((11, d)).astype(np.float32), device=DEV).to(dtype)
        x = _lattice(rng, 9, 11)
        assert _front(obj_h, t(x, device=DEV), weight).tolist() == x.argmax(1).tolist()


# ---- kernel B ----------------------------------------------------------------------------------------------------------------------

def _label_sets(rng, rows, K):
    one = np.full(rows, K // 2, np.int32)  # all rows one class
    few = rng.choice(np.arange(0, K, 3), rows).astype(np.int32) if K >= 3 else np.zeros(rows, np.int32)  # two thirds of the classes: nobody
    return [one, few]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,d", [(37, 64), (37, 256), (1849, 256), (5, 70), (1, 64)])
def test_embedding_gradient(K, d, dtype):
    from grit_amd.ops.det_attr import embed_grad
    rng = np.random.default_rng(2307 + K + d)
    for rows in (1, 300):
        for labels in _label_sets(rng, rows, K):
            dcat = t(rng.standard_normal((rows, 2 * d)).astype(np.float32), device=DEV).to(dtype)
            lab = t(labels, device=DEV)
            out = torch.full((K, d), float('nan'), dtype=dtype, device=DEV)
            got = embed_grad(dcat, lab, K, out=out)
            again = embed_grad(dcat, lab, K, out=torch.full((K, d), float('nan'), dtype=dtype, device=DEV))
            assert torch.equal(got, again), "two runs bit-equal"
            terms = dcat[:, d:].double().cpu()
            index = t(labels).long()
            ref = torch.zeros(K, d, dtype=torch.float64).index_add_(0, index, terms)
            mass = torch.zeros(K, d, dtype=torch.float64).index_add_(0, index, terms.abs())
            n = torch.bincount(index, minlength=K).double()[:, None]
            bound = (n - 1).clamp(min=0) * 2.0 ** -24 * mass
            if dtype == torch.bfloat16:
                bound = bound + 2.0 ** -8 * (ref.abs() + bound)  # the result rounded to bf16: 8 significant bits
            err = (got.double().cpu() - ref).abs()
            assert bool((err <= bound).all()), float((err - bound).max())
            assert not bool(got[t(np.bincount(labels, minlength=K) == 0, device=DEV)].any()), "classes nobody chose: zeros"


# ---- the loss ----------------------------------------------------------------------------------------------------------------------

class _Packed(object):
    def __init__(self, attrs, flags, A):
        counts = [len(a) for a in attrs]
        self.attributes = t(np.concatenate(list(attrs) + [np.zeros((1, A), np.uint8)]), device=DEV)
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(DEV)
        self.has_attr = flags if isinstance(flags, torch.Tensor) else torch.tensor(list(flags), dtype=torch.bool).to(DEV)
        self.counts = counts

    def __len__(self):
        return len(self.counts)


def _raw_loss(x, packed, match_t, upstream):
    """The two entry points themselves on poisoned outputs -> (loss, dlogits)."""
    from grit_amd import lib
    B, Q, A = x.shape
    chunks = (Q + lib.DET_LOSS_ROWS - 1) // lib.DET_LOSS_ROWS
    partials = torch.full((B * chunks, 2), float('nan'), dtype=torch.float64, device=DEV)
    counts = torch.full((B * chunks, 2), -7, dtype=torch.int64, device=DEV)
    ticket = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), float('nan'), device=DEV)
    totals = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    dlogits = torch.full_like(x, float('nan'))
    up = torch.tensor([upstream], dtype=torch.float32).to(DEV)
    p, l = lib.ptr, lib.load()
    lib.check(l.grit_det_attr_fwd_f32(p(x), p(packed.attributes), p(packed.offsets), p(packed.has_attr), p(match_t), B, Q, A, p(partials),
                                      p(counts), p(ticket), p(loss), p(totals), lib.current_stream_ptr()), "fwd")
    lib.check(l.grit_det_attr_bwd_f32(p(x), p(packed.attributes), p(packed.offsets), p(packed.has_attr), p(match_t), B, Q, A, p(totals),
                                      p(up), p(dlogits), lib.current_stream_ptr()), "bwd")
    return loss, dlogits, totals


def _check_loss(x, attrs, flags, match_t, ref_loss, ref_grad, dev32, seen, upstream=0.37):
    """ref_loss / ref_grad: float64 values of the loss and of its gradient (upstream 1) -> failures; `seen` collects the deviations."""
    from grit_amd.ops.det_attr import attr_loss
    B, Q, A = x.shape
    packed = _Packed(attrs, flags, A)
    xd = t(x, device=DEV).requires_grad_(True)
    mt = t(match_t, device=DEV)
    loss = attr_loss(xd, mt, packed)
    (loss * upstream).backward()
    raw_loss, raw_grad, totals = _raw_loss(xd.detach(), packed, mt, upstream)
    assert torch.equal(raw_loss.view(()), loss.detach()) and torch.equal(raw_grad, xd.grad), "two runs bit-equal, every element written"
    sel = np.asarray(flags, bool)[:, None] & (match_t >= 0)
    y = np.zeros((B, Q, A))
    off = np.concatenate([[0], np.cumsum([len(a) for a in attrs])])
    allattr = np.concatenate(list(attrs) + [np.zeros((1, A), np.uint8)])
    for b, q in zip(*np.nonzero(sel)):
        y[b, q] = allattr[off[b] + match_t[b, q]] != 0
    assert totals.tolist() == [int((y * sel[..., None]).sum()), int(((1 - y) * sel[..., None]).sum())], "N1, N0 as integers"
    grad = xd.grad.double().cpu().numpy() / upstream
    assert not grad[~sel].any(), "exactly zero on unmatched rows and on images without attributes"
    failures = []
    got = float(loss.detach())
    if ref_loss == 0.0:
        if got != 0.0 or grad.any():
            failures.append(('loss', got, 0.0))
        return failures
    dev = abs(got - ref_loss) / abs(ref_loss)
    seen['loss'] = max(seen['loss'], dev)
    if dev > min(CAP, max(4 * MEASURED['loss'], 4 * dev32)):
        failures.append(('loss', got, ref_loss, dev))
    gmax = np.abs(ref_grad).max()
    dev = np.abs(grad - ref_grad).max() / gmax
    seen['dlogits'] = max(seen['dlogits'], dev)
    if dev > min(CAP, 4 * MEASURED['dlogits']):
        failures.append(('dlogits', dev))
    dev = abs(np.abs(grad).sum() - np.abs(ref_grad).sum()) / np.abs(ref_grad).sum()
    seen['abs_sum'] = max(seen['abs_sum'], dev)
    if dev > min(CAP, 4 * MEASURED['abs_sum']):
        failures.append(('abs_sum', dev))
    return failures


def _host64(x, attrs, flags, match_t):
    from grit_amd.ops.det_attr import attr_loss_host
    A = x.shape[-1]
    lg = t(x).double().requires_grad_(True)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(a) for a in attrs])]), dtype=torch.int32)
    loss = attr_loss_host(lg, t(np.concatenate(list(attrs) + [np.zeros((1, A), np.uint8)])), offsets, torch.tensor(list(flags)), t(match_t))
    loss.backward()
    return float(loss.detach()), lg.grad.numpy()


@pytest.mark.parametrize("kind", A23.LOSS_KINDS)
def test_loss_and_gradient_against_float64_reference(g23, kind):
    g, meta = g23
    seen = {'loss': 0.0, 'dlogits': 0.0, 'abs_sum': 0.0}
    failures = []
    for A in A23.LOSS_AS:
        for Q in A23.LOSS_QS:
            info = meta['loss']['%s/%d/%d' % (kind, A, Q)]
            x, attrs, flags, pairs = A23.loss_case(kind, A, Q)
            match_t = A23.match_t_of(pairs, Q)
            # the whole float64 gradient from the host form, itself held to the fixture's samples (here and in the CPU tests)
            loss64, grad64 = _host64(x, attrs, flags, match_t)
            assert abs(loss64 - info['loss64']) <= 1e-12 * max(abs(info['loss64']), 1.0)
            rows = [grad64[b, q] for b, (f, (q, _)) in enumerate(zip(flags, pairs)) if f and len(q)]
            if rows:
                assert np.abs(np.concatenate(rows).reshape(-1)[::A23.STRIDE] - g['loss/%s/%d/%d/grad' % (kind, A, Q)]).max() <= 1e-12 * info['grad_max']
            dev32 = abs(info['loss32'] - info['loss64']) / max(abs(info['loss64']), 1e-30)
            failures += [(A, Q) + f for f in _check_loss(x, attrs, flags, match_t, info['loss64'], grad64, dev32, seen)]
    print("det attr loss %s: deviations %s" % (kind, {k: float('%.3e' % v) for k, v in seen.items()}))
    assert not failures, failures


@pytest.mark.parametrize("Q", [1, 19, 21, 150])
def test_loss_around_the_row_chunk_and_lane_count(Q):
    """Q around the 20-row chunk of a block, A around the 64 lanes of a row's wave; T > Q included."""
    seen = {'loss': 0.0, 'dlogits': 0.0, 'abs_sum': 0.0}
    failures = []
    for A in (1, 37, 64, 400):
        rng = np.random.default_rng(2350 + Q * 7 + A)
        x = (2.0 * rng.standard_normal((3, Q, A))).astype(np.float32)
        attrs, pairs = [], []
        for T in (Q + 3, 0, 5):
            a = (rng.random((T, A)) < 0.3).astype(np.uint8)
            if A == 1 and T:
                a[0, 0], a[-1, 0] = 1, 0
            n = min(Q, T)
            attrs.append(a)
            pairs.append((np.sort(rng.permutation(Q)[:n]), rng.permutation(T)[:n]))
        flags = (True, True, True)
        match_t = A23.match_t_of(pairs, Q)
        loss64, grad64 = _host64(x, attrs, flags, match_t)
        failures += [(A,) + f for f in _check_loss(x, attrs, flags, match_t, loss64, grad64, 0.0, seen, upstream=-1.75)]
    print("det attr loss Q %d: deviations %s" % (Q, {k: float('%.3e' % v) for k, v in seen.items()}))
    assert not failures, failures


# ---- model level -------------------------------------------------------------------------------------------------------------------

def _g19_criterion_inputs():
    meta = json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))['crit']['37']
    L, B, Q, K = D.CRIT_L, D.CRIT_B, D.CRIT_Q, 37
    logits = np.zeros((L, B, Q, K), np.float32)
    boxes = np.zeros((L, B, Q, 4), np.float32)
    for l in range(L):
        for b in range(B):
            logits[l, b], boxes[l, b] = D.predictions(meta['seeds'][l][b], Q, K)
    targets = []
    for b, T in enumerate(D.CRIT_T):
        labels, tb = D.targets(meta['target_seeds'][b], T, K)
        targets.append({'labels': t(labels, device=DEV), 'boxes': t(tb, device=DEV)})
    return t(logits, device=DEV), t(boxes, device=DEV), targets


def _criterion(K, L):
    from models.detection.od_losses import HungarianMatcher, SetCriterion
    c = D.COST_WEIGHTS
    w = dict(D.LOSS_WEIGHTS, loss_attr=1.0)
    for i in range(L - 1):
        w.update({'%s_%d' % (k, i): v for k, v in D.LOSS_WEIGHTS.items()})
    return SetCriterion(K, HungarianMatcher(c['class'], c['bbox'], c['giou']), w, ['labels', 'boxes', 'cardinality'], 0.25)


def _outputs(logits, boxes, attr_logits=None):
    L = logits.shape[0]
    out = {'pred_logits': logits[-1], 'pred_boxes': boxes[-1],
           'aux_outputs': [{'pred_logits': logits[i], 'pred_boxes': boxes[i]} for i in range(L - 1)]}
    if attr_logits is not None:
        out['attr_logits'] = attr_logits
    return out


def test_criterion_with_attributes_keeps_every_other_loss_and_never_waits_for_the_host():
    from grit_amd.ops import det_loss
    from grit_amd.ops.det_attr import attr_loss_host
    logits, boxes, targets = _g19_criterion_inputs()
    A = 37
    rng = np.random.default_rng(2360)
    attr_logits = t((2.0 * rng.standard_normal((D.CRIT_B, D.CRIT_Q, A))).astype(np.float32), device=DEV).requires_grad_(True)
    crit = _criterion(37, D.CRIT_L)
    plain = crit(_outputs(logits, boxes), targets)
    assert 'loss_attr' not in plain
    with_attr = [dict(tg) for tg in targets]
    with_attr[1].update(attributes=t((rng.random((5, A)) < 0.1).astype(np.uint8), device=DEV), has_attr=True)
    with_attr[2].update(attributes=t((rng.random((40, A)) < 0.1).astype(np.int64), device=DEV), has_attr=torch.tensor(True, device=DEV))
    crit(_outputs(logits, boxes, attr_logits), with_attr)['loss_attr'].backward()  # first call: workspaces
    attr_logits.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = crit(_outputs(logits, boxes, attr_logits), with_attr)
        total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict)
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert set(losses) == set(plain) | {'loss_attr'}
    for k in plain:
        assert torch.equal(losses[k], plain[k]), k
    # loss_attr is the host form's on the last layer's match
    packed = det_loss.pack_targets(with_attr, num_attr=A)
    assert packed.has_attr.tolist() == [False, True, True] and tuple(packed.attributes.shape) == (46, A)
    _, match_t = crit.matcher.match_layers(logits, boxes, packed)
    x64 = attr_logits.detach().double().cpu().requires_grad_(True)
    ref = attr_loss_host(x64, packed.attributes.cpu(), packed.offsets.cpu(), packed.has_attr.cpu(), match_t[-1].cpu())
    ref.backward()
    assert abs(float(losses['loss_attr']) - float(ref.detach())) <= CAP * float(ref.detach())
    assert float((attr_logits.grad.double().cpu() - x64.grad).abs().max()) <= CAP * float(x64.grad.abs().max())
    # a batch nobody annotated with attributes: 0 with a zero gradient; a wrong class count is an error
    attr_logits.grad = None
    zero = crit(_outputs(logits, boxes, attr_logits), targets)['loss_attr']
    zero.backward()
    assert float(zero) == 0.0 and not bool(attr_logits.grad.any())
    with pytest.raises(det_loss._lib.GritHipError, match="attribute classes"):
        crit(_outputs(logits, boxes, attr_logits[..., :20]), with_attr)


@pytest.mark.parametrize("K", A23.HEAD_KS)
def test_head_forward_and_backward_against_reference(g23, K):
    from models.detection.heads import AttrHead
    g, meta = g23
    info = meta['head'][str(K)]
    assert info['margin'] >= A23.HEAD_MARGIN
    obj_h, logits, w = A23.head_inputs(info['seed'], K)
    head = deterministic_fill_(AttrHead(A23.HEAD_D, A23.HEAD_A, K), 'g23.head.%d.' % K).to(DEV)
    h, lg, w = t(obj_h, device=DEV).requires_grad_(True), t(logits, device=DEV).requires_grad_(True), t(w, device=DEV)
    from grit_amd.ops.det_attr import attr_embed_cat
    _, labels = attr_embed_cat(h, lg, head.od_cls_embed.weight)
    assert labels.cpu().tolist() == g['head/%d/labels' % K].tolist()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = head(h, lg)['attr_logits']
        (out * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert lg.grad is None, "no gradient reaches pred_logits"
    chosen = np.unique(g['head/%d/labels' % K])
    rest = np.ones(K, bool)
    rest[chosen] = False
    dembed = head.od_cls_embed.weight.grad
    assert not bool(dembed[t(rest, device=DEV)].any())
    got = {'attr_logits': out, 'dobj_h': h.grad, 'dembed': dembed[t(chosen.astype(np.int64), device=DEV)],
           'dattr_linear1_weight': head.attr_linear1.weight.grad, 'dattr_linear1_bias': head.attr_linear1.bias.grad,
           'dattr_linear2_weight': head.attr_linear2.weight.grad, 'dattr_linear2_bias': head.attr_linear2.bias.grad}
    seen, failures = {}, []
    for name, value in got.items():
        ref = g['head/%d/%s' % (K, name)]
        sample = value.detach().double().reshape(-1)[::A23.STRIDE].cpu().numpy()
        assert sample.shape == ref.shape, name
        seen[name] = float(np.abs(sample - ref).max() / info['max'][name])
        bound = min(CAP, max(4 * MEASURED['head'][name], 4 * info['dev32'][name] / info['max'][name]))
        if seen[name] > bound:
            failures.append((name, seen[name], bound))
    print("det attr head K = %d: deviations %s" % (K, {k: float('%.3e' % v) for k, v in seen.items()}))
    assert not failures, failures


def _tiny_detector(e):
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
                              'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model'],
                              'model.det_module.dropout': 0.0, 'model.has_attr_head': True, 'model.num_attr_classes': e['num_attr_classes'],
                              'model.det_module.loss.attr_loss_coef': 1.0, 'optimizer.sp_names': ['attr_head']})
    model, criterion, _ = build_detector(cfg)
    deterministic_fill_(model)
    model.to(DEV).train()
    disable_drop_path(model)
    images, tg = D.end_to_end_batch(e['seed'], num_classes=e['num_classes'], counts=tuple(e['counts']))
    extra = A23.e2e_attributes(e['seed'], e['counts'], e['num_attr_classes'])
    targets = [{'labels': t(l, device=DEV), 'boxes': t(b, device=DEV), 'attributes': t(a, device=DEV), 'has_attr': f}
               for (l, b), (a, f) in zip(tg, extra)]
    return cfg, model, criterion, t(images, device=DEV), targets


def test_end_to_end_losses_match_reference(g23):
    from grit_amd.utils.misc import NestedTensor
    e = g23[1]['e2e']
    assert len(e['margins']) == 14 and min(e['margins']) >= 1e-2 and e['label_gap'] >= A23.HEAD_MARGIN
    _, model, criterion, images, targets = _tiny_detector(e)
    samples = NestedTensor(images, torch.zeros(images.shape[0], 224, 224, dtype=torch.bool, device=DEV))
    with torch.no_grad():
        outputs = model(samples)
        losses = criterion(outputs, targets)
        model.eval()
        assert tuple(model(samples)['attr_logits'].shape) == (2, e['num_queries'], e['num_attr_classes'])  # in evaluation as well
    assert tuple(outputs['attr_logits'].shape) == (2, e['num_queries'], e['num_attr_classes'])
    assert set(losses) == set(e['losses'])
    bad = {k: (float(losses[k]), ref) for k, ref in e['losses'].items() if abs(float(losses[k]) - ref) > 1e-4 * abs(ref)}
    total = sum(float(losses[k]) * criterion.weight_dict[k] for k in losses if k in criterion.weight_dict)
    print("det attr end to end: total %.6f (reference %.6f), loss_attr %.6f (%.6f)" % (total, e['total'], float(losses['loss_attr']), e['losses']['loss_attr']))
    assert not bad, bad
    assert abs(total - e['total']) <= 1e-4 * abs(e['total'])


@pytest.mark.parametrize("bf16", [False, True])
def test_train_step_moves_the_attribute_head(g23, bf16):
    from engine.det_engine import build_optimizers_schedulers, train_step
    from grit_amd.utils.misc import NestedTensor
    cfg, model, criterion, images, targets = _tiny_detector(g23[1]['e2e'])
    if bf16:
        from grit_amd.amp import Bf16Compute
        model = Bf16Compute(model)
    optimizers, _ = build_optimizers_schedulers(model, cfg)
    assert len(optimizers) == 2, "the head has its own optimizer (sp_names)"
    named = dict(model.named_master_parameters()) if bf16 else dict(model.named_parameters())
    head = {n: p for n, p in named.items() if 'attr_head.' in n}
    assert len(head) == 5
    before = {n: p.detach().clone() for n, p in head.items()}
    samples = NestedTensor(images, torch.zeros(images.shape[0], 224, 224, dtype=torch.bool, device=DEV))
    total, losses = train_step(model, criterion, optimizers, samples, targets, max_norm=0.1)
    assert 'loss_attr' in losses
    assert np.isfinite(float(total)) and all(np.isfinite(float(v)) for v in losses.values())
    for n, p in head.items():
        assert not torch.equal(p.detach(), before[n]), n
