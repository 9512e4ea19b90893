"""The attribute head of detector pre-training, the pieces that need no GPU: the host forms of grit_amd/ops/det_attr.py against the
reference (fixture G23, tests/golden/make_det_attr_golden.py), import path and state-dict keys, target packing, the ABI, the
refusals, the configuration and the captioner's start from a detector checkpoint that carries the head."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, deterministic_fill_, t

import det_attr_draws as A23  # tests/golden, put on the path by tests.helpers


@pytest.fixture(scope="module")
def g23():
    with np.load(os.path.join(GOLDEN, "det_attr_g23.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    return arrays, json.load(open(os.path.join(GOLDEN, "det_attr_g23.json")))


def _sample(a):
    return a.detach().double().reshape(-1)[::A23.STRIDE].numpy()


@pytest.mark.parametrize("K", A23.HEAD_KS)
def test_head_host_form_matches_reference(g23, K):
    from models.detection.heads import AttrHead
    g, meta = g23
    info = meta['head'][str(K)]
    assert info['margin'] >= A23.HEAD_MARGIN
    obj_h, logits, w = A23.head_inputs(info['seed'], K)
    assert A23.top_gap(logits) == info['margin']
    head = deterministic_fill_(AttrHead(A23.HEAD_D, A23.HEAD_A, K), 'g23.head.%d.' % K)
    with torch.no_grad():
        out32 = head(t(obj_h), t(logits))['attr_logits']
    assert np.abs(_sample(out32) - g['head/%d/attr_logits' % K]).max() <= 4 * info['dev32']['attr_logits']
    head = head.double()
    h, lg = t(obj_h).double().requires_grad_(True), t(logits).double().requires_grad_(True)
    out = head(h, lg)['attr_logits']
    (out * t(w).double()).sum().backward()
    assert lg.grad is None
    from grit_amd.ops.det_attr import attr_labels_host
    labels = attr_labels_host(t(logits))
    assert labels.numpy().tolist() == g['head/%d/labels' % K].tolist()
    chosen = np.unique(g['head/%d/labels' % K])
    rest = np.ones(K, bool)
    rest[chosen] = False
    dembed = head.od_cls_embed.weight.grad
    assert not bool(dembed[t(rest)].any())
    got = {'attr_logits': out, 'dobj_h': h.grad, 'dembed': dembed[t(chosen.astype(np.int64))],
           'dattr_linear1_weight': head.attr_linear1.weight.grad, 'dattr_linear1_bias': head.attr_linear1.bias.grad,
           'dattr_linear2_weight': head.attr_linear2.weight.grad, 'dattr_linear2_bias': head.attr_linear2.bias.grad}
    for name, value in got.items():
        ref = g['head/%d/%s' % (K, name)]
        assert np.abs(_sample(value) - ref).max() <= 1e-12 * info['max'][name], name


def test_labels_are_the_first_maximum_of_the_fp32_sigmoid():
    from grit_amd.ops.det_attr import attr_embed_cat_host
    logits = torch.full((2, 12), -3.0)
    logits[0, 3], logits[0, 9] = 19.0, 25.0  # both sigmoids are 1.0f: the first index wins
    logits[1, 5], logits[1, 7] = 2.0, 2.0
    weight = torch.arange(12 * 4, dtype=torch.float32).reshape(12, 4)
    obj = torch.randn(2, 4)
    cat, labels = attr_embed_cat_host(obj, logits, weight)
    assert labels.dtype == torch.int32 and labels.tolist() == [3, 5]
    assert torch.equal(cat[:, :4], obj) and torch.equal(cat[:, 4:], weight[[3, 5]])
    from grit_amd.ops.det_attr import attr_embed_grad_host
    dcat = torch.arange(3 * 8, dtype=torch.float32).reshape(3, 8)
    dweight = attr_embed_grad_host(dcat, torch.tensor([5, 3, 5], dtype=torch.int32), 12)
    assert tuple(dweight.shape) == (12, 4) and torch.equal(dweight[5], dcat[0, 4:] + dcat[2, 4:]) and torch.equal(dweight[3], dcat[1, 4:])
    assert not bool(dweight[[0, 1, 2, 4, 6, 7, 8, 9, 10, 11]].any())


@pytest.mark.parametrize("kind", A23.LOSS_KINDS)
def test_loss_host_form_matches_reference(g23, kind):
    from grit_amd.ops.det_attr import attr_loss_host
    g, meta = g23
    for A in A23.LOSS_AS:
        for Q in A23.LOSS_QS:
            info = meta['loss']['%s/%d/%d' % (kind, A, Q)]
            x, attrs, flags, pairs = A23.loss_case(kind, A, Q)
            counts = [len(a) for a in attrs]
            offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
            packed = t(np.concatenate(attrs + [np.zeros((1, A), np.uint8)]))
            lg = t(x).double().requires_grad_(True)
            loss = attr_loss_host(lg, packed, offsets, torch.tensor(flags), t(A23.match_t_of(pairs, Q)))
            loss.backward()
            loss = loss.detach()
            assert abs(float(loss) - info['loss64']) <= 1e-12 * max(abs(info['loss64']), 1.0)
            grad = lg.grad.numpy()
            assert abs(np.abs(grad).sum() - info['grad_abs_sum']) <= 1e-12 * max(info['grad_abs_sum'], 1.0)
            rows = [grad[b, q] for b, (f, (q, _)) in enumerate(zip(flags, pairs)) if f and len(q)]
            rows = np.concatenate(rows) if rows else np.zeros((0, A))
            ref = g['loss/%s/%d/%d/grad' % (kind, A, Q)]
            got = rows.reshape(-1)[::A23.STRIDE]
            assert got.shape == ref.shape
            if ref.size:
                assert np.abs(got - ref).max() <= 1e-12 * max(info['grad_max'], 1e-30)
            if kind == 'none':
                assert float(loss) == 0.0 and not grad.any()


def test_import_path_and_state_dict_keys(g23):
    import grit_amd.models.detection.heads as own
    import models.detection.heads as heads
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    assert heads is own
    head = heads.AttrHead(16, 7, 5)
    assert sorted(head.state_dict()) == ['attr_linear1.bias', 'attr_linear1.weight', 'attr_linear2.bias', 'attr_linear2.weight',
                                         'od_cls_embed.weight']
    assert head.od_cls_embed.weight.shape == (5, 16) and head.attr_linear1.weight.shape == (16, 32) and head.attr_linear2.weight.shape == (7, 16)
    e = g23[1]['e2e']
    over = {'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
            'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model']}
    plain = json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))['state_dict_keys']
    model, _, _ = build_detector(detection_config(**over))
    assert not model.has_attr_head and sorted(model.state_dict()) == plain
    cfg = detection_config(**dict(over, **{'model.has_attr_head': True, 'model.num_attr_classes': e['num_attr_classes']}))
    assert cfg.model.has_attr_head is True and cfg.model.num_attr_classes == e['num_attr_classes']
    assert detection_config().model.num_attr_classes == 400 and detection_config().model.has_attr_head is False
    model, criterion, _ = build_detector(cfg)
    keys = sorted(model.state_dict())
    assert keys == e['state_dict_keys']
    assert sorted(set(keys) - set(plain)) == ['attr_head.attr_linear1.bias', 'attr_head.attr_linear1.weight', 'attr_head.attr_linear2.bias',
                                              'attr_head.attr_linear2.weight', 'attr_head.od_cls_embed.weight']
    assert model.attr_head.od_cls_embed.weight.shape == (e['num_classes'], e['d_model'])
    assert model.attr_head.attr_linear2.weight.shape[0] == e['num_attr_classes']
    assert 'loss_attr' in criterion.weight_dict


def test_head_without_a_detection_module_is_refused():
    import models.detection.detector as det
    with pytest.raises(NotImplementedError, match="detection module"):
        det.Detector(None, None, has_attr_head=True)  # raised before `backbone` (None here) is touched


def test_packing_of_attributes_and_has_attr():
    from grit_amd.ops import det_loss
    cpu = torch.device('cpu')
    a0 = torch.tensor([[0, 1, 0], [2, 0, 0]], dtype=torch.int64)
    a2 = torch.tensor([[1.0, 0.0, 1.0]])
    targets = [{'attributes': a0, 'has_attr': True}, {'has_attr': torch.tensor(True)}, {'attributes': a2}, {}]
    attributes, has_attr = det_loss._pack_attributes(targets, [2, 3, 1, 0], cpu, None)
    assert attributes.dtype == torch.uint8 and tuple(attributes.shape) == (7, 3)
    assert attributes.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 1], [0, 0, 0]]
    assert has_attr.dtype == torch.bool and has_attr.tolist() == [True, True, False, False]
    attributes, has_attr = det_loss._pack_attributes([{}, {}], [2, 1], cpu, 5)  # neither key: zero rows, False
    assert tuple(attributes.shape) == (4, 5) and not attributes.any() and has_attr.tolist() == [False, False]
    attributes, has_attr = det_loss._pack_attributes([{'has_attr': False}], [2], cpu, None)
    assert attributes is None and has_attr.tolist() == [False]
    with pytest.raises(det_loss._lib.GritHipError, match="attribute classes"):
        det_loss._pack_attributes(targets, [2, 3, 1, 0], cpu, 4)
    with pytest.raises(det_loss._lib.GritHipError, match="attributes"):
        det_loss._pack_attributes([{'attributes': a0}], [3], cpu, None)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        det_loss.pack_targets([{'labels': torch.zeros(2, dtype=torch.long), 'boxes': torch.full((2, 4), 0.5), 'attributes': a0}])


def test_abi_version_and_symbols():
    from grit_amd import lib
    assert lib.ABI_VERSION >= 58
    names = ('grit_attr_embed_cat', 'grit_attr_embed_grad', 'grit_det_attr_fwd_f32', 'grit_det_attr_bwd_f32')
    dll = ctypes.CDLL(lib.LIB_PATH)
    for name in names:
        assert name in lib.SIGNATURES and hasattr(dll, name), name
    assert len(lib.SIGNATURES['grit_attr_embed_cat']) == 11 and len(lib.SIGNATURES['grit_attr_embed_grad']) == 10
    assert len(lib.SIGNATURES['grit_det_attr_fwd_f32']) == 14 and len(lib.SIGNATURES['grit_det_attr_bwd_f32']) == 12
    assert dll.grit_abi_version() == lib.ABI_VERSION


def test_cpu_tensors_are_rejected_by_the_loss():
    from grit_amd.ops import det_attr
    from models.detection.od_losses import HungarianMatcher, SetCriterion
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        det_attr.attr_loss(torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        det_attr.embed_cat(torch.zeros(4, 8), torch.zeros(4, 3), torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        det_attr.embed_grad(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int32), 3)
    out = {'pred_logits': torch.zeros(1, 4, 5), 'pred_boxes': torch.full((1, 4, 4), 0.5), 'attr_logits': torch.zeros(1, 4, 3)}
    tg = [{'labels': torch.zeros(2, dtype=torch.long), 'boxes': torch.full((2, 4), 0.5), 'attributes': torch.zeros(2, 3), 'has_attr': True}]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        SetCriterion(5, HungarianMatcher(2, 5, 2), {}, ['labels'])(out, tg)


def test_synthetic_attribute_targets():
    from train_detector import add_synthetic_attributes
    g = torch.Generator().manual_seed(3)
    targets = [{'labels': torch.zeros(n, dtype=torch.long)} for n in (40, 7, 25, 1)]
    add_synthetic_attributes(g, targets, 400, 'cpu')
    assert [t['has_attr'] for t in targets] == [True, False, True, False]
    for t_, n in zip(targets, (40, 7, 25, 1)):
        assert ('attributes' in t_) == t_['has_attr']
        if t_['has_attr']:
            assert t_['attributes'].dtype == torch.uint8 and tuple(t_['attributes'].shape) == (n, 400)
    share = float(torch.cat([t_['attributes'] for t_ in targets[::2]]).float().mean())
    assert 0.01 < share < 0.03
    again = [{'labels': torch.zeros(n, dtype=torch.long)} for n in (40, 7, 25, 1)]
    add_synthetic_attributes(torch.Generator().manual_seed(3), again, 400, 'cpu')
    assert all(torch.equal(a['attributes'], b['attributes']) for a, b in zip(targets[::2], again[::2]))


def test_captioner_detector_skips_the_attribute_head_of_a_checkpoint(tmp_path):
    """The captioner starts from the pre-trained detector's checkpoint (models/caption/detector.py build_detector); one made with the
    attribute head carries attr_head.* keys the captioner has no module for: they are skipped, everything else is loaded."""
    from grit_amd.config import default_config
    from grit_amd.models.caption.detector import build_detector
    path = str(tmp_path / "detector.pth")
    detector = build_detector(default_config())
    state = {k: v.clone() for k, v in detector.state_dict().items()}
    marked = 'det_module.query_embed.weight'
    state[marked] = torch.full_like(state[marked], 0.125)
    state['attr_head.od_cls_embed.weight'] = torch.zeros(1849, 512)
    for name, shape in (('attr_linear1', (512, 1024)), ('attr_linear2', (400, 512))):
        state['attr_head.%s.weight' % name] = torch.zeros(shape)
        state['attr_head.%s.bias' % name] = torch.zeros(shape[0])
    torch.save({'model': state}, path)
    loaded = build_detector(default_config(**{'model.detector.checkpoint': path}))
    assert not hasattr(loaded, 'attr_head')
    assert bool((loaded.state_dict()[marked] == 0.125).all())
    assert not any(k.startswith('attr_head') for k in loaded.state_dict())
