"""The detector's input pipeline on the host: the transforms' draws and targets against fixture G20 (the reference's classes on
Pillow and torch), the bilinear tap tables, the numpy model the GPU tests use, the folding of a plan into descriptors, and the
argument checks of the entry point.  No GPU."""
import ctypes
import os
import pickle
import random

import numpy as np
import pytest
import torch

from grit_amd import lib as _lib
from grit_amd.datasets.detection import transforms as T
from grit_amd.ops import image_batch as ib
from tests import det_transforms_model as model

TARGET_KEYS = ('boxes', 'labels', 'area', 'iscrowd', 'attributes', 'size', 'orig_size')
SMALL = [48, 56, 64]


def small_recipe():
    return T.Compose([T.RandomHorizontalFlip(),
                      T.RandomSelect(T.RandomResize(SMALL, max_size=100),
                                     T.Compose([T.RandomRatioResize((0.5, 1.5)), T.RandomSizeCrop(24, 60), T.RandomResize(SMALL, max_size=100)])),
                      T.Compose([T.ToTensor(), T.Normalize(list(ib.MEAN), list(ib.STD))])])


def steps_of(plan):
    rows = [{'hflip': (0, 0, 0, 0, 0), 'resize': (1,) + tuple(op[1:]) + (0, 0), 'crop': (2,) + tuple(op[1:])}[op[0]] for op in plan]
    return np.asarray(rows, np.int64).reshape(-1, 5)


def plan_of(steps):
    return tuple([('hflip',), ('resize', a, b), ('crop', a, b, c, d)][code] for code, a, b, c, d in steps.tolist())


def target_in(g, i):
    return {k: torch.from_numpy(g['in%d_%s' % (i, k)]) for k in TARGET_KEYS}


def replay_pixels(g):
    """The pixel part of G20 through our transforms, after the fixture's seeds: [(record, target)]."""
    random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    recipe = small_recipe()
    return [recipe(g['in%d' % i], target_in(g, i)) for i in range(int(g['count']))]


def vg_targets(g):
    offs = np.concatenate([[0], np.cumsum(g['vg_in_counts'])])
    return [{k: torch.from_numpy(g['vg_in_' + k][i] if k in ('size', 'orig_size') else g['vg_in_' + k][offs[i]:offs[i + 1]])
             for k in TARGET_KEYS} for i in range(len(g['vg_sizes']))]


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "det_transforms_g20.npz"))


def test_g20_plans_targets_and_draws(g20):
    g = g20
    for i, (record, target) in enumerate(replay_pixels(g)):
        np.testing.assert_array_equal(steps_of(record.plan), g['steps%d' % i], err_msg="image %d" % i)
        assert record.size == g['u8_%d' % i].shape[1::-1] and record.to_tensor and record.normalize == (ib.MEAN, ib.STD)
        assert set(target) == set(TARGET_KEYS)
        for k in TARGET_KEYS:
            want = torch.from_numpy(g['out%d_%s' % (i, k)])
            assert target[k].dtype == want.dtype and torch.equal(target[k], want), "image %d, %s" % (i, k)
        pickle.loads(pickle.dumps(record))
    # the draws at full size, through the real recipes; pixels are never touched: the "image" is a shape
    sizes, targets = g['vg_sizes'].tolist(), vg_targets(g)
    starts, offs, n = g['vg_starts'], np.concatenate([[0], np.cumsum(g['vg_counts'])]), 0
    for split, phase in (('train', 'train'), ('train', 'pretrain-od'), ('valid', 'train')):
        recipe = T.make_transforms(split, phase)
        for (w, h), tgt in zip(sizes, targets):
            record, target = recipe(T.Planned(np.broadcast_to(np.uint8(0), (h, w, 3))), tgt)
            np.testing.assert_array_equal(steps_of(record.plan), g['vg_steps'][starts[n]:starts[n + 1]], err_msg="%s %s item %d" % (split, phase, n))
            for k in TARGET_KEYS:
                want = g['vg_out_' + k][n] if k in ('size', 'orig_size') else g['vg_out_' + k][offs[n]:offs[n + 1]]
                assert torch.equal(target[k], torch.from_numpy(want)), "%s %s item %d, %s" % (split, phase, n, k)
            n += 1
    assert n == len(starts) - 1
    assert random.random() == float(g['next_random'])
    assert int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) == int(g['next_randint'])


def test_model_reproduces_g20_pixels(g20):
    g = g20
    for i in range(int(g['count'])):
        plan = plan_of(g['steps%d' % i])
        np.testing.assert_array_equal(model.chain(g['in%d' % i], plan), g['u8_%d' % i], err_msg="image %d" % i)
        np.testing.assert_array_equal(model.chain_folded(g['in%d' % i], plan), g['u8_%d' % i], err_msg="image %d, folded" % i)
    # ToTensor / Normalize / padding as the GPU tests build them
    for b in range(int(g['count']) // 5):
        want, mask = g['tensors_b%d' % b], g['mask_b%d' % b]
        for k in range(5):
            u8 = g['u8_%d' % (5 * b + k)]
            h, w = u8.shape[:2]
            np.testing.assert_array_equal(model.normalized(u8, ib.MEAN, ib.STD), want[k, :, :h, :w])
            assert not mask[k, :h, :w].any() and mask[k].sum() == mask[k].size - h * w
            assert not want[k, :, h:].any() and not want[k, :, :, w:].any()


def test_model_reproduces_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (57, 83, 3), dtype=np.uint8)
    pil = Image.fromarray(img, 'RGB')
    flip = lambda p: p.transpose(Image.FLIP_LEFT_RIGHT)
    cases = [((('hflip',), ('resize', 40, 61)), flip(pil).resize((61, 40), Image.BILINEAR)),
             ((('hflip',), ('resize', 90, 200)), flip(pil).resize((200, 90), Image.BILINEAR)),
             ((('crop', 5, 7, 41, 30), ('resize', 64, 50)), pil.crop((7, 5, 37, 46)).resize((50, 64), Image.BILINEAR)),
             ((('resize', 70, 90), ('crop', 3, 5, 50, 61), ('resize', 33, 47)),
              pil.resize((90, 70), Image.BILINEAR).crop((5, 3, 66, 53)).resize((47, 33), Image.BILINEAR)),
             ((('hflip',), ('resize', 70, 90), ('crop', 20, 29, 50, 61), ('hflip',), ('resize', 9, 300)),
              flip(flip(pil).resize((90, 70), Image.BILINEAR).crop((29, 20, 90, 70))).resize((300, 9), Image.BILINEAR)),
             ((('resize', 57, 20),), pil.resize((20, 57), Image.BILINEAR)),
             ((('hflip',), ('crop', 0, 50, 57, 33)), flip(pil).crop((50, 0, 83, 57)))]
    for plan, want in cases:
        np.testing.assert_array_equal(model.chain(img, plan), np.asarray(want), err_msg=str(plan))
        np.testing.assert_array_equal(model.chain_folded(img, plan), np.asarray(want), err_msg="folded " + str(plan))


@pytest.mark.parametrize("pair", [(1, 9), (9, 1), (1, 1), (13, 13), (7, 8), (8, 7), (100, 13), (37, 61), (150, 60), (230, 60), (260, 60),
                                  (400, 60), (30, 97), (375, 800), (1333, 200)], ids=lambda p: "%d_%d" % p)
def test_bilinear_taps_equal_the_model(pair):
    ksize, bounds, taps = ib.axis_taps(pair[0], pair[1], 'bilinear')
    want = model.taps(*pair)
    assert ksize == want[0] and bounds.dtype == np.int32 and taps.dtype == np.int32
    np.testing.assert_array_equal(bounds, want[1])
    np.testing.assert_array_equal(taps, want[2])
    if pair[0] == pair[1]:  # an unchanged axis is the identity tap
        assert (taps[:, 0] == 1 << 22).all() and not taps[:, 1:].any() and (bounds[:, 0] == np.arange(pair[0])).all()
    _, mb, mt = ib.mirrored_taps(pair[0], pair[1], 'bilinear')
    np.testing.assert_array_equal(mb, model.mirrored(*pair)[1])
    np.testing.assert_array_equal(mt, model.mirrored(*pair)[2])


def test_axis_taps_default_is_bicubic():
    assert ib.axis_taps(50, 20)[0] == ib.axis_taps(50, 20, 'bicubic')[0] == 11 and ib.axis_taps(50, 20, 'bilinear')[0] == 7
    assert ib.axis_taps(50, 20) is ib.axis_taps(50, 20)  # the two-argument cache key still hits
    with pytest.raises(ValueError):
        ib.axis_taps(50, 20, 'lanczos')
    lib = _lib.load()
    assert lib.grit_resample_taps_bilinear(0, 5, None, None, 0) == -_lib.ERR_BAD_ARG
    small = np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.grit_resample_taps_bilinear(8, 4, p(small), p(small), 4) == -_lib.ERR_BAD_ARG  # capacity below 4 * 5


def record(geo, which):
    keys = ('buf', 'off', 'pitch', 'src_h', 'dst_h', 'dst_w', 'kx', 'ky', 'xb_off', 'xt_off', 'yb_off', 'yt_off', 'tmp_off', 'out_off')
    return dict(zip(keys, geo[2 + 14 * which:16 + 14 * which].tolist()))


def table(p, off, rows, cols):
    return p.tables[off:off + rows * cols].reshape(rows, cols)


def test_plan_geo_descriptors():
    # a flip alone: one identity resize whose x taps are mirrored, second image of the blob
    p = ib.plan_geo([(4, 6), (5, 7)], [(), (('hflip',),)])
    assert p.geo.shape == (2, ib.GEO_FIELDS) and p.geo[:, 0].tolist() == [1, 1] and not p.geo[:, 2:16].any()
    assert p.src_offsets == [0, 72] and p.src_bytes == 72 + 105 and p.sizes == [(4, 6), (5, 7)] and p.work_bytes == 0
    assert p.a_max == (0, 0, 0, 0) and p.b_max == (5, 5, 7, 3)
    r = record(p.geo[1], 1)
    assert (r['buf'], r['off'], r['pitch'], r['src_h'], r['dst_h'], r['dst_w'], r['kx'], r['ky']) == (0, 72, 21, 5, 5, 7, 3, 3)
    assert r['tmp_off'] == 4 * 20 and p.tmp_bytes == 4 * 20 + 5 * 24 and r['out_off'] == 0
    assert table(p, r['xb_off'], 7, 2).tolist() == [[6 - x, 1] if x == 6 else [5 - x, 2] for x in range(7)]  # first' = w - first - count
    assert table(p, r['xt_off'], 7, 3).tolist() == [[1 << 22, 0, 0] if x == 6 else [0, 1 << 22, 0] for x in range(7)]
    assert table(p, r['yb_off'], 5, 2)[:, 0].tolist() == [0, 1, 2, 3, 4]
    # a crop at an odd offset, then a resize: the window starts at byte 3 * (2 * 11 + 3) and its rows stay 33 bytes apart
    p = ib.plan_geo([(9, 11)], [(('crop', 2, 3, 5, 7), ('resize', 10, 14))])
    r = record(p.geo[0], 1)
    assert (r['buf'], r['off'], r['pitch'], r['src_h'], r['dst_h'], r['dst_w']) == (0, 75, 33, 5, 10, 14)
    assert np.array_equal(table(p, r['xb_off'], 14, 2), model.taps(7, 14)[1]) and np.array_equal(table(p, r['yt_off'], 10, 3), model.taps(5, 10)[2])
    # the same crop inside a flip counts its left edge from the right: columns 11 - 3 - 7 = 1 .. 7 of the stored rows
    p = ib.plan_geo([(9, 11)], [(('hflip',), ('crop', 2, 3, 5, 7), ('resize', 10, 14))])
    r = record(p.geo[0], 1)
    assert r['off'] == 3 * (2 * 11 + 1) and np.array_equal(table(p, r['xt_off'], 14, 3), model.mirrored(7, 14)[2])
    # two resizes: A (8 x 10 -> 16 x 21, pitch 64 in the work buffer), B reads rows 3 .. 12, columns 5 .. 16 of A's result
    p = ib.plan_geo([(8, 10)], [(('resize', 16, 21), ('crop', 3, 5, 10, 12), ('hflip',), ('resize', 7, 9))])
    a, b = record(p.geo[0], 0), record(p.geo[0], 1)
    assert p.geo[0, 0] == 2 and p.a_max == (8, 16, 21, 3) and p.b_max == (10, 7, 9, 5) and p.sizes == [(7, 9)]
    assert (a['buf'], a['off'], a['pitch'], a['src_h'], a['dst_h'], a['dst_w'], a['tmp_off'], a['out_off']) == (0, 0, 30, 8, 16, 21, 0, 0)
    assert (b['buf'], b['off'], b['pitch'], b['src_h'], b['dst_h'], b['dst_w'], b['tmp_off']) == (1, 3 * 64 + 15, 64, 10, 7, 9, 8 * 64)
    assert p.work_bytes == 16 * 64 and p.tmp_bytes == 8 * 64 + 10 * 28
    assert np.array_equal(table(p, b['xb_off'], 9, 2), model.mirrored(12, 9)[1])
    assert all(record(p.geo[0], w)[k] % 2 == 0 for w in (0, 1) for k in ('xb_off', 'xt_off', 'yb_off', 'yt_off'))


def test_plan_geo_rejects_what_it_cannot_fold():
    with pytest.raises(ValueError, match="at most two resizes"):
        ib.plan_geo([(8, 10)], [(('resize', 4, 4), ('resize', 5, 5), ('resize', 6, 6))])
    with pytest.raises(ValueError, match="at most two resizes"):
        ib.plan_geo([(8, 10)], [(('resize', 4, 4), ('resize', 5, 5), ('hflip',))])
    for bad in (('crop', 0, 4, 8, 7), ('crop', 1, 0, 8, 10), ('crop', -1, 0, 4, 4), ('crop', 0, 0, 0, 4)):
        with pytest.raises(ValueError, match="crop"):
            ib.plan_geo([(8, 10)], [(bad,)])
    with pytest.raises(ValueError, match="crop"):
        ib.plan_geo([(8, 10)], [(('resize', 4, 5), ('crop', 0, 0, 5, 5))])  # outside the CURRENT image
    with pytest.raises(ValueError):
        ib.plan_geo([(8, 10)], [(('rotate', 3),)])


def test_cpu_tensors_and_unsupported_transforms_raise():
    with pytest.raises(_lib.GritHipError, match="Not implemented on the CPU"):
        ib.image_batch_geo([np.zeros((4, 4, 3), np.uint8)], [()], device='cpu')
    item = T.make_transforms('valid', 'train')(np.zeros((6, 8, 3), np.uint8), {'boxes': torch.zeros(0, 4), 'labels': torch.zeros(0, dtype=torch.int64)})
    with pytest.raises(_lib.GritHipError, match="Not implemented on the CPU"):
        T.collate_detection([item], device='cpu')
    with pytest.raises(TypeError):
        T.collate_detection([(T.Planned(np.zeros((6, 8, 3), np.uint8)), {})], device='cpu')  # no ToTensor / Normalize
    for make in (lambda: T.PadOrCrop((448, 448)), lambda: T.RandomPad(10), lambda: T.RandomErasing(), lambda: T.pad(None, None, (1, 1))):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(NotImplementedError, match="masks"):
        T.hflip(np.zeros((6, 8, 3), np.uint8), {'masks': torch.zeros(1, 6, 8)})
    with pytest.raises(ValueError):
        T.make_transforms('test', 'train')
    for phase in ('train', 'finetune', 'pretrain-od', 'pretrain-vl'):
        for split in ('train', 'valid'):
            assert isinstance(T.make_transforms(split, phase), T.Compose)


def test_crop_classes_follow_torchvision():
    img = np.zeros((20, 30, 3), np.uint8)
    tgt = {'boxes': torch.tensor([[2., 3., 12., 13.], [25., 1., 29., 4.]]), 'labels': torch.tensor([4, 5])}
    record, out = T.CenterCrop((10, 16))(img, tgt)
    assert record.plan == (('crop', 5, 7, 10, 16),) and out['boxes'].tolist() == [[0., 0., 5., 8.]] and out['labels'].tolist() == [4]
    state = torch.get_rng_state()
    assert T.RandomCrop((20, 30))(img, tgt)[0].plan == (('crop', 0, 0, 20, 30),) and torch.equal(state, torch.get_rng_state())
    torch.manual_seed(5)
    i, j = int(torch.randint(0, 20 - 7 + 1, (1,))), int(torch.randint(0, 30 - 9 + 1, (1,)))
    torch.manual_seed(5)
    assert T.RandomCrop((7, 9))(img, tgt)[0].plan == (('crop', i, j, 7, 9),)


def test_normal_policy_is_a_bilinear_fixed_resize():
    from grit_amd.datasets.caption.transforms import Deferred, FixedResize, collate_images, get_transform

    class Cfg(object):
        size, resize_name, randaug = (48, 64), 'normal', False

    policy = get_transform(Cfg())['train']
    assert isinstance(policy, FixedResize) and policy.filter == 'bilinear'
    item = policy(np.zeros((60, 80, 3), np.uint8))
    assert item.size == (48, 64) and item.filter == 'bilinear' and Deferred(None, (1, 1)).filter == 'bicubic'
    Cfg.resize_name = 'maxwh'
    assert get_transform(Cfg())['train'](np.zeros((60, 80, 3), np.uint8)).filter == 'bicubic'
    Cfg.resize_name, Cfg.size = 'normal', 48
    with pytest.raises(ValueError, match="pair"):
        get_transform(Cfg())
    with pytest.raises(_lib.GritHipError, match="Not implemented on the CPU"):
        collate_images([item], device='cpu')


def test_entry_point_checks_arguments_before_any_device_work():
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    P = ctypes.c_void_p
    good = dict(src=base, geo=base + 256, tables=base + 512, tmp=base + 768, work=base + 1024, lut=base + 1280, out=base + 1536, mask=base + 1792)

    def call(a_src_h=0, b_src_h=4, b_dst_w=4, out_w=4, batch=1, **over):
        a = dict(good, **over)
        return lib.grit_image_batch_geo_fwd(P(a['src']), P(a['geo']), P(a['tables']), P(a['tmp']), P(a['work']), P(a['lut']), batch,
                                            a_src_h, 4 if a_src_h else 0, 4 if a_src_h else 0, 3 if a_src_h else 0, b_src_h, b_dst_w, 3,
                                            4, out_w, P(a['out']), P(a['mask']), None)

    for name in ('src', 'geo', 'tables', 'tmp', 'lut', 'out', 'mask'):
        assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
    assert call(a_src_h=4, work=None) == _lib.ERR_BAD_ARG  # two-resize images need the work buffer
    for name in ('src', 'tmp', 'work', 'geo'):
        assert call(**{name: good[name] + 1}) == _lib.ERR_BAD_ARG, name
    assert call(geo=good['geo'] + 4) == _lib.ERR_BAD_ARG
    assert call(batch=0) == _lib.ERR_BAD_ARG and call(b_src_h=0) == _lib.ERR_BAD_ARG and call(b_dst_w=5) == _lib.ERR_BAD_ARG
    assert call(a_src_h=-1) == _lib.ERR_BAD_ARG
    assert call(b_src_h=65536) == _lib.ERR_UNSUPPORTED and call(batch=65536) == _lib.ERR_UNSUPPORTED
