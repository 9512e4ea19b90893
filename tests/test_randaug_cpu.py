"""RandAugment, host side: the plan drawn from `random` equals what the reference's class did (fixture G17, made by
tests/golden/make_randaug_golden.py), the descriptor the device reads holds Pillow's integers, and the numpy model the GPU
tests compare with (tests/randaug_model.py) equals G17 and Pillow."""
import os
import pickle
import random

import numpy as np
import pytest

from grit_amd.datasets.caption.transforms import Deferred, MaxWHResize, RandAugment, augment_list, get_transform
from grit_amd.ops import image_batch as ib
from tests import randaug_model as model

CANVASES = [((48, 64), 0, 16), ((96, 128), 16, 24)]


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "randaug_g17.npz"))


def fixture_plan(g, i):
    return tuple((str(g['names'][i, k]), float(g['values'][i, k]), bool(g['negate'][i, k])) for k in range(4))


def test_plans_equal_the_reference_draws(g17):
    random.seed(int(g17['seed']))
    augment = RandAugment()
    policy = MaxWHResize((48, 64))
    for i in range(int(g17['count'])):
        item = augment(policy(g17['in%d' % i]))
        assert isinstance(item, Deferred) and item.pixels is not None
        assert item.augment == fixture_plan(g17, i), i  # names, magnitudes (exact doubles) and signs, in order
    assert random.random() == float(g17['next_random'])  # the same number of draws was consumed


def test_plan_is_plain_data_and_survives_pickle(g17):
    random.seed(3)
    item = RandAugment()(MaxWHResize((48, 64))(g17['in0']))
    assert all(type(n) is str and type(v) is float and type(s) is bool for n, v, s in item.augment)
    back = pickle.loads(pickle.dumps(item))
    assert back.augment == item.augment and back.size == item.size and np.array_equal(back.pixels, item.pixels)
    assert MaxWHResize((48, 64))(g17['in0']).augment is None
    with pytest.raises(TypeError):
        RandAugment()(g17['in0'])  # augmentation follows the resize
    with pytest.raises(ValueError):
        RandAugment()(item)


def test_augment_list_is_the_reference_table():
    assert augment_list() == [('Identity', 0, 100), ('AutoContrast', 0, 100), ('Rotate', 0, 8), ('Color', 0.5, 1.5),
                              ('Contrast', 0.5, 1.5), ('Brightness', 0.5, 1.5), ('Sharpness', 0.5, 1.5), ('ShearX', 0.0, 0.12),
                              ('ShearY', 0.0, 0.12), ('TranslateXabs', 0.0, 80), ('TranslateYabs', 0.0, 80)]
    assert RandAugment().n_augments == 4


def test_get_transform_entries():
    class Cfg(object):
        size, resize_name, randaug = (48, 64), 'maxwh', 'device'

    t = get_transform(Cfg())
    assert sorted(t) == ['train', 'valid']
    img = np.zeros((60, 80, 3), np.uint8)
    train, valid = t['train'](img), t['valid'](img)
    assert train.size == valid.size == (48, 64) and valid.augment is None and len(train.augment) == 4
    Cfg.randaug = True
    with pytest.raises(NotImplementedError, match="'device'"):
        get_transform(Cfg())
    Cfg.randaug = False
    t = get_transform(Cfg())
    assert t['train'] is t['valid'] and t['train'](img).augment is None


def test_descriptor_hand_checked_cases():
    # shear by 0: Pillow takes the table walk (a1 == a3 == 0), both tables are the identity
    aug, extra, n_stages, work = ib.plan_augment([(5, 7)], [(('ShearX', 0.0, False),)], table_base=10)
    assert n_stages == 1 and work == 5 * ib.tmp_pitch(7) == 5 * 24
    assert aug[0, :2].tolist() == [0, 1] and aug[0, 4:7].tolist() == [ib.AUG_AFFINE_TABLE, 10, 17]
    assert extra.tolist() == list(range(7)) + list(range(5))
    # translation to the left by more than the width: xo = -9 + 0.5 < 0 for every column -> all outside
    aug, extra, n_stages, _ = ib.plan_augment([(3, 4)], [(('TranslateXabs', 9.0, True),)])
    assert extra[:4].tolist() == [-1, -1, -1, -1] and extra[4:].tolist() == [0, 1, 2]
    # to the right by 2.5: xo = 3.0, 4.0, ... -> indices 3, 4, 5, 6 of which only 3 exists in a width of 4
    assert ib.affine_axis_table(2.5, 1.0, 4).tolist() == [3, 4, 5, 6]
    assert ib.affine_axis_table(-0.75, 1.0, 3).tolist() == [-1, 0, 1]  # -0.25 < 0 -> -1, then int(0.75), int(1.75)
    # rotate by 0.0 is Pillow's copy, Identity changes nothing: neither takes a stage
    aug, extra, n_stages, _ = ib.plan_augment([(3, 4), (3, 4)], [(('Rotate', 0.0, True), ('Identity', 55.0, False)), ()])
    assert n_stages == 0 and extra.size == 0 and not aug[:, 1:].any() and aug[:, 0].tolist() == [0, 3 * 12]
    # shear x by 0.5 on 4 x 4: A = FIX(1), FIX(.5), FIX(0 + .5 + .25), 0, FIX(1), FIX(.5)
    assert ib.affine_fixed((1, 0.5, 0, 0, 1, 0), 4, 4) == (65536, 32768, 49152, 0, 65536, 32768)
    aug, _, _, _ = ib.plan_augment([(4, 4)], [(('ShearX', 0.5, True), ('Brightness', 1.5, False), ('AutoContrast', 7.0, False))])
    assert aug[0, 4:11].tolist() == [ib.AUG_AFFINE_FIXED, 65536, -32768, 16384, 0, 65536, 32768]
    assert aug[0, 12:14].tolist() == [6, 0x3fc00000] and aug[0, 20] == ib.AUG_AUTOCONTRAST and aug[0, 1] == 3
    # rotate by 90 degrees about the centre of a 4 x 4 image: cos rounds to 0, sin to 1 (r = -pi/2 -> sin = -1)
    a = ib.affine_coefficients('Rotate', 90.0, 4, 4)
    assert a == (0.0, -1.0, 4.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        ib.plan_augment([(4, 4)], [(('Identity', 0.0, False),) * 5])
    with pytest.raises(ValueError):
        ib.affine_fixed((1, 0.5, 40000.0, 0, 1, 0), 4, 4)


def test_model_chains_equal_g17_from_pillow_resize(g17):
    """The model applied to the reference's RESIZED image must give the reference's augmented image: the resized image is
    recovered without Pillow from the bicubic C oracle (bit-exact, fixture G11's bar)."""
    from oracle import image as oimg
    for (canvas, lo, hi) in CANVASES:
        policy = MaxWHResize(canvas)
        for i in range(lo, hi):
            src = g17['in%d' % i]
            size = policy.output_size(*src.shape[:2])
            resized = oimg.resize_bicubic(src, *size)
            np.testing.assert_array_equal(model.chain(resized, fixture_plan(g17, i)), g17['u8_%d' % i], err_msg=str(i))


SIZES = [(384, 640), (1, 1), (1, 5), (2, 2), (3, 3), (2, 7), (3, 1), (5, 7), (48, 63), (97, 130)]


def _images(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([40 + x * 150 // max(w - 1, 1), 20 + y * 200 // max(h - 1, 1), np.full((h, w), 77)], -1).astype(np.uint8)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), smooth]  # noise; ramps with a constant channel


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_model_equals_pillow_per_operation(size):
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance, ImageOps = pytest.importorskip("PIL.ImageEnhance"), pytest.importorskip("PIL.ImageOps")
    rng = np.random.default_rng(size[0] * 1000 + size[1])

    def pillow(img, name, v):  # the published Pillow calls behind each operation name
        if name == 'Identity':
            return img
        if name == 'AutoContrast':
            return ImageOps.autocontrast(img)
        if name == 'Rotate':
            return img.rotate(v)
        if name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
            return getattr(ImageEnhance, name)(img).enhance(v)
        a = {'ShearX': (1, v, 0, 0, 1, 0), 'ShearY': (1, 0, 0, v, 1, 0), 'TranslateXabs': (1, 0, v, 0, 1, 0),
             'TranslateYabs': (1, 0, 0, 0, 1, v)}[name]
        return img.transform(img.size, Image.AFFINE, a)

    for arr in _images(rng, *size):
        img = Image.fromarray(arr, 'RGB')
        for name, lo, hi in augment_list():
            values = [lo, hi, (lo + hi) / 2, lo + (hi - lo) * 0.137]
            if lo == 0.5:
                values += [0.5, 1.0, 1.5, 0.0, 1.9]
            for val in values:
                for negate in ((False, True) if name in model.GEOMETRIC else (False,)):
                    want = np.asarray(pillow(img, name, -val if negate else val))
                    np.testing.assert_array_equal(model.apply(arr, name, val, negate), want, err_msg="%s %r %s" % (name, val, negate))


def test_entry_point_rejects_bad_arguments_before_any_device_work():
    import ctypes
    from grit_amd import lib as _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()  # any non-null, 16-byte aligned address: bad arguments return before it is used
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    good = dict(n_stages=4, work_bytes=64, batch=1, max_src_h=4, max_dst_h=4, max_dst_w=4, max_kx=5, out_h=4, out_w=4)

    def call(null=None, **over):
        a = dict(good, **over)
        ptrs = {k: (None if k == null else p) for k in ('src', 'desc', 'tables', 'tmp', 'lut', 'aug', 'work', 'stats', 'out', 'mask')}
        return lib.grit_image_batch_aug_fwd(ptrs['src'], ptrs['desc'], ptrs['tables'], ptrs['tmp'], ptrs['lut'], ptrs['aug'],
                                            a['n_stages'], ptrs['work'], a['work_bytes'], ptrs['stats'], a['batch'], a['max_src_h'],
                                            a['max_dst_h'], a['max_dst_w'], a['max_kx'], a['out_h'], a['out_w'], ptrs['out'],
                                            ptrs['mask'], None)

    for name in ('src', 'desc', 'tables', 'tmp', 'lut', 'aug', 'work', 'stats', 'out', 'mask'):
        assert call(null=name) == _lib.ERR_BAD_ARG, name
    for over in (dict(n_stages=5), dict(n_stages=-1), dict(work_bytes=0), dict(work_bytes=6), dict(batch=0), dict(max_dst_w=5),
                 dict(max_dst_h=5), dict(max_kx=0)):
        assert call(**over) == _lib.ERR_BAD_ARG, over
    assert call(max_dst_w=40000, out_w=40000) == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GritHipError, match="Not implemented on the CPU"):
        ib.image_batch([np.zeros((4, 4, 3), np.uint8)], [(2, 2)], device='cpu', augment=[()])
