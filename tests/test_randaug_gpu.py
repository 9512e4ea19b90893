"""RandAugment on the device (grit_image_batch_aug_fwd through image_batch(..., augment=plans) and collate_images) against
fixture G17 (the reference's classes on Pillow) and, at sizes the fixture does not reach, the numpy model
tests/randaug_model.py on top of the bicubic C oracle.  Every comparison is bit-exact."""
import itertools
import os
import random

import numpy as np
import pytest
import torch

from grit_amd.datasets.caption.transforms import MaxWHResize, RandAugment, augment_list, collate_images
from grit_amd.ops.image_batch import MEAN, STD, image_batch
from oracle import image as oimg
from tests import randaug_model as model

pytestmark = pytest.mark.gpu

OPS = [(name, lo, hi) for name, lo, hi in augment_list() if name != 'Identity']


def expected(images, sizes, plans, pad_to=None):
    """Oracle resize -> model chain -> ToTensor / Normalize with torch's float ops -> zero padding and mask."""
    H, W = pad_to if pad_to is not None else (max(s[0] for s in sizes), max(s[1] for s in sizes))
    mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]
    tensors, mask = torch.zeros(len(images), 3, H, W), torch.ones(len(images), H, W, dtype=torch.bool)
    for i, (img, (oh, ow), plan) in enumerate(zip(images, sizes, plans)):
        u8 = model.chain(oimg.resize_bicubic(np.asarray(img), oh, ow), plan)
        tensors[i, :, :oh, :ow] = torch.from_numpy(u8).permute(2, 0, 1).to(torch.float32).div(255).sub(mean).div(std)
        mask[i, :oh, :ow] = False
    return tensors.numpy(), mask.numpy()


def check(images, sizes, plans, pad_to=None, feed=None):
    want_t, want_m = expected(images, sizes, plans, pad_to)
    got_t, got_m = image_batch(images if feed is None else feed, sizes, device='cuda', pad_to=pad_to, augment=plans)
    np.testing.assert_array_equal(got_m.cpu().numpy(), want_m)
    got_t = got_t.cpu().numpy()
    for i in range(len(images)):  # per image, so that a failure names the plan
        np.testing.assert_array_equal(got_t[i], want_t[i], err_msg="image %d, plan %s" % (i, plans[i]))


def limited_noise(rng, h, w):
    """Noise that does not span 0..255, with a different range per channel (AutoContrast has something to do)."""
    return np.stack([rng.integers(lo, hi, (h, w), dtype=np.uint8) for lo, hi in ((30, 200), (0, 120), (77, 256))], -1)


def single_op_plans(rng):
    plans = []
    for name, lo, hi in OPS:
        for negate in ((False, True) if name in model.GEOMETRIC else (False,)):
            plans.append(((name, float(rng.uniform(lo, hi)), negate),))
            plans.append(((name, float(hi), negate),))
    plans += [(('Color', 0.5, False),), (('Sharpness', 1.0, False),), (('Contrast', 1.5, False),), (('Brightness', 1.0, False),),
              (('ShearX', 0.0, False),), (('Rotate', 0.0, True),), (('Identity', 3.0, False),), (('TranslateXabs', 0.25, True),)]
    return plans


def test_fixture_g17_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "randaug_g17.npz"))
    random.seed(int(g['seed']))
    augment = RandAugment()
    start = 0
    for canvas, count in (((48, 64), 16), ((96, 128), 8)):
        policy = MaxWHResize(canvas)
        items = [augment(policy(g['in%d' % i])) for i in range(start, start + count)]
        nt = collate_images(items, device='cuda')
        assert nt.tensors.dtype == torch.float32 and nt.mask.dtype == torch.bool
        np.testing.assert_array_equal(nt.mask.cpu().numpy(), g['mask_%dx%d' % canvas])
        got = nt.tensors.cpu().numpy()
        for k in range(count):
            np.testing.assert_array_equal(got[k], g['tensors_%dx%d' % canvas][k], err_msg="image %d: %s" % (start + k, items[k].augment))
        start += count
    assert random.random() == float(g['next_random'])


@pytest.mark.parametrize("size", [(384, 640), (37, 61), (50, 66), (1, 1), (1, 7), (2, 3), (3, 2), (3, 3), (5, 1), (4, 9)],
                         ids=lambda s: "%dx%d" % s)
def test_each_operation_alone(size):
    """Every operation, both signs, random and extreme magnitudes, on an image that is not resized (target = source size)."""
    rng = np.random.default_rng(100 + size[0] * 7 + size[1])
    plans = single_op_plans(rng)
    img = limited_noise(rng, *size)
    check([img] * len(plans), [size] * len(plans), plans)


@pytest.mark.parametrize("size", [(37, 61), (3, 3), (2, 5)], ids=lambda s: "%dx%d" % s)
def test_every_ordered_pair(size):
    """All 100 ordered pairs of the ten operations: the second one reads the first one's bytes, and the statistics of
    AutoContrast / Contrast in second place are gathered by the stage that runs the first."""
    rng = np.random.default_rng(200 + size[0])
    plans = []
    for (n1, lo1, hi1), (n2, lo2, hi2) in itertools.product(OPS, OPS):
        plans.append(((n1, float(rng.uniform(lo1, hi1)), bool(rng.integers(2))), (n2, float(rng.uniform(lo2, hi2)), bool(rng.integers(2)))))
    img = limited_noise(rng, *size)
    check([img] * len(plans), [size] * len(plans), plans)


def test_pairs_around_the_reductions_at_full_size():
    """384 x 640: every operation before and after AutoContrast and Contrast, geometric ones with either sign."""
    rng = np.random.default_rng(300)
    plans = []
    for name, lo, hi in OPS:
        for stat in ('AutoContrast', 'Contrast'):
            one = (name, float(rng.uniform(lo, hi)), bool(rng.integers(2)))
            two = (stat, float(rng.uniform(0.5, 1.5)), False)
            plans += [(one, two), (two, one)]
    img = limited_noise(rng, 384, 640)
    check([img] * len(plans), [(384, 640)] * len(plans), plans)


def test_autocontrast_table_exhaustive():
    """Every (lo, hi), 0 <= lo < hi <= 255: a one-row image holding lo..hi must come out as Python's
    int(i * scale + offset) with scale = 255.0 / (hi - lo), offset = -lo * scale -- a fused or reassociated fp64
    expression on the device would differ somewhere in these 32 640 tables."""
    pairs = [(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)]
    lut = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)[None, :].sub(torch.tensor(MEAN)[:, None]).div(torch.tensor(STD)[:, None]).numpy()
    plan = (('AutoContrast', 0.0, False),)
    for part in range(4):
        chunk = pairs[part::4]
        images = [np.repeat(np.arange(lo, hi + 1, dtype=np.uint8)[None, :, None], 3, 2) for lo, hi in chunk]
        sizes = [(1, im.shape[1]) for im in images]
        got, mask = image_batch(images, sizes, device='cuda', augment=[plan] * len(chunk))
        got, mask = got.cpu().numpy(), mask.cpu().numpy()
        for k, (lo, hi) in enumerate(chunk):
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = np.array([min(max(int(i * scale + offset), 0), 255) for i in range(lo, hi + 1)])
            n = hi - lo + 1
            assert not mask[k, 0, :n].any() and mask[k, 0, n:].all()
            np.testing.assert_array_equal(got[k, :, 0, :n], lut[:, want], err_msg="lo %d hi %d" % (lo, hi))


@pytest.mark.parametrize("on_device", [False, True])
def test_coco_like_ragged_batch_of_32(on_device):
    rng = np.random.default_rng(41)
    shapes = [(480, 640), (427, 640), (640, 480), (333, 500), (375, 500), (500, 375), (96, 128), (1200, 1600)] * 4
    images = [limited_noise(rng, *s) for s in shapes]
    policy = MaxWHResize((384, 640))
    sizes = [policy.output_size(*s) for s in shapes]
    random.seed(41)
    augment = RandAugment()
    plans = [augment.draw() for _ in shapes]
    feed = [torch.from_numpy(im).cuda() for im in images] if on_device else None
    check(images, sizes, plans, feed=feed)


def test_mixed_empty_and_full_plans_and_pad_to():
    rng = np.random.default_rng(42)
    images = [limited_noise(rng, 50, 70), limited_noise(rng, 80, 40), limited_noise(rng, 33, 47), limited_noise(rng, 64, 64)]
    sizes = [(40, 56), (64, 32), (33, 47), (21, 23)]
    random.seed(42)
    augment = RandAugment()
    plans = [augment.draw(), (), (('Contrast', 1.3, False),), augment.draw()]
    check(images, sizes, plans)
    check(images, sizes, plans, pad_to=(96, 101))  # odd canvas width: scalar stores of the last stage
    check(images, sizes, plans, pad_to=(64, 56))
    with pytest.raises(ValueError):
        image_batch(images, sizes, device='cuda', augment=plans[:3])


def test_no_plans_equal_the_plain_path():
    """augment=None takes today's two launches; all-empty plans take the augmented entry point with zero stages: same bytes."""
    rng = np.random.default_rng(43)
    shapes = [(480, 640), (640, 427), (96, 128), (7, 5)]
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    sizes = [MaxWHResize((384, 640)).output_size(*s) for s in shapes]
    want_t, want_m = oimg.image_batch(images, sizes)
    for kwargs in ({}, {'augment': None}, {'augment': [()] * 4}, {'augment': [(('Identity', 1.0, False),)] * 4}):
        got_t, got_m = image_batch(images, sizes, device='cuda', **kwargs)
        np.testing.assert_array_equal(got_t.cpu().numpy(), want_t)
        np.testing.assert_array_equal(got_m.cpu().numpy(), want_m)


def test_results_do_not_depend_on_the_run():
    """The statistics are integer atomics: two runs of the same batch give the same bytes."""
    rng = np.random.default_rng(44)
    images = [limited_noise(rng, 384, 640) for _ in range(4)]
    plans = [(('AutoContrast', 0.0, False), ('Contrast', 0.7, False), ('Rotate', 5.0, True), ('Contrast', 1.4, False))] * 4
    a, _ = image_batch(images, [(384, 640)] * 4, device='cuda', augment=plans)
    b, _ = image_batch(images, [(384, 640)] * 4, device='cuda', augment=plans)
    assert torch.equal(a, b)


def test_plans_of_every_length_in_one_batch():
    """0 .. 4 operations, Identity in the middle: an image skips the stages past its plan and the last launch reads it
    from the buffer its own count leaves it in."""
    rng = np.random.default_rng(45)
    ops = [('Contrast', 0.6, False), ('ShearY', 0.1, True), ('AutoContrast', 0.0, False), ('Sharpness', 1.4, False)]
    plans = [tuple(ops[:k]) for k in range(5)] + [(ops[0], ('Identity', 9.0, False), ops[2]), (('Identity', 1.0, False),) * 4,
                                                  (('Rotate', 0.0, False), ops[3], ops[1])]
    images = [limited_noise(rng, 40 + 3 * i, 50 + 5 * i) for i in range(len(plans))]
    sizes = [(30 + 2 * i, 41 + 3 * i) for i in range(len(plans))]
    check(images, sizes, plans)
    check(images[::-1], sizes[::-1], plans[::-1], pad_to=(64, 80))
