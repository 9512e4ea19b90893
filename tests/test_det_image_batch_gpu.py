"""The detector's input pipeline on the device (grit_image_batch_geo_fwd through image_batch_geo and collate_detection) against
fixture G20 (the reference's transforms on Pillow) and, at sizes the fixture does not reach, the numpy model
tests/det_transforms_model.py.  Every comparison is bit-exact."""
import os
import random

import numpy as np
import pytest
import torch

from grit_amd.datasets.detection import collate_detection, make_transforms
from grit_amd.ops.image_batch import MEAN, STD, image_batch_geo
from tests import det_transforms_model as model
from tests.test_det_transforms_cpu import TARGET_KEYS, replay_pixels

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def expected(images, plans, pad_to=None):
    """Model chain -> ToTensor / Normalize with torch's float ops -> zero padding and mask."""
    results = [model.chain_folded(np.asarray(img), plan) for img, plan in zip(images, plans)]
    H, W = pad_to if pad_to is not None else (max(r.shape[0] for r in results), max(r.shape[1] for r in results))
    tensors, mask = np.zeros((len(images), 3, H, W), np.float32), np.ones((len(images), H, W), bool)
    for i, u8 in enumerate(results):
        tensors[i, :, :u8.shape[0], :u8.shape[1]] = model.normalized(u8, MEAN, STD)
        mask[i, :u8.shape[0], :u8.shape[1]] = False
    return tensors, mask


def check(images, plans, pad_to=None, feed=None):
    want_t, want_m = expected(images, plans, pad_to)
    got_t, got_m = image_batch_geo(images if feed is None else feed, plans, device=DEV, pad_to=pad_to)
    assert got_t.dtype == torch.float32 and got_m.dtype == torch.bool
    np.testing.assert_array_equal(got_m.cpu().numpy(), want_m)
    got_t = got_t.cpu().numpy()
    for i in range(len(images)):  # per image, so that a failure names the plan
        np.testing.assert_array_equal(got_t[i], want_t[i], err_msg="image %d, plan %s" % (i, plans[i]))
    return got_t, got_m


def noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_fixture_g20_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "det_transforms_g20.npz"))
    items = replay_pixels(g)
    for b in range(len(items) // 5):
        nt, targets = collate_detection(items[5 * b:5 * b + 5], device=DEV)
        assert nt.tensors.dtype == torch.float32 and nt.mask.dtype == torch.bool
        np.testing.assert_array_equal(nt.mask.cpu().numpy(), g['mask_b%d' % b])
        got = nt.tensors.cpu().numpy()
        for k in range(5):
            i = 5 * b + k
            np.testing.assert_array_equal(got[k], g['tensors_b%d' % b][k], err_msg="image %d: %s" % (i, items[i][0].plan))
            for key in TARGET_KEYS:
                assert targets[k][key].is_cuda and torch.equal(targets[k][key].cpu(), torch.from_numpy(g['out%d_%s' % (i, key)]))


@pytest.mark.parametrize("w,ow,ksize", [(150, 60, 7), (230, 60, 9), (260, 60, 11), (400, 60, 15), (30, 97, 3)])
def test_every_row_kernel(w, ow, ksize):
    """One resize per tap-count variant of the horizontal pass (7, 9, 13 taps in registers, any count), straight and
    mirrored, from the blob and from the work buffer; the height stays (identity taps) or changes."""
    assert model.taps(w, ow)[0] == ksize
    rng = np.random.default_rng(ksize)
    images = [noise(rng, 9, w), noise(rng, 9, w), noise(rng, 13, w), noise(rng, 11, w)]
    plans = [(('resize', 9, ow),), (('hflip',), ('resize', 9, ow)), (('resize', 6, ow),),
             (('resize', 11, w), ('hflip',), ('resize', 17, ow))]  # A keeps every byte, B reads the work buffer
    check(images, plans)
    check(images[:3], plans[:3])  # two launches


def test_crop_windows_at_every_byte_misalignment():
    rng = np.random.default_rng(4)
    images = [noise(rng, 21, 37) for _ in range(8)]
    plans = [(('crop', 2, left, 15, 30), ('resize', 12, 19)) for left in range(4)]  # windows of the blob
    plans += [(('resize', 25, 41), ('crop', 3, left, 20, 33), ('resize', 14, 50)) for left in range(4)]  # windows of the work buffer
    check(images, plans)
    check(images, [(('hflip',),) + p for p in plans])


@pytest.mark.parametrize("ow,ksize", [(10, 13), (40, 5)])
def test_window_ending_with_the_buffer(ow, ksize):
    """The last image's window ends at the last pixel of its last row, in the blob and in the work buffer: the row pass
    fetches whole dwords past it (the widest fetch is the 13-tap variant's) and must find them readable."""
    assert model.taps(55, ow)[0] == ksize
    rng = np.random.default_rng(5)
    images = [noise(rng, 16, 60), noise(rng, 16, 60)]
    check(images, [(('resize', 8, 30),), (('crop', 5, 5, 11, 55), ('resize', 7, ow))])
    check(images, [(('resize', 8, 30),), (('resize', 20, 75), ('crop', 9, 20, 11, 55), ('resize', 7, ow))])


@pytest.mark.parametrize("pad_to", [None, (64, 96)])
def test_mixed_batch_and_determinism(pad_to):
    rng = np.random.default_rng(6)
    images = [noise(rng, 33, 47), noise(rng, 40, 61), noise(rng, 57, 83), noise(rng, 50, 70), noise(rng, 1, 1)]
    plans = [(), (('hflip',),), (('hflip',), ('resize', 48, 70)),
             (('hflip',), ('resize', 61, 85), ('crop', 4, 9, 50, 63), ('resize', 56, 71)), (('resize', 3, 5),)]
    first_t, first_m = check(images, plans, pad_to)
    again_t, again_m = image_batch_geo([torch.from_numpy(im).to(DEV) for im in images], plans, device=DEV, pad_to=pad_to)
    assert np.array_equal(again_t.cpu().numpy(), first_t) and torch.equal(again_m, first_m)


def test_recipe_size():
    rng = np.random.default_rng(7)
    image = noise(rng, 375, 500)
    plan = (('hflip',), ('resize', 450, 600), ('crop', 37, 41, 400, 533), ('resize', 800, 1066))
    check([image], [plan])


def test_bicubic_path_still_equals_g11(golden_dir):
    from grit_amd.datasets.caption.transforms import MaxWHResize, MinMaxResize, collate_images
    g = np.load(os.path.join(golden_dir, "image_g11.npz"))
    for name, policy in (('maxwh', MaxWHResize((48, 64))), ('minmax', MinMaxResize((64, 128)))):
        nt = collate_images([policy(g['%s_in%d' % (name, i)]) for i in range(5)], device=DEV)
        np.testing.assert_array_equal(nt.tensors.cpu().numpy(), g[name + '_tensors'])
        np.testing.assert_array_equal(nt.mask.cpu().numpy(), g[name + '_mask'])


def test_normal_policy_on_the_device():
    from grit_amd.datasets.caption.transforms import collate_images, get_transform

    class Cfg(object):
        size, resize_name, randaug = (48, 64), 'normal', False

    rng = np.random.default_rng(8)
    images = [noise(rng, 60, 80), noise(rng, 31, 97)]
    policy = get_transform(Cfg())['valid']
    nt = collate_images([policy(im) for im in images], device=DEV)
    want_t, want_m = expected(images, [(('resize', 48, 64),)] * 2)
    assert np.array_equal(nt.tensors.cpu().numpy(), want_t) and np.array_equal(nt.mask.cpu().numpy(), want_m) and not nt.any_padding


def test_two_augmented_training_steps(golden_dir):
    import json
    import train_detector
    from engine.det_engine import train_step
    from grit_amd.config import detection_config
    from models.detection.detector import build_detector
    from tests.helpers import deterministic_fill_, disable_drop_path
    e = json.load(open(os.path.join(golden_dir, "det_loss_g19.json")))['e2e']
    cfg = detection_config(**{'model.backbone.pre_trained': 'none', 'model.det_module.num_classes': e['num_classes'],
                              'model.det_module.num_queries': e['num_queries'], 'model.det_module.reduced_dim': e['d_model'],
                              'model.det_module.dropout': 0.0})
    model, criterion, _ = build_detector(cfg)
    deterministic_fill_(model)
    model.to(DEV).train()
    disable_drop_path(model)
    optimizer = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    random.seed(3)
    torch.manual_seed(3)
    generator, transform = torch.Generator().manual_seed(3), make_transforms('train', 'train')
    for _ in range(2):
        samples, targets = train_detector.augmented_batch(generator, 2, e['num_classes'], 6, DEV, transform)
        assert samples.tensors.is_cuda and samples.tensors.shape[0] == 2 and 480 <= min(samples.tensors.shape[2:]) and max(samples.tensors.shape[2:]) <= 1333
        assert all(t['boxes'].is_cuda and t['labels'].is_cuda and len(t['labels']) > 0 for t in targets)
        assert all(float(t['boxes'].min()) >= 0 and float(t['boxes'].max()) <= 1 for t in targets)
        total, losses = train_step(model, criterion, optimizer, samples, targets, max_norm=0.1)
        assert np.isfinite(float(total)) and all(np.isfinite(float(v)) for v in losses.values())
