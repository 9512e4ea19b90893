"""Fixture G20, tests/golden/det_transforms_g20.npz: the reference's detection transforms on the CPU, pixels and boxes.

    python tests/golden/make_det_transforms_golden.py [--scan]

Like make_golden.py this runs only where the reference tree and Pillow are present; what is committed is data.  The reference's
datasets/detection/transforms.py is loaded by path.  `torchvision` and `matplotlib` are replaced by stub modules of our own:
`functional.resize / crop / hflip / to_tensor / normalize` are the Pillow and torch calls torchvision makes for a PIL image
(Image.resize(size[::-1], BILINEAR), Image.crop, Image.transpose(FLIP_LEFT_RIGHT), uint8 -> float32 / 255, sub_(mean).div_(std))
and `RandomCrop.get_params` restates torchvision's (0.8 and later): no draw when the crop equals the image, else
torch.randint for the top, then for the left edge.  The three geometric stubs also log what they were asked to do, which is
how the fixture records every plan and every intermediate size.

Two parts after ONE random.seed(SEED) and ONE torch.manual_seed(SEED), in this order:

  pixels   20 smooth seeded images of 40..140 pixels a side (more would not fit a committed file) with 0..12 boxes each go through the reference's classes composed
           like the `train` recipe, with small numbers: RandomHorizontalFlip, RandomSelect(RandomResize([48, 56, 64], 100),
           Compose([RandomRatioResize((0.5, 1.5)), RandomSizeCrop(24, 60), RandomResize([48, 56, 64], 100)])), ToTensor,
           Normalize.  Stored: inputs, input targets, the logged steps, the uint8 result, the final targets, and per batch of
           5 the padded tensors / mask of nested_tensor_from_tensor_list.
  draws    200 items of Visual-Genome-like sizes go through the real make_transforms('train', 'train'),
           ('train', 'pretrain-od') and ('valid', 'train'), on an image object that only carries its size.  Stored: the
           logged steps and the final targets.

and then the next random.random() and the next torch.randint.  Steps are rows (code, a, b, c, d): 0 hflip; 1 resize to
(a, b) = (oh, ow); 2 crop (a, b, c, d) = (top, left, h, w).

Asserted on the pixel part, so that the fixture cannot pass vacuously: both flip outcomes in both RandomSelect branches; crops
whose left edge is 0, 1, 2 and 3 modulo 4 (every dword misalignment of 3 * left); a crop touching the right and one touching
the bottom edge; a crop equal to the image (no torch draw); a box removed by a crop; an image left with no box; an unchanged
axis in some resize.  SEED is the first seed that meets them."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402

SEED = 7
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
VG_SIZES = [(500, 375), (375, 500), (500, 333), (333, 500), (640, 480), (480, 640), (1024, 768), (800, 600), (500, 500), (1280, 960),
            (400, 300), (500, 281), (612, 612), (768, 1024), (500, 400), (359, 500)]  # (w, h)
RECIPES = [('train', 'train'), ('train', 'pretrain-od'), ('valid', 'train')]
TARGET_KEYS = ('boxes', 'labels', 'area', 'iscrowd', 'attributes', 'size', 'orig_size')
LOG, SEEN_U8 = [], []


class SizeOnly(object):
    """What the draws need of a PIL image."""

    def __init__(self, w, h):
        self.size, self.width, self.height = (w, h), w, h


class ShapeOnly(object):
    def __init__(self, h, w):
        self.shape = (3, h, w)


def install_stubs():
    from PIL import Image
    tv = sys.modules["torchvision"]  # import_reference's version object
    T, F, ops, boxes, mpl, plt = (types.ModuleType(n) for n in ("torchvision.transforms", "torchvision.transforms.functional",
                                                                "torchvision.ops", "torchvision.ops.boxes", "matplotlib", "matplotlib.pyplot"))
    boxes.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])  # imported by the reference's utils/box_ops.py, not used here

    def resize(img, size):
        oh, ow = size
        LOG.append((1, oh, ow, 0, 0))
        return SizeOnly(ow, oh) if isinstance(img, SizeOnly) else img.resize((ow, oh), Image.BILINEAR)

    def crop(img, top, left, height, width):
        LOG.append((2, top, left, height, width))
        return SizeOnly(width, height) if isinstance(img, SizeOnly) else img.crop((left, top, left + width, top + height))

    def hflip(img):
        LOG.append((0, 0, 0, 0, 0))
        return img if isinstance(img, SizeOnly) else img.transpose(Image.FLIP_LEFT_RIGHT)

    def to_tensor(pic):
        if isinstance(pic, SizeOnly):
            return ShapeOnly(pic.height, pic.width)
        SEEN_U8[:] = [np.array(pic, np.uint8, copy=True)]
        return torch.from_numpy(SEEN_U8[0]).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def normalize(tensor, mean, std):
        if isinstance(tensor, ShapeOnly):
            return tensor
        mean, std = torch.as_tensor(mean, dtype=tensor.dtype), torch.as_tensor(std, dtype=tensor.dtype)
        return tensor.clone().sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))

    class RandomCrop(object):
        @staticmethod
        def get_params(img, output_size):
            w, h = img.size
            th, tw = output_size
            if w == tw and h == th:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw

    F.resize, F.crop, F.hflip, F.to_tensor, F.normalize = resize, crop, hflip, to_tensor, normalize
    T.RandomCrop, T.functional, tv.transforms, ops.boxes, tv.ops, mpl.pyplot = RandomCrop, F, T, boxes, ops, plt
    sys.modules.update({m.__name__: m for m in (T, F, ops, boxes, mpl, plt)})


def load_reference_transforms():
    import_reference()
    install_stubs()
    spec = importlib.util.spec_from_file_location('ref_det_transforms', os.path.join(REF, 'datasets/detection/transforms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth_image(rng, h, w):
    """Waves, a different range and direction per channel."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(3):
        lo, hi = rng.integers(0, 90), rng.integers(150, 256)
        fx, fy, ph = rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(0, 6.28)
        planes.append(np.clip(lo + (hi - lo) * (0.5 + 0.5 * np.sin(x * fx + y * fy + ph)), 0, 255))
    return np.stack(planes, -1).astype(np.uint8)


def make_target(rng, w, h, count):
    x0, y0 = rng.uniform(0, w - 2, count), rng.uniform(0, h - 2, count)
    x1, y1 = x0 + rng.uniform(1, w / 2, count), y0 + rng.uniform(1, h / 2, count)
    boxes = np.stack([x0, y0, np.minimum(x1, w), np.minimum(y1, h)], 1).astype(np.float32).reshape(-1, 4)
    return {'boxes': torch.from_numpy(boxes), 'labels': torch.from_numpy(rng.integers(0, 1849, count)),
            'area': torch.from_numpy((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])),
            'iscrowd': torch.zeros(count, dtype=torch.int64), 'attributes': torch.from_numpy(rng.integers(0, 2, (count, 5))),
            'size': torch.tensor([h, w]), 'orig_size': torch.tensor([h, w])}


def inputs():
    rng = np.random.default_rng(20)
    shapes = [(40, 44), (42, 40), (44, 47), (140, 90), (64, 100), (57, 83), (100, 61), (77, 77)] + \
        [(int(rng.integers(40, 101)), int(rng.integers(40, 101))) for _ in range(12)]  # (h, w)
    counts = [0, 3, 12, 1] + [int(rng.integers(0, 13)) for _ in range(16)]
    images = [smooth_image(rng, h, w) for h, w in shapes]
    targets = [make_target(rng, w, h, n) for (h, w), n in zip(shapes, counts)]
    targets[3]['boxes'][0] = torch.tensor([0.0, 0.0, 2.0, 2.0])  # a corner box: most crops remove it
    sizes = [VG_SIZES[i] for i in rng.integers(0, len(VG_SIZES), 200)]
    return images, targets, sizes, [make_target(rng, w, h, int(rng.integers(0, 13))) for w, h in sizes]


def put(out, prefix, target):
    for k in TARGET_KEYS:
        out[prefix + k] = target[k].numpy()


def main(seed=SEED, write=True):
    from PIL import Image
    ref = load_reference_transforms()
    from engine.utils import nested_tensor_from_tensor_list
    images, targets, vg_sizes, vg_targets = inputs()
    small = [48, 56, 64]
    recipe = ref.Compose([ref.RandomHorizontalFlip(),
                          ref.RandomSelect(ref.RandomResize(small, max_size=100),
                                           ref.Compose([ref.RandomRatioResize((0.5, 1.5)), ref.RandomSizeCrop(24, 60),
                                                        ref.RandomResize(small, max_size=100)])),
                          ref.Compose([ref.ToTensor(), ref.Normalize(MEAN, STD)])])
    out = {'seed': np.int64(seed), 'count': np.int64(len(images)), 'vg_sizes': np.asarray(vg_sizes, np.int64)}
    random.seed(seed)
    torch.manual_seed(seed)
    seen = {'flip_branch': set(), 'left_mod4': set(), 'right': False, 'bottom': False, 'full_crop': False, 'box_removed': False,
            'no_box_left': False, 'unchanged_axis': False}
    batch = []
    for i, (img, tgt) in enumerate(zip(images, targets)):
        del LOG[:]
        out['in%d' % i] = img
        put(out, 'in%d_' % i, tgt)
        before = torch.get_rng_state()
        result, final = recipe(Image.fromarray(img, 'RGB'), tgt)
        steps = np.asarray(LOG, np.int64).reshape(-1, 5)
        out['steps%d' % i] = steps
        put(out, 'out%d_' % i, final)
        out['u8_%d' % i] = SEEN_U8[0]  # what ToTensor was given
        batch.append(result)
        if len(batch) == 5:
            nt = nested_tensor_from_tensor_list(batch)
            out['tensors_b%d' % (i // 5)], out['mask_b%d' % (i // 5)] = nt.tensors.numpy(), nt.mask.numpy()
            batch = []
        # what happened
        flipped, two = bool((steps[:, 0] == 0).any()), int((steps[:, 0] == 1).sum()) == 2
        seen['flip_branch'].add((flipped, two))
        w, h = img.shape[1], img.shape[0]
        for code, a, b, c, d in steps.tolist():
            if code == 1:
                seen['unchanged_axis'] |= a == h or b == w
                h, w = a, b
            elif code == 2:
                seen['left_mod4'].add(b % 4)
                seen['right'] |= b + d == w and b > 0
                seen['bottom'] |= a + c == h and a > 0
                if (c, d) == (h, w):
                    seen['full_crop'] = True
                    assert torch.equal(before, torch.get_rng_state())  # no torch draw
                h, w = c, d
        seen['box_removed'] |= len(final['labels']) < len(tgt['labels'])
        seen['no_box_left'] |= len(tgt['labels']) > 0 and len(final['labels']) == 0
    assert not batch
    steps, starts, finals = [], [0], []
    for split, phase in RECIPES:
        recipe = ref.make_transforms(split, phase)
        for (w, h), tgt in zip(vg_sizes, vg_targets):
            del LOG[:]
            _, final = recipe(SizeOnly(w, h), tgt)
            steps += LOG
            starts.append(len(steps))
            finals.append(final)
    out['vg_steps'], out['vg_starts'] = np.asarray(steps, np.int64).reshape(-1, 5), np.asarray(starts, np.int64)
    out['vg_counts'] = np.asarray([len(f['labels']) for f in finals], np.int64)
    for k in TARGET_KEYS:
        out['vg_in_' + k] = torch.cat([t[k].reshape((-1,) + tuple(t[k].shape[1:])) if k not in ('size', 'orig_size') else t[k][None]
                                       for t in vg_targets]).numpy()
        out['vg_out_' + k] = torch.cat([f[k] if k not in ('size', 'orig_size') else f[k][None] for f in finals]).numpy()
    out['vg_in_counts'] = np.asarray([len(t['labels']) for t in vg_targets], np.int64)
    out['next_random'] = np.float64(random.random())
    out['next_randint'] = np.int64(torch.randint(0, 2 ** 31 - 1, (1,)).item())

    missing = [k for k, v in seen.items() if v is False]
    missing += ['flip_branch %s' % (k,) for k in ((f, t) for f in (False, True) for t in (False, True)) if k not in seen['flip_branch']]
    missing += ['left %% 4 == %d' % m for m in range(4) if m not in seen['left_mod4']]
    if not write:
        return not missing
    assert not missing, "never happens with seed %d: %s" % (seed, missing)
    path = os.path.join(HERE, 'det_transforms_g20.npz')
    np.savez_compressed(path, **out)
    print('g20 seed %d: %d images, %d + %d steps; %d bytes' % (seed, len(images), sum(len(out['steps%d' % i]) for i in range(len(images))),
                                                               len(steps), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    if '--scan' in sys.argv:  # the first seed that meets the conditions
        print(next(s for s in range(1000) if main(s, write=False)))
    else:
        main()
