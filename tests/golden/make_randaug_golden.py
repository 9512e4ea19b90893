"""Fixture G17, tests/golden/randaug_g17.npz: the reference's MaxWHResize + RandAugment on the CPU.

    python tests/golden/make_randaug_golden.py

Like make_golden.py this runs only where the reference tree and Pillow are present; what is committed is data.  The
reference's classes are loaded from their files by path (datasets/caption/transforms/utils.py and randaug.py; the package
__init__ needs torchvision).  24 seeded images of different sizes go through `MaxWHResize` into (48, 64) / (96, 128)
canvases and through ONE `RandAugment()` instance after a single `random.seed(SEED)`, in order.  Every entry of the
instance's `augment_list` is wrapped to record what the reference actually did: operation name, magnitude, the sign draw of
the geometric operations (peeked from the `random` state and put back, so the stream is untouched) and whether the
operation changed a byte.  ToTensor / Normalize / padding are built as make_golden.py's make_g11 builds them.

Stored: SEED, the inputs, per image the four (name, magnitude, negate), the uint8 result, the padded `tensors` / `mask` per
canvas, and the next `random.random()` after the 24 draws.

Asserted, so that the fixture cannot pass vacuously: all eleven operations occur; each geometric one with both signs; each
of the 15 kinds (10 non-Identity operations, the 5 geometric ones per sign) changes at least one byte in at least one of
its applications.  The inputs are smooth and do not span 0..255 in every channel (on uniform noise AutoContrast is the
identity).  SEED was picked as the first seed that meets the three conditions on these inputs."""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402

SEED = 0
GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXabs', 'TranslateYabs')
SHAPES = [(60, 80), (75, 50), (64, 64), (31, 97), (120, 160), (48, 64), (50, 90), (100, 61), (77, 77), (40, 110), (90, 45), (57, 83),
          (66, 99), (33, 40), (128, 96), (51, 67),  # -> (48, 64)
          (88, 117), (110, 90), (96, 128), (70, 141), (104, 98), (97, 131), (100, 140), (111, 120)]  # -> (96, 128)
CANVASES = [((48, 64), 16), ((96, 128), 8)]


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth_image(rng, h, w):
    """Waves inside a per-channel range narrower than 0..255, one grey level of noise on top."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(3):
        lo, hi = rng.integers(5, 90), rng.integers(150, 250)
        fx, fy, ph = rng.uniform(0.02, 0.3), rng.uniform(0.02, 0.3), rng.uniform(0, 6.28)
        wave = 0.5 + 0.5 * np.sin(x * fx + y * fy + ph)
        planes.append(np.clip(lo + (hi - lo) * wave + rng.integers(-1, 2, (h, w)), 0, 255))
    return np.stack(planes, -1).astype(np.uint8)


def main(seed=SEED, write=True):
    from PIL import Image
    tu = load('ref_transform_utils', 'datasets/caption/transforms/utils.py')
    ra = load('ref_randaug', 'datasets/caption/transforms/randaug.py')
    import_reference()
    from engine.utils import nested_tensor_from_tensor_list
    mean = torch.as_tensor([0.485, 0.456, 0.406], dtype=torch.float32)[:, None, None]
    std = torch.as_tensor([0.229, 0.224, 0.225], dtype=torch.float32)[:, None, None]
    rng = np.random.default_rng(17)
    images = [smooth_image(rng, h, w) for h, w in SHAPES]

    log = []

    def wrap(fn):
        name = fn.__name__

        def recorded(img, v):
            negate = False
            if name in GEOMETRIC:  # the operation's own next draw, without consuming it
                state = random.getstate()
                negate = random.random() > 0.5
                random.setstate(state)
            out = fn(img, v)
            log.append((name, float(v), negate, not np.array_equal(np.asarray(out), np.asarray(img))))
            return out
        return recorded

    augment = ra.RandAugment()
    augment.augment_list = [(wrap(fn), lo, hi) for fn, lo, hi in augment.augment_list]
    out = {'seed': np.int64(seed), 'count': np.int64(len(images))}
    random.seed(seed)
    start, tensors = 0, []
    for canvas, count in CANVASES:
        policy = tu.MaxWHResize(canvas)
        tensors = []
        for i in range(start, start + count):
            out['in%d' % i] = images[i]
            u8 = torch.from_numpy(np.asarray(augment(policy(Image.fromarray(images[i], 'RGB')))).copy())
            out['u8_%d' % i] = u8.numpy()
            tensors.append(u8.permute(2, 0, 1).to(torch.float32).div(255).sub_(mean).div_(std))
        nt = nested_tensor_from_tensor_list(tensors)
        out['tensors_%dx%d' % canvas] = nt.tensors.numpy()
        out['mask_%dx%d' % canvas] = nt.mask.numpy()
        start += count
    out['next_random'] = np.float64(random.random())
    assert len(log) == 4 * len(images)
    out['names'] = np.asarray([e[0] for e in log]).reshape(len(images), 4)
    out['values'] = np.asarray([e[1] for e in log], np.float64).reshape(len(images), 4)
    out['negate'] = np.asarray([e[2] for e in log], bool).reshape(len(images), 4)

    names = [fn.__name__ for fn, _, _ in ra.augment_list()]
    kinds = [(n, s) for n in names if n != 'Identity' for s in ((False, True) if n in GEOMETRIC else (False,))]
    assert len(kinds) == 15
    missing = [n for n in names if not any(e[0] == n for e in log)]
    unseen = [k for k in kinds if not any((e[0], e[2]) == k for e in log)]
    inert = [k for k in kinds if not any((e[0], e[2]) == k and e[3] for e in log)]
    ok = not (missing or unseen or inert)
    if not write:
        return ok
    assert not missing, "operations that never occur: %s" % missing
    assert not unseen, "kinds that never occur: %s" % unseen
    assert not inert, "kinds that never change a byte: %s" % inert
    noops = sum(1 for e in log if e[0] != 'Identity' and not e[3])
    path = os.path.join(HERE, 'randaug_g17.npz')
    np.savez_compressed(path, **out)
    print('g17 seed %d: %d applications, %d of the non-Identity ones change nothing; %d bytes'
          % (seed, len(log), noops, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    if '--scan' in sys.argv:  # which seeds meet the conditions
        print([s for s in range(8) if main(s, write=False)])
    else:
        main()
