"""numpy statement of the detector's image chain with Pillow's arithmetic (8 bits per channel, RGB): horizontal flip, crop and
Image.resize(..., BILINEAR), the three things torchvision does to a PIL image in the reference's detection transforms.

Independent of grit_amd: the GPU tests compare the device path with this model at sizes the fixture G20 does not reach
(neither Pillow nor the reference is available where they run); the CPU tests pin the model itself to G20 and to Pillow.

    taps(in_size, out_size)      -> (ksize, bounds [out, 2], taps [out, ksize]): Pillow's precompute_coeffs, 22-bit
    resize(img, oh, ow)          -> the two integer passes
    chain(img, plan)             -> the plan step by step on the array: img[:, ::-1], a slice, resize
    chain_folded(img, plan)      -> the same plan folded as the device does it: every resize reads a window of what is stored,
                                    a crop only moves the window, a flip only mirrors the taps of the next horizontal pass

plan = (('hflip',) | ('resize', oh, ow) | ('crop', top, left, h, w), ...)"""
import functools
import math

import numpy as np

PRECISION_BITS = 22


@functools.lru_cache(maxsize=None)
def taps(in_size, out_size):
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    table = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        last = min(int(center + support + 0.5), in_size)
        k = []
        for x in range(last - first):
            v = abs((x + first - center + 0.5) * (1.0 / filterscale))
            k.append(1.0 - v if v < 1.0 else 0.0)
        total = 0.0
        for v in k:
            total += v
        for x, v in enumerate(k):
            if total != 0.0:
                v = v / total
            table[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = first, last - first
    return ksize, bounds, table


def mirrored(in_size, out_size):
    """The taps of resize(row[::-1]) as taps on `row`: reversed per output, first' = in_size - first - count."""
    ksize, bounds, table = taps(in_size, out_size)
    flipped = np.zeros_like(table)
    for xx, (first, count) in enumerate(bounds.tolist()):
        flipped[xx, :count] = table[xx, :count][::-1]
    return ksize, np.stack([in_size - bounds[:, 0] - bounds[:, 1], bounds[:, 1]], 1), flipped


def dense(in_size, bounds, table):
    m = np.zeros((len(bounds), in_size), np.int64)
    for xx, (first, count) in enumerate(bounds.tolist()):
        m[xx, first:first + count] = table[xx, :count]
    return m


def clip8(s):
    return np.clip((s + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_window(stored, top, left, h, w, mirror, oh, ow):
    """Resize of stored[top:top + h, left:left + w] (read back to front along x when `mirror`) without taking the slice apart:
    the horizontal pass into a uint8 intermediate, then the vertical pass."""
    _, xb, xt = mirrored(w, ow) if mirror else taps(w, ow)
    _, yb, yt = taps(h, oh)
    window = stored[top:top + h, left:left + w].astype(np.int64)
    rows = clip8(np.einsum('ox,yxc->yoc', dense(w, xb, xt), window))
    return clip8(np.einsum('oy,yxc->oxc', dense(h, yb, yt), rows.astype(np.int64)))


def resize(img, oh, ow):
    return resize_window(img, 0, 0, img.shape[0], img.shape[1], False, oh, ow)


def chain(img, plan):
    for op in plan:
        if op[0] == 'hflip':
            img = img[:, ::-1]
        elif op[0] == 'crop':
            img = img[op[1]:op[1] + op[3], op[2]:op[2] + op[4]]
        else:
            img = resize(img, op[1], op[2])
    return np.ascontiguousarray(img)


def chain_folded(img, plan):
    stored = img
    top, left, h, w, mirror = 0, 0, img.shape[0], img.shape[1], False
    for op in plan:
        if op[0] == 'hflip':
            mirror = not mirror
        elif op[0] == 'crop':
            top, left = top + op[1], left + (w - op[2] - op[4] if mirror else op[2])
            h, w = op[3], op[4]
        else:
            stored = resize_window(stored, top, left, h, w, mirror, op[1], op[2])
            top, left, h, w, mirror = 0, 0, op[1], op[2], False
    if mirror or (top, left, h, w) != (0, 0) + stored.shape[:2]:
        stored = resize_window(stored, top, left, h, w, mirror, h, w)  # identity taps
    return stored


def normalized(u8, mean, std):
    """ToTensor + Normalize with torch's float ops -> [3, h, w] float32 (numpy)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).to(torch.float32).div(255)
    return t.sub(torch.tensor(mean)[:, None, None]).div(torch.tensor(std)[:, None, None]).numpy()
