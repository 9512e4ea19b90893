"""numpy statement of the eleven RandAugment operations with Pillow's arithmetic (8 bits per channel, RGB).

Independent of grit_amd: the GPU tests compare the device path with this model at sizes the fixture G17 does not reach
(neither Pillow nor the reference is available where they run); the CPU tests pin the model itself to G17 and to Pillow.

    apply(img [h, w, 3] uint8, name, val, negate) -> [h, w, 3] uint8
    chain(img, plan) with plan = ((name, val, negate), ...)

`val` is the magnitude the reference draws, `negate` the sign draw of the five geometric operations."""
import math

import numpy as np

GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXabs', 'TranslateYabs')
F32 = np.float32


def grey(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, factor):
    """Image.blend(degenerate, image, factor): fp32 multiply, then fp32 add."""
    alpha = F32(factor)
    if alpha == 0:
        return deg.copy()
    if alpha == 1:
        return img.copy()
    d = deg.astype(F32)
    t = d + alpha * (img.astype(F32) - d)  # numpy rounds each operation; the difference of two bytes is exact
    assert t.dtype == F32
    if 0 <= alpha <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: 3 x 3 (1,1,1,1,5,1,1,1,1) / 13 in fp32; border rows and columns unchanged."""
    h, w = img.shape[:2]
    out = img.copy()
    if h < 3 or w < 3:
        return out
    k = [F32(v / 13.0) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    p = img.astype(F32)

    def row(r, k0, k1, k2):  # (left * k0 + centre * k1) + right * k2 of the interior pixels, rows r .. r + h - 2
        return (p[r:r + h - 2, 0:w - 2] * k0 + p[r:r + h - 2, 1:w - 1] * k1) + p[r:r + h - 2, 2:w] * k2

    s = np.full((h - 2, w - 2, 3), 0.5, F32)
    s = s + row(2, k[0], k[1], k[2])  # the row below first, as Pillow's loop does
    s = s + row(1, k[3], k[4], k[5])
    s = s + row(0, k[6], k[7], k[8])
    assert s.dtype == F32
    out[1:h - 1, 1:w - 1] = np.where(s <= 0, 0, np.where(s >= 255, 255, np.clip(s, 0, 255).astype(np.int32))).astype(np.uint8)
    return out


def autocontrast(img):
    out = img.copy()
    for c in range(3):
        lo, hi = int(img[..., c].min()), int(img[..., c].max())
        if hi <= lo:
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        lut = np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], np.uint8)
        out[..., c] = lut[img[..., c]]
    return out


def contrast_mean(img):
    l = grey(img)
    return int(int(l.sum(dtype=np.int64)) / l.size + 0.5)


def fix(t):
    return int(math.floor(t * 65536.0 + 0.5))


def affine(img, a):
    """Image.transform(size, AFFINE, a): nearest neighbour, fill 0; a maps output (x, y) to input."""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    if a[1] != 0 or a[3] != 0:  # 16.16 fixed point
        A0, A1, A3, A4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
        A2 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5)
        A5 = fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
        y, x = np.mgrid[0:h, 0:w].astype(np.int64)
        xin = (A2 + A0 * x + A1 * y) >> 16
        yin = (A5 + A3 * x + A4 * y) >> 16
        ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
        out[ok] = img[yin[ok], xin[ok]]
        return out

    def walk(start, step, n):  # repeated double additions, as Pillow tabulates them
        idx, o = [], start + step * 0.5
        for _ in range(n):
            idx.append(-1 if o < 0.0 else int(o))
            o += step
        return np.asarray(idx, np.int64)

    xin, yin = walk(a[2], a[0], w), walk(a[5], a[4], h)
    okx, oky = (xin >= 0) & (xin < w), (yin >= 0) & (yin < h)
    ok = oky[:, None] & okx[None, :]
    gathered = img[np.clip(yin, 0, h - 1)[:, None], np.clip(xin, 0, w - 1)[None, :]]
    out[ok] = gathered[ok]
    return out


def rotate_matrix(v, w, h):
    """Image.rotate(v) of a w x h image -> affine coefficients, or None for a plain copy."""
    angle = v % 360.0
    if angle == 0:
        return None
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def apply(img, name, val, negate=False):
    v = -val if (negate and name in GEOMETRIC) else val
    h, w = img.shape[:2]
    if name == 'Identity':
        return img.copy()
    if name == 'AutoContrast':
        return autocontrast(img)
    if name == 'Rotate':
        m = rotate_matrix(v, w, h)
        return img.copy() if m is None else affine(img, m)
    if name == 'ShearX':
        return affine(img, (1, v, 0, 0, 1, 0))
    if name == 'ShearY':
        return affine(img, (1, 0, 0, v, 1, 0))
    if name == 'TranslateXabs':
        return affine(img, (1, 0, v, 0, 1, 0))
    if name == 'TranslateYabs':
        return affine(img, (1, 0, 0, 0, 1, v))
    if name == 'Color':
        return blend(np.repeat(grey(img)[..., None], 3, -1), img, val)
    if name == 'Contrast':
        return blend(np.full_like(img, contrast_mean(img)), img, val)
    if name == 'Brightness':
        return blend(np.zeros_like(img), img, val)
    if name == 'Sharpness':
        return blend(smooth(img), img, val)
    raise ValueError(name)


def chain(img, plan):
    for name, val, negate in plan:
        img = apply(img, name, val, negate)
    return img
