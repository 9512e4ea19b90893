"""Decoded RGB images -> the model's input batch, on the device.

    [h_i, w_i, 3] uint8  --bicubic resize to (oh_i, ow_i), Pillow's 8-bit arithmetic-->  --/255, (x - mean) / std-->
    --zero padding to (max oh, max ow)-->  tensors [B, 3, H, W] f32,  mask [B, H, W] bool (True on padding)

Replaces the per-image host chain of the reference -- PIL `x.resize(..., Image.BICUBIC)` in MaxWHResize / MinMaxResize
(datasets/caption/transforms/utils.py:4-45), ToTensor + Normalize (transforms/__init__.py:6-32) and
nested_tensor_from_tensor_list (engine/utils.py:278-295) -- by one pinned upload and two launches per batch
(grit_image_batch_fwd).  The uint8 stage is bit-identical to Pillow; the float stage is a lookup in a 3 x 256 table that
is built here with the same torch ops ToTensor / Normalize apply (`v.float().div(255)`, `.sub(mean).div(std)`).

The tap tables depend only on (source size, target size) per axis; they are computed by the library's host function
grit_resample_taps_bicubic and cached.

With `augment` (one plan per image, drawn by datasets/caption/transforms/randaug.py) the resized uint8 image goes through
the reference's RandAugment operations before the float stage (grit_image_batch_aug_fwd: one launch per stage for the
whole batch, every image with its own operation).  The host turns a plan into integers only -- operation codes, the bits
of the fp32 factors, Pillow's 16.16 fixed-point affine coefficients, the index tables of the translations (`plan_augment`)
-- which travel in the same pinned blob; the result is bit-identical to Pillow's.

`image_batch_geo` is the detector's input (datasets/detection/transforms.py): per image a plan of ('hflip',), ('resize', oh, ow)
and ('crop', top, left, h, w) steps, resized with Pillow's BILINEAR taps as torchvision's `resize` does.  `plan_geo` folds a
plan into at most two resizes over source windows -- a crop moves the window, a flip mirrors the taps of the next horizontal
pass -- and grit_image_batch_geo_fwd runs them: two launches per batch, four when some image resizes twice."""
import ctypes
import functools
import math

import numpy as np
import torch

from grit_amd import lib as _lib
from grit_amd.ops.jpeg import EncodedJpeg, decode_batch
from grit_amd.ops.staging import Staging as _Staging

MEAN = (0.485, 0.456, 0.406)  # transforms/__init__.py:6-7
STD = (0.229, 0.224, 0.225)
DESC_FIELDS, SRC_PAD = _lib.IMAGE_DESC_FIELDS, _lib.IMAGE_SRC_PAD
AUG_STAGES, AUG_FIELDS = _lib.IMAGE_AUG_STAGES, _lib.IMAGE_AUG_FIELDS
AUG_COPY, AUG_AUTOCONTRAST, AUG_AFFINE_FIXED, AUG_AFFINE_TABLE = (_lib.AUG_COPY, _lib.AUG_AUTOCONTRAST, _lib.AUG_AFFINE_FIXED,
                                                                  _lib.AUG_AFFINE_TABLE)
AUG_BLEND = {'Color': _lib.AUG_COLOR, 'Contrast': _lib.AUG_CONTRAST, 'Brightness': _lib.AUG_BRIGHTNESS, 'Sharpness': _lib.AUG_SHARPNESS}


def tmp_pitch(dst_w):
    return (3 * dst_w + 3) & ~3  # GRIT_IMAGE_TMP_PITCH


@functools.lru_cache(maxsize=4096)
def axis_taps(in_size, out_size, filter='bicubic'):
    """-> (ksize, bounds int32 [out_size, 2], taps int32 [out_size, ksize]) of one axis (host, cached); filter: Pillow's
    'bicubic' or 'bilinear'."""
    lib = _lib.load()
    if filter not in ('bicubic', 'bilinear'):
        raise ValueError("unknown resampling filter %r" % (filter,))
    name = "grit_resample_taps_" + filter
    build = getattr(lib, name)
    ksize = build(in_size, out_size, None, None, 0)
    if ksize <= 0:
        raise _lib.GritHipError("%s(%d, %d) failed" % (name, in_size, out_size))
    bounds = np.empty((out_size, 2), np.int32)
    taps = np.empty((out_size, ksize), np.int32)
    got = build(in_size, out_size, bounds.ctypes.data_as(ctypes.c_void_p), taps.ctypes.data_as(ctypes.c_void_p), taps.size)
    if got != ksize:
        raise _lib.GritHipError("%s(%d, %d) failed" % (name, in_size, out_size))
    return ksize, bounds, taps


@functools.lru_cache(maxsize=4096)
def mirrored_taps(in_size, out_size, filter='bilinear'):
    """axis_taps for a row that is read back to front: resize(hflip(row)) = these taps on the row as stored.  Each output's
    taps are reversed and first' = in_size - first - count; integer sums, so the order of the terms does not matter."""
    ksize, bounds, taps = axis_taps(in_size, out_size, filter)
    first, count = bounds[:, 0], bounds[:, 1]
    source = count[:, None] - 1 - np.arange(ksize, dtype=np.int32)[None, :]
    flipped = np.where(source >= 0, np.take_along_axis(taps, np.maximum(source, 0), 1), 0).astype(np.int32)
    return ksize, np.stack([in_size - first - count, count], 1).astype(np.int32), flipped


@functools.lru_cache(maxsize=16)
def _lut(mean, std, device):
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)  # ToTensor
    m = torch.as_tensor(mean, dtype=torch.float32)[:, None]
    s = torch.as_tensor(std, dtype=torch.float32)[:, None]
    return v[None, :].sub(m).div(s).contiguous().to(device)  # Normalize


_pixels_staging, _tables_staging = _Staging(), _Staging()


def _as_u8(img):
    if isinstance(img, EncodedJpeg):  # decoded by the device, straight into the source blob (_upload_pixels)
        return img
    if isinstance(img, torch.Tensor):
        t = img
    else:
        arr = np.ascontiguousarray(np.asarray(img))  # numpy array or PIL image (decoded, RGB)
        t = torch.from_numpy(arr if arr.flags.writeable else arr.copy())  # PIL hands out read-only views
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("expected decoded RGB images as [h, w, 3] uint8, got %s %s" % (tuple(t.shape), t.dtype))
    return t.contiguous()


def plan(shapes, sizes):
    """Host side of one batch: -> (desc int64 [B, 12], tables int32 [n], tmp_bytes, src_bytes)."""
    desc = np.empty((len(shapes), DESC_FIELDS), np.int64)
    parts, n, src_off, tmp_off = [], 0, 0, 0
    placed = {}

    def place(key, arr):
        nonlocal n
        if key not in placed:
            placed[key] = n
            parts.append(arr.reshape(-1))
            n += arr.size
            if n % 2:  # the kernels read (first, count) pairs as one 8-byte load
                parts.append(np.zeros(1, np.int32))
                n += 1
        return placed[key]

    for i, ((h, w), (oh, ow)) in enumerate(zip(shapes, sizes)):
        if min(h, w, oh, ow) <= 0:
            raise ValueError("empty image or target size: %s -> %s" % ((h, w), (oh, ow)))
        kx, xb, xt = axis_taps(w, ow)
        ky, yb, yt = axis_taps(h, oh)
        desc[i] = (src_off, h, w, oh, ow, kx, ky, place(('b', w, ow), xb), place(('t', w, ow), xt),
                   place(('b', h, oh), yb), place(('t', h, oh), yt), tmp_off)
        src_off += h * w * 3
        tmp_off += h * tmp_pitch(ow)
    return desc, np.concatenate(parts), tmp_off, src_off


def affine_coefficients(name, v, w, h):
    """The six coefficients Pillow's Image.transform(AFFINE) receives for one geometric operation on a w x h image (output
    (x, y) -> input), in Python doubles; None when Pillow returns a plain copy (Image.rotate by a multiple of 360)."""
    if name == 'ShearX':
        return (1, v, 0, 0, 1, 0)
    if name == 'ShearY':
        return (1, 0, 0, v, 1, 0)
    if name == 'TranslateXabs':
        return (1, 0, v, 0, 1, 0)
    if name == 'TranslateYabs':
        return (1, 0, 0, 0, 1, v)
    if name != 'Rotate':
        raise ValueError("not a geometric operation: %r" % (name,))
    angle = v % 360.0  # Image.rotate
    if angle == 0:
        return None
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def affine_fixed(a, w, h):
    """Pillow's affine_fixed: the six 16.16 integers A0..A5 of xin = (A2 + A0 x + A1 y) >> 16, yin = (A5 + A3 x + A4 y) >> 16."""
    for x, y in ((0, 0), (w, 0), (0, h), (w, h)):  # Pillow's check_fixed: the walk must stay inside 16.16
        if not (abs(x * a[0] + y * a[1] + a[2]) < 32768.0 and abs(x * a[3] + y * a[4] + a[5]) < 32768.0):
            raise ValueError("affine coefficients %s leave the 16.16 fixed-point range on a %d x %d image" % (a, w, h))
    fix = lambda t: int(math.floor(t * 65536.0 + 0.5))
    return (fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5))


@functools.lru_cache(maxsize=4096)
def affine_axis_table(start, step, n):
    """Pillow's ImagingScaleAffine index table of one axis: a running double `start + step / 2`, `+= step` per index (repeated
    additions, not a product), -1 where it is negative.  int32 [n]; entries >= the source size also mean "outside"."""
    walk = np.full(n, step, np.float64)
    walk[0] = start + step * 0.5
    walk = np.cumsum(walk)  # sequential: ((o + step) + step) + ..., one rounding per addition like the C loop
    return np.where(walk < 0.0, -1, np.minimum(walk, 2.0 ** 31 - 1)).astype(np.int32)  # the cast truncates toward zero


def plan_augment(sizes, plans, table_base=0):
    """Host side of the augmentation: sizes [(oh, ow)], one plan ((name, magnitude, negate), ...) per image ->
    (aug int32 [B, 36], extra int32 tables (placed at element `table_base` of the tables blob), n_stages, work_bytes).
    Operations that leave every byte alone (Identity, a rotation Pillow turns into a copy) take no stage."""
    aug = np.zeros((len(sizes), AUG_FIELDS), np.int32)
    parts, n, placed, off, n_stages = [], 0, {}, 0, 0

    def place(key):
        nonlocal n
        if key not in placed:
            placed[key] = table_base + n
            parts.append(affine_axis_table(*key))
            n += key[2]
        return placed[key]

    for i, ((h, w), ops) in enumerate(zip(sizes, plans)):
        if len(ops) > AUG_STAGES:
            raise ValueError("at most %d operations per image, got %d" % (AUG_STAGES, len(ops)))
        records = []
        for name, val, negate in ops:
            if name == 'Identity':
                continue
            if name == 'AutoContrast':
                records.append((AUG_AUTOCONTRAST,))
            elif name in AUG_BLEND:
                records.append((AUG_BLEND[name], int(np.float32(val).view(np.int32))))
            else:
                a = affine_coefficients(name, -val if negate else val, w, h)
                if a is None:
                    continue
                if a[1] != 0 or a[3] != 0:
                    records.append((AUG_AFFINE_FIXED,) + affine_fixed(a, w, h))
                else:
                    records.append((AUG_AFFINE_TABLE, place((float(a[2]), float(a[0]), w)), place((float(a[5]), float(a[4]), h))))
        aug[i, 0], aug[i, 1] = off, len(records)
        for s, rec in enumerate(records):
            aug[i, 4 + 8 * s:4 + 8 * s + len(rec)] = rec
        n_stages = max(n_stages, len(records))
        off += h * tmp_pitch(w)
        if off >= 2 ** 31:
            raise ValueError("resized batch exceeds 2 GiB")
    extra = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return aug, extra, n_stages, off


def _upload_pixels(imgs, offsets, src_bytes, device):
    """The packed source blob on the device, GRIT_IMAGE_SRC_PAD readable bytes behind the last image."""
    encoded = [k for k, im in enumerate(imgs) if isinstance(im, EncodedJpeg)]
    if encoded:  # one reconstruction for all of them, written where the resize reads; decoded entries are copied next to them
        src = torch.empty(src_bytes + SRC_PAD, dtype=torch.uint8, device=device)
        decode_batch([imgs[k] for k in encoded], device, out=src, offsets=[offsets[k] for k in encoded])
        for im, off in zip(imgs, offsets):
            if not isinstance(im, EncodedJpeg):
                src[off:off + im.numel()].copy_(im.reshape(-1), non_blocking=im.is_cuda or im.is_pinned())
        return src
    if all(im.is_cuda for im in imgs):
        return torch.cat([im.reshape(-1) for im in imgs] + [torch.zeros(SRC_PAD, dtype=torch.uint8, device=device)])
    if all(im.is_cuda or im.is_pinned() for im in imgs):  # decoder wrote into pinned memory: no staging copy
        src = torch.empty(src_bytes + SRC_PAD, dtype=torch.uint8, device=device)
        for im, off in zip(imgs, offsets):
            src[off:off + im.numel()].copy_(im.reshape(-1), non_blocking=True)
        return src
    slot = _pixels_staging.take(src_bytes + SRC_PAD)  # one pinned staging blob, one asynchronous upload
    for im, off in zip(imgs, offsets):
        slot[0][off:off + im.numel()].copy_(im.reshape(-1))
    return _pixels_staging.upload(slot, src_bytes + SRC_PAD, device)


def _upload_tables(device, *arrays):
    """Descriptor (int64) and tables (int32) travel in one pinned blob: -> one device view per array (None stays None)."""
    sizes = [0 if a is None else a.dtype.itemsize * a.size for a in arrays]
    slot = _tables_staging.take(sum(sizes))
    at = 0
    for a, n in zip(arrays, sizes):
        if n:
            slot[0][at:at + n].copy_(torch.from_numpy(a.reshape(-1)).view(torch.uint8))
        at += n
    dev = _tables_staging.upload(slot, at, device)
    views, at = [], 0
    for n in sizes:
        views.append(dev[at:at + n])
        at += n
    return views


def image_batch(images, sizes, mean=MEAN, std=STD, device=None, pad_to=None, augment=None):
    """images: list of [h, w, 3] uint8 (torch / numpy / PIL, host or device) or EncodedJpeg (ops/jpeg.py: reconstructed on
    the device by one decode_batch in front of the launches); sizes: list of (oh, ow).
    augment: None, or one RandAugment plan ((name, magnitude, negate), ...) per image (may be empty), applied to the
    resized uint8 image before ToTensor as Pillow would.

    -> (tensors [B, 3, H, W] f32, mask [B, H, W] bool) on `device`, H = max oh, W = max ow -- or `pad_to` = (H, W), the
    fixed canvas the feature extractor needs (the reference gets it by appending a dummy H x W image to every batch,
    tools/extract_features.py:103)."""
    imgs = [_as_u8(im) for im in images]
    if len(imgs) == 0 or len(imgs) != len(sizes):
        raise ValueError("need one target size per image and at least one image")
    if augment is not None and len(augment) != len(imgs):
        raise ValueError("need one augmentation plan per image")
    if device is None:
        device = imgs[0].device if imgs[0].is_cuda else torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.GritHipError("Not implemented on the CPU: the image pipeline runs as HIP kernels")
    lib = _lib.load()
    desc, tables, tmp_bytes, src_bytes = plan([tuple(im.shape[:2]) for im in imgs], [tuple(s) for s in sizes])
    H, W = int(desc[:, 3].max()), int(desc[:, 4].max())
    max_dst_h, max_dst_w = H, W
    if augment is not None:
        aug, extra, n_stages, work_bytes = plan_augment([tuple(s) for s in sizes], augment, tables.size)
        tables = np.concatenate([tables, extra])
    if pad_to is not None:
        if pad_to[0] < H or pad_to[1] < W:
            raise ValueError("pad_to %s is smaller than the largest resized image (%d, %d)" % (tuple(pad_to), H, W))
        H, W = int(pad_to[0]), int(pad_to[1])
    B = len(imgs)
    with _lib.device_guard(device):
        src = _upload_pixels(imgs, desc[:, 0].tolist(), src_bytes, device)
        d_desc, d_tables, d_aug = _upload_tables(device, desc, tables, aug if augment is not None else None)
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=device)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
        mask = torch.empty(B, H, W, dtype=torch.bool, device=device)
        p = _lib.ptr
        if augment is not None:
            work = torch.empty(2 * work_bytes, dtype=torch.uint8, device=device)
            blocks = ((max_dst_h * ((max_dst_w + 3) // 4) + 255) // 256 + 7) // 8 * 8  # GRIT_IMAGE_AUG_BLOCKS
            stats = torch.empty(B * AUG_STAGES * blocks * 8, dtype=torch.int32, device=device)
            st = lib.grit_image_batch_aug_fwd(p(src), p(d_desc), p(d_tables), p(tmp), p(_lut(tuple(mean), tuple(std), device)),
                                              p(d_aug), n_stages, p(work), work_bytes, p(stats), B, int(desc[:, 1].max()),
                                              max_dst_h, max_dst_w, int(desc[:, 5].max()), H, W, p(out), p(mask),
                                              _lib.current_stream_ptr())
            _lib.check(st, "grit_image_batch_aug_fwd")
            return out, mask
        st = lib.grit_image_batch_fwd(p(src), p(d_desc), p(d_tables), p(tmp), p(_lut(tuple(mean), tuple(std), device)),
                                      B, int(desc[:, 1].max()), max_dst_w, int(desc[:, 5].max()), H, W, p(out), p(mask), _lib.current_stream_ptr())
        _lib.check(st, "grit_image_batch_fwd")
    return out, mask


GEO_FIELDS = _lib.IMAGE_GEO_FIELDS


def fold_geo(h, w, ops):
    """One image's plan -> its resizes, each (top, left, win_h, win_w, mirrored, oh, ow): the window of the image that resize
    reads (the [h, w] source for the first, the previous result for the second) and whether its rows are read back to front.
    A crop moves the window (inside a pending flip its left edge is counted from the right), a flip toggles `mirrored` of the
    next resize; a flip or crop with no resize after it, or an empty plan, gets an identity resize."""
    resizes = []
    top, left, ch, cw, mirrored = 0, 0, h, w, False
    full = (h, w)  # size of the image the window lies in
    for op in ops:
        if op[0] == 'hflip' and len(op) == 1:
            mirrored = not mirrored
        elif op[0] == 'crop' and len(op) == 5:
            t, l, hh, ww = (int(v) for v in op[1:])
            if t < 0 or l < 0 or hh <= 0 or ww <= 0 or t + hh > ch or l + ww > cw:
                raise ValueError("crop (top %d, left %d, %d x %d) leaves the %d x %d image" % (t, l, hh, ww, ch, cw))
            top += t
            left += cw - l - ww if mirrored else l
            ch, cw = hh, ww
        elif op[0] == 'resize' and len(op) == 3:
            oh, ow = int(op[1]), int(op[2])
            if oh <= 0 or ow <= 0:
                raise ValueError("empty target size: %s" % (op,))
            resizes.append((top, left, ch, cw, mirrored, oh, ow))
            top, left, ch, cw, mirrored, full = 0, 0, oh, ow, False, (oh, ow)
        else:
            raise ValueError("unknown plan step %r" % (op,))
    if not resizes or mirrored or (top, left, ch, cw) != (0, 0) + full:
        resizes.append((top, left, ch, cw, mirrored, ch, cw))
    if len(resizes) > 2:
        raise ValueError("a plan folds into at most two resizes, this one needs %d: %s" % (len(resizes), tuple(ops)))
    return resizes


class GeoPlan(object):
    """Host side of one detector batch, see plan_geo."""
    __slots__ = ('geo', 'tables', 'tmp_bytes', 'work_bytes', 'src_bytes', 'src_offsets', 'sizes', 'a_max', 'b_max')


def plan_geo(shapes, plans, filter='bilinear'):
    """shapes [(h, w)], one plan per image -> GeoPlan: geo int64 [B, 30] (grit_hip.h), tables int32 [n], the bytes of the
    intermediate, of the work buffer (without its readable tail) and of the source blob, every image's offset in the blob,
    the final (oh, ow) per image, and the maxima (src_h, dst_h, dst_w, kx) over the A and the B records (A: zeros when no
    image resizes twice)."""
    p = GeoPlan()
    p.geo = np.zeros((len(shapes), GEO_FIELDS), np.int64)
    parts, n, placed = [], 0, {}
    p.src_offsets, p.sizes = [], []
    src_off = tmp_off = work_off = 0
    a_max, b_max = [0, 0, 0, 0], [0, 0, 0, 0]

    def place(key, arr):
        nonlocal n
        if key not in placed:
            placed[key] = n
            parts.append(arr.reshape(-1))
            n += arr.size
            if n % 2:  # the kernels read (first, count) pairs as one 8-byte load
                parts.append(np.zeros(1, np.int32))
                n += 1
        return placed[key]

    for i, ((h, w), ops) in enumerate(zip(shapes, plans)):
        if min(h, w) <= 0:
            raise ValueError("empty image: %s" % ((h, w),))
        resizes = fold_geo(int(h), int(w), ops)
        p.geo[i, 0] = len(resizes)
        buf, base, pitch = 0, src_off, 3 * w  # where the first resize reads
        for which, (top, left, wh, ww, mirrored, oh, ow) in enumerate(resizes, 2 - len(resizes)):  # a single resize is record B
            kx, xb, xt = (mirrored_taps if mirrored else axis_taps)(ww, ow, filter)
            ky, yb, yt = axis_taps(wh, oh, filter)
            out_off = work_off if which == 0 else 0
            p.geo[i, 2 + 14 * which:16 + 14 * which] = (
                buf, base + top * pitch + 3 * left, pitch, wh, oh, ow, kx, ky,
                place(('b', ww, ow, mirrored), xb), place(('t', ww, ow, mirrored), xt),
                place(('b', wh, oh, False), yb), place(('t', wh, oh, False), yt), tmp_off, out_off)
            tmp_off += wh * tmp_pitch(ow)
            m = a_max if which == 0 else b_max
            m[:] = max(m[0], wh), max(m[1], oh), max(m[2], ow), max(m[3], kx)
            if which == 0:  # the second resize reads this one's rows in the work buffer
                buf, base, pitch = 1, work_off, tmp_pitch(ow)
                work_off += oh * tmp_pitch(ow)
        p.src_offsets.append(src_off)
        p.sizes.append((oh, ow))
        src_off += h * w * 3
    if max(src_off, tmp_off, work_off) >= 2 ** 31:
        raise ValueError("batch exceeds 2 GiB")
    p.tables = np.concatenate(parts)
    p.tmp_bytes, p.work_bytes, p.src_bytes, p.a_max, p.b_max = tmp_off, work_off, src_off, tuple(a_max), tuple(b_max)
    return p


def image_batch_geo(images, plans, mean=MEAN, std=STD, device=None, pad_to=None):
    """images: list of [h, w, 3] uint8 (torch / numpy / PIL, host or device) or EncodedJpeg; plans: per image a sequence of ('hflip',),
    ('resize', oh, ow) and ('crop', top, left, h, w) in the order a PIL chain would apply them (at most two resizes; resizes
    are Pillow's BILINEAR, what torchvision.transforms.functional.resize does to a PIL image).

    -> (tensors [B, 3, H, W] f32, mask [B, H, W] bool) on `device` as image_batch returns them."""
    imgs = [_as_u8(im) for im in images]
    if len(imgs) == 0 or len(imgs) != len(plans):
        raise ValueError("need one plan per image and at least one image")
    if device is None:
        device = imgs[0].device if imgs[0].is_cuda else torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.GritHipError("Not implemented on the CPU: the image pipeline runs as HIP kernels")
    lib = _lib.load()
    g = plan_geo([tuple(im.shape[:2]) for im in imgs], plans)
    H, W = max(s[0] for s in g.sizes), max(s[1] for s in g.sizes)
    if pad_to is not None:
        if pad_to[0] < H or pad_to[1] < W:
            raise ValueError("pad_to %s is smaller than the largest resized image (%d, %d)" % (tuple(pad_to), H, W))
        H, W = int(pad_to[0]), int(pad_to[1])
    B = len(imgs)
    with _lib.device_guard(device):
        src = _upload_pixels(imgs, g.src_offsets, g.src_bytes, device)
        d_geo, d_tables = _upload_tables(device, g.geo, g.tables)
        tmp = torch.empty(g.tmp_bytes, dtype=torch.uint8, device=device)
        # the row pass of resize B fetches whole dwords past a window that ends with the buffer: the blob's readable tail
        work = torch.empty(g.work_bytes + SRC_PAD, dtype=torch.uint8, device=device) if g.work_bytes else None
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
        mask = torch.empty(B, H, W, dtype=torch.bool, device=device)
        p = _lib.ptr
        st = lib.grit_image_batch_geo_fwd(p(src), p(d_geo), p(d_tables), p(tmp), p(work), p(_lut(tuple(mean), tuple(std), device)), B,
                                          g.a_max[0], g.a_max[1], g.a_max[2], g.a_max[3], g.b_max[0], g.b_max[2], g.b_max[3],
                                          H, W, p(out), p(mask), _lib.current_stream_ptr())
        _lib.check(st, "grit_image_batch_geo_fwd")
    return out, mask
