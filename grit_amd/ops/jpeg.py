"""JPEG files -> decoded RGB images on the device (DESIGN "JPEG decoding").

    file bytes --probe (markers)--> EncodedJpeg --entropy (Huffman, host, one thread per image)--> int16 coefficient planes
    --one pinned upload, two launches per batch (grit_jpeg_reconstruct)-->  [h, w, 3] uint8, the pixels of
    PIL's Image.open(path).convert('RGB') bit for bit (libjpeg-turbo defaults: JDCT_ISLOW, fancy upsampling)

Replaces the host decode of the reference's dataset workers (datasets/caption/field.py:65, tools/extract_features.py:42)
for baseline files.  Everything outside the accepted subset -- progressive, CMYK, other sampling factors, damaged streams; the
list stands at grit_jpeg_probe in include/grit_hip.h -- is refused: `probe` / `entropy` return None and the caller decodes
that file on the host as before.  `probe` and `entropy` need no GPU."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from grit_amd import lib as _lib
from grit_amd.ops.staging import Staging

JpegInfo, JpegJob = _lib.JpegInfo, _lib.JpegJob
SRC_PAD = _lib.IMAGE_SRC_PAD  # the buffer of decode_batch can be handed to image_batch as it is
_staging = Staging()


class EncodedJpeg(object):
    """One accepted file: `info` (grit_jpeg_info), `data` (the file's bytes) and, once the entropy stage ran, `coef` (int16
    [info.coef_bytes / 2], the component planes back to back).  `.shape` is that of the decoded image, so the resize
    policies take it where they take an array."""
    __slots__ = ('info', 'data', 'coef')
    is_cuda = False

    def __init__(self, info, data, coef=None):
        self.info, self.data, self.coef = info, data, coef

    @property
    def shape(self):
        return (self.info.height, self.info.width, 3)

    def __reduce__(self):  # dataset workers hand it to the main process; the file's bytes are done with once decoded
        return (_rebuild, (bytes(self.info), self.data if self.coef is None else None, self.coef))


def _rebuild(info, data, coef):
    return EncodedJpeg(JpegInfo.from_buffer_copy(info), data, coef)


def _address(data):
    return ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)


def probe(data_or_path):
    """bytes or a path -> EncodedJpeg (without coefficients), or None when the file is outside the accepted subset."""
    if isinstance(data_or_path, (str, os.PathLike)):
        with open(data_or_path, 'rb') as f:
            data = f.read()
    else:
        data = bytes(data_or_path)
    info = JpegInfo()
    st = _lib.load().grit_jpeg_probe(_address(data), len(data), ctypes.byref(info))
    if st == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(st, "grit_jpeg_probe")
    return EncodedJpeg(info, data)


def _entropy_into(item, coef):
    """The Huffman stage of `item` into the int16 array `coef`; the library's status."""
    return _lib.load().grit_jpeg_entropy(_address(item.data), len(item.data), ctypes.byref(item.info),
                                         coef.ctypes.data_as(ctypes.c_void_p), coef.nbytes)


def entropy(item):
    """Host only: fills item.coef and returns the item, or None when the stream is refused (damaged, or a coefficient outside
    the bound): decode that file on the host."""
    coef = np.empty(item.info.coef_bytes // 2, np.int16)
    st = _entropy_into(item, coef)
    if st == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(st, "grit_jpeg_entropy")
    item.coef = coef
    return item


def load(data_or_path):
    """probe + entropy: an EncodedJpeg ready for decode_batch, or None (decode on the host)."""
    item = probe(data_or_path)
    return entropy(item) if item is not None else None


def default_threads():
    return min(16, len(os.sched_getaffinity(0)))


def _align(n, to=16):
    return (n + to - 1) // to * to


def decode_batch(items, device, threads=None, out=None, offsets=None):
    """items: EncodedJpeg list -> list of [h, w, 3] uint8 device tensors, views of one buffer in which the images stand back
    to back.  Items without coefficients are entropy-decoded here, in a pool of `threads` (default: min(16, the CPUs this
    process may use)), straight into the pinned upload buffer; one whose stream the entropy stage refuses is decoded by PIL on the host, like the
    files probe refuses (its slot of the buffer is filled by a copy).  out / offsets: write image i at byte offsets[i] of the uint8
    device buffer `out` instead (image_batch's source blob) -- the views then are views of `out`."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.GritHipError("Not implemented on the CPU: the JPEG reconstruction runs as HIP kernels")
    n = len(items)
    if n == 0:
        raise ValueError("need at least one image")
    for it in items:
        if not isinstance(it, EncodedJpeg):
            raise TypeError("decode_batch expects EncodedJpeg items (ops.jpeg.probe), got %s" % type(it).__name__)
    lib = _lib.load()
    jobs = (JpegJob * n)()
    jobs_bytes = _align(ctypes.sizeof(jobs))
    coef_at, plane_at, out_at = [], 0, 0
    total = jobs_bytes
    own_out = out is None
    if not own_out and (not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or offsets is None or len(offsets) != n):
        raise ValueError("out must be a flat uint8 device buffer with one offset per image")
    for i, it in enumerate(items):
        info, job = it.info, jobs[i]
        coef_at.append(total)
        elem, plane = (total - jobs_bytes) // 2, plane_at
        for c in range(info.ncomp):
            job.coef_off[c], job.plane_off[c] = elem, plane
            blocks = info.block_cols[c] * info.block_rows[c]
            elem, plane = elem + 64 * blocks, plane + 64 * blocks
        job.out_off = out_at if own_out else int(offsets[i])
        if not own_out and not 0 <= job.out_off <= out.numel() - info.height * info.width * 3:
            raise ValueError("image %d does not fit into `out` at offset %d" % (i, job.out_off))
        job.width, job.height, job.ncomp, job.hmax, job.vmax = info.width, info.height, info.ncomp, info.hmax, info.vmax
        job.block_cols, job.block_rows, job.quant = info.block_cols, info.block_rows, info.quant
        total += info.coef_bytes
        plane_at += lib.grit_jpeg_planes_bytes(ctypes.byref(info))
        out_at += info.height * info.width * 3
    with _lib.device_guard(device):
        slot = _staging.take(total)
        blob = slot[0].numpy()
        views = [blob[at:at + it.info.coef_bytes].view(np.int16) for at, it in zip(coef_at, items)]
        todo, refused = [], []
        for it, view in zip(items, views):
            if it.coef is None:
                todo.append((it, view))
            else:
                view[:] = it.coef
        if todo:
            threads = default_threads() if threads is None else int(threads)
            if threads > 1 and len(todo) > 1:
                with ThreadPoolExecutor(min(threads, len(todo))) as pool:  # ctypes releases the GIL during the call
                    status = list(pool.map(lambda iv: _entropy_into(*iv), todo))
            else:
                status = [_entropy_into(it, view) for it, view in todo]
            for (it, _), st in zip(todo, status):
                if st == _lib.ERR_UNSUPPORTED:  # the stream is outside the subset after all: this image takes the host decode
                    refused.append(next(k for k, other in enumerate(items) if other is it))
                else:
                    _lib.check(st, "grit_jpeg_entropy")
        for k in refused:  # the launches skip an image without components
            jobs[k].ncomp = jobs[k].width = jobs[k].height = 0
        blob[:ctypes.sizeof(jobs)] = np.frombuffer(jobs, np.uint8)
        dev = _staging.upload(slot, total, device)
        planes = torch.empty(max(plane_at, 16), dtype=torch.uint8, device=device)
        if own_out:
            out = torch.empty(out_at + SRC_PAD, dtype=torch.uint8, device=device)
        max_blocks = max(it.info.block_cols[0] * it.info.block_rows[0] for it in items)  # luma has the most
        max_pixels = max(it.info.height * it.info.width for it in items)
        st = lib.grit_jpeg_reconstruct(_lib.ptr(dev), n, max_blocks, max_pixels, _lib.ptr(dev[jobs_bytes:]), _lib.ptr(planes),
                                       _lib.ptr(out), _lib.current_stream_ptr())
        _lib.check(st, "grit_jpeg_reconstruct")
    result = []
    for i, it in enumerate(items):
        at, size = jobs[i].out_off, it.info.height * it.info.width * 3
        result.append(out[at:at + size].view(it.info.height, it.info.width, 3))
    for k in refused:
        result[k].copy_(torch.from_numpy(_host_decode(items[k])))
    return result


def _host_decode(item):
    """The fallback of the format, not of a kernel: a file whose stream the entropy stage refuses (damage, a coefficient outside
    the bound) is decoded by PIL like every file that probe refuses."""
    import io
    from PIL import Image
    pixels = np.array(Image.open(io.BytesIO(item.data)).convert('RGB'))
    if pixels.shape != item.shape:
        raise _lib.GritHipError("host decode gave %s for a file probed as %s" % (pixels.shape, item.shape))
    return pixels
