"""JPEG decoding: the hybrid path (host entropy stage + two launches, grit_amd/ops/jpeg.py) next to Pillow, one process,
alternating rounds.  `python tools/bench_jpeg.py [--images 64] [--batch 32] [--rounds 5] [--out profiles/jpeg_decode/bench_jpeg.json]`

Input: seeded 640 x 480 images (low-frequency structure plus noise, so the files have the size of photographs), encoded by
Pillow at 4:2:0, quality 90 (`--files DIR` takes prepared files instead, e.g. where Pillow is missing).  Measured:
  * Pillow `Image.open(...).convert('RGB')` per image, 1 thread and `--threads` threads (host clock)
  * probe + entropy stage per image at the same thread counts (host clock)
  * the two launches of grit_jpeg_reconstruct for a batch, coefficients resident (HIP events), against the bytes they move:
    coefficients read, planes written and read, pixels written
  * the whole new path -- decode_batch from file bytes to device pixels, synchronised -- in images/s, against Pillow at
    `--threads` threads followed by image_batch's own upload of decoded arrays (one pinned blob, one copy): what the host
    path pays to get the same pixels to the device; the host-only rate is reported next to it
Every figure is the fastest round.  Needs a GPU; without Pillow the new path is reported alone."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grit_amd import lib as _lib  # noqa: E402
from grit_amd.ops import image_batch, jpeg  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None


def synthesise(n, seed=0):
    rng = np.random.default_rng(seed)
    files = []
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    for _ in range(n):
        img = np.zeros((480, 640, 3), np.float32)
        for _ in range(6):  # a few soft blobs and edges per channel
            cx, cy, r = rng.uniform(0, 640), rng.uniform(0, 480), rng.uniform(30, 200)
            img += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))[:, :, None] * rng.uniform(-120, 120, 3)
            img += (xx * rng.uniform(-1, 1) + yy * rng.uniform(-1, 1) > rng.uniform(-200, 400))[:, :, None] * rng.uniform(-40, 40, 3)
        img += 128 + rng.normal(0, 6, img.shape)
        b = io.BytesIO()
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(b, 'JPEG', quality=90, subsampling=2)
        files.append(b.getvalue())
    return files


def per_image(fn, files, threads):
    """Host milliseconds per image of fn over all files with `threads` threads."""
    t0 = time.perf_counter()
    if threads == 1:
        for f in files:
            fn(f)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(fn, files))
    return (time.perf_counter() - t0) * 1e3 / len(files)


def pillow_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def host_stage(data):
    item = jpeg.load(data)
    assert item is not None
    return item


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--threads', type=int, default=jpeg.default_threads())
    ap.add_argument('--files', default='')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py measures on the GPU: no HIP device visible")
    if a.files:
        names = sorted(n for n in os.listdir(a.files) if n.lower().endswith(('.jpg', '.jpeg')))
        files = [open(os.path.join(a.files, n), 'rb').read() for n in names]
    elif Image is None:
        raise SystemExit("no Pillow to encode the synthetic images with: pass --files DIR")
    else:
        files = synthesise(a.images)
    batch = files[:a.batch]
    result = {'images': len(files), 'batch': len(batch), 'threads': a.threads, 'affinity_cpus': len(os.sched_getaffinity(0)),
              'device': torch.cuda.get_device_name(0), 'file_bytes_mean': float(np.mean([len(f) for f in files])),
              'pillow': None if Image is None else Image.__version__}

    # correctness at the size that is timed
    items = [host_stage(f) for f in batch]
    pixels = jpeg.decode_batch(items, 'cuda')
    if Image is not None:
        assert all(np.array_equal(p.cpu().numpy(), pillow_decode(f)) for p, f in zip(pixels, batch)), "pixels differ from Pillow's"
        result['equal_to_pillow'] = True

    # the two launches alone
    lib = _lib.load()
    n = len(items)
    jobs = (jpeg.JpegJob * n)()
    elem = plane = out_at = 0
    for job, it in zip(jobs, items):
        info = it.info
        for c in range(info.ncomp):
            job.coef_off[c], job.plane_off[c] = elem, plane
            elem, plane = elem + 64 * info.block_cols[c] * info.block_rows[c], plane + 64 * info.block_cols[c] * info.block_rows[c]
        job.out_off, out_at = out_at, out_at + 3 * info.width * info.height
        job.width, job.height, job.ncomp, job.hmax, job.vmax = info.width, info.height, info.ncomp, info.hmax, info.vmax
        job.block_cols, job.block_rows, job.quant = info.block_cols, info.block_rows, info.quant
    d_jobs = torch.from_numpy(np.frombuffer(jobs, np.uint8).copy()).cuda()
    d_coef = torch.from_numpy(np.concatenate([it.coef for it in items])).cuda()
    d_planes = torch.empty(plane, dtype=torch.uint8, device='cuda')
    d_out = torch.empty(out_at + 64, dtype=torch.uint8, device='cuda')
    max_blocks = max(it.info.block_cols[0] * it.info.block_rows[0] for it in items)
    max_pixels = max(it.info.width * it.info.height for it in items)

    def launches():
        _lib.check(lib.grit_jpeg_reconstruct(_lib.ptr(d_jobs), n, max_blocks, max_pixels, _lib.ptr(d_coef), _lib.ptr(d_planes),
                                             _lib.ptr(d_out), _lib.current_stream_ptr()), "grit_jpeg_reconstruct")

    def kernels_ms(iters=200):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            launches()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def new_path():
        t0 = time.perf_counter()
        jpeg.decode_batch([jpeg.probe(f) for f in batch], 'cuda', threads=a.threads)
        torch.cuda.synchronize()
        return len(batch) / (time.perf_counter() - t0)

    def pillow_path():
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as pool:
            arrays = list(pool.map(pillow_decode, batch))
        host = time.perf_counter() - t0
        imgs = [image_batch._as_u8(arr) for arr in arrays]  # the host path's own upload: one pinned blob, one copy
        sizes = [im.numel() for im in imgs]
        offsets = [sum(sizes[:k]) for k in range(len(sizes))]
        image_batch._upload_pixels(imgs, offsets, sum(sizes), torch.device('cuda'))
        torch.cuda.synchronize()
        return len(batch) / host, len(batch) / (time.perf_counter() - t0)

    for _ in range(3):  # warm up: code objects, pinned slots, thread start-up
        launches()
        new_path()
    torch.cuda.synchronize()
    best = {}

    def keep(name, value, smaller=True):
        best[name] = value if name not in best else (min if smaller else max)(best[name], value)

    for _ in range(a.rounds):
        for threads in (1, a.threads):
            if Image is not None:
                keep('pillow_ms_per_image_%dt' % threads, per_image(pillow_decode, files, threads))
            keep('entropy_ms_per_image_%dt' % threads, per_image(host_stage, files, threads))
        keep('launches_ms_per_batch', kernels_ms())
        keep('new_path_images_per_s', new_path(), smaller=False)
        if Image is not None:
            host, with_upload = pillow_path()
            keep('pillow_images_per_s_host_only', host, smaller=False)
            keep('pillow_images_per_s_with_upload', with_upload, smaller=False)
    result.update(best)
    moved = d_coef.numel() * 2 + 2 * plane + out_at
    result['launch_bytes'] = moved
    result['launch_GB_per_s'] = moved / (best['launches_ms_per_batch'] * 1e-3) / 1e9
    if Image is not None:
        result['entropy_over_pillow_1t'] = best['entropy_ms_per_image_1t'] / best['pillow_ms_per_image_1t']
        result['new_over_pillow_with_upload'] = best['new_path_images_per_s'] / best['pillow_images_per_s_with_upload']
        result['new_over_pillow_host_only'] = best['new_path_images_per_s'] / best['pillow_images_per_s_host_only']
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
