"""Writes tests/golden/g22_jpeg.npz: small JPEG files (and three files the decoder must refuse) with the pixels Pillow
(libjpeg-turbo) decodes from them.  Needs Pillow and the built library; run by hand from the repository root:

    python tests/golden/make_jpeg_golden.py

Before writing, every accepted file goes through the library's host stage and the numpy model (tests/jpeg_model.py) and must
equal Pillow's pixels in every byte.  The family: every size x sampling in colour (noise or smooth in turn, so that neither
content is tied to a sampling), 4:2:2 and 4:2:0 with and without restart markers, 4:4:4 with one of the two at every other
size, and one grey file per size.  Contents of the archive: `meta` (JSON: one record per file -- name, accepted, width,
height, ncomp, hmax, vmax, restart, twin = index of the restart-free file of the same pixels and quality or -1), `f<i>` the
file's bytes, `p<i>` Pillow's Image.open(...).convert('RGB')."""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from grit_amd.ops import jpeg  # noqa: E402
from tests import jpeg_model  # noqa: E402

SIZES = [(1, 1), (2, 3), (3, 5), (5, 4), (8, 8), (9, 17), (16, 16), (17, 33), (24, 40), (31, 47), (33, 18)]  # (w, h)
SAMPLINGS = [(0, 1, 1), (1, 2, 1), (2, 2, 2)]  # Pillow's subsampling value, hmax, vmax
MAX_FILE = 2048


def content(kind, w, h, rng):
    if kind == 'noise':
        return Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'smooth':
        a = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1)
        return Image.fromarray(a.astype(np.uint8))
    grey = ((xx * 7 + yy * 13) % 256 + rng.integers(0, 40, (h, w))).clip(0, 255)
    return Image.fromarray(grey.astype(np.uint8), 'L')


def encode(img, fmt='JPEG', **kw):
    b = io.BytesIO()
    img.save(b, fmt, **kw)
    return b.getvalue()


def encode_small(img, quality, **kw):
    """At `quality`, or the next lower one at which the file keeps to MAX_FILE bytes with and without restart markers."""
    while True:
        data = encode(img, quality=quality, **kw)
        if len(data) <= MAX_FILE:
            return quality, data
        quality -= 5


def main():
    rng = np.random.default_rng(22)
    files = []  # (record, bytes, pixels)

    def add(name, data, accepted, restart=0, twin=-1):
        pixels = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        files.append(({'name': name, 'accepted': accepted, 'restart': restart, 'twin': twin}, data, pixels))
        return len(files) - 1

    for si, (w, h) in enumerate(SIZES):
        restart = (1, 3)[si % 2]
        for sj, (sub, _, _) in enumerate(SAMPLINGS):
            # colour at every size x sampling; content and sampling are not tied: noise and smooth both meet h2v1 and h2v2
            kind = ('noise', 'smooth')[(si + sj) % 2]
            img = content(kind, w, h, rng)
            quality = 30 + 10 * ((3 * si + sj) % 8)  # 30 .. 100
            quality, with_restart = encode_small(img, quality, subsampling=sub, restart_marker_blocks=restart)
            quality, plain = encode_small(img, quality, subsampling=sub)
            with_restart = encode(img, quality=quality, subsampling=sub, restart_marker_blocks=restart)
            assert len(with_restart) <= MAX_FILE
            base = '%dx%d_s%d_%s_q%d' % (w, h, sub, kind, quality)
            if sub == 0 and si % 2:  # thinning: 4:4:4 has no upsampling to cover, every other size goes without its plain twin
                add(base + '_r%d' % restart, with_restart, True, restart)
                continue
            twin = add(base, plain, True)
            add(base + '_r%d' % restart, with_restart, True, restart, twin)
        grey = content('grey', w, h, rng)  # one component, once per size, with and without restarts in turn
        quality = 40 + 10 * (si % 6)
        if si % 2:
            add('%dx%d_grey_q%d_r%d' % (w, h, quality, restart), encode(grey, quality=quality, restart_marker_blocks=restart), True, restart)
        else:
            add('%dx%d_grey_q%d' % (w, h, quality), encode(grey, quality=quality, subsampling=(0, 2)[si % 4 == 0]), True)
    add('optimize', encode(content('noise', 24, 20, rng), quality=85, subsampling=2, optimize=True), True)
    add('one_mcu_420', encode(content('noise', 16, 16, rng), quality=75, subsampling=2), True)
    add('progressive', encode(content('smooth', 24, 20, rng), quality=85, progressive=True), False)
    add('cmyk', encode(content('smooth', 16, 12, rng).convert('CMYK'), quality=85), False)
    add('png', encode(content('smooth', 16, 12, rng), 'PNG'), False)

    out = {}
    for i, (rec, data, pixels) in enumerate(files):
        item = jpeg.probe(data)
        assert (item is not None) == rec['accepted'], rec
        if item is not None:
            assert jpeg.entropy(item) is not None, rec
            info = item.info
            rec.update(width=info.width, height=info.height, ncomp=info.ncomp, hmax=info.hmax, vmax=info.vmax)
            assert info.restart_interval == rec['restart'], (rec, info.restart_interval)
            assert np.array_equal(jpeg_model.reconstruct_item(item), pixels), rec  # the model IS Pillow on this file
        else:
            rec.update(width=pixels.shape[1], height=pixels.shape[0], ncomp=0, hmax=0, vmax=0)
        out['f%d' % i] = np.frombuffer(data, np.uint8)
        out['p%d' % i] = pixels
    out['meta'] = np.array(json.dumps([rec for rec, _, _ in files]))
    path = os.path.join(ROOT, 'tests', 'golden', 'g22_jpeg.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 256 * 1024, size
    print('wrote %s: %d files (%d accepted), %d bytes' % (path, len(files), sum(r['accepted'] for r, _, _ in files), size))


if __name__ == '__main__':
    main()
