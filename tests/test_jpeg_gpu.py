"""Device side of the JPEG decoder (grit_amd/ops/jpeg.py, grit_amd/csrc/jpeg.hip) against fixture G22: the pixels are
Pillow's in every byte, alone, batched, and behind the resize of image_batch / image_batch_geo."""
import ctypes

import numpy as np
import pytest
import torch

from grit_amd import lib as _lib
from grit_amd.datasets.caption.transforms import collate_images
from grit_amd.datasets.caption.transforms.utils import FixedResize, MaxWHResize
from grit_amd.ops import jpeg
from tests import jpeg_model
from tests.jpeg_fixture import Fixture, with_quant

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g22():
    return Fixture()


def fresh(g22, i, with_coef=True):
    """A new item of file i: decode_batch must not depend on state left in a shared one."""
    it = jpeg.probe(g22.data[i])
    return jpeg.entropy(it) if with_coef else it


def test_whole_fixture_in_one_batch(g22):
    """Mixed sizes, samplings, tables and restart intervals; half of the items arrive without coefficients (thread pool)."""
    items = [fresh(g22, i, with_coef=k % 2 == 0) for k, i in enumerate(g22.accepted)]
    out = jpeg.decode_batch(items, 'cuda')
    base = out[0].untyped_storage().data_ptr()
    for k, i in enumerate(g22.accepted):
        assert out[k].dtype == torch.uint8 and out[k].is_cuda and out[k].untyped_storage().data_ptr() == base
        assert np.array_equal(out[k].cpu().numpy(), g22.pixels[i]), g22.meta[i]['name']
    again = jpeg.decode_batch([fresh(g22, i) for i in g22.accepted], 'cuda', threads=1)
    assert all(torch.equal(a, b) for a, b in zip(out, again))  # two calls, identical bytes


@pytest.mark.parametrize('size', [(1, 1), (5, 4), (9, 17), (17, 33)])
def test_single_images(g22, size):
    picked = [i for i in g22.accepted if (g22.meta[i]['width'], g22.meta[i]['height']) == size]
    for sampling in ((2, 2), (2, 1)):  # in colour, with and without restart markers; 4:4:4 and grey besides
        assert g22.colour(size, sampling, False) and g22.colour(size, sampling, True), sampling
    assert {g22.meta[i]['ncomp'] for i in picked} == {1, 3} and len(picked) >= 6
    for i in picked:
        out, = jpeg.decode_batch([fresh(g22, i)], 'cuda')
        assert tuple(out.shape) == g22.pixels[i].shape
        assert np.array_equal(out.cpu().numpy(), g22.pixels[i]), g22.meta[i]['name']


def reconstruct_raw(blocks_per_image):
    """blocks_per_image: list of [6, 64] int16 -- the four Y blocks, Cb, Cr of ONE 4:2:0 MCU (16 x 16 pixels), unit
    quantisation -- through grit_jpeg_reconstruct directly -> (device pixels [n, 16, 16, 3], model pixels)."""
    n = len(blocks_per_image)
    jobs = (jpeg.JpegJob * n)()
    for i, job in enumerate(jobs):
        job.coef_off[:] = [i * 384, i * 384 + 256, i * 384 + 320]
        job.plane_off[:] = [i * 384, i * 384 + 256, i * 384 + 320]
        job.out_off = i * 768
        job.width, job.height, job.ncomp, job.hmax, job.vmax = 16, 16, 3, 2, 2
        job.block_cols[:], job.block_rows[:] = [2, 1, 1], [2, 1, 1]
        job.quant[:] = [1] * 192
    coef = torch.from_numpy(np.stack(blocks_per_image).astype(np.int16)).cuda()
    d_jobs = torch.from_numpy(np.frombuffer(jobs, np.uint8).copy()).cuda()
    planes = torch.empty(n * 384, dtype=torch.uint8, device='cuda')
    out = torch.empty(n * 768, dtype=torch.uint8, device='cuda')
    st = _lib.load().grit_jpeg_reconstruct(_lib.ptr(d_jobs), n, 4, 256, _lib.ptr(coef), _lib.ptr(planes), _lib.ptr(out),
                                           _lib.current_stream_ptr())
    _lib.check(st, "grit_jpeg_reconstruct")
    want = [jpeg_model.reconstruct(16, 16, 2, 2, [b[:4].reshape(2, 2, 64), b[4:5].reshape(1, 1, 64), b[5:6].reshape(1, 1, 64)],
                                   [np.ones(64, np.int64)] * 3) for b in blocks_per_image]
    return out.view(n, 16, 16, 3).cpu().numpy(), np.stack(want)


def test_extreme_blocks():
    """The widest intermediates of both passes and the wrap branch of the range limit: every coefficient at +-8191 in
    alternating signs, DC alone at +-8191, one AC coefficient at each of the 63 positions."""
    B = 8191
    images = []
    checker = np.where((np.arange(64) // 8 + np.arange(64) % 8) % 2 == 0, B, -B)
    stripes = np.where(np.arange(64) % 2 == 0, B, -B)
    images.append(np.stack([checker, -checker, stripes, -stripes, checker, -stripes]))
    images.append(np.stack([np.full(64, B), np.full(64, -B), checker, stripes, np.full(64, -B), np.full(64, B)]))
    for signs in ((1, -1, 1, -1, 1, -1), (-1, 1, 1, -1, -1, 1), (1, 1, 1, 1, -1, -1)):
        dc = np.zeros((6, 64), np.int64)
        dc[:, 0] = np.array(signs) * B
        images.append(dc)
    for sign in (1, -1):
        for first in range(1, 64, 6):  # six positions per MCU, one per block
            ac = np.zeros((6, 64), np.int64)
            for b in range(6):
                ac[b, 1 + (first - 1 + b) % 63] = sign * B if b % 2 == 0 else -sign * B
            images.append(ac)
    got, want = reconstruct_raw(images)
    assert set(np.unique(want)) - {0, 255}, "the patterns must reach more than the clamped ends"
    wild = jpeg_model.idct_islow(np.stack(images[:2]).reshape(-1, 8, 8))
    assert len(np.unique(wild)) > 2  # wrapped samples: a clamp would give 0 and 255 only
    for k in range(len(images)):
        assert np.array_equal(got[k], want[k]), "pattern %d" % k


def picks(g22):
    """The accepted files large enough for every policy below: five sizes, every sampling, grey, with and without restarts."""
    chosen = [i for i in g22.accepted if min(g22.meta[i]['width'], g22.meta[i]['height']) >= 16]
    kinds = {(g22.meta[i]['ncomp'], g22.meta[i]['hmax'], g22.meta[i]['vmax']) for i in chosen}
    assert kinds == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)} and {g22.meta[i]['restart'] for i in chosen} == {0, 1, 3}
    odd = [i for i in chosen if g22.meta[i]['width'] % 2 and g22.meta[i]['height'] % 2]
    assert {(g22.meta[i]['hmax'], g22.meta[i]['vmax'], g22.meta[i]['restart'] > 0) for i in odd if g22.meta[i]['ncomp'] == 3} >= {
        (2, 2, False), (2, 2, True), (2, 1, False), (2, 1, True)}
    assert len({g22.pixels[i].shape for i in chosen}) >= 5
    return chosen


def same_batch(a, b):
    assert a.tensors.dtype == torch.float32 and torch.equal(a.tensors, b.tensors) and torch.equal(a.mask, b.mask)


@pytest.mark.parametrize('policy, pad_to', [(MaxWHResize((24, 40)), None), (FixedResize((20, 28)), None),
                                            (MaxWHResize((24, 40)), (32, 64)), (FixedResize((20, 28)), (32, 32))],
                         ids=['maxwh', 'normal', 'maxwh-pad', 'normal-pad'])
def test_collate_images_on_encoded_items(g22, policy, pad_to):
    chosen = picks(g22)
    encoded = collate_images([policy(fresh(g22, i)) for i in chosen], 'cuda', pad_to=pad_to)
    decoded = collate_images([policy(g22.pixels[i]) for i in chosen], 'cuda', pad_to=pad_to)
    same_batch(encoded, decoded)
    mixed = collate_images([policy(fresh(g22, i, with_coef=k % 3 == 0) if k % 2 else g22.pixels[i]) for k, i in enumerate(chosen)],
                           'cuda', pad_to=pad_to)
    same_batch(mixed, decoded)


def test_stream_refused_by_the_entropy_stage_takes_the_host_decode(g22):
    """A file that passes the probe and whose stream is refused (here: a coefficient outside the bound) is decoded by PIL
    inside decode_batch, next to images that take the kernels; the one test that reads live PIL output."""
    pytest.importorskip('PIL')
    import io
    from PIL import Image
    i, j = g22.index('optimize'), g22.index('one_mcu_420')
    wild = with_quant(g22.data[i], 255)
    assert jpeg.entropy(jpeg.probe(wild)) is None
    want = np.asarray(Image.open(io.BytesIO(wild)).convert('RGB'))
    a, b, c = jpeg.decode_batch([fresh(g22, j), jpeg.probe(wild), fresh(g22, i, with_coef=False)], 'cuda')
    assert np.array_equal(b.cpu().numpy(), want)
    assert np.array_equal(a.cpu().numpy(), g22.pixels[j]) and np.array_equal(c.cpu().numpy(), g22.pixels[i])
    alone, = jpeg.decode_batch([jpeg.probe(wild)], 'cuda')
    assert np.array_equal(alone.cpu().numpy(), want)


def test_bad_arguments(g22):
    it = fresh(g22, g22.accepted[0])
    with pytest.raises(TypeError):
        jpeg.decode_batch([g22.pixels[g22.accepted[0]]], 'cuda')
    with pytest.raises(ValueError):
        jpeg.decode_batch([it], 'cuda', out=torch.empty(4, dtype=torch.uint8, device='cuda'), offsets=[0, 0])
    with pytest.raises(ValueError):  # does not fit
        jpeg.decode_batch([it], 'cuda', out=torch.empty(2, dtype=torch.uint8, device='cuda'), offsets=[0])
    lib = _lib.load()
    assert lib.grit_jpeg_reconstruct(None, 1, 1, 1, None, None, None, None) == _lib.ERR_BAD_ARG
    assert lib.grit_jpeg_planes_bytes(ctypes.byref(it.info)) == (it.info.plane_bytes + 15) // 16 * 16
