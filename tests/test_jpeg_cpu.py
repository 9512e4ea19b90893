"""Host side of the device JPEG decoder (grit_amd/ops/jpeg.py, grit_amd/csrc/jpeg_host.h) against fixture G22
(tests/golden/make_jpeg_golden.py): probe, the entropy stage through the numpy model of the reconstruction, the dataset
plumbing, and a sanitizer run of the host stage as a stand-alone program.  No GPU."""
import json
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pytest

from grit_amd import lib as _lib
from grit_amd.datasets.caption.field import ImageField
from grit_amd.datasets.caption.transforms.utils import FixedResize, MaxWHResize, MinMaxResize
from grit_amd.ops import jpeg
from tests import jpeg_model
from tests.conftest import ROOT
from tests.jpeg_fixture import LISTED_SIZES, Fixture, with_quant


@pytest.fixture(scope='module')
def g22():
    return Fixture()


def test_fixture_covers_the_family(g22):
    """Every listed size in COLOUR at 4:2:0 and 4:2:2, with and without restart markers, and at 4:4:4; a grey file per size;
    noise and smooth content under every sampling."""
    assert len(g22.accepted) >= 60 and sorted(g22.meta[i]['name'] for i in g22.refused) == ['cmyk', 'png', 'progressive']
    for size in LISTED_SIZES:
        for sampling in ((2, 2), (2, 1)):
            for restart in (False, True):
                assert g22.colour(size, sampling, restart), (size, sampling, restart)
        assert g22.colour(size, (1, 1), False) or g22.colour(size, (1, 1), True), size
        assert any((g22.meta[i]['width'], g22.meta[i]['height'], g22.meta[i]['ncomp']) == size + (1,) for i in g22.accepted), size
    for sampling in ((1, 1), (2, 1), (2, 2)):
        kinds = {kind for i in g22.accepted for kind in ('noise', 'smooth')
                 if kind in g22.meta[i]['name'] and (g22.meta[i]['ncomp'], g22.meta[i]['hmax'], g22.meta[i]['vmax']) == (3,) + sampling}
        assert kinds == {'noise', 'smooth'}, sampling
    acc = [g22.meta[i] for i in g22.accepted]
    assert {m['restart'] for m in acc} == {0, 1, 3}
    assert {m['restart'] > 0 for m in acc if m['ncomp'] == 1} == {False, True}
    assert all(len(g22.data[i]) <= 2048 for i in g22.accepted)


def test_probe_accepts_and_refuses(g22):
    for i, m in enumerate(g22.meta):
        it = jpeg.probe(g22.data[i])
        assert (it is not None) == m['accepted'], m['name']
        if it is None:
            continue
        info = it.info
        assert it.shape == g22.pixels[i].shape == (m['height'], m['width'], 3), m['name']
        assert (info.ncomp, info.hmax, info.vmax, info.restart_interval) == (m['ncomp'], m['hmax'], m['vmax'], m['restart']), m['name']
        mcu_cols, mcu_rows = -(-m['width'] // (8 * info.hmax)), -(-m['height'] // (8 * info.vmax))
        assert (info.mcu_cols, info.mcu_rows) == (mcu_cols, mcu_rows)
        blocks = 0
        for c in range(info.ncomp):
            hs, vs = (info.hmax, info.vmax) if c == 0 else (1, 1)
            assert (info.block_cols[c], info.block_rows[c]) == (mcu_cols * hs, mcu_rows * vs), m['name']
            blocks += info.block_cols[c] * info.block_rows[c]
            assert all(1 <= q <= 255 for q in info.quant[64 * c:64 * c + 64])
        assert info.coef_bytes == 128 * blocks and info.plane_bytes == 64 * blocks
        assert g22.data[i][info.scan_offset - 3:info.scan_offset] == b'\x00\x3f\x00'  # the end of the SOS header
    assert jpeg.probe(b'') is None and jpeg.probe(b'\xff\xd8\xff') is None


def test_probe_reads_a_path(g22, tmp_path):
    path = tmp_path / 'a.jpg'
    path.write_bytes(g22.data[g22.accepted[5]])
    assert jpeg.probe(str(path)).shape == g22.pixels[g22.accepted[5]].shape
    assert jpeg.load(path).coef is not None


def test_entropy_then_model_equals_pillow(g22):
    for i in g22.accepted:
        assert np.array_equal(jpeg_model.reconstruct_item(g22.item(i)), g22.pixels[i]), g22.meta[i]['name']


def test_restart_files_carry_their_twins_coefficients(g22):
    pairs = [(i, g22.meta[i]['twin']) for i in g22.accepted if g22.meta[i]['twin'] >= 0]
    twinned = {(g22.meta[i]['width'], g22.meta[i]['height'], g22.meta[i]['hmax'], g22.meta[i]['vmax']) for i, _ in pairs}
    assert twinned >= {size + sampling for size in LISTED_SIZES for sampling in ((2, 1), (2, 2))}  # every size, both subsamplings
    for i, twin in pairs:
        assert g22.meta[i]['restart'] > 0 and g22.meta[twin]['restart'] == 0
        assert np.array_equal(g22.item(i).coef, g22.item(twin).coef), g22.meta[i]['name']
        assert np.array_equal(g22.pixels[i], g22.pixels[twin])


def test_entropy_refuses_damage_and_wrong_arguments(g22):
    i = g22.index('one_mcu_420')
    data = g22.data[i]
    assert jpeg.entropy(jpeg.EncodedJpeg(jpeg.probe(data).info, data[:-2])) is None  # no EOI
    assert jpeg.entropy(jpeg.EncodedJpeg(jpeg.probe(data).info, data[:-20] + data[-2:])) is None  # scan cut short
    other = jpeg.probe(g22.data[g22.accepted[0]])
    with pytest.raises(_lib.GritHipError):  # the record of another file
        jpeg.entropy(jpeg.EncodedJpeg(other.info, data))
    it = jpeg.probe(data)
    short = np.empty(it.info.coef_bytes // 2 - 1, np.int16)
    assert jpeg._entropy_into(it, short) == _lib.ERR_BAD_ARG


def test_coefficient_bound_is_refused(g22):
    """|coefficient * quant| <= 8191: the same stream is taken under a quantiser that keeps inside and refused under one that
    does not."""
    i = max(g22.accepted, key=lambda k: int(np.abs(g22.item(k).coef).max()))
    top = int(np.abs(g22.item(i).coef).max())
    assert 8191 // 255 < top <= 8191
    inside, outside = 8191 // top, min(255, 8191 // top + 1)
    assert top * inside <= 8191 < top * outside
    it = jpeg.probe(with_quant(g22.data[i], inside))
    assert set(it.info.quant[:64 * it.info.ncomp]) == {inside}
    assert jpeg.entropy(it) is not None and np.array_equal(it.coef, g22.item(i).coef)
    assert jpeg.entropy(jpeg.probe(with_quant(g22.data[i], outside))) is None


def _with_size(data, width, height):
    data = bytearray(data)
    at = data.index(b'\xff\xc0') + 5
    data[at:at + 4] = struct.pack('>HH', height, width)
    return bytes(data)


def test_probe_refuses_zero_quantisers_and_oversized_images(g22):
    i = g22.index('one_mcu_420')
    assert jpeg.probe(with_quant(g22.data[i], 0)) is None  # |coefficient| would be unbounded
    assert jpeg.probe(_with_size(g22.data[i], 9459, 9459)) is not None  # 89 472 681 pixels
    assert jpeg.probe(_with_size(g22.data[i], 9460, 9459)) is None  # past PIL's MAX_IMAGE_PIXELS: its guard decides
    assert jpeg.probe(_with_size(g22.data[i], 65535, 65535)) is None


def test_entropy_stops_where_the_stream_ends(g22):
    """A file that claims far more blocks than it carries is refused at the first block past its data, not after a walk
    over the whole claimed image: none of the coefficient buffer behind that block is touched."""
    i = g22.index('one_mcu_420')
    it = jpeg.probe(_with_size(g22.data[i], 4096, 4096))
    coef = np.full(it.info.coef_bytes // 2, 0x5A5A, np.int16)
    assert jpeg._entropy_into(it, coef) == _lib.ERR_UNSUPPORTED
    touched = np.flatnonzero(coef != 0x5A5A)
    assert 0 < touched.size <= 7 * 64  # the six blocks of the first MCU (in their three planes) and the one that ran out of data


def test_encoded_item_pickles(g22):
    it = pickle.loads(pickle.dumps(g22.item(g22.accepted[3])))
    assert bytes(it.info) == bytes(g22.item(g22.accepted[3]).info) and np.array_equal(it.coef, g22.item(g22.accepted[3]).coef)


def test_decode_batch_needs_a_device(g22):
    with pytest.raises(_lib.GritHipError, match="Not implemented on the CPU"):
        jpeg.decode_batch([g22.item(g22.accepted[0])], 'cpu')
    assert 1 <= jpeg.default_threads() <= 16


def test_image_field_device_decode(g22, tmp_path):
    i = g22.index('optimize')
    good = tmp_path / 'good_000000000001.jpg'
    good.write_bytes(g22.data[i])
    policy = MaxWHResize((20, 30))
    out = ImageField(transform=policy, decode='device').preprocess(str(good))
    assert isinstance(out.pixels, jpeg.EncodedJpeg) and out.pixels.coef is not None
    assert out.size == policy(g22.pixels[i]).size and out.filter == 'bicubic'
    assert isinstance(ImageField(decode='device').preprocess(str(good)), jpeg.EncodedJpeg)
    with pytest.raises(ValueError):
        ImageField(decode='gpu')


def test_image_field_falls_back_to_the_host(g22, tmp_path):
    pytest.importorskip('PIL')
    for name in ('progressive', 'cmyk', 'png'):
        i = g22.index(name)
        path = tmp_path / ('%s_000000000002.%s' % (name, 'png' if name == 'png' else 'jpg'))
        path.write_bytes(g22.data[i])
        today = ImageField().preprocess(str(path))
        got = ImageField(decode='device').preprocess(str(path))
        assert isinstance(got, np.ndarray) and np.array_equal(got, today) and np.array_equal(got, g22.pixels[i])
    # host mode on an accepted file is what it was
    i = g22.index('optimize')
    path = tmp_path / 'x_000000000003.jpg'
    path.write_bytes(g22.data[i])
    assert np.array_equal(ImageField().preprocess(str(path)), g22.pixels[i])


def test_resize_policies_take_an_encoded_item(g22):
    for i in g22.accepted[::7]:
        it = g22.item(i)
        for policy in (MaxWHResize((384, 640)), MinMaxResize((64, 96)), FixedResize((32, 48))):
            a, b = policy(it), policy(g22.pixels[i])
            assert a.size == b.size and a.filter == b.filter and a.pixels is it


def test_host_stage_under_sanitizers(g22, tmp_path):
    """The header alone, in a program with its own main, under ASan + UBSan: every fixture file, and for the three smallest
    accepted files every truncation and every byte replaced by 0x00, 0xFF and byte ^ 0x55."""
    gxx = shutil.which('g++')
    assert gxx, "the robustness run needs g++"
    exe = str(tmp_path / 'jpeg_host_check')
    # the sanitizer runtimes are linked statically: the program starts whatever the environment preloads
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',
                            os.path.join(ROOT, 'tests', 'jpeg_host_check.cc'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    smallest = sorted(g22.accepted, key=lambda i: len(g22.data[i]))[:3]
    blob = [struct.pack('<I', len(g22.data))]
    for i, data in enumerate(g22.data):
        blob.append(struct.pack('<II', (1 if g22.meta[i]['accepted'] else 0) | (2 if i in smallest else 0), len(data)) + data)
    cases = tmp_path / 'cases.bin'
    cases.write_bytes(b''.join(blob))
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    calls, decoded = (int(v) for v in run.stdout.split()[1::2])
    assert calls == len(g22.data) + 4 * sum(len(g22.data[i]) for i in smallest)
    assert len(g22.accepted) <= decoded < calls  # whole files decode, most damaged ones do not


def test_image_folder_device_decode(g22, tmp_path):
    """extract_features.ImageFolder(decode='device') hands out probed items (the batch's entropy decode is decode_batch's)
    and today's array for a refused file."""
    pytest.importorskip('PIL')
    from extract_features import ImageFolder
    (tmp_path / 'a_000000000007.jpg').write_bytes(g22.data[g22.index('optimize')])
    (tmp_path / 'b_000000000008.png').write_bytes(g22.data[g22.index('png')])
    folder = ImageFolder(str(tmp_path), decode='device')
    assert folder.img_ids == [7, 8] and len(folder) == 2
    assert isinstance(folder[0], jpeg.EncodedJpeg) and folder[0].coef is None and folder[0].shape == g22.pixels[g22.index('optimize')].shape
    assert isinstance(folder[1], np.ndarray) and np.array_equal(folder[1], g22.pixels[g22.index('png')])
    host = ImageFolder(str(tmp_path))
    assert np.array_equal(host[0], g22.pixels[g22.index('optimize')])
