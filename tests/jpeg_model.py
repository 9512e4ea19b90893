"""numpy model (int64) of the JPEG reconstruction stage: dequantised blocks -> jidctint.c's jpeg_idct_islow -> range limit ->
jdsample.c's fancy upsampling -> jdcolor.c's YCbCr -> RGB.  A helper for the tests and for tests/golden/make_jpeg_golden.py,
written from the rules, independent of the kernels (which work in 32 bits)."""
import numpy as np

CONST_BITS, PASS1_BITS = 13, 2


def _pass(d):
    """One 1-D pass over the last axis ([..., 8] int64) -> the eight sums before the descale."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    z1 = (d2 + d6) * 4433
    tmp2 = z1 + d6 * -15137
    tmp3 = z1 + d2 * 6270
    tmp0 = (d0 + d4) << CONST_BITS
    tmp1 = (d0 - d4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d7, d5, d3, d1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                     tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)


def range_limit(x):
    i = x & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def idct_islow(blocks):
    """[..., 8, 8] dequantised coefficients (row, column) -> [..., 8, 8] samples 0..255 (int64)."""
    b = np.asarray(blocks, np.int64)
    n = CONST_BITS - PASS1_BITS
    cols = (_pass(np.swapaxes(b, -1, -2)) + (1 << (n - 1))) >> n  # [..., column, row]
    ws = np.swapaxes(cols, -1, -2)
    n = CONST_BITS + PASS1_BITS + 3
    return range_limit((_pass(ws) + (1 << (n - 1))) >> n)


def plane_samples(coef, quant):
    """coef [block_rows, block_cols, 64] (natural order), quant [64] -> the sample plane [block_rows * 8, block_cols * 8]."""
    br, bc = coef.shape[:2]
    deq = (np.asarray(coef, np.int64) * np.asarray(quant, np.int64)).reshape(br, bc, 8, 8)
    return idct_islow(deq).transpose(0, 2, 1, 3).reshape(br * 8, bc * 8)


def _h2v1(p, w):
    dh, dw = p.shape
    out = np.empty((dh, 2 * dw), np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out[:, :w]


def _h2v2(p, h, w):
    dh, dw = p.shape
    rows = np.arange(h)
    near = rows >> 1
    far = np.clip(np.where(rows & 1, near + 1, near - 1), 0, dh - 1)
    s = 3 * p[near] + p[far]  # [h, dw]
    out = np.empty((h, 2 * dw), np.int64)
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    out[:, 0], out[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    return out[:, :w]


def upsample(plane, h, w, hmax, vmax):
    """The chroma plane (block-padded) -> [h, w].  Its real size is ceil(w / hmax) x ceil(h / vmax)."""
    dw, dh = -(-w // hmax), -(-h // vmax)
    p = np.asarray(plane, np.int64)[:dh, :dw]
    if hmax == 1 and vmax == 1:
        return p
    if dw <= 2:  # the fancy filters are off: replication
        return np.repeat(np.repeat(p, vmax, 0), hmax, 1)[:h, :w]
    return _h2v1(p, w) if vmax == 1 else _h2v2(p, h, w)


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def reconstruct(width, height, hmax, vmax, planes_coef, quants):
    """planes_coef: per component [block_rows, block_cols, 64] int16; quants: per component [64] -> [height, width, 3] uint8."""
    planes = [plane_samples(c, q) for c, q in zip(planes_coef, quants)]
    y = planes[0][:height, :width]
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    return ycc_to_rgb(y, upsample(planes[1], height, width, hmax, vmax), upsample(planes[2], height, width, hmax, vmax))


def reconstruct_item(item):
    """An EncodedJpeg with coefficients (grit_amd/ops/jpeg.py) -> [h, w, 3] uint8."""
    info, at, planes, quants = item.info, 0, [], []
    for c in range(info.ncomp):
        br, bc = info.block_rows[c], info.block_cols[c]
        planes.append(np.asarray(item.coef[at:at + br * bc * 64]).reshape(br, bc, 64))
        quants.append(np.array(info.quant[64 * c:64 * c + 64]))
        at += br * bc * 64
    return reconstruct(info.width, info.height, info.hmax, info.vmax, planes, quants)
