"""grit_grad_norm_flat and grit_adamw_flat_dev through the C ABI (grit_amd/csrc/adamw.hip), in the style of the flat-Adam section of
tests/test_stream_numerics_gpu.py: every reference is torch in float64 on the same dtype-rounded inputs, every buffer carries a
sentinel guard behind n.  Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from grit_amd import lib as binding

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, BAD_ARG, UNSUPPORTED = binding.OK, binding.ERR_BAD_ARG, binding.ERR_UNSUPPORTED
SENTINEL = -12345.0  # exactly representable in bf16 and fp32
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64  # elements behind n in every buffer
NORM_MAX_RANGES, NORM_BLOCK_CAP = binding.NORM_MAX_RANGES, binding.NORM_BLOCK_CAP
NORM_PASS = NORM_BLOCK_CAP * 256  # 16-byte units (8 bf16 or 4 fp32 elements) one pass of the capped grid covers
ADAM_BLOCK_CAP = 8192 * 256  # quads one pass of the capped Adam grid covers
LR, BETA1, BETA2, ADAM_EPS = 1e-2, 0.9, 0.999, 1e-8


_ptr = binding.ptr


def _lib():
    return binding.load(), binding.current_stream_ptr()


def _f32(v):
    return float(np.float32(v))


def _bits(t):
    return t.detach().cpu().view(torch.int32).tolist()


def _ulps(a, b):
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def test_constants_match_the_binding():
    assert binding.ABI_VERSION >= 51
    assert ctypes.sizeof(binding.NormRange) == 16


# ---------------------------------------------------------------------------------------------------------------- gradient norm

def _pass_plus_5(dtype):
    return [(8 if dtype == BF16 else 4) * NORM_PASS + 4 * 5]


# name -> (range sizes, element offset of each range's start inside its buffer, magnitude, grad_scale, max_norm)
NORM_CASES = {
    "one_quad": ([4], 0, 0.1, 1.0, 0.1),
    "257_quads": ([4 * 257], 0, 0.1, 0.125, 0.1),
    "pass_plus_5_quads": (_pass_plus_5, 0, 0.01, 0.125, 0.1),
    "pass_plus_5_quads_odd_start": (_pass_plus_5, 4, 0.01, 0.5, 0.1),
    "three_ranges": ([4 * 3, 4 * 1031, 4 * 64], (0, 4, 4), 0.1, 0.5, 0.1),
    "chained_launches": ([8] * (NORM_MAX_RANGES + 3), 0, 0.1, 1.0, 0.1),
    "huge_1e20": ([1024], 0, 1e20, 1.0, 0.1),
    "tiny_1e-25": ([1024], 0, 1e-25, 1.0, 0.1),
    "zeros": ([4 * 257], 0, 0.0, 0.125, 0.1),
    "below_max_norm": ([4 * 257], 0, 1e-3, 0.125, 0.1),
    "above_max_norm": ([4 * 257], 0, 1.0, 0.125, 0.1),
    "one_nan": ([4 * 257], 0, 0.1, 0.125, 0.1),
}


@functools.lru_cache(maxsize=None)
def _norm_case(name, dtype):
    """(buffers, ranges, float64 sum of squares): a range is a view of n elements at its offset, a sentinel guard behind it (and in
    front of an offset start).  Never modified."""
    sizes, offsets, mag, _, _ = NORM_CASES[name]
    sizes = sizes(dtype) if callable(sizes) else sizes
    offsets = offsets if isinstance(offsets, tuple) else (offsets,) * len(sizes)
    gen = torch.Generator(device=DEV).manual_seed(len(name) + sum(sizes) % 1000003)
    buffers, ranges = [], []
    for n, off in zip(sizes, offsets):
        buf = torch.full((off + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        g = mag * (1.0 + 0.25 * torch.randn(n, device=DEV, generator=gen)) * (torch.randint(0, 2, (n,), device=DEV, generator=gen) * 2 - 1)
        buf[off:off + n] = g.to(dtype)
        buffers.append(buf)
        ranges.append(buf[off:off + n])
    if name == "one_nan":
        ranges[0][sizes[0] // 2] = float("nan")
    total = sum((r.double() ** 2).sum() for r in ranges)
    return buffers, ranges, total


def _norm_call(ranges, grad_scale, max_norm, partials=None, ticket=None, out=None, table=None):
    from grit_amd import lib as L
    lib, stream = _lib()
    launches = -(-max(len(ranges), 1) // NORM_MAX_RANGES)
    if table is None:
        table = (L.NormRange * max(len(ranges), 1))()
        for i, r in enumerate(ranges):
            table[i].grad, table[i].n = r.data_ptr(), r.numel()
    partials = torch.full((launches * NORM_BLOCK_CAP + GUARD,), SENTINEL, dtype=torch.float64, device=DEV) if partials is None else partials
    ticket = torch.full((1 + GUARD,), 77, dtype=torch.int32, device=DEV) if ticket is None else ticket
    out = torch.full((3 + GUARD,), SENTINEL, dtype=F32, device=DEV) if out is None else out
    dtype_flag = int(ranges[0].dtype == BF16) if ranges else 1
    st = lib.grit_grad_norm_flat(table, len(ranges), dtype_flag, grad_scale, max_norm, _ptr(partials), _ptr(ticket), _ptr(out), stream)
    return st, partials, ticket, out


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("name", sorted(NORM_CASES))
def test_grad_norm_hard_points(name, dtype):
    """total_norm within 2 fp32 ulps of the rounded float64 value (the kernel's float64 sum is accurate far below fp32 resolution:
    its result is one rounding of it); clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 on the kernel's own total_norm
    within 1 ulp; clip_scale = grad_scale * clip_coef within 1 ulp.  Two calls give identical bits; gradients and guards untouched."""
    _, _, mag, grad_scale, max_norm = NORM_CASES[name]
    buffers, ranges, total = _norm_case(name, dtype)
    before = [b.clone() for b in buffers]
    st, partials, ticket, out = _norm_call(ranges, grad_scale, max_norm)
    st2, _, _, out2 = _norm_call(ranges, grad_scale, max_norm)
    assert st == OK and st2 == OK
    torch.cuda.synchronize()
    launches = -(-len(ranges) // NORM_MAX_RANGES)
    assert bool((out[3:] == SENTINEL).all()) and bool((ticket[1:] == 77).all())
    assert bool((partials[launches * NORM_BLOCK_CAP:] == SENTINEL).all())
    for b, b0 in zip(buffers, before):
        assert torch.equal(b.view(torch.int16 if dtype == BF16 else torch.int32), b0.view(torch.int16 if dtype == BF16 else torch.int32))
    assert _bits(out[:3]) == _bits(out2[:3])
    got_norm, got_scale, got_coef = (np.float32(x) for x in out[:3].cpu().numpy())
    print("%s %s: total_norm %r clip_scale %r clip_coef %r" % (name, dtype, got_norm, got_scale, got_coef))
    if name == "one_nan":
        assert np.isnan(got_norm) and np.isnan(got_scale) and np.isnan(got_coef)
        return
    want_norm = np.float32(float(total.sqrt()) * grad_scale)
    assert np.isfinite(want_norm) and _ulps(got_norm, want_norm) <= 2, (got_norm, want_norm)
    with np.errstate(over="ignore"):
        q = np.float32(max_norm) / (got_norm + np.float32(1e-6))
    want_coef = np.float32(1.0) if q > 1.0 else q
    assert _ulps(got_coef, want_coef) <= 1, (got_coef, want_coef)
    assert _ulps(got_scale, np.float32(grad_scale) * got_coef) <= 1, (got_scale, got_coef)
    if name == "zeros":
        assert got_norm == 0.0 and got_coef == 1.0
    if name in ("zeros", "below_max_norm", "tiny_1e-25"):
        assert got_coef == 1.0 and _bits(out[1:2]) == _bits(torch.tensor([grad_scale], dtype=F32))
    if name in ("above_max_norm", "huge_1e20"):
        assert 0.0 < got_coef < 1.0 and got_norm > max_norm
    if name == "huge_1e20":
        assert not np.isfinite(np.float32(mag) * np.float32(mag))  # the squares overflow fp32, the norm does not
    if name == "tiny_1e-25":
        assert np.float32(mag) * np.float32(mag) == 0.0 and got_norm > 0.0


def test_grad_norm_rejections():
    """A misaligned pointer (bf16 off by 2 bytes, fp32 off by 8) or n % 4 != 0: GRIT_ERR_UNSUPPORTED; zero ranges, a negative
    max_norm, a null range pointer, n <= 0, null workspaces or outputs: GRIT_ERR_BAD_ARG.  All answered on the host: nothing is written."""
    from grit_amd import lib as L
    buf = torch.full((4 * 64 + GUARD,), 0.5, dtype=BF16, device=DEV)
    buf32 = buf.float()
    good = [buf[:4 * 64]]
    st, partials, ticket, out = _norm_call(good, 1.0, 0.1)
    assert st == OK
    torch.cuda.synchronize()
    kept = [x.clone() for x in (partials, ticket, out)]
    ws = dict(partials=partials, ticket=ticket, out=out)
    assert _norm_call([buf[1:4 * 64 - 3]], 1.0, 0.1, **ws)[0] == UNSUPPORTED
    assert _norm_call([buf32[2:4 * 64 - 2]], 1.0, 0.1, **ws)[0] == UNSUPPORTED
    assert _norm_call([buf[:4 * 64 - 1]], 1.0, 0.1, **ws)[0] == UNSUPPORTED
    assert _norm_call(good + [buf[8:14]], 1.0, 0.1, **ws)[0] == UNSUPPORTED
    assert _norm_call([], 1.0, 0.1, **ws)[0] == BAD_ARG
    assert _norm_call(good, 1.0, -0.1, **ws)[0] == BAD_ARG
    table = (L.NormRange * 1)()
    table[0].grad, table[0].n = None, 64
    assert _norm_call(good, 1.0, 0.1, table=table, **ws)[0] == BAD_ARG
    table[0].grad, table[0].n = buf.data_ptr(), 0
    assert _norm_call(good, 1.0, 0.1, table=table, **ws)[0] == BAD_ARG
    lib, stream = _lib()
    table[0].n = 64
    for args in ((None, _ptr(ticket), _ptr(out)), (_ptr(partials), None, _ptr(out)), (_ptr(partials), _ptr(ticket), None)):
        assert lib.grit_grad_norm_flat(table, 1, 1, 1.0, 0.1, *args, stream) == BAD_ARG
    assert lib.grit_grad_norm_flat(None, 1, 1, 1.0, 0.1, _ptr(partials), _ptr(ticket), _ptr(out), stream) == BAD_ARG
    torch.cuda.synchronize()
    for x, x0 in zip((partials, ticket, out), kept):
        assert torch.equal(x, x0)


# ---------------------------------------------------------------------------------------------------------------- flat AdamW

def _bias_corrections(step):
    return _f32(1.0 - BETA1 ** step), _f32((1.0 - BETA2 ** step) ** 0.5)


def _hyper_row(step, weight_decay):
    """The row as the host passes it: fp32 {lr / bc1, 1 / sqrt(bc2), 1 - lr * wd, 0}."""
    bc1, bc2s = _bias_corrections(step)
    return torch.tensor([np.float32(LR) / np.float32(bc1), np.float32(1.0) / np.float32(bc2s), np.float32(1.0 - LR * weight_decay), 0.0],
                        dtype=F32, device=DEV)


@functools.lru_cache(maxsize=None)
def _adam_state(n, grad_dtype):
    """(p, g, m, v) with GUARD sentinels behind n; gradients ~0.1, non-zero prior moments; a few elements at the front, in the
    middle and at the end have g = 0 and v = 0 (denominator = eps), every other one m = 0 as well.  Never modified."""
    gen = torch.Generator(device=DEV).manual_seed(n % 1000003)
    total = n + GUARD
    p = torch.randn(total, device=DEV, generator=gen)
    g = (0.1 * torch.randn(total, device=DEV, generator=gen)).to(grad_dtype)
    m = 0.05 * torch.randn(total, device=DEV, generator=gen)
    v = 0.01 * torch.rand(total, device=DEV, generator=gen)
    zero = torch.tensor(sorted({1, n // 2 + 1, n - 2, n - 1}), device=DEV)
    g[zero] = 0
    v[zero] = 0
    m[zero[::2]] = 0
    for t in (p, g, m, v):
        t[n:] = SENTINEL
    return p, g, m, v


def _adam_fresh(n, grad_dtype):
    p, g, m, v = (t.clone() for t in _adam_state(n, grad_dtype))
    return p, g, m, v, torch.full((n + GUARD,), SENTINEL, dtype=BF16, device=DEV)


def _adamw_call(n, p, g, m, v, compute, grad_scale, hyper, clip=None):
    lib, stream = _lib()
    return lib.grit_adamw_flat_dev(_ptr(p), _ptr(g), int(g.dtype == BF16), _ptr(m), _ptr(v), None if compute is None else _ptr(compute), n,
                                   BETA1, BETA2, ADAM_EPS, grad_scale, _ptr(hyper), None if clip is None else _ptr(clip), stream)


ADAMW_SIZES = [4, 4 * 257, 4 * (ADAM_BLOCK_CAP + 5)]


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4, 0.5])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("grad_dtype", [BF16, F32])
@pytest.mark.parametrize("n", ADAMW_SIZES)
def test_adamw_flat_one_step_vs_float64(n, grad_dtype, step, weight_decay, clipped):
    """p <- p * hyper[2], then adam_flat's lines, in float64 with the hyper-parameters rounded to fp32 as the host passes them.
    rtol 2e-6 / atol 2e-7 on masters and moments: the bound of test_adam_flat_one_step_vs_float64; the decay multiply adds one fp32
    rounding of p (relative 6e-8), inside it.  The bf16 compute copy is bit-equal to the rounded master.  `clipped`: the gradient
    factor is a clip cell holding 0.25 (the scalar argument, 1.0, must then be ignored); otherwise the scalar 0.125."""
    p, g, m, v, compute = _adam_fresh(n, grad_dtype)
    hyper = _hyper_row(step, weight_decay)
    cell = torch.tensor([0.25, SENTINEL], dtype=F32, device=DEV) if clipped else None
    assert _adamw_call(n, p, g, m, v, compute, 1.0 if clipped else 0.125, hyper, cell) == OK
    torch.cuda.synchronize()
    p0, g0, m0, v0 = (t[:n].double() for t in _adam_state(n, grad_dtype))
    h = [float(x) for x in hyper.cpu()]
    b1, b2, eps = _f32(BETA1), _f32(BETA2), _f32(ADAM_EPS)
    gs = g0 * (0.25 if clipped else 0.125)
    m_ref = m0 + (gs - m0) * (1.0 - b1)
    v_ref = b2 * v0 + (1.0 - b2) * gs * gs
    p_ref = p0 * h[2] - h[0] * (m_ref / (v_ref.sqrt() * h[1] + eps))
    assert torch.isfinite(p_ref).all()
    for name, got, ref in (("exp_avg", m, m_ref), ("exp_avg_sq", v, v_ref), ("param", p, p_ref)):
        assert torch.isfinite(got[:n]).all(), name
        bad = (got[:n].double() - ref).abs() > 2e-7 + 2e-6 * ref.abs()
        assert not bool(bad.any()), (name, int(bad.sum()), int(bad.nonzero()[0]))
    assert torch.equal(compute[:n], p[:n].bfloat16())
    for t in (p, m, v, compute, g):
        assert bool((t[n:] == SENTINEL).all())
    assert torch.equal(g, _adam_state(n, grad_dtype)[1])
    if clipped:
        assert _bits(cell) == _bits(torch.tensor([0.25, SENTINEL], dtype=F32))


@pytest.mark.parametrize("grad_dtype", [BF16, F32])
@pytest.mark.parametrize("n", [4 * 257, 4 * (ADAM_BLOCK_CAP + 5)])
def test_adamw_flat_bit_equalities(n, grad_dtype):
    """hyper[2] = 1 and no clip cell: bit-equal to grit_adam_flat_dev on the same inputs (masters, moments, compute copy); a null
    `compute` leaves masters and moments identical; a clip cell holding exactly grad_scale equals the call without a cell."""
    lib, stream = _lib()
    step, grad_scale = 7, 0.125
    hyper = _hyper_row(step, 0.0)
    assert float(hyper[2]) == 1.0
    want = _adam_fresh(n, grad_dtype)
    p, g, m, v, c = want
    hyper2 = hyper[:2].clone()
    assert lib.grit_adam_flat_dev(_ptr(p), _ptr(g), int(g.dtype == BF16), _ptr(m), _ptr(v), _ptr(c), n, BETA1, BETA2, ADAM_EPS, grad_scale,
                                  _ptr(hyper2), stream) == OK
    same = _adam_fresh(n, grad_dtype)
    assert _adamw_call(n, *same, grad_scale, hyper) == OK
    torch.cuda.synchronize()
    for i, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq", "compute")):
        assert torch.equal(same[i], want[i]), name
    assert not torch.equal(want[0][:n], _adam_state(n, grad_dtype)[0][:n])  # (a step was taken)
    # with decay: null compute and the clip cell
    hyper = _hyper_row(step, 0.5)
    want = _adam_fresh(n, grad_dtype)
    assert _adamw_call(n, *want, grad_scale, hyper) == OK
    null = _adam_fresh(n, grad_dtype)
    assert _adamw_call(n, *null[:4], None, grad_scale, hyper) == OK
    cell = torch.tensor([grad_scale], dtype=F32, device=DEV)
    celled = _adam_fresh(n, grad_dtype)
    assert _adamw_call(n, *celled, 1.0, hyper, cell) == OK
    torch.cuda.synchronize()
    for i, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
        assert torch.equal(null[i], want[i]), name
        assert torch.equal(celled[i], want[i]), name
    assert torch.equal(celled[4], want[4])
    assert bool((null[4] == SENTINEL).all())


def test_adamw_flat_rejections():
    """As grit_adam_flat_dev: n % 4 != 0 and misaligned master / moment / gradient / compute pointers GRIT_ERR_UNSUPPORTED; a missing
    hyper row, one that is not 16-byte aligned (off by 4 or by 8 bytes), n <= 0, null buffers GRIT_ERR_BAD_ARG.  No buffer changes."""
    n = 4 * 64
    bufs = _adam_fresh(n, BF16)
    p, g, m, v, compute = bufs
    before = [t.clone() for t in bufs]
    table = torch.ones(8, device=DEV)
    hyper = table[:4]

    def call(p_=p, g_=g, m_=m, v_=v, c_=compute, n_=n, h_=hyper):
        lib, stream = _lib()
        return lib.grit_adamw_flat_dev(_ptr(p_), _ptr(g_), int(g_.dtype == BF16), _ptr(m_), _ptr(v_), _ptr(c_), n_, BETA1, BETA2, ADAM_EPS, 1.0,
                                       None if h_ is None else _ptr(h_), None, stream)

    assert call(n_=n - 1) == UNSUPPORTED
    assert call(p_=p[1:], n_=n - 4) == UNSUPPORTED
    assert call(m_=m[1:], n_=n - 4) == UNSUPPORTED
    assert call(v_=v[1:], n_=n - 4) == UNSUPPORTED
    assert call(g_=g[1:], n_=n - 4) == UNSUPPORTED
    assert call(g_=g.float()[2:], n_=n - 4) == UNSUPPORTED
    assert call(c_=compute[1:], n_=n - 4) == UNSUPPORTED
    assert call(n_=0) == BAD_ARG
    assert call(h_=None) == BAD_ARG
    assert call(h_=table[1:5]) == BAD_ARG
    assert call(h_=table[2:6]) == BAD_ARG
    lib, stream = _lib()
    assert lib.grit_adamw_flat_dev(None, _ptr(g), 1, _ptr(m), _ptr(v), _ptr(compute), n, BETA1, BETA2, ADAM_EPS, 1.0, _ptr(hyper), None,
                                   stream) == BAD_ARG
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, before):
        assert torch.equal(t, t0)
    assert call(h_=table[4:8]) == OK  # (the same call with an aligned row is taken)
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0])
