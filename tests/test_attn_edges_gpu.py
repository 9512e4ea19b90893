"""Attention core (grit_attn_*; attn.hip, attn_mfma.hip, ops/attention.py) at the places the shape list of test_attn_gpu.py does
not reach: every tile edge of the matrix-core kernels, the bf16 fallback onto the fp32-arithmetic kernels (by shape and by
layout), guard rows around strided views, the step-wise decode shapes, backward through packed projections, scale / head count /
mask forms, run-to-run determinism and the dropout keep-mask across the kernel families.

Every value comparison is against oracle.torch_ref.attention in float64 (bf16 cases: on the same bf16-rounded inputs) at the
project's bounds: fp32 assert_allclose(rtol=1e-4, atol=1e-4); bf16 max error < 3e-2 and mean error < 4e-3 of max|ref|."""
import math

import numpy as np
import pytest
import torch

from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
NAMES = ("out", "dq", "dk", "dv")
# tile edges of the matrix-core kernels: 16-key S tiles, 32-key P V / dS steps, 16-query waves, the 160-row limit
E = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 143, 144, 145, 159, 160)
MASK_KINDS = (None, "key", "query", "shared")


@pytest.fixture(autouse=True, scope="module")
def _at_most_16_reference_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _fn():
    from grit_amd.ops.attention import _AttentionFn, attention
    return attention, _AttentionFn


# ---------------------------------------------------------------------------------------------------------------
# inputs, reference, runner, bounds
# ---------------------------------------------------------------------------------------------------------------
def _inputs(B, Tq, Nk, H, dtype, seed=0, gain=1.0):
    """q, k (times `gain`: large logits), v, cotangent on the CPU, rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed * 1000003 + Tq * 1009 + Nk)
    q = torch.randn(B, Tq, H, 64, generator=g) * gain
    k = torch.randn(B, Nk, H, 64, generator=g) * gain
    v = torch.randn(B, Nk, H, 64, generator=g)
    cot = torch.randn(B, Tq, H * 64, generator=g)
    return tuple(x.to(dtype) for x in (q, k, v, cot))


def _mask(kind, B, Tq, Nk, seed=0):
    """True = masked; key 0 stays visible in every row."""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed * 7919 + Tq * 263 + Nk)
    shape = {"key": (B, 1, 1, Nk), "key1": (1, 1, 1, Nk), "query": (B, 1, Tq, Nk), "shared": (1, 1, Tq, Nk)}[kind]
    m = torch.rand(shape, generator=g) < 0.3
    m[..., 0] = False
    return m


def _ref(q, k, v, cot, mask=None, scale=None, keep=None, p=0.0):
    """float64 oracle: out, dq, dk, dv.  keep [B,H,Tq,Nk] bool: the dropout keep-mask the kernel drew (autograd through P * keep / (1-p))."""
    q, k, v = (x.detach().cpu().double().requires_grad_(True) for x in (q, k, v))
    if keep is None:
        out = torch_ref.attention(q, k, v, mask, scale=scale)
    else:
        B, Tq, H, D = q.shape
        s = torch.matmul(q.permute(0, 2, 1, 3), k.permute(0, 2, 3, 1)) * (1.0 / math.sqrt(D) if scale is None else scale)
        if mask is not None:
            s = s.masked_fill(mask.bool(), float("-inf"))
        pm = torch.softmax(s, -1) * (keep.cpu().double() / (1.0 - p))
        out = torch.matmul(pm, v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B, Tq, H * D)
    out.backward(cot.detach().cpu().double())
    return out.detach(), q.grad, k.grad, v.grad


def _run(q, k, v, cot, mask=None, scale=None, p=0.0, seed_dev=None):
    """The kernels, forward and backward, on tensors that are already on the device (views are passed as they are)."""
    attention, Fn = _fn()
    q, k, v = (x.detach().requires_grad_(True) for x in (q, k, v))  # detach keeps offset and strides
    if p > 0:
        out = Fn.apply(q, k, v, mask, 0.125 if scale is None else float(scale), p, 0, seed_dev)
    else:
        out = attention(q, k, v, mask, scale=scale)
    out.backward(cot)
    return out.detach(), q.grad, k.grad, v.grad


def _dev(*xs):
    return tuple(None if x is None else x.to(DEV) for x in xs)


def _errors(dtype, ref, got, tag=""):
    """-> list of failure strings (empty = within the project's bounds).
    Where the reference is EXACTLY zero (one visible key: P = 1, dS = P (dP - sum P dP) = 0, so dq = dk = 0 in any arithmetic that
    forms delta from the same dP), 3e-2 * max|ref| is no bound: 0 < 0 fails an exact result too.  Only there, a bf16 tensor is held to
    the project's absolute bound instead, the atol = 1e-4 of the fp32 comparison: bf16 storage is not asked to beat what the fp32
    kernels are allowed."""
    bad = []
    for name, r, o in zip(NAMES, ref, got):
        assert o.dtype == dtype, (tag, name, o.dtype)
        r, o = r.float(), o.detach().float().cpu()
        assert r.shape == o.shape, (tag, name, r.shape, o.shape)
        err = (o - r).abs()
        within_fp32 = bool((err <= 1e-4 + 1e-4 * r.abs()).all())  # NaN fails
        if dtype == F32 or r.abs().max().item() == 0.0:
            if not within_fp32:
                bad.append("%s %s: |err| %.3e beyond rtol=1e-4, atol=1e-4" % (tag, name, (err - 1e-4 - 1e-4 * r.abs()).max().item()))
        else:
            scale = r.abs().max().item() + 1e-6
            emax, emean = err.max().item(), err.mean().item()
            bmax, bmean = 3e-2 * scale, 4e-3 * scale
            if not emax < bmax:
                bad.append("%s %s: bf16 max err %.3e >= %.3e (3e-2 * %.3e)" % (tag, name, emax, bmax, scale))
            if not emean < bmean:
                bad.append("%s %s: bf16 mean err %.3e >= %.3e (4e-3 * %.3e)" % (tag, name, emean, bmean, scale))
    return bad


def _check(dtype, ref, got, tag=""):
    bad = _errors(dtype, ref, got, tag)
    assert not bad, "\n".join(bad)


def _case(B, Tq, Nk, H, dtype, mask_kind=None, seed=0, gain=1.0, scale=None):
    """One shape, forward and backward, kernels against the oracle -> failure strings."""
    q, k, v, cot = _inputs(B, Tq, Nk, H, dtype, seed, gain)
    mask = _mask(mask_kind, B, Tq, Nk, seed)
    ref = _ref(q, k, v, cot, mask, scale)
    got = _run(*_dev(q, k, v, cot, mask), scale=scale)
    return _errors(dtype, ref, got, "(Tq %d, Nk %d, %s, gain %g)" % (Tq, Nk, mask_kind, gain))


def _bits(a, b):
    """Bit for bit (NaN patterns included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------
# 1. tile-edge sweep of the matrix-core kernels
# ---------------------------------------------------------------------------------------------------------------
def _sweep_kind(Tq, Nk):
    return MASK_KINDS[(E.index(Tq) + E.index(Nk)) % 4]


@pytest.mark.parametrize("Tq", E)
def test_mfma_tile_edges(Tq):
    """Every (Tq, Nk) of E x E at unit gain: staging of min(160, ceil32(Nk)) rows, helper waves, dS tail fill, key / query clamps."""
    bad = []
    for Nk in E:
        bad += _case(2, Tq, Nk, 2, BF16, _sweep_kind(Tq, Nk))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("Tq", E)
def test_mfma_tile_edges_large_logits(Tq):
    """q and k times 4 (logits of standard deviation 16: max subtraction, exp2 / log2 folding) on the diagonal and the rows Tq = 1, 160.

    The row Tq = 1 is where max|ref| of dq / dk is itself a small difference (0.01 .. 0.9 where dv has 3): a backward that takes
    delta = rowsum(dO * O) from the stored bf16 output misses the bound there by up to 1.7 x (measured: Nk 15, 64, 129), one that sums
    delta = sum_k P dP in fp32 stays 10 x inside it.  The same row on the fallback kernel: test_bf16_fallback_by_layout_large_logits_single_row."""
    bad = []
    for Nk in (E if Tq in (E[0], E[-1]) else (Tq,)):
        bad += _case(2, Tq, Nk, 2, BF16, _sweep_kind(Tq, Nk), seed=1, gain=4.0)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# 2. the fp32-arithmetic kernels: chunks of 64 key lanes, 32-row forward blocks, the 8-wave backward stride
# ---------------------------------------------------------------------------------------------------------------
NK_F32 = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)


@pytest.mark.parametrize("Tq", (1, 7, 8, 9, 31, 32, 33, 64, 161, 300))
def test_fp32_kernel_edges(Tq):
    bad = []
    for i, Nk in enumerate(NK_F32):
        bad += _case(2, Tq, Nk, 2, F32, MASK_KINDS[(i + Tq) % 4])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("Tq,Nk", [(1, 129), (33, 256), (161, 64), (64, 193)])
def test_fp32_kernel_large_logits(Tq, Nk):
    bad = _case(2, Tq, Nk, 2, F32, "query", seed=1, gain=4.0)
    assert not bad, "\n".join(bad)


FALLBACK_SHAPES = [(tq, nk) for nk in (161, 192, 255, 256) for tq in (1, 5, 54, 150)] + \
                  [(tq, nk) for tq in (161, 300) for nk in (20, 160)]


@pytest.mark.parametrize("Tq,Nk", FALLBACK_SHAPES)
def test_bf16_fallback_by_shape(Tq, Nk):
    """Nk in 161..256 or Tq > 160: bf16 storage on attn_{fwd,bwd}_kernel<__hip_bfloat16> (grid tokens of an 832 x 832 image: 169 keys)."""
    bad = _case(2, Tq, Nk, 2, BF16, MASK_KINDS[(Tq + Nk) % 4])
    bad += _case(2, Tq, Nk, 2, BF16, MASK_KINDS[(Tq + Nk + 1) % 4], seed=1, gain=4.0)
    assert not bad, "\n".join(bad)


def test_bf16_families_agree_across_the_160_key_boundary():
    """Nk = 161 with the 161st key masked (fallback kernels) against Nk = 160 without it (matrix-core kernels), equal inputs otherwise."""
    B, Tq, H = 2, 37, 4
    q, k, v, cot = _inputs(B, Tq, 161, H, BF16, seed=2)
    m161 = torch.zeros(B, 1, 1, 161, dtype=torch.bool)
    m161[..., 160] = True
    ref = _ref(q, k[:, :160], v[:, :160], cot)
    dq_, dk_, dv_, dc_, dm_ = _dev(q, k, v, cot, m161)
    fall = _run(dq_, dk_, dv_, dc_, dm_)
    mfma = _run(dq_, dk_[:, :160].contiguous(), dv_[:, :160].contiguous(), dc_)
    assert not fall[2][:, 160].any() and not fall[3][:, 160].any()  # the masked key receives exactly zero
    fall = (fall[0], fall[1], fall[2][:, :160], fall[3][:, :160])
    _check(BF16, ref, fall, "fallback")
    _check(BF16, ref, mfma, "mfma")
    for name, r, a, b in zip(NAMES, ref, fall, mfma):
        scale = r.abs().max().item() + 1e-6
        d = (a.float() - b.float()).abs()
        assert d.max().item() < 3e-2 * scale and d.mean().item() < 4e-3 * scale, (name, d.max().item(), d.mean().item(), scale)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_than_256_keys_are_refused(dtype):
    attention, _ = _fn()
    q, k, v, cot = _dev(*_inputs(1, 3, 257, 2, dtype))
    with pytest.raises(RuntimeError, match="not supported"):
        attention(q, k, v)
    out = attention(q, k[:, :256], v[:, :256])
    out.sum().item()  # the device is still usable and 256 keys are accepted
    assert out.shape == (1, 3, 128)


# ---------------------------------------------------------------------------------------------------------------
# 3. fallback by layout
# ---------------------------------------------------------------------------------------------------------------
def _relayout(x, how):
    """The values of x [B, T, H, 64] (device) in a view the matrix-core kernels refuse."""
    B, T, H, D = x.shape
    if how == "offset4":  # base pointer 8 bytes past a 16-byte boundary
        buf = torch.zeros(x.numel() + 4, dtype=x.dtype, device=x.device)
        y = buf[4:].view(B, T, H, D)
    elif how == "row516":  # row stride 516: [.., :512] of a last dimension of 516 (H = 8)
        buf = torch.zeros(B, T, H * D + 4, dtype=x.dtype, device=x.device)
        y = buf[..., :H * D].view(B, T, H, D)
    elif how == "batch+4":  # batch stride T * 512 + 4
        buf = torch.zeros(B, T * H * D + 4, dtype=x.dtype, device=x.device)
        y = buf[:, :T * H * D].view(B, T, H, D)
    else:
        raise ValueError(how)
    y.copy_(x)
    assert y.stride(3) == 1 and y.stride(2) == D  # what ops.attention._rows keeps as a view
    assert y.data_ptr() % 16 or y.stride(1) % 8 or y.stride(0) % 8
    return y


@pytest.mark.parametrize("which", ("q", "k", "v", "qkv"))
@pytest.mark.parametrize("how", ("offset4", "row516", "batch+4"))
def test_bf16_fallback_by_layout(how, which):
    """Dispatch happens behind the C ABI, so that the fp32-arithmetic kernel ran is seen indirectly: its forward keeps P in fp32 where the
    matrix-core kernel rounds P to bf16, so the two outputs of 30 720 elements agree within the bound and NOT bit for bit (both forwards
    are deterministic; were fits() relaxed, the matrix-core kernel would meet itself and the outputs would be identical)."""
    B, Tq, Nk, H = 3, 20, 37, 8
    q, k, v, cot = _inputs(B, Tq, Nk, H, BF16, seed=3)
    mask = _mask("query", B, Tq, Nk)
    ref = _ref(q, k, v, cot, mask)
    q, k, v, cot, mask = _dev(q, k, v, cot, mask)
    mfma = _run(q, k, v, cot, mask)
    laid = [_relayout(x, how) if n in which else x for n, x in zip("qkv", (q, k, v))]
    fall = _run(*laid, cot, mask)
    _check(BF16, ref, mfma, "aligned")
    _check(BF16, ref, fall, how + " " + which)
    assert not _bits(fall[0], mfma[0]), "the refused layout gave the matrix-core kernel's bits: did the fallback run?"
    for name, r, a, b in zip(NAMES, ref, fall, mfma):
        scale = r.abs().max().item() + 1e-6
        d = (a.float() - b.float()).abs()
        assert d.max().item() < 3e-2 * scale and d.mean().item() < 4e-3 * scale, (name, d.max().item(), d.mean().item(), scale)


def test_bf16_fallback_by_layout_large_logits_single_row():
    """The case that caught delta = rowsum(dO * O) in the matrix-core backward (Tq = 1, q and k times 4, every Nk of E), on
    attn_bwd_kernel<__hip_bfloat16>, reached at these small shapes through a base pointer off 16 bytes."""
    bad = []
    for Nk in E:
        q, k, v, cot = _inputs(2, 1, Nk, 2, BF16, seed=1, gain=4.0)
        mask = _mask(_sweep_kind(1, Nk), 2, 1, Nk, 1)
        ref = _ref(q, k, v, cot, mask)
        q, k, v, cot, mask = _dev(q, k, v, cot, mask)
        got = _run(*(_relayout(x, "offset4") for x in (q, k, v)), cot, mask)
        bad += _errors(BF16, ref, got, "(Tq 1, Nk %d, offset4, gain 4)" % Nk)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# 4. guard rows: a kernel that reads one row too far meets a NaN
# ---------------------------------------------------------------------------------------------------------------
def _guarded(x):
    """x [B, T, H, 64] as big[:, 3:3+T] of a buffer whose other rows are NaN (row and batch strides stay multiples of 8, base aligned)."""
    B, T, H, D = x.shape
    big = torch.full((B, T + 7, H, D), float("nan"), dtype=x.dtype, device=x.device)
    big[:, 3:3 + T] = x
    return big[:, 3:3 + T]


def _atomics(dtype, Tq, Nk):
    """True when the backward is attn_bwd_kernel<T> (float32, or bf16 storage that does not fit the matrix-core kernels by shape)."""
    return dtype == F32 or Tq > 160 or Nk > 160


def _same(dtype, name, a, b, Tq, Nk):
    """Bit for bit wherever the path is deterministic; dk / dv of the atomically summed backward within 1e-4 (bf16 storage: the fp32
    sums differ by their order, ~1e-6, which can move a stored value across one rounding boundary: one bf16 ulp, 2^-8 relative)."""
    if name in ("out", "dq") or not _atomics(dtype, Tq, Nk):
        assert _bits(a, b), name
    elif dtype == F32:
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=name)
    else:
        np.testing.assert_allclose(a.float().cpu().numpy(), b.float().cpu().numpy(), rtol=2.0 ** -7, atol=1e-4, err_msg=name)


GUARD_SHAPES = [(1, 1), (5, 20), (17, 33), (150, 150), (160, 160)]
GUARD_CASES = [pytest.param(tq, nk, dt, id="%d-%d-%s" % (tq, nk, n))
               for n, dt, shapes in (("f32", F32, GUARD_SHAPES + [(33, 256)]), ("bf16", BF16, GUARD_SHAPES)) for tq, nk in shapes]


@pytest.mark.parametrize("mask_kind", (None, "query"))
@pytest.mark.parametrize("Tq,Nk,dtype", GUARD_CASES)
def test_guard_rows(Tq, Nk, dtype, mask_kind):
    B, H = 2, 4
    q, k, v, cot = _inputs(B, Tq, Nk, H, dtype, seed=4)
    mask = _mask(mask_kind, B, Tq, Nk)
    ref = _ref(q, k, v, cot, mask)
    q, k, v, cot, mask = _dev(q, k, v, cot, mask)
    plain = _run(q, k, v, cot, mask)
    views = [_guarded(x) for x in (q, k, v)]
    assert all(not x.is_contiguous() or x.shape[0] == 1 for x in views)
    guard = _run(*views, cot, mask)
    for name, a, b in zip(NAMES, guard, plain):
        assert not torch.isnan(a).any(), name
        _same(dtype, name, a, b, Tq, Nk)
    _check(dtype, ref, guard, "guarded")


# ---------------------------------------------------------------------------------------------------------------
# 5. decode shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beam", (1, 3, 5, 8))
@pytest.mark.parametrize("images", (1, 3, 64))
def test_decode_self_attention_over_the_fused_cache(images, beam, dtype):
    """Steps t = 0..19 of step-wise decoding: q / k / v are the thirds of one packed [rows, 1, 1536] projection, the cache comes
    from grit_kv_append (one history per image at t = 0, `beam` of them after; some steps re-gather by a surviving-beam index)."""
    from grit_amd.ops import kv_cache
    attention, _ = _fn()
    g = torch.Generator().manual_seed(100 * images + beam)
    K = V = None
    hk = hv = None  # the same history kept with plain indexing on the CPU
    bad = []
    for t in range(20):
        rows = images if t == 0 else images * beam
        packed = torch.randn(rows, 1, 1536, generator=g).to(dtype)
        dp = packed.to(DEV)
        src = None  # None: every row continues its own history
        if t == 1 or (t > 1 and t % 3 == 0):
            src = torch.randint(0, 1 if t == 1 else beam, (images, beam), generator=g)
        if t > 0:
            if src is not None:
                cur = hk.shape[0] // images
                idx = (torch.arange(images)[:, None] * cur + src).reshape(-1)
                hk, hv = hk[idx], hv[idx]
            hk = torch.cat([hk, packed[..., 512:1024]], 1)
            hv = torch.cat([hv, packed[..., 1024:]], 1)
        else:
            hk, hv = packed[..., 512:1024].clone(), packed[..., 1024:].clone()
        K, V = kv_cache.append(K, V, None if src is None else src.to(DEV), dp[..., 512:1024], dp[..., 1024:],
                               beam=1 if src is None else beam)
        assert _bits(K.cpu(), hk) and _bits(V.cpu(), hv), t
        qh = dp[..., :512].view(rows, 1, 8, 64)  # strided: row stride 1536
        out = attention(qh, K.view(rows, t + 1, 8, 64), V.view(rows, t + 1, 8, 64))
        ref = torch_ref.attention(packed[..., :512].double().view(rows, 1, 8, 64), hk.double().view(rows, t + 1, 8, 64),
                                  hv.double().view(rows, t + 1, 8, 64))
        bad += _errors(dtype, (ref,), (out,), "step %d" % t)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beam", (1, 3, 5, 8))
@pytest.mark.parametrize("images", (1, 3, 64))
def test_decode_cross_attention_groups_beams_onto_one_memory(images, beam, dtype):
    """The beams of an image are `beam` query rows on ONE copy of its K / V (Attention.forward, bk != b); mask [images,1,1,Nk]."""
    attention, _ = _fn()
    g = torch.Generator().manual_seed(7 * images + beam)
    rows = images * beam
    bad = []
    for Nk in (100, 150, 60):
        packed = torch.randn(rows, 1, 1536, generator=g).to(dtype)
        k = torch.randn(images, Nk, 8, 64, generator=g).to(dtype)
        v = torch.randn(images, Nk, 8, 64, generator=g).to(dtype)
        for mask in (_mask("key", images, 1, Nk, seed=beam), None):
            dp, dk, dv, dm = _dev(packed, k, v, mask)
            qg = dp[..., :512].view(images, beam, 8, 64)
            assert qg.data_ptr() == dp.data_ptr() and (rows == 1 or not qg.is_contiguous())  # a view of the packed projection
            out = attention(qg, dk, dv, dm).view(rows, 1, 512)
            qc = packed[..., :512].double().reshape(images, beam, 8, 64)
            ref = torch.stack([torch_ref.attention(qc[:, j:j + 1], k.double(), v.double(), mask) for j in range(beam)], 1)
            bad += _errors(dtype, (ref.reshape(rows, 1, 512),), (out,), "Nk %d mask %s" % (Nk, mask is not None))
            if dtype == F32:  # one query row does not depend on its neighbours: grouped == un-grouped, bit for bit
                one = attention(dp[..., :512].view(rows, 1, 8, 64), dk.repeat_interleave(beam, 0), dv.repeat_interleave(beam, 0),
                                None if dm is None else dm.repeat_interleave(beam, 0))
                assert _bits(one, out), (Nk, mask is not None)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# 9 (helper used by 6). recovering the dropout keep-mask
# ---------------------------------------------------------------------------------------------------------------
def _keep_mask(dtype, B, H, Tq, Nk, p, seed_dev, mask=None, layout=None):
    """The keep-mask [B,H,Tq,Nk] (bool) the forward kernel draws.  q = 0 makes P uniform over the visible keys (no tiny probabilities);
    V with an identity block on keys [64c, 64c+64) makes the output of run c the dropped P of those keys.  Masked keys read False."""
    _, Fn = _fn()
    q = torch.zeros(B, Tq, H, 64, dtype=dtype, device=DEV)
    k = torch.ones(B, Nk, H, 64, dtype=dtype, device=DEV)
    keep = torch.zeros(B, H, Tq, Nk, dtype=torch.bool, device=DEV)
    for c in range((Nk + 63) // 64):
        n = min(64, Nk - 64 * c)
        v = torch.zeros(B, Nk, H, 64, dtype=dtype, device=DEV)
        v[:, 64 * c:64 * c + n] = torch.eye(64, dtype=dtype, device=DEV)[:n, None, :]
        qq, kk, vv = ((_relayout(x, layout) for x in (q, k, v)) if layout else (q, k, v))
        out = Fn.apply(qq, kk, vv, mask, 0.125, p, 0, seed_dev).view(B, Tq, H, 64)
        keep[..., 64 * c:64 * c + n] = (out[..., :n] != 0).permute(0, 2, 1, 3)
    return keep


# ---------------------------------------------------------------------------------------------------------------
# 6. backward through strided inputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_through_packed_projection(dtype, p):
    """q and k are the halves of one packed [2, 150, 1024] leaf (the detector's q|k GEMM): the backward reads q.stride(1) / stride(0)
    of the saved views, and the gradient arrives on the packed leaf."""
    attention, Fn = _fn()
    g = torch.Generator().manual_seed(6)
    qk = torch.randn(2, 150, 1024, generator=g).to(dtype)
    vv = torch.randn(2, 150, 512, generator=g).to(dtype)
    cot = torch.randn(2, 150, 512, generator=g).to(dtype)
    seed_dev = torch.tensor([20240607], dtype=torch.int64, device=DEV) if p > 0 else None
    keep = _keep_mask(dtype, 2, 8, 150, 150, p, seed_dev) if p > 0 else None

    lq, lv = qk.to(DEV).requires_grad_(True), vv.to(DEV).requires_grad_(True)
    q, k = lq[..., :512].view(2, 150, 8, 64), lq[..., 512:].view(2, 150, 8, 64)
    assert q.stride(1) == 1024 and not q.is_contiguous()
    if p > 0:
        out = Fn.apply(q, k, lv.view(2, 150, 8, 64), None, 0.125, p, 0, seed_dev)
    else:
        out = attention(q, k, lv.view(2, 150, 8, 64))
    out.backward(cot.to(DEV))

    rq, rv = qk.double(), vv.double()
    r = _ref(rq[..., :512].reshape(2, 150, 8, 64), rq[..., 512:].reshape(2, 150, 8, 64), rv.view(2, 150, 8, 64), cot, keep=keep, p=p)
    ref = (r[0], torch.cat([r[1].reshape(2, 150, 512), r[2].reshape(2, 150, 512)], -1), r[3].reshape(2, 150, 512))
    bad = _errors(dtype, ref, (out, lq.grad, lv.grad), "p %g" % p)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# 7. contract details
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", (1.0, 0.05))
def test_scale(scale, dtype):
    bad = _case(2, 33, 70, 8, dtype, "query", seed=7, scale=scale) + _case(2, 20, 200, 8, dtype, "key", seed=7, scale=scale)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", (1, 3, 16))
def test_head_count(H, dtype):
    bad = _case(2, 21, 50, H, dtype, "shared", seed=8) + _case(3, 9, 170, H, dtype, "key", seed=8)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_2560_workgroups(dtype):
    """320 beams x 8 heads, un-grouped (one query each on 20 keys)."""
    bad = _case(320, 1, 20, 8, dtype, "key", seed=9)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_forms(dtype):
    attention, _ = _fn()
    B, Tq, Nk, H = 2, 19, 45, 4
    q, k, v, cot = _inputs(B, Tq, Nk, H, dtype, seed=10)
    dq, dk, dv, dc = _dev(q, k, v, cot)
    for kind in ("key", "key1", "query", "shared"):  # the four accepted shapes
        m = _mask(kind, B, Tq, Nk)
        ref = _ref(q, k, v, cot, m)
        got = _run(dq, dk, dv, dc, m.to(DEV))
        _check(dtype, ref, got, kind)
        as_u8 = _run(dq, dk, dv, dc, m.to(DEV).to(torch.uint8))
        assert _bits(as_u8[0], got[0]) and _bits(as_u8[1], got[1]), kind  # bool and uint8 are the same mask
        if kind == "key":  # an expanded (stride 0) mask is the mask it expands
            e = m.to(DEV).expand(B, 1, Tq, Nk)
            assert e.stride(2) == 0
            ex = _run(dq, dk, dv, dc, e)
            assert _bits(ex[0], got[0]) and _bits(ex[1], got[1])
    key = _mask("key", B, Tq, Nk).to(DEV)
    for wrong in (key[:, 0], key.expand(B, 2, 1, Nk), torch.zeros(B, 1, 1, Nk + 1, dtype=torch.bool, device=DEV),
                  torch.zeros(B + 1, 1, 1, Nk, dtype=torch.bool, device=DEV), torch.zeros(B, 1, Tq + 1, Nk, dtype=torch.bool, device=DEV),
                  torch.zeros(B, 1, Tq, Nk - 1, dtype=torch.bool, device=DEV)):
        with pytest.raises(RuntimeError, match="attention mask must be"):
            attention(dq, dk, dv, wrong)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Tq,Nk", [(20, 45), (54, 160), (33, 200)])
def test_values_at_masked_keys_do_not_matter(Tq, Nk, dtype):
    """K / V at keys masked for every query replaced by other finite values: out, dq, and dk / dv of the visible keys do not move;
    dk / dv of the masked keys are exactly zero."""
    B, H = 2, 4
    q, k, v, cot = _inputs(B, Tq, Nk, H, dtype, seed=11)
    mask = _mask("key", B, Tq, Nk)
    dead = mask[:, 0, 0, :, None, None].expand(B, Nk, H, 64)
    g = torch.Generator().manual_seed(12)
    k2 = torch.where(dead, (torch.randn(k.shape, generator=g) * 3).to(dtype), k)
    v2 = torch.where(dead, (torch.randn(v.shape, generator=g) * 3).to(dtype), v)
    q, k, v, cot, mask, k2, v2, dead = _dev(q, k, v, cot, mask, k2, v2, dead)
    a, b = _run(q, k, v, cot, mask), _run(q, k2, v2, cot, mask)
    for name, x, y in zip(NAMES, a, b):
        if name in ("dk", "dv"):
            assert not x[dead].any() and not y[dead].any(), name
        _same(dtype, name, x, y, Tq, Nk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Tq,Nk", [(20, 45), (150, 150), (9, 200)])
def test_constant_shift_of_every_key(Tq, Nk, dtype):
    """k + c shifts every logit of a row by q.c: softmax, and so `out`, is unchanged.  Values on a 1/16 grid with |k|, |c| <= 4 so that
    k + c is exact in bf16 too: the oracle of the unshifted problem is the reference."""
    attention, _ = _fn()
    B, H = 2, 4
    g = torch.Generator().manual_seed(13)
    q = torch.randn(B, Tq, H, 64, generator=g).to(dtype)
    k = (torch.randint(-64, 65, (B, Nk, H, 64), generator=g) / 16.0).to(dtype)
    v = torch.randn(B, Nk, H, 64, generator=g).to(dtype)
    c = (torch.randint(-64, 65, (B, 1, H, 64), generator=g) / 16.0).to(dtype)
    ks = (k.double() + c.double()).to(dtype)
    assert torch.equal(ks.double(), k.double() + c.double())
    mask = _mask("query", B, Tq, Nk)
    ref = torch_ref.attention(q.double(), k.double(), v.double(), mask)
    dq, dk, dks, dv, dm = _dev(q, k, ks, v, mask)
    _check(dtype, (ref,), (attention(dq, dk, dv, dm),), "unshifted")
    _check(dtype, (ref,), (attention(dq, dks, dv, dm),), "shifted")


def test_fully_masked_row_on_the_mfma_path():
    """NaN in that row (as torch.softmax over all -inf), and only there: the other rows of its 16-row tile match the oracle."""
    attention, _ = _fn()
    B, Tq, Nk, H = 2, 20, 37, 4
    q, k, v, _ = _inputs(B, Tq, Nk, H, BF16, seed=14)
    mask = _mask("query", B, Tq, Nk)
    mask[0, 0, 5] = True
    ref = torch_ref.attention(q.double(), k.double(), v.double(), mask)
    out = attention(*_dev(q, k, v, mask)).cpu()
    assert torch.isnan(out[0, 5]).all() and torch.isnan(ref[0, 5]).all()
    keep = torch.ones(B, Tq, dtype=torch.bool)
    keep[0, 5] = False
    assert not torch.isnan(out[keep]).any()
    _check(BF16, (ref[keep],), (out[keep],), "live rows")


# ---------------------------------------------------------------------------------------------------------------
# 8. determinism
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Tq,Nk", [pytest.param(dt, tq, nk, id="%s-%d-%d" % (n, tq, nk)) for n, dt, tq, nk in (
    ("bf16", BF16, 150, 150), ("bf16", BF16, 54, 100), ("f32", F32, 150, 150), ("f32", F32, 33, 256), ("bf16", BF16, 54, 200))])
def test_determinism(dtype, Tq, Nk):
    """Three runs on the same inputs.  The matrix-core kernels have no atomics: forward and backward bit-identical (what the graph-step
    tests rely on).  fp32-arithmetic kernels (float32, and bf16 storage on the fallback): forward and dq bit-identical; dk / dv are
    summed in LDS with atomic adds from eight waves whose order is not fixed, so they are held to 1e-4 of each other.
    Observed on MI355X: exactly that -- dk and dv of (150, 150) and (33, 256) in float32 and of the bf16 fallback at (54, 200) differed
    in their last bits between runs, every other tensor of every case was bit-identical in all three runs."""
    B, H = 2, 8
    q, k, v, cot = _inputs(B, Tq, Nk, H, dtype, seed=15)
    mask = _mask("query", B, Tq, Nk)
    args = _dev(q, k, v, cot, mask)
    runs = [_run(*args) for _ in range(3)]
    for other in runs[1:]:
        for name, a, b in zip(NAMES, runs[0], other):
            _same(dtype, name, a, b, Tq, Nk)


# ---------------------------------------------------------------------------------------------------------------
# 9. dropout
# ---------------------------------------------------------------------------------------------------------------
def _seed(n):
    return torch.tensor([n], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("masked", (False, True))
def test_dropout_mask_is_the_same_in_every_kernel_family(masked):
    """One seed_dev, index ((b H + h) Tq + q) Nk + k: fp32, bf16 matrix-core and bf16 fallback (forced by layout, and by Nk > 160)
    must drop the same elements."""
    B, H, p = 2, 4, 0.3
    for Tq, Nk in ((40, 100), (17, 160)):
        mask = _mask("key", B, Tq, Nk).to(DEV) if masked else None
        seed = _seed(555 + Nk)
        f32 = _keep_mask(F32, B, H, Tq, Nk, p, seed, mask)
        mfma = _keep_mask(BF16, B, H, Tq, Nk, p, seed, mask)
        fall = _keep_mask(BF16, B, H, Tq, Nk, p, seed, mask, layout="offset4")
        assert torch.equal(f32, mfma), (Tq, Nk)
        assert torch.equal(f32, fall), (Tq, Nk)
        if masked:
            assert not f32[mask.expand_as(f32)].any()
        assert not torch.equal(f32, _keep_mask(F32, B, H, Tq, Nk, p, _seed(556 + Nk), mask))  # another seed, another mask
    mask = _mask("key", B, 40, 200).to(DEV) if masked else None
    assert torch.equal(_keep_mask(F32, B, H, 40, 200, p, _seed(9), mask), _keep_mask(BF16, B, H, 40, 200, p, _seed(9), mask))


def _within_5_sigma(rate, expect, n, what):
    sigma = math.sqrt(expect * (1 - expect) / n)
    assert 5 * sigma < 0.05, (what, n)
    assert abs(rate - expect) <= 5 * sigma, (what, rate, expect, 5 * sigma)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", (0.1, 0.5))
def test_dropout_keep_rate_and_independence(p, dtype):
    """Keep rate 1 - p within 5 sigma in every (b, h) slice and every 16-row band; the masks of two heads, two batches and two
    adjacent rows agree on p^2 + (1-p)^2 of their elements within 5 sigma (a slice that copied another would agree on all)."""
    B, H, Tq, Nk = 2, 4, 160, 160
    keep = _keep_mask(dtype, B, H, Tq, Nk, p, _seed(31337)).cpu()
    for b in range(B):
        for h in range(H):
            _within_5_sigma(keep[b, h].float().mean().item(), 1 - p, Tq * Nk, ("slice", b, h))
    for r in range(0, Tq, 16):
        _within_5_sigma(keep[:, :, r:r + 16].float().mean().item(), 1 - p, B * H * 16 * Nk, ("band", r))
    agree = p * p + (1 - p) * (1 - p)
    for h in range(1, H):
        _within_5_sigma((keep[:, 0] == keep[:, h]).float().mean().item(), agree, B * Tq * Nk, ("heads 0", h))
    _within_5_sigma((keep[0] == keep[1]).float().mean().item(), agree, H * Tq * Nk, "batches")
    _within_5_sigma((keep[:, :, :-1] == keep[:, :, 1:]).float().mean().item(), agree, B * H * (Tq - 1) * Nk, "adjacent rows")
    _within_5_sigma((keep[..., :-1] == keep[..., 1:]).float().mean().item(), agree, B * H * Tq * (Nk - 1), "adjacent keys")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_edges_of_p(dtype):
    attention, Fn = _fn()
    q, k, v, cot = _dev(*_inputs(2, 20, 45, 4, dtype, seed=16))
    ev = _run(q, k, v, cot)
    qq, kk, vv = (x.detach().requires_grad_(True) for x in (q, k, v))
    out = Fn.apply(qq, kk, vv, None, 0.125, 0.0, 77, _seed(5))  # p = 0 with seeds present: nothing is dropped or rescaled
    out.backward(cot)
    for name, a, b in zip(NAMES, (out.detach(), qq.grad, kk.grad, vv.grad), ev):
        _same(dtype, name, a, b, 20, 45)
    assert _bits(attention(q, k, v, dropout_p=0.0, training=True), ev[0])
    assert _bits(attention(q, k, v, dropout_p=0.4, training=False), ev[0])
    with pytest.raises(RuntimeError, match="not supported"):
        attention(q, k, v, dropout_p=1.0, training=True)
