"""Streaming kernels at the points where they can be wrong unnoticed: statistics of inputs whose mean is large next to their
spread, the edges of the row loops (fewer rows than a workgroup holds, the ragged last trip of the persistent LayerNorm backward,
the nontemporal store path), and the flat Adam kernel called directly (capped grid: main loop + tail, both gradient types, device
hyper-parameters, rejections).  Every reference is torch in float64 on the same dtype-rounded inputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from grit_amd import lib as binding

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, BAD_ARG, UNSUPPORTED = binding.OK, binding.ERR_BAD_ARG, binding.ERR_UNSUPPORTED
GN_CHUNKS = binding.GN_CHUNKS
EPS = 1e-5
SENTINEL = -12345.0  # exactly representable in bf16 and fp32
BF16, F32 = torch.bfloat16, torch.float32


_ptr = binding.ptr


def _lib():
    return binding.load(), binding.current_stream_ptr()


def _close(got, want, rtol, atol, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy(), rtol=rtol, atol=atol,
                               err_msg=what)


def _close_scaled(got, want, frac, what=""):
    """max |got - want| <= frac * max |want| (how the existing tests bound gradients; <= so that an exactly zero gradient passes)"""
    scale = want.abs().max().item()
    err = (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()
    assert np.isfinite(err) and err <= frac * scale, (what, err, scale)


# ---------------------------------------------------------------------------------------------------------------- GroupNorm

def _group_offsets(B, G, C, mean, gen):
    """[B, 1, C]: +-mean per (image, group), random sign -- a global constant would cancel in any single shifted sum"""
    sign = torch.randint(0, 2, (B, G), generator=gen).double() * 2 - 1
    return (sign * mean).repeat_interleave(C // G, dim=1).view(B, 1, C)


@functools.lru_cache(maxsize=None)
def _gn_case(C, G, B, Ts, dtype, wdtype, mean, std):
    """Inputs (dtype-rounded, on the host) and the float64 reference of one offset case; computed once, never modified."""
    gen = torch.Generator().manual_seed(C + int(mean) + len(Ts))
    xs = [(torch.randn(B, T, C, generator=gen).double() * std + _group_offsets(B, G, C, mean, gen)).to(dtype) for T in Ts]
    ws = [(1 + 0.2 * torch.randn(C, generator=gen)).to(wdtype) for _ in Ts]
    bs = [(0.1 * torch.randn(C, generator=gen)).to(wdtype) for _ in Ts]
    cot = torch.randn(B, sum(Ts), C, generator=gen).to(dtype)
    xr, wr, br = ([z.double().requires_grad_(True) for z in zs] for zs in (xs, ws, bs))
    ref = torch.cat([F.group_norm(x.transpose(1, 2), G, w, b, EPS).transpose(1, 2) for x, w, b in zip(xr, wr, br)], 1)
    ref.backward(cot.double())
    stats = []
    for x in xs:
        xg = x.double().view(B, x.shape[1], G, C // G).transpose(1, 2).reshape(B, G, -1)
        stats.append((xg.mean(-1), xg.var(-1, unbiased=False)))
    return dict(xs=xs, ws=ws, bs=bs, cot=cot, ref=ref.detach(), dx=[x.grad for x in xr], dw=[w.grad for w in wr],
                db=[b.grad for b in br], stats=stats)


GN_OFFSETS = [(F32, F32, 0.0, 1.0), (F32, F32, 30.0, 1.0), (F32, F32, 100.0, 0.25),
              (BF16, BF16, 32.0, 2.0), (BF16, BF16, 100.0, 4.0), (BF16, F32, 32.0, 2.0), (BF16, F32, 100.0, 4.0)]
GN_SHAPE = dict(B=2, G=32, Ts=(1601, 33))


@pytest.mark.parametrize("dtype,wdtype,mean,std", GN_OFFSETS)
@pytest.mark.parametrize("C", [256, 512])
def test_group_norm_offset_groups_forward_and_backward(C, dtype, wdtype, mean, std):
    """group_norm_levels on groups whose mean is up to 400 x their spread (sign drawn per (image, group)) against the float64
    F.group_norm composition: y, dx, dgamma, dbeta within the tolerances test_group_norm_levels_vs_torch uses for friendly inputs.
    The one-pass statistics this kernel had (var = E[x^2] - E[x]^2 of the raw values, A - mu*B in the backward) put y off by up to
    0.16 at mean 100 / std 0.25 (95 % of the elements outside the tolerance, rstd 3 % wrong); statistics of x - pivot do not.
    The reference is checked first: finite, and normalised to unit spread ((y_ref - beta) / gamma has std 1 up to eps / var)."""
    from grit_amd.ops.group_norm import group_norm_levels
    B, G, Ts = GN_SHAPE["B"], GN_SHAPE["G"], GN_SHAPE["Ts"]
    case = _gn_case(C, G, B, Ts, dtype, wdtype, mean, std)
    start = 0
    for T, w, b in zip(Ts, case["ws"], case["bs"]):
        yn = (case["ref"][:, start:start + T] - b.double()) / w.double()
        assert torch.isfinite(yn).all() and abs(yn.std().item() - 1.0) < 1e-2, yn.std().item()
        start += T
    xd, wd, bd = ([z.to(DEV).requires_grad_(True) for z in case[k]] for k in ("xs", "ws", "bs"))
    out = group_norm_levels(xd, wd, bd, G, EPS)
    assert out.shape == (B, sum(Ts), C) and out.dtype == dtype and out.is_contiguous()
    out.backward(case["cot"].to(DEV))
    tol = 3e-2 if dtype == BF16 else 2e-4
    _close(out, case["ref"], tol, tol, "y")
    for l in range(len(Ts)):
        _close_scaled(xd[l].grad, case["dx"][l], tol, "dx level %d" % l)
        _close_scaled(wd[l].grad, case["dw"][l], 2e-2 if wdtype == BF16 else 3e-3, "dgamma level %d" % l)
        _close_scaled(bd[l].grad, case["db"][l], 2e-2 if wdtype == BF16 else 3e-3, "dbeta level %d" % l)


def _gn_fwd_direct(x, w, b, G, y=None, y_bstride=None):
    """grit_groupnorm_tokens_fwd on device tensors -> (status, y, mean, rstd)"""
    lib, stream = _lib()
    B, T, C = x.shape
    if y is None:
        y = torch.empty(B, T, C, dtype=x.dtype, device=x.device)
        y_bstride = T * C
    mean = torch.full((B, G), SENTINEL, device=x.device)
    rstd = torch.full((B, G), SENTINEL, device=x.device)
    work = torch.empty(B * GN_CHUNKS * 2 * max(G, 1), device=x.device)
    st = lib.grit_groupnorm_tokens_fwd(_ptr(x), x.stride(0), _ptr(w), _ptr(b), B, T, C, G, EPS, int(x.dtype == BF16),
                                       int(w.dtype == BF16), _ptr(y), y_bstride, _ptr(mean), _ptr(rstd), _ptr(work), stream)
    torch.cuda.synchronize()
    return st, y, mean, rstd


@pytest.mark.parametrize("dtype,wdtype,mean,std", GN_OFFSETS)
@pytest.mark.parametrize("C", [256, 512])
def test_group_norm_saved_statistics(C, dtype, wdtype, mean, std):
    """mean / rstd as grit_groupnorm_tokens_fwd saves them for the backward, against float64 statistics of the same inputs.

    rstd: relative error <= 1e-5.  A numpy fp32 restatement of the kernel's two launches (T = 1601, 16 channels per group, 16
    chunks) gives 2e-8 ... 1.3e-7 with sums of x - pivot, and 1.1e-4 (mean 30 / std 1) to 4.2e-4 (mean 100 / std 0.25) with the
    one-pass sums of raw x: the bound sits 100 x above the first and 10 x below the second.  This is the check that sees the fault
    with bf16 inputs, where the rounding of y (tolerance 3e-2) hides it.  Measured on an MI355X at T = 1601: the one-pass kernel
    1.9e-4 (30 / 1), 3.1e-2 (100 / 0.25), 2.8e-5 (bf16 32 / 2), 6.9e-5 (bf16 100 / 4); the shifted sums 1.3e-7 ... 6.6e-7.
    mean: |error| <= 2 * 2^-24 * |mean| + 1e-5 * std -- the stored fp32 mean is pivot + shifted mean, two roundings at the
    magnitude of the mean, and the shifted mean is a statistic of the spread held to the same 1e-5 as rstd."""
    B, G, Ts = GN_SHAPE["B"], GN_SHAPE["G"], GN_SHAPE["Ts"]
    case = _gn_case(C, G, B, Ts, dtype, wdtype, mean, std)
    for l, T in enumerate(Ts):
        st, _, got_mean, got_rstd = _gn_fwd_direct(case["xs"][l].to(DEV), case["ws"][l].to(DEV), case["bs"][l].to(DEV), G)
        assert st == OK
        ref_mean, ref_var = case["stats"][l]
        ref_rstd = (ref_var + EPS).rsqrt()
        rel = ((got_rstd.double().cpu() - ref_rstd) / ref_rstd).abs().max().item()
        err_mean = (got_mean.double().cpu() - ref_mean).abs()
        print("T=%d rstd max rel. error %.3g, mean max abs. error %.3g" % (T, rel, err_mean.max().item()))
        assert rel <= 1e-5, (T, rel)
        assert bool((err_mean <= 2 * 2.0 ** -24 * ref_mean.abs() + 1e-5 * ref_var.sqrt()).all()), (T, err_mean.max().item())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,G", [(512, 1), (512, 8), (512, 64), (256, 1), (256, 32)])
def test_group_norm_edges(C, G, dtype):
    """Levels of 1, 7 and 17 tokens (fewer rows than the 16 chunks; a chunk of 2 rows with one left over) at 64, 8, 1, 32 and 1
    lanes per group; the levels are slices [:, :T] of longer buffers whose remainder is NaN (nothing outside [0, T) may be read:
    one NaN read would poison a whole group); two constant groups.
    Constant group, image 0 / first group: gamma = 1 there and a constant cotangent, so the exact dx is 0: y == beta, and
    |dx| <= rstd * |dy| * 1e-5 = 316 * 0.75 * 1e-5 (the group mean of gamma * dy must reproduce 0.75 to the 1e-5 the statistics
    are held to, and the difference is scaled by rstd = 1 / sqrt(eps)).  Constant group, image 1 / last group: random cotangent,
    dx = rstd * (gamma * dy - mean(gamma * dy)) as the float64 reference has it.  Saved rstd == 1 / sqrt(eps) for both."""
    from grit_amd.ops.group_norm import group_norm_levels
    B, Ts, cpg = 3, (1, 7, 17), C // G
    gen = torch.Generator().manual_seed(C + G)
    bufs, xs = [], []
    for T in Ts:
        buf = torch.full((B, T + 5, C), float("nan"), dtype=dtype)
        buf[:, :T] = (torch.randn(B, T, C, generator=gen) + 3.0).to(dtype)
        buf[0, :T, :cpg] = 2.5
        buf[1, :T, C - cpg:] = -1.5
        bufs.append(buf)
        xs.append(buf[:, :T])
    ws = [(1 + 0.2 * torch.randn(C, generator=gen)).to(dtype) for _ in Ts]
    for w in ws:
        w[:cpg] = 1.0
    bs = [(0.1 * torch.randn(C, generator=gen)).to(dtype) for _ in Ts]
    cot = torch.randn(B, sum(Ts), C, generator=gen).to(dtype)
    cot[0, :, :cpg] = 0.75
    xr, wr, br = ([z.double().requires_grad_(True) for z in zs] for zs in (xs, ws, bs))
    ref = torch.cat([F.group_norm(x.transpose(1, 2), G, w, b, EPS).transpose(1, 2) for x, w, b in zip(xr, wr, br)], 1)
    ref.backward(cot.double())
    assert torch.isfinite(ref).all()
    dev_bufs = [buf.to(DEV) for buf in bufs]
    xd = [buf[:, :T].requires_grad_(True) for buf, T in zip(dev_bufs, Ts)]
    assert all(x.stride(0) == (T + 5) * C for x, T in zip(xd, Ts))
    wd, bd = ([z.to(DEV).requires_grad_(True) for z in zs] for zs in (ws, bs))
    out = group_norm_levels(xd, wd, bd, G, EPS)
    assert out.grad_fn is not None and "GroupNormLevels" in type(out.grad_fn).__name__  # the kernels, not the fallback
    out.backward(cot.to(DEV))
    tol = 3e-2 if dtype == BF16 else 2e-4
    _close(out, ref, tol, tol, "y")
    start = 0
    for l, T in enumerate(Ts):
        dx = xd[l].grad
        assert torch.isfinite(dx).all() and torch.isfinite(wd[l].grad).all() and torch.isfinite(bd[l].grad).all()
        # the constant group of image 1 has gradients 1 / sqrt(eps) = 316 x larger than the rest: bounded on their own scale
        got_rest, ref_rest = dx.detach().clone(), xr[l].grad.clone()
        got_rest[1, :, C - cpg:] = 0
        ref_rest[1, :, C - cpg:] = 0
        _close_scaled(got_rest, ref_rest, tol, "dx level %d" % l)
        _close_scaled(dx[1, :, C - cpg:], xr[l].grad[1, :, C - cpg:], tol, "dx of the constant group, level %d" % l)
        _close_scaled(wd[l].grad, wr[l].grad, 2e-2 if dtype == BF16 else 3e-3, "dgamma level %d" % l)
        _close_scaled(bd[l].grad, br[l].grad, 2e-2 if dtype == BF16 else 3e-3, "dbeta level %d" % l)
        y0 = out[0, start:start + T, :cpg].detach().float().cpu()
        _close(y0, bs[l][:cpg].float().expand(T, cpg), 0, tol, "y of a constant group is beta")
        assert dx[0, :, :cpg].abs().max().item() <= EPS ** -0.5 * 0.75 * 1e-5
        start += T
    # saved statistics and the strided write: the C entry writing level 1 into its slice of a flat map full of sentinels
    S, s0, T = sum(Ts), Ts[0], Ts[1]
    flat = torch.full((B, S, C), SENTINEL, dtype=dtype, device=DEV)
    st, _, mean, rstd = _gn_fwd_direct(xd[1].detach(), wd[1].detach(), bd[1].detach(), G, y=flat[:, s0:s0 + T], y_bstride=S * C)
    assert st == OK
    assert torch.equal(flat[:, s0:s0 + T], out.detach()[:, s0:s0 + T])
    assert bool((flat[:, :s0] == SENTINEL).all()) and bool((flat[:, s0 + T:] == SENTINEL).all())
    for b_, g_, c_ in ((0, 0, 2.5), (1, G - 1, -1.5)):
        assert abs(rstd[b_, g_].item() * EPS ** 0.5 - 1.0) <= 1e-5 and abs(mean[b_, g_].item() - c_) <= 2 * 2.0 ** -24 * abs(c_)
    # the buffers behind the slices still hold their NaN, the rows in front of them their values
    for buf, host in zip(dev_bufs, bufs):
        assert torch.equal(buf.detach().cpu().view(torch.int16 if dtype == BF16 else torch.int32),
                           host.view(torch.int16 if dtype == BF16 else torch.int32))


@pytest.mark.parametrize("C,G,dtype,wdtype", [(384, 32, F32, F32), (512, 3, F32, F32), (512, 128, F32, F32), (256, 64, BF16, BF16),
                                               (512, 32, F32, BF16)])
def test_group_norm_rejections(C, G, dtype, wdtype):
    """A channel count other than 256 / 512, a group count that does not divide C, more than 64 groups, channels per group not
    a multiple of 8, fp32 maps with bf16 parameters: both C entry points answer GRIT_ERR_UNSUPPORTED before any launch (outputs
    keep their sentinels), and group_norm_levels takes the library composition, equal to the float64 reference.  (torch has no
    GroupNorm for fp32 maps with bf16 parameters and G = 3 does not divide 512 for torch either: there only the return codes are
    checked.)"""
    from grit_amd.ops import group_norm as GN
    lib, stream = _lib()
    B, T = 2, 33
    gen = torch.Generator().manual_seed(C + G)
    x = (torch.randn(B, T, C, generator=gen) + 1.0).to(dtype).to(DEV)
    w = (1 + 0.2 * torch.randn(C, generator=gen)).to(wdtype).to(DEV)
    b = (0.1 * torch.randn(C, generator=gen)).to(wdtype).to(DEV)
    y = torch.full((B, T, C), SENTINEL, dtype=dtype, device=DEV)
    st, _, mean, rstd = _gn_fwd_direct(x, w, b, G, y=y, y_bstride=T * C)
    assert st == UNSUPPORTED
    dx = torch.full((B, T, C), SENTINEL, dtype=dtype, device=DEV)
    dwb = torch.full((2, C), SENTINEL, dtype=wdtype, device=DEV)
    work = torch.empty(B * GN_CHUNKS * 2 * C, device=DEV)
    st = lib.grit_groupnorm_tokens_bwd(_ptr(x), T * C, _ptr(x), T * C, _ptr(w), _ptr(mean), _ptr(rstd), B, T, C, G, int(dtype == BF16),
                                       int(wdtype == BF16), _ptr(dx), _ptr(dwb[0]), _ptr(dwb[1]), _ptr(work), stream)
    assert st == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (y, mean, rstd, dx, dwb):
        assert bool((t == SENTINEL).all())
    assert not GN._fits([x], [w], [b], G)
    if C % G or dtype != wdtype:
        return
    xd, wd, bd = (z.clone().requires_grad_(True) for z in (x, w, b))
    cot = torch.randn(B, T, C, generator=gen).to(dtype)
    out = GN.group_norm_levels([xd], [wd], [bd], G, EPS)
    out.backward(cot.to(DEV))
    xr, wr, br = (z.detach().double().cpu().requires_grad_(True) for z in (x, w, b))
    ref = F.group_norm(xr.transpose(1, 2), G, wr, br, EPS).transpose(1, 2)
    ref.backward(cot.double())
    tol = 3e-2 if dtype == BF16 else 2e-4
    _close(out, ref, tol, tol, "y")
    _close_scaled(xd.grad, xr.grad, tol, "dx")
    _close_scaled(wd.grad, wr.grad, 2e-2 if wdtype == BF16 else 3e-3, "dgamma")
    _close_scaled(bd.grad, br.grad, 2e-2 if wdtype == BF16 else 3e-3, "dbeta")


# ---------------------------------------------------------------------------------------------------------------- LayerNorm

LN_DTYPES = [(BF16, BF16), (BF16, F32), (F32, F32)]


def _rows_per_block(C):
    return 4 * (64 // min(C // 8, 64))  # 16, 8, 4 for C = 128, 256, >= 512


def _ln_tols(dtype, offset=0.0, std=1.0):
    """(rtol, atol) of y and dx: the tolerance of test_layer_norm_kernels_vs_torch, plus for offset rows 8 * 2^-24 * |offset| / std
    -- a rounding bound of the fp32 row mean (a few roundings at the magnitude of the offset), seen through 1 / std."""
    tol = 2e-2 if dtype == BF16 else 1e-5
    return tol, tol + 8 * 2.0 ** -24 * abs(offset) / std


def _ln_params(C, wdtype, gen):
    return (1 + 0.2 * torch.randn(C, generator=gen)).to(wdtype), (0.1 * torch.randn(C, generator=gen)).to(wdtype)


def _ln_reference(x, w, b, cot):
    xr, wr, br = (z.double().requires_grad_(True) for z in (x, w, b))
    y = F.layer_norm(xr, (x.shape[-1],), wr, br, EPS)
    y.backward(cot.double())
    return y.detach(), xr.grad, wr.grad, br.grad


def _ln_run(x, w, b, cot):
    from grit_amd.ops.layer_norm import layer_norm
    xd, wd, bd = (z.to(DEV, copy=True).requires_grad_(True) for z in (x, w, b))
    y = layer_norm(xd, wd, bd, EPS)
    y.backward(cot.to(DEV))
    return y.detach(), xd.grad, wd.grad, bd.grad


def _ln_compare(got, ref, dtype, wdtype, offset=0.0, std=1.0):
    rtol, atol = _ln_tols(dtype, offset, std)
    _close(got[0], ref[0], rtol, atol, "y")
    _close(got[1], ref[1], rtol, atol, "dx")
    _close_scaled(got[2], ref[2], 2e-2 if wdtype == BF16 else 2e-3, "dgamma")
    _close_scaled(got[3], ref[3], 2e-2 if wdtype == BF16 else 2e-3, "dbeta")


def _offset_rows(rows, C, dtype, gen):
    """per-row mean drawn from {0, +64, -64}; std 1 (bf16: 4, so that the spread is a few bf16 steps at 64)"""
    std = 4.0 if dtype == BF16 else 1.0
    mu = (torch.randint(0, 3, (rows, 1), generator=gen) - 1).double() * 64.0
    return (torch.randn(rows, C, generator=gen).double() * std + mu).to(dtype), std


@pytest.mark.parametrize("C", [128, 512, 2048])
@pytest.mark.parametrize("dtype,wdtype", LN_DTYPES)
def test_layer_norm_offset_rows(C, dtype, wdtype):
    """Rows with mean 0 / +64 / -64 and std 1 (bf16: 4): the two-pass statistics on the register copy keep y, dx, dgamma, dbeta at
    the friendly-input tolerance plus the rounding bound of the fp32 mean (_ln_tols)."""
    gen = torch.Generator().manual_seed(C)
    rows = 203
    x, std = _offset_rows(rows, C, dtype, gen)
    w, b = _ln_params(C, wdtype, gen)
    cot = torch.randn(rows, C, generator=gen).to(dtype)
    _ln_compare(_ln_run(x, w, b, cot), _ln_reference(x, w, b, cot), dtype, wdtype, 64.0, std)


@pytest.mark.parametrize("C", [128, 256, 512, 2048])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_layer_norm_tiny_row_counts_and_constant_rows(C, dtype):
    """1 row, 3 rows, one row fewer and one row more than a workgroup holds (idle lanes clamp to the last row and must not store
    or add to the sums); row 0 is constant: variance 0, y == bias, dx = rstd * (gamma * dy - mean(gamma * dy)) finite and within the
    relative tolerance of its own largest element (rstd = 316 amplifies the fp32 rounding of the cotangent's mean, so the absolute
    tolerance of the ordinary rows does not apply to it)."""
    rpb = _rows_per_block(C)
    for rows in sorted({1, 3, rpb - 1, rpb + 1}):
        gen = torch.Generator().manual_seed(C + rows)
        x = (torch.randn(rows, C, generator=gen) * 2 + 0.5).to(dtype)
        x[0] = 3.0
        w, b = _ln_params(C, dtype, gen)
        cot = torch.randn(rows, C, generator=gen).to(dtype)
        got, ref = _ln_run(x, w, b, cot), _ln_reference(x, w, b, cot)
        assert all(torch.isfinite(t).all() for t in got), rows
        rtol, atol = _ln_tols(dtype)
        _close(got[0], ref[0], rtol, atol, "y, %d rows" % rows)
        _close(got[0][0], b, 0, atol, "y of the constant row is the bias")
        # dx of the constant row is 1 / sqrt(eps) = 316 x the centred cotangent: bounded on its own scale, the other rows as usual
        _close_scaled(got[1][0], ref[1][0], rtol, "dx of the constant row, %d rows" % rows)
        _close(got[1][1:], ref[1][1:], rtol, atol, "dx, %d rows" % rows)
        _close_scaled(got[2], ref[2], 2e-2 if dtype == BF16 else 2e-3, "dgamma, %d rows" % rows)
        _close_scaled(got[3], ref[3], 2e-2 if dtype == BF16 else 2e-3, "dbeta, %d rows" % rows)


@pytest.mark.parametrize("C,rows", [(128, 2 * 1024 * 16 + 17), (512, 2 * 1024 * 4 + 5)])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_layer_norm_backward_ragged_third_trip(C, rows, dtype):
    """The persistent backward (grid capped at 1024 workgroups): two full passes and a third in which one workgroup is full and
    the next holds a single live row -- `live` false inside a running wave, and waves with two trips beside waves with three."""
    gen = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, C, generator=gen) * 2 + 0.5).to(dtype)
    w, b = _ln_params(C, dtype, gen)
    cot = torch.randn(rows, C, generator=gen).to(dtype)
    _ln_compare(_ln_run(x, w, b, cot), _ln_reference(x, w, b, cot), dtype, dtype)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_add_layer_norm_backward_ragged_third_trip_with_branch_sums(dtype):
    """grit_add_layernorm_bwd at 8197 rows of 512 channels (7 samples of 1171 rows, drop-path factors 0 and 1.25): the gradient
    of the branch and its column sums (the bias gradient of the Linear in front, a third accumulator carried through the row
    loop) against the float64 composition.  The column sums are a bias gradient and bounded like one: 2e-2 (bf16) / 2e-3 (fp32)
    of the largest reference sum, the constants the LayerNorm tests use for dgamma / dbeta."""
    from grit_amd.ops.layer_norm import _add_layer_norm_backward, add_layer_norm
    C, B, L = 512, 7, 1171
    gen = torch.Generator().manual_seed(L)
    sc, br = (torch.randn(B, L, C, generator=gen) * 1.5).to(dtype), torch.randn(B, L, C, generator=gen).to(dtype)
    w, b = _ln_params(C, dtype, gen)
    scale = torch.tensor([1.25, 0.0, 1.25, 1.25, 0.0, 1.25, 1.25])
    cot_x, cot_y = torch.randn(B, L, C, generator=gen).to(dtype), torch.randn(B, L, C, generator=gen).to(dtype)
    s64, b64, w64, bb64 = (z.double().requires_grad_(True) for z in (sc, br, w, b))
    sum64 = s64 + b64 * scale.double().view(-1, 1, 1)
    x_ref = sum64 + (sum64.detach().to(dtype).double() - sum64.detach())  # the sum is stored in the tensor dtype
    y_ref = F.layer_norm(x_ref, (C,), w64, bb64, EPS)
    torch.autograd.backward([x_ref, y_ref], [cot_x.double(), cot_y.double()])
    sd, bd, wd, bbd = (z.to(DEV).requires_grad_(True) for z in (sc, br, w, b))
    x, y = add_layer_norm(sd, bd, scale.to(DEV), wd, bbd, EPS)
    tol = 2e-2 if dtype == BF16 else 1e-5
    _close(y, y_ref, tol, tol, "y")
    x2, weight, mean, rstd, scale_dev = y.grad_fn.saved_tensors
    dx, d_branch, sums = _add_layer_norm_backward(x2, weight, mean, rstd, scale_dev, cot_x.to(DEV), cot_y.to(DEV), B, True, 0.0, None)
    gtol = 4e-2 if dtype == BF16 else 1e-4
    _close(dx.view(B, L, C), s64.grad, gtol, gtol, "d shortcut")
    _close(d_branch.view(B, L, C), b64.grad, gtol, gtol * 1.25, "d branch")
    assert not d_branch.view(B, L, C)[1].any() and not d_branch.view(B, L, C)[4].any()  # dropped samples
    frac = 2e-2 if dtype == BF16 else 2e-3
    _close_scaled(sums[0], w64.grad, frac, "dgamma")
    _close_scaled(sums[1], bb64.grad, frac, "dbeta")
    _close_scaled(sums[2], b64.grad.sum((0, 1)), frac, "column sums of d branch")


@pytest.mark.parametrize("C,dtype", [(4096, BF16), (2048, F32)])
def test_layer_norm_nontemporal_path(C, dtype):
    """2049 rows: just above the 16 MB at which forward and backward switch to nontemporal stores.  Equal to the float64
    reference, and y / dx bit-equal, row by row, to the same rows run in calls of 512 rows (below the threshold): the store
    flavour changes no value."""
    rows = 2049
    gen = torch.Generator().manual_seed(C)
    x = (torch.randn(rows, C, generator=gen) * 2 + 0.5).to(dtype)
    w, b = _ln_params(C, dtype, gen)
    cot = torch.randn(rows, C, generator=gen).to(dtype)
    assert x.numel() * x.element_size() >= 16 << 20 > 512 * C * x.element_size()
    got = _ln_run(x, w, b, cot)
    _ln_compare(got, _ln_reference(x, w, b, cot), dtype, dtype)
    for r0 in (0, 512, 1024, 1536, rows - 512):
        part = _ln_run(x[r0:r0 + 512], w, b, cot[r0:r0 + 512])
        assert torch.equal(part[0], got[0][r0:r0 + 512]) and torch.equal(part[1], got[1][r0:r0 + 512]), r0


@pytest.mark.parametrize("B,H,W,C,dtype", [(2, 8, 12, 128, BF16), (1, 10, 6, 512, F32)])
def test_patch_merging_layer_norm_offset_rows(B, H, W, C, dtype):
    """merge_layer_norm on a map whose 2 x 2 patches carry a common offset of 0 / +64 / -64 (so the merged rows do) against
    float64 F.layer_norm of the materialised merged view; tolerances of the offset-row test."""
    from grit_amd.ops.layer_norm import merge_layer_norm
    gen = torch.Generator().manual_seed(B * H + C)
    std = 4.0 if dtype == BF16 else 1.0
    mu = (torch.randint(0, 3, (B, H // 2, 1, W // 2, 1, 1), generator=gen) - 1).double() * 64.0
    x = (torch.randn(B, H // 2, 2, W // 2, 2, C, generator=gen).double() * std + mu).to(dtype).view(B, H * W, C)
    w, b = _ln_params(4 * C, dtype, gen)
    cot = torch.randn(B, (H // 2) * (W // 2), 4 * C, generator=gen).to(dtype)
    xr, wr, br = (z.double().requires_grad_(True) for z in (x, w, b))
    merged = xr.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, (H // 2) * (W // 2), 4 * C)
    y_ref = F.layer_norm(merged, (4 * C,), wr, br, EPS)
    y_ref.backward(cot.double())
    xd, wd, bd = (z.to(DEV).requires_grad_(True) for z in (x, w, b))
    y = merge_layer_norm(xd, H, W, wd, bd, EPS)
    assert y is not None
    y.backward(cot.to(DEV))
    _ln_compare((y.detach(), xd.grad, wd.grad, bd.grad), (y_ref.detach(), xr.grad, wr.grad, br.grad), dtype, dtype, 64.0, std)


def test_patch_embedding_offset_tokens():
    """grit_patch_embed_ln_fwd on tokens with mean 64 and std 4: conv weights in {-0.5, 0, 0.5}, integer pixels in [-2, 2] and
    biases 64 + {-2 ... 2} make every conv output a multiple of 0.5 below 128 -- exact in fp32 in any summation order and exact in
    bf16, so the LayerNorm input is the same on both sides and only the statistics are compared.  Against float64 LayerNorm of
    those tokens, within the bounds test_patch_embedding_in_one_pass uses (bf16 output: max 0.06, mean 4e-3)."""
    from grit_amd.models.common.swin_model import PatchEmbed
    from grit_amd.ops.layer_norm import LayerNorm
    B, H, W, C = 2, 64, 128, 128
    gen = torch.Generator().manual_seed(C + H)
    pe = PatchEmbed(patch_size=4, in_chans=3, embed_dim=C, norm_layer=LayerNorm).to(DEV).to(BF16)
    with torch.no_grad():
        pe.proj.weight.copy_((torch.randint(0, 3, (C, 3, 4, 4), generator=gen) - 1) * 0.5)
        pe.proj.bias.copy_(64.0 + torch.randint(-2, 3, (C,), generator=gen))
        pe.norm.weight.copy_(1.0 + 0.1 * torch.randn(C, generator=gen))
        pe.norm.bias.copy_(0.1 * torch.randn(C, generator=gen))
    for p in pe.parameters():
        p.requires_grad_(False)
    img = torch.randint(-2, 3, (B, 3, H, W), generator=gen).float().to(DEV)
    with torch.no_grad():
        fused = pe._fused_tokens(img)
        assert fused is not None and fused.shape == (B, (H // 4) * (W // 4), C) and fused.dtype == BF16
        conv = F.conv2d(img.cpu().double(), pe.proj.weight.cpu().double(), pe.proj.bias.cpu().double(), stride=4)
        tok = conv.flatten(2).transpose(1, 2)
        assert torch.equal(tok, tok.to(BF16).double()) and abs(tok.mean().item() - 64.0) < 1.0 and 3.0 < tok.std().item() < 5.0
        ref = F.layer_norm(tok, (C,), pe.norm.weight.cpu().double(), pe.norm.bias.cpu().double(), pe.norm.eps)
    err = (fused.cpu().double() - ref).abs()
    assert float(err.max()) <= 0.06 and float(err.mean()) <= 4e-3, (float(err.max()), float(err.mean()))


# ---------------------------------------------------------------------------------------------------------------- flat Adam

ADAM_GUARD = 64  # elements behind n in every buffer
LR, BETA1, BETA2, ADAM_EPS = 1e-2, 0.9, 0.999, 1e-8
ADAM_BLOCK_CAP = 8192 * 256  # quads one pass of the capped grid covers


def _f32(v):
    return float(np.float32(v))


def _bias_corrections(step):
    return _f32(1.0 - BETA1 ** step), _f32((1.0 - BETA2 ** step) ** 0.5)


@functools.lru_cache(maxsize=None)
def _adam_state(n, grad_dtype):
    """(p, g, m, v) with ADAM_GUARD sentinels behind n; gradients ~0.1, non-zero prior moments; a few elements at the front, in
    the middle and at the end have g = 0 and v = 0 (denominator = eps), every other one m = 0 as well.  Never modified."""
    gen = torch.Generator(device=DEV).manual_seed(n % 1000003)
    total = n + ADAM_GUARD
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


def _adam_call(n, p, g, m, v, compute, step, grad_scale, hyper=None):
    lib, stream = _lib()
    bc1, bc2s = _bias_corrections(step)
    head = (_ptr(p), _ptr(g), int(g.dtype == BF16), _ptr(m), _ptr(v), None if compute is None else _ptr(compute), n)
    if hyper is None:
        return lib.grit_adam_flat(*head, LR, BETA1, BETA2, ADAM_EPS, bc1, bc2s, grad_scale, stream)
    return lib.grit_adam_flat_dev(*head, BETA1, BETA2, ADAM_EPS, grad_scale, _ptr(hyper), stream)


def _adam_fresh(n, grad_dtype):
    p, g, m, v = (t.clone() for t in _adam_state(n, grad_dtype))
    return p, g, m, v, torch.full((n + ADAM_GUARD,), SENTINEL, dtype=BF16, device=DEV)


ADAM_SIZES = [4, 4 * 257, 4 * (ADAM_BLOCK_CAP + 5), 4 * (2 * ADAM_BLOCK_CAP + 1000)]


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("grad_dtype", [BF16, F32])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_flat_one_step_vs_float64(n, grad_dtype, grad_scale, step):
    """One grit_adam_flat step against the formula of adam.hip's header in float64 (hyper-parameters rounded to fp32 as the C
    call receives them): 1 quad, 257 quads (a second workgroup with one live thread), and two sizes beyond the 8192-workgroup
    cap -- cap + 5 quads (five threads take a main-loop trip, all others the tail) and 2 * cap + 1000 (every thread a main-loop
    trip, the first 1000 a tail as well).  Masters and moments within rtol 2e-6 / atol 2e-7, the bound of the FlatAdam test
    against torch.optim.Adam; the bf16 compute copy bit-equal to the rounded master; the guard behind n untouched."""
    p, g, m, v, compute = _adam_fresh(n, grad_dtype)
    assert _adam_call(n, p, g, m, v, compute, step, grad_scale) == OK
    torch.cuda.synchronize()
    p0, g0, m0, v0 = (t[:n].double() for t in _adam_state(n, grad_dtype))
    bc1, bc2s = _bias_corrections(step)
    b1, b2, lr, eps = _f32(BETA1), _f32(BETA2), _f32(LR), _f32(ADAM_EPS)
    gs = g0 * grad_scale
    m_ref = m0 + (gs - m0) * (1.0 - b1)
    v_ref = b2 * v0 + (1.0 - b2) * gs * gs
    p_ref = p0 - (lr / bc1) * (m_ref / (v_ref.sqrt() / bc2s + eps))
    assert torch.isfinite(p_ref).all()
    for name, got, ref in (("exp_avg", m, m_ref), ("exp_avg_sq", v, v_ref), ("param", p, p_ref)):
        assert torch.isfinite(got[:n]).all(), name
        bad = (got[:n].double() - ref).abs() > 2e-7 + 2e-6 * ref.abs()
        assert not bool(bad.any()), (name, int(bad.sum()), int(bad.nonzero()[0]))
    assert torch.equal(compute[:n], p[:n].bfloat16())
    for t in (p, m, v, compute, g):
        assert bool((t[n:] == SENTINEL).all())
    assert torch.equal(g, _adam_state(n, grad_dtype)[1])


@pytest.mark.parametrize("grad_dtype", [BF16, F32])
@pytest.mark.parametrize("n", [4 * 257, 4 * (ADAM_BLOCK_CAP + 5)])
def test_adam_flat_null_compute_and_device_hyper(n, grad_dtype):
    """compute == NULL leaves masters and moments identical to a call that writes a compute copy; grit_adam_flat_dev with
    hyper = {lr / bc1, 1 / sqrt(bc2)} in device memory (fp32 quotients, as the host form computes them) is bit-equal to the
    scalar form of the same step, compute copy included."""
    step, grad_scale = 7, 0.125
    want = _adam_fresh(n, grad_dtype)
    assert _adam_call(n, *want, step, grad_scale) == OK
    null = _adam_fresh(n, grad_dtype)
    assert _adam_call(n, *null[:4], None, step, grad_scale) == OK
    bc1, bc2s = _bias_corrections(step)
    hyper = torch.tensor([np.float32(LR) / np.float32(bc1), np.float32(1.0) / np.float32(bc2s)], dtype=F32, device=DEV)
    dev = _adam_fresh(n, grad_dtype)
    assert _adam_call(n, *dev, step, grad_scale, hyper=hyper) == OK
    torch.cuda.synchronize()
    for i, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
        assert torch.equal(null[i], want[i]), name
        assert torch.equal(dev[i], want[i]), name
    assert torch.equal(dev[4], want[4])
    assert not torch.equal(want[0][:n], _adam_state(n, grad_dtype)[0][:n])  # (a step was taken)


def test_adam_flat_rejections():
    """n % 4 != 0, a master / moment pointer off by 4 bytes, a bf16 gradient pointer off by 2 bytes, a compute pointer off by 2
    bytes: GRIT_ERR_UNSUPPORTED; a hyper pointer off by 4 bytes or missing, a bias correction <= 0, n <= 0: GRIT_ERR_BAD_ARG.  All
    are answered on the host before any launch: no buffer changes."""
    lib, stream = _lib()
    n = 4 * 64
    bufs = _adam_fresh(n, BF16)
    p, g, m, v, compute = bufs
    before = [t.clone() for t in bufs]
    hyper = torch.ones(4, device=DEV)
    bc1, bc2s = _bias_corrections(3)

    def scalar(p_, g_, m_, v_, c_, n_, bc1_=bc1, bc2s_=bc2s):
        return lib.grit_adam_flat(_ptr(p_), _ptr(g_), 1, _ptr(m_), _ptr(v_), _ptr(c_), n_, LR, BETA1, BETA2, ADAM_EPS, bc1_, bc2s_, 1.0,
                                  stream)

    def device(h_):
        return lib.grit_adam_flat_dev(_ptr(p), _ptr(g), 1, _ptr(m), _ptr(v), _ptr(compute), n, BETA1, BETA2, ADAM_EPS, 1.0, h_, stream)

    assert scalar(p, g, m, v, compute, n - 1) == UNSUPPORTED
    assert scalar(p[1:], g, m, v, compute, n - 4) == UNSUPPORTED
    assert scalar(p, g, m[1:], v, compute, n - 4) == UNSUPPORTED
    assert scalar(p, g, m, v[1:], compute, n - 4) == UNSUPPORTED
    assert scalar(p, g[1:], m, v, compute, n - 4) == UNSUPPORTED
    assert scalar(p, g, m, v, compute[1:], n - 4) == UNSUPPORTED
    assert scalar(p, g, m, v, compute, n, bc1_=0.0) == BAD_ARG
    assert scalar(p, g, m, v, compute, n, bc2s_=-1.0) == BAD_ARG
    assert scalar(p, g, m, v, compute, 0) == BAD_ARG
    assert device(_ptr(hyper[1:])) == BAD_ARG
    assert device(None) == BAD_ARG
    # fp32 gradients want 16 bytes
    g32 = g.float()
    assert lib.grit_adam_flat(_ptr(p), _ptr(g32[2:]), 0, _ptr(m), _ptr(v), _ptr(compute), n - 4, LR, BETA1, BETA2, ADAM_EPS, bc1, bc2s,
                              1.0, stream) == UNSUPPORTED
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, before):
        assert torch.equal(t, t0)
    assert device(_ptr(hyper)) == OK  # (the same call with an aligned table is taken)
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0])
