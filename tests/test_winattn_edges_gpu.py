"""Window attention where tests/test_winattn_gpu.py does not reach: the persistent window loop at full grids (three and more trips,
ragged last trips, every workgroup -> (head, group) mapping), the explicit-mask backward, near one-hot softmax rows, the drop-path
skip at the ends of its range and the MFMA backward on maps smaller than a window.  Conventions of that file: `_inputs`, the float
oracle torch_ref.window_attention on the bf16-rounded inputs, RTOL / ATOL for the forward and bounds relative to the oracle's largest
entry for the gradients."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests.test_winattn_gpu import ATOL, RTOL, _inputs

gpu = pytest.mark.gpu
DEV = "cuda"
WS, N, HD = 12, 144, 32
SCALE = HD**-0.5
GRAD_MAX, GRAD_MEAN = 4e-2, 6e-3  # test_backward_vs_oracle: |got - ref| relative to max |ref|
_CHILD = os.environ.get("GRIT_WINATTN_FWD_DMA") == "0" or os.environ.get("GRIT_WINATTN_BWD_DMA") == "0"


# ---------------------------------------------------------------------------------------------------
# inputs, references, comparisons
# ---------------------------------------------------------------------------------------------------
def _hard_inputs(B, H, W, nH, seed, gain):
    """`_inputs` with the q and k slices of qkv and pad_qkv multiplied by `gain` (v as it is).  The gains are powers of two, so scaling
    the bf16 values is bit for bit the scaling before the bf16 rounding."""
    qkv, bias, pad = _inputs(B, H, W, nH, seed=seed)
    C = HD * nH
    assert gain in (1, 2, 4, 8)
    qkv[..., :2 * C] *= gain
    pad[:2 * C] *= gain
    return qkv, bias, pad


def _cotangent(B, H, W, nH, seed=1):
    return torch.randn(B, H * W, HD * nH, generator=torch.Generator().manual_seed(seed)).bfloat16()


def _oracle_with_grads(qkv, bias, pad, cot, H, W, nH, shift, mask=None, dtype=torch.float32):
    a, b_, c = (x.detach().to(dtype).clone().requires_grad_(True) for x in (qkv, bias, pad))  # (fresh leaves: the inputs are shared)
    ref = torch_ref.window_attention(a, b_, c, H, W, nH, WS, shift, SCALE, mask=None if mask is None else mask.to(dtype))
    ref.backward(cot.to(dtype))
    return {"out": ref.detach(), "dqkv": a.grad, "dbias": b_.grad, "dpad": c.grad}  # (dpad None: no window padding at this geometry)


@functools.lru_cache(maxsize=None)
def _case(B, H, W, nH, shift, gain=1):
    """Inputs, cotangent and the float oracle's forward and gradients of one geometry: computed once, shared, never modified."""
    qkv, bias, pad = _hard_inputs(B, H, W, nH, H * W + shift, gain)
    cot = _cotangent(B, H, W, nH)
    case = {"qkv": qkv, "bias": bias, "pad": pad, "cot": cot}
    case.update(_oracle_with_grads(qkv, bias, pad, cot, H, W, nH, shift))
    return case


def _check_forward(got, ref, rtol=RTOL, atol=ATOL, mean=4e-3):
    got, ref = got.detach().float().cpu(), ref.float()
    print("forward: max %.3g mean %.3g" % ((got - ref).abs().max().item(), (got - ref).abs().mean().item()))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=rtol, atol=atol)
    if mean is not None:
        assert (got - ref).abs().mean().item() < mean


def _check_grads(got, ref, max_rel=GRAD_MAX, mean_rel=GRAD_MEAN):
    """got / ref: dicts with dqkv, dbias, dpad.  Bounds relative to the largest entry of the reference gradient."""
    for name in ("dqkv", "dbias", "dpad"):
        g, r = got[name], ref[name]
        if r is None:  # no window padding at this geometry: the oracle never touches pad_qkv
            assert not g.any(), name
            continue
        g, r = g.detach().float().cpu(), r.float()
        assert bool(torch.isfinite(g).all()), name
        scale = r.abs().max().item() + 1e-6
        err, avg = (g - r).abs().max().item(), (g - r).abs().mean().item()
        print("%s: max %.3g mean %.3g of scale %.3g" % (name, err / scale, avg / scale, scale))
        assert err < max_rel * scale, (name, err, scale)
        if mean_rel is not None:
            assert avg < mean_rel * scale, (name, avg, scale)


def _run_op(qkv, bias, pad, cot, H, W, nH, shift, mask=None, dtype=torch.bfloat16):
    """Forward and backward through grit_amd.ops.window_attention; also the saved log-sum-exps (log2 units)."""
    from grit_amd.ops.window_attention import window_attention
    x, y, z = (qkv.to(DEV, dtype).requires_grad_(True), bias.to(DEV).requires_grad_(True), pad.to(DEV, dtype).requires_grad_(True))
    m = None if mask is None else mask.to(DEV).requires_grad_(True)
    out = window_attention(x, y, z, H, W, nH, WS, shift, SCALE, mask=m)
    assert out.dtype == dtype and out.shape == (qkv.shape[0], H * W, HD * nH)
    fn = out.grad_fn if out.grad_fn is not None and hasattr(out.grad_fn, "saved_tensors") else None
    lse2 = fn.saved_tensors[5].clone() if fn is not None else None
    out.backward(cot.to(DEV, dtype))
    assert m is None or m.grad is None  # the mask receives no gradient
    return {"out": out.detach(), "dqkv": x.grad, "dbias": y.grad, "dpad": z.grad, "lse2": lse2}


# ---------------------------------------------------------------------------------------------------
# CPU model of the kernels' storage precision
# ---------------------------------------------------------------------------------------------------
def _to_windows(x, fill, H, W, shift):
    """[B, H*W, X] in token order -> [B * windows, N, X]: the oracle's pad (with `fill` [X], or zeros) / roll / partition."""
    B, X = x.shape[0], x.shape[-1]
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    x = x.view(B, H, W, X)
    if (Hp, Wp) != (H, W):
        full = (torch.zeros(X, dtype=x.dtype) if fill is None else fill).view(1, 1, 1, X).expand(B, Hp, Wp, X).clone()
        full[:, :H, :W] = x
        x = full
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    return torch_ref._partition(x, WS).view(-1, N, X)


def _from_windows(o, B, H, W, shift):
    """[B * windows, N, X] -> [B, H*W, X]: the oracle's reverse / roll back / crop."""
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    o = torch_ref._reverse(o.reshape(-1, WS, WS, o.shape[-1]), WS, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o[:, :H, :W, :].contiguous().view(B, H * W, -1)


def _heads(xw, nH):
    return xw.view(xw.shape[0], N, nH, HD).transpose(1, 2)  # [B_, nH, N, hd]


def _logits(q, k, bias, H, W, nH, shift, mask):
    """The oracle's logits (natural units) [B_, nH, N, N] from window-ordered q, k [B_, nH, N, hd]."""
    t = (q * SCALE) @ k.transpose(-2, -1) + bias.to(q.dtype).unsqueeze(0)
    if mask is None and shift > 0:
        mask = torch_ref.shift_mask(-(-H // WS) * WS, -(-W // WS) * WS, WS, shift, q.device, q.dtype)
    if mask is not None:
        nW = mask.shape[0]
        t = (t.view(-1, nW, nH, N, N) + mask.to(q.dtype).unsqueeze(1).unsqueeze(0)).view(-1, nH, N, N)
    return t


def _r16(x):
    return x.bfloat16().to(x.dtype)


def _storage_model(qkv, bias, pad, H, W, nH, shift, cot=None, mask=None):
    """The oracle's steps in float32 with a bf16 rounding wherever the MFMA kernels keep a value in bf16, and nothing else of the
    kernels (no tiles, no log2 domain, no summation order).  Forward: exp(t - max) rounded to bf16 before PV, the row sum over the
    unrounded terms, bf16 output.  Backward: P = exp(t - lse) and dS = P (dP - delta) in float32 for d(bias), rounded to bf16 as the
    operands of dV = P^T dO, dK = dS^T Q and dQ = dS K; delta = rowsum(dO * O) from the bf16 output; dq / dk / dv stored as bf16, the
    padding tokens' share summed in float32 and rounded once."""
    B, C = qkv.shape[0], HD * nH
    a, c = qkv.float().requires_grad_(cot is not None), pad.float().requires_grad_(cot is not None)
    xw = _to_windows(a, c, H, W, shift)  # [B_, N, 3C]
    q, k, v = (_heads(s, nH) for s in xw.detach().split(C, dim=-1))
    t = _logits(q, k, bias.float(), H, W, nH, shift, mask)
    m = t.amax(-1, keepdim=True)
    e = torch.exp(t - m)
    s = e.sum(-1, keepdim=True)
    o = _r16((_r16(e) @ v) / s)  # [B_, nH, N, hd]
    lse = m + torch.log(s)
    res = {"out": _from_windows(o.transpose(1, 2).reshape(-1, N, C), B, H, W, shift), "lse": lse.squeeze(-1)}
    if cot is None:
        return res
    do = _heads(_to_windows(cot.float(), None, H, W, shift), nH)
    p = torch.exp(t - lse)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-2, -1) - delta)
    dv = _r16(p).transpose(-2, -1) @ do
    dk = (_r16(ds).transpose(-2, -1) @ q) * SCALE
    dq = (_r16(ds) @ k) * SCALE
    g = torch.cat([x.transpose(1, 2).reshape(-1, N, C) for x in (dq, dk, dv)], dim=-1)
    xw.backward(g)
    res.update(dqkv=_r16(a.grad), dbias=ds.sum(0), dpad=torch.zeros_like(c) if c.grad is None else _r16(c.grad))
    return res


# ---------------------------------------------------------------------------------------------------
# 1. full grids
# ---------------------------------------------------------------------------------------------------
def _grid(B, H, W, nH, target=256):
    """Host rule of grid_blocks / with_xcd_mapping (winattn.hip): windows, window groups per head, trips of the window loop, windows
    of a ragged last trip (0: even split), XCD-pair mapping."""
    windows = B * -(-H // WS) * -(-W // WS)
    groups = max(1, min(-(-target // nH), windows))
    pairs = (nH % 8 == 0 and nH >= 16) or (nH == 8 and groups % 2 == 0) or (nH == 4 and groups % 4 == 0)
    return windows, groups, -(-windows // groups), windows % groups, pairs


#              B   H    W   nH shift  windows groups trips last  XCD pairs
FULL_GRIDS = [(2, 118, 120, 4, 6,     200,    64,    4,    8,    True),    # 4-head mapping at its full 64 groups, buffer 0 reused twice
              (3, 72, 60, 8, 6,       90,     32,    3,    26,   True),    # 8-head mapping at its full 32 groups
              (2, 48, 60, 16, 6,      40,     16,    3,    8,    True),
              (3, 36, 36, 32, 0,      27,     8,     4,    3,    True),
              (1, 36, 60, 8, 6,       15,     15,    1,    0,    False),   # odd group count: plain mapping with 8 heads
              (1, 30, 26, 4, 6,       9,      9,     1,    0,    False),   # groups % 4 != 0: plain mapping with 4 heads
              (2, 84, 80, 3, 6,       98,     86,    2,    12,   False),
              (3, 84, 84, 2, 0,       147,    128,   2,    19,   False),
              (2, 144, 140, 1, 6,     288,    256,   2,    32,   False)]


@gpu
@pytest.mark.parametrize("B,H,W,nH,shift,windows,groups,trips,last,pairs", FULL_GRIDS)
def test_full_grid_vs_oracle_through_the_c_entry_points(B, H, W, nH, shift, windows, groups, trips, last, pairs):
    """grit_winattn_fwd_bf16 / grit_winattn_bwd_bf16 on grids where every workgroup makes up to four trips through the window loop
    (the DMA double buffers wrap, the last trip is ragged) and on every (head, group) mapping at its full group count.  The images sit
    between two NaN images and every output arrives full of NaN: a window that is not written, written twice from different staging
    buffers, read from a neighbour image or written outside the B images shows."""
    if os.environ.get("GRIT_WINATTN_BLOCKS"):
        pytest.skip("GRIT_WINATTN_BLOCKS changes the grid these shapes were chosen for")
    assert _grid(B, H, W, nH) == (windows, groups, trips, last, pairs)  # a new grid policy must choose new shapes
    from grit_amd import lib as _lib
    lib, p = _lib.load(), _lib.ptr
    case = _case(B, H, W, nH, shift)
    C, T, wpi, nan = HD * nH, H * W, windows // B, float("nan")

    def framed(rows, width, dtype, fill=None):  # [B + 2 images] of NaN, the B real ones filled
        t_ = torch.full((B + 2, rows, width), nan, dtype=dtype, device=DEV)
        if fill is not None:
            t_[1:B + 1] = fill.to(DEV)
        return t_

    qkv, dout = framed(T, 3 * C, torch.bfloat16, case["qkv"]), framed(T, C, torch.bfloat16, case["cot"])
    bias, pad = case["bias"].to(DEV), case["pad"].to(DEV)

    def run():
        out, dqkv = framed(T, C, torch.bfloat16), framed(T, 3 * C, torch.bfloat16)
        lse = framed(wpi * nH, N, torch.float32)
        acc = torch.zeros(bias.numel() + 3 * C, dtype=torch.float32, device=DEV)
        dbias, dpad = acc[:bias.numel()].view_as(bias), acc[bias.numel():]
        st = lib.grit_winattn_fwd_bf16(p(qkv[1]), p(bias), p(pad), p(None), 0, B, H, W, C, nH, WS, shift, SCALE, p(out[1]), p(lse[1]),
                                       _lib.current_stream_ptr())
        assert st == 0
        st = lib.grit_winattn_bwd_bf16(p(qkv[1]), p(bias), p(pad), p(None), 0, p(out[1]), p(dout[1]), p(lse[1]), B, H, W, C, nH, WS,
                                       shift, SCALE, p(dqkv[1]), p(dbias), p(dpad), _lib.current_stream_ptr())
        assert st == 0
        torch.cuda.synchronize()
        for name, t_ in (("out", out), ("lse", lse), ("dqkv", dqkv)):
            assert bool(torch.isnan(t_[0]).all()) and bool(torch.isnan(t_[B + 1]).all()), name + ": canary image written"
            assert bool(torch.isfinite(t_[1:B + 1].float()).all()), name + ": a row was not written, or read from a NaN image"
        return {"out": out[1:B + 1].clone(), "dqkv": dqkv[1:B + 1].clone(), "dbias": dbias.clone(), "dpad": dpad.clone()}

    first = run()
    _check_forward(first["out"], case["out"])
    _check_grads(first, case)
    again = run()  # every token is written exactly once: a difference is a race in the staging
    assert torch.equal(again["out"], first["out"]) and torch.equal(again["dqkv"], first["dqkv"])


# ---------------------------------------------------------------------------------------------------
# 2. explicit mask, forward and backward
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mask_case(H, W, kind, nWm):
    B, nH, shift = 2, 4, 6
    qkv, bias, pad = _inputs(B, H, W, nH, seed=H * W + nWm)
    cot = _cotangent(B, H, W, nH, seed=3)
    if kind == "shift":
        mask = torch_ref.shift_mask(-(-H // WS) * WS, -(-W // WS) * WS, WS, shift, "cpu")
        assert mask.shape[0] == nWm
    else:  # 0 / -100 entries plus small float offsets
        g = torch.Generator().manual_seed(100 + nWm)
        mask = torch.where(torch.rand(nWm, N, N, generator=g) < 0.3, -100.0, 0.0) + 0.25 * torch.randn(nWm, N, N, generator=g)
    case = {"qkv": qkv, "bias": bias, "pad": pad, "cot": cot, "mask": mask, "geom": (H, W, nH, shift)}
    case.update(_oracle_with_grads(qkv, bias, pad, cot, H, W, nH, shift, mask=mask))
    return case


MASK_CASES = [(24, 36, "shift", 6), (26, 30, "shift", 9),
              (24, 36, "random", 6), (24, 36, "random", 3), (24, 36, "random", 1),   # 12 windows: one image, wrapping inside, broadcast
              (26, 30, "random", 9), (26, 30, "random", 3), (26, 30, "random", 1)]   # 18 windows


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,W,kind,nWm", MASK_CASES)
def test_explicit_mask_forward_and_backward_vs_oracle(H, W, kind, nWm, dtype):
    """window_attention(..., mask=) in both directions (the <true> instantiations of winattn_bwd_dma / winattn_bwd and the masked path
    of winattn_bwd_f32) against the oracle given the same mask; `win % nWm` with nWm below the windows of an image and 1.  The shift
    mask passed explicitly must also agree with the analytic-mask kernels on the same inputs."""
    case = _mask_case(H, W, kind, nWm)
    geom = case["geom"]
    got = _run_op(case["qkv"], case["bias"], case["pad"], case["cot"], *geom, mask=case["mask"], dtype=dtype)
    runs = [got]
    if kind == "shift":
        runs.append(_run_op(case["qkv"], case["bias"], case["pad"], case["cot"], *geom, mask=None, dtype=dtype))
    for r in runs:
        if dtype == torch.bfloat16:
            _check_forward(r["out"], case["out"])
            _check_grads(r, case)
        else:  # test_fp32_kernels_vs_oracle
            _check_forward(r["out"], case["out"], rtol=1e-4, atol=1e-5, mean=None)
            _check_grads(r, case, max_rel=1e-4, mean_rel=None)


# ---------------------------------------------------------------------------------------------------
# 3. hard softmax rows
# ---------------------------------------------------------------------------------------------------
HARD_SHAPES = [(2, 20, 20, 4, 6), (3, 13, 30, 2, 6), (1, 24, 36, 8, 0)]
# Backward bounds at large logits, relative to the largest entry of the oracle's gradient: the existing bound or four times the
# storage model's measured error against the float64 oracle, whichever is larger -- the existing one at both gains (measurements in
# the docstring of test_hard_softmax_rows_vs_oracle).
HARD_GRAD_MAX = {4: GRAD_MAX, 8: GRAD_MAX}
HARD_GRAD_MEAN = {4: GRAD_MEAN, 8: GRAD_MEAN}


@pytest.mark.parametrize("gain", [4, 8])
@pytest.mark.parametrize("B,H,W,nH,shift", HARD_SHAPES)
def test_storage_model_meets_the_forward_bounds_at_large_logits(B, H, W, nH, shift, gain):
    """CPU: the reference alone, with nothing but the kernels' bf16 storage added, stays inside the forward bounds where the softmax
    rows are nearly one-hot -- so a kernel that misses them there is wrong and not merely bf16."""
    case = _case(B, H, W, nH, shift, gain)
    peak = torch.softmax(_case_logits(case, H, W, nH, shift), -1).amax(-1).median().item()
    # (diffuse inputs: 0.06 - 0.08; the 13 x 30 map is lowest, its many window-padding keys are identical and share a row's weight)
    assert peak > (0.5 if gain == 4 else 0.9), peak
    model = _storage_model(case["qkv"], case["bias"], case["pad"], H, W, nH, shift)
    _check_forward(model["out"], case["out"])


def _case_logits(case, H, W, nH, shift, mask=None, dtype=torch.float32):
    C = HD * nH
    xw = _to_windows(case["qkv"].to(dtype), case["pad"].to(dtype), H, W, shift)
    q, k, _ = (_heads(s, nH) for s in xw.split(C, dim=-1))
    return _logits(q, k, case["bias"].to(dtype), H, W, nH, shift, mask)


@gpu
@pytest.mark.parametrize("gain", [4, 8])
@pytest.mark.parametrize("B,H,W,nH,shift", HARD_SHAPES)
def test_hard_softmax_rows_vs_oracle(B, H, W, nH, shift, gain):
    """q and k times 4 (median largest probability ~0.95) and times 8 (~1.0, logits of hundreds in log2 units): a wrong row maximum, a
    log-sum-exp in the wrong domain (the backward recomputes P = exp2(t - lse2)) or one wrong key decide the row here.  Forward at the
    file's bounds; the saved log-sum-exps against the oracle's; backward at the bounds of HARD_GRAD_MAX / HARD_GRAD_MEAN.

    Backward bound: _storage_model against the float64 oracle on these three shapes, relative to the largest entry of the float64
    gradient, worst shape (max | mean):
        gain 4:  dqkv 5.4e-3 | 1.4e-4   dbias 7.1e-3 | 3.7e-5   dpad 4.8e-3 | 3.1e-4
        gain 8:  dqkv 5.0e-3 | 5.6e-5   dbias 6.7e-3 | 1.8e-5   dpad 6.8e-3 | 1.3e-4
    (diffuse inputs, gain 1: 4.6e-3 | 1.5e-4, 1.3e-3 | 1.3e-5, 2.7e-3 | 2.2e-4; the model's forward: max 0.0156 / mean 7.9e-4 at gain 4,
    0.0108 / 3.1e-4 at gain 8).  Four times that (MFMA summation order, the bf16 bias slab of the DMA backward) is at most 2.8e-2 | 1.2e-3,
    below test_backward_vs_oracle's 4e-2 | 6e-3: the existing bounds are kept at both gains."""
    case = _case(B, H, W, nH, shift, gain)
    got = _run_op(case["qkv"], case["bias"], case["pad"], case["cot"], H, W, nH, shift)
    _check_forward(got["out"], case["out"])
    t = _case_logits(case, H, W, nH, shift, dtype=torch.float64)
    lse = torch.logsumexp(t, -1)
    lse_got = got["lse2"].double().cpu().view_as(lse) * math.log(2.0)
    assert bool(torch.isfinite(lse_got).all())
    # float32 logits of magnitude up to 2^9 in log2 units: a handful of roundings of 2^-15 each
    assert (lse_got - lse).abs().max().item() < 1e-3 + 1e-6 * t.abs().max().item()
    _check_grads(got, case, max_rel=HARD_GRAD_MAX[gain], mean_rel=HARD_GRAD_MEAN[gain])


@gpu
def test_row_whose_own_region_keys_are_all_very_negative():
    """Constructed: 24 x 24 map, shift 6, query 0 of every window carries a bias of -300 on keys (i < 6, j < 6).  In the last window
    (four mask regions of 6 x 6) these are exactly the keys of the query's own region, so every key of that row sits at -100 or below:
    the row maximum comes from masked keys and the log-sum-exp is near -95 (-137 in the kernel's log2 units).  It must come out finite
    and equal to the oracle's, and the row's gradients finite and within the usual bounds."""
    B, H, W, nH, shift = 1, 24, 24, 2, 6
    qkv, bias, pad = _inputs(B, H, W, nH, seed=21)
    own = torch.tensor([12 * i + j for i in range(6) for j in range(6)])
    bias[:, 0, own] = -300.0  # (exact in bf16: the DMA backward's bias slab keeps it)
    cot = _cotangent(B, H, W, nH, seed=4)
    case = {"qkv": qkv, "bias": bias, "pad": pad}
    ref = _oracle_with_grads(qkv, bias, pad, cot, H, W, nH, shift)
    t = _case_logits(case, H, W, nH, shift, dtype=torch.float64)
    lse = torch.logsumexp(t, -1)  # [4 windows, nH, N]
    assert lse[3, :, 0].max().item() < -90.0 and t[3, :, 0].max().item() < -90.0  # the case is what it claims to be
    got = _run_op(qkv, bias, pad, cot, H, W, nH, shift)
    lse_got = got["lse2"].double().cpu().view_as(lse) * math.log(2.0)
    assert bool(torch.isfinite(lse_got).all())
    assert (lse_got - lse).abs().max().item() < 1e-3 + 1e-6 * t.abs().max().item()  # as in test_hard_softmax_rows_vs_oracle
    _check_forward(got["out"], ref["out"])
    _check_grads(got, ref)


# ---------------------------------------------------------------------------------------------------
# 4. drop-path skip at the ends of its range
# ---------------------------------------------------------------------------------------------------
DROP_CASES = [(64, 12, 12, 1, 6, (0, 31, 32, 63)), (64, 13, 12, 2, 6, (5, 62, 63)), (64, 12, 12, 1, 0, tuple(range(63))),
              (65, 12, 12, 1, 6, (1, 64)), (2, 13, 30, 2, 6, (0,)), (2, 13, 30, 2, 6, (1,))]


@gpu
@pytest.mark.parametrize("B,H,W,nH,shift,drop", DROP_CASES, ids=["B64-1head", "B64-2heads", "B64-only-63-kept", "B65-falls-back",
                                                                 "B2-drop-0", "B2-drop-1"])
def test_drop_path_skip_at_the_ends_of_its_range(B, H, W, nH, shift, drop):
    """The scheme of test_backward_skips_the_windows_of_dropped_images at B = 64 (the 64-bit keep mask is full: image 63 dropped, image
    63 the only one kept), B = 65 (the host falls back to the plain kernels: out and dqkv bit for bit those of a call without factors,
    nothing planted) and B = 2 (the smallest batch the skipping kernels take), each image dropped in turn."""
    from grit_amd.ops.window_attention import _WindowAttentionFn
    qkv, bias, pad = _inputs(B, H, W, nH, seed=B + H)
    cot = _cotangent(B, H, W, nH, seed=2)
    scale = torch.full((B,), 1.0 / 0.8)
    for b in drop:
        scale[b] = 0.0
        cot[b] = 0
    args = (None, H, W, nH, WS, shift, SCALE)
    skipping = 2 <= B <= 64 and not _CHILD and os.environ.get("GRIT_WINATTN_ROW_SKIP") != "0"  # (else: every window is computed)

    def run(row_scale, poison):
        x, y, z = qkv.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True), pad.to(DEV).requires_grad_(True)
        out = _WindowAttentionFn.apply(x, y, z, *args, row_scale)
        result = out.detach().clone()
        if poison:  # what the backward would read for the dropped images: saved q / k / v, O and the log-sum-exps
            with torch.no_grad():
                saved = out.grad_fn.saved_tensors
                for b in drop:  # (.data: no version bump -- autograd must not notice)
                    saved[0].data[b] = float("nan")
                    saved[4].data[b] = float("nan")
                    nw = saved[5].shape[0] // B
                    saved[5].data[b * nw:(b + 1) * nw] = float("nan")
        out.backward(cot.to(DEV))
        return x.grad, y.grad, z.grad, result

    plain = run(None, False)
    skipped = run(scale.to(DEV), skipping)
    assert all(bool(torch.isfinite(t_.float()).all()) for t_ in skipped)
    assert torch.equal(skipped[0], plain[0])
    for b in drop:
        assert not bool(skipped[0][b].any())
    kept = [b for b in range(B) if b not in drop]
    assert torch.equal(skipped[3][kept], plain[3][kept])
    if skipping:
        for b in drop:
            assert not bool(skipped[3][b].any())
    else:
        assert torch.equal(skipped[3], plain[3])
    for got, ref in zip(skipped[1:3], plain[1:3]):  # d(bias), d(pad): the order of the float atomics is free
        assert float((got.float() - ref.float()).abs().max()) <= 1e-4 * float(ref.float().abs().max()) + 1e-5


# ---------------------------------------------------------------------------------------------------
# 5. small maps on the MFMA backward
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,H,W,nH,shift", [(1, 12, 12, 1, 0), (1, 7, 5, 3, 6), (2, 12, 12, 3, 0), (1, 5, 50, 2, 6)])
def test_backward_vs_oracle_on_small_maps(B, H, W, nH, shift):
    """One window, a map smaller than a window, 1 and 3 heads, a single row of windows: test_backward_vs_oracle's bounds."""
    case = _case(B, H, W, nH, shift)
    got = _run_op(case["qkv"], case["bias"], case["pad"], case["cot"], H, W, nH, shift)
    _check_forward(got["out"], case["out"])
    _check_grads(got, case)


# ---------------------------------------------------------------------------------------------------
# 6. both kernel variants
# ---------------------------------------------------------------------------------------------------
@gpu
def test_register_staged_variants_pass_this_file():
    """The defaults are the DMA-staged kernels; GRIT_WINATTN_FWD_DMA=0 GRIT_WINATTN_BWD_DMA=0 select the register-staged ones.  The
    library reads the knobs once per process: this file again in a fresh child process (which never recurses into this test)."""
    if _CHILD:
        pytest.skip("already a child run")
    env = dict(os.environ, GRIT_WINATTN_FWD_DMA="0", GRIT_WINATTN_BWD_DMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " passed" in r.stdout
