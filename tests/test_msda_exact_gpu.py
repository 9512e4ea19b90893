"""Every kernel variant of grit_amd/csrc/msda.hip, compared with `==` against the float64 oracle.  Needs an MI355X.

Which case reaches which kernel (conditions as written in launch_fwd, launch_bwd, grit_msda_fwd_bf16_strided and
grit_msda_bwd_bf16_sorted; LP = L*P, configurations by their name in tests/msda_lattice.py::CONFIGS):

  kernel                     entry point                     selected when                               test case
  -------------------------  ------------------------------  ------------------------------------------  -----------------------------------------
  msda_fwd_vec4<16, 1>       op, f32 (grit_msda_fwd_f32)      aligned, D = 64, (LP + 3) / 4 = 1           test_f32_op_exact[d64_lp4]
  msda_fwd_vec4<16, 2>       "                                ... = 2 (LP = 6: half a round dead)         test_f32_op_exact[d64_lp6], [d64_lp8]
  msda_fwd_vec4<16, 3>       "                                ... = 3                                     test_f32_op_exact[d64_lp12]
  msda_fwd_vec4<16, 4>       "                                ... = 4                                     test_f32_op_exact[d64_lp16], [.._1row], [.._100]
  msda_fwd_vec4<16, 6>       "                                ... = 6                                     test_f32_op_exact[d64_lp24], [d64_lp21] (one point in the last round)
  msda_fwd_vec4<16, 8>       "                                ... = 8                                     test_f32_op_exact[d64_lp32], [d64_lp29] (one point in the last round)
  msda_fwd_vec4<16, 4 | 8>   "                                NaN under dead corners                      test_dead_corners_do_not_leak[vec4-16], [vec4-32]
  msda_fwd_generic<float>    "                                D = 64, (LP + 3) / 4 in {5, 7}: no case     test_f32_op_exact[d64_lp17], [d64_lp20], [d64_lp28]
  msda_fwd_generic<float>    "                                value not 16-byte aligned                   test_f32_forward_unaligned_value[d64_lp16], [d32_lp8]
  msda_fwd_vec4<8, 1..4>     "                                aligned, D = 32, (LP + 7) / 8 = 1..4        test_f32_op_exact[d32_lp5], [d32_lp8], [d32_lp16], [d32_lp24], [d32_lp32]
    one point in last round  "                                LP = 9, 17, 25                              test_f32_op_exact[d32_lp9], [d32_lp17], [d32_lp25]
  msda_fwd_generic<float>    "                                D not in {32, 64}                           test_f32_op_exact[d1_lp6], [d7_lp6], [d130_lp5]
  msda_fwd_generic<double>   op, f64 (grit_msda_fwd_f64)      always                                      test_f64_op_exact[d64_lp16], [d7_lp6]
  msda_fwd_bf16_rows4<2>     op, bf16 (.._fwd_bf16_strided)   LP <= 16, map below 4 GB, no environment    test_bf16_forward_op[d64_lp4 | lp6 | lp8 | lp9 | lp12 | lp16 | lp16_1row | lp16_100]
  msda_fwd_bf16_rows4<2>     grit_msda_fwd_bf16_strided       same, pixel_stride = 3 M D                  test_bf16_forward_strided_slice
  msda_fwd_bf16_rows4<1|4|8> op, bf16, child process          GRIT_MSDA_FWD_BATCH = 1, 4, 8               test_bf16_forward_batch_variants[1], [4], [8]
  msda_fwd_bf16_d64<1>, <2>  op, bf16, child process          GRIT_MSDA_FWD_BATCH = 0, (LP + 7) / 8       test_bf16_forward_batch_variants[0] (LP = 6; 9 and 16)
  msda_fwd_bf16_d64<3>       grit_msda_fwd_bf16               16 < LP <= 32, (LP + 7) / 8 = 3             test_bf16_forward_row_per_wave[d64_lp17], [d64_lp20]
  msda_fwd_bf16_d64<4>       "                                ... = 4                                     test_bf16_forward_row_per_wave[d64_lp32], [d64_lp25], [d64_lp29]
  msda_fwd_bf16_d64<3 | 4>   "                                NaN under dead corners                      test_dead_corners_do_not_leak[bf16-17], [bf16-20], [bf16-32]
  msda_bwd_d64<float>        op, f32 (grit_msda_bwd_f32)      D = 64, LP <= 16                            test_f32_op_exact[d64_lp4 | lp6 | lp8 | lp12 | lp16...]
  msda_bwd_generic<float, 4> "                                otherwise, LP % 4 == 0                      test_f32_op_exact[d64_lp32], [d64_lp24], [d32_lp8], [d32_lp16]
  msda_bwd_generic<float, 1> "                                otherwise, LP % 4 != 0                      test_f32_op_exact[d7_lp6], [d130_lp5], [d1_lp6], [d64_lp17]
  msda_bwd_generic<double,.> op, f64 (grit_msda_bwd_f64)      always (4: LP = 16, 1: LP = 6)              test_f64_op_exact[d64_lp16], [d7_lp6]
  msda_bwd_d64<bf16>         grit_msda_bwd_bf16               D = 64, LP <= 16                            test_bf16_backward_forms[dense-*]
  ..d64_pk<kStaged> + flush  grit_msda_bwd_bf16_staged        D = 64, LP <= 16                            test_bf16_backward_forms[staged-*]
    merged / pair branch     "                                P = 4, LP = 16, points share a cell         test_bf16_backward_forms[staged-d64_cluster]
    neither branch           "                                P = 2                                       test_bf16_backward_forms[staged-d64_lp8_p2]
    image-interleaved order  "                                B > 1, (Lq M) % 4 == 0                      [..-d64_lp8], [..-d64_cluster], [..-d64_lp16_100]; not: [..-d64_lp16]
  msda_bwd_d64_pk<kPacked>   grit_msda_bwd_bf16acc            D = 64, LP <= 16 (coarse lattice)           test_bf16_backward_forms[packed-pk_*]
    merged / pair branch     "                                P = 4, LP = 16, points share a cell         test_bf16_backward_forms[packed-pk_cluster]
    neither branch           "                                P = 2                                       test_bf16_backward_forms[packed-pk_lp8_p2]
  msda_bwd_value + rows4<2>  grit_msda_bwd_bf16_sorted        value 16-byte aligned, map below 4 GB       test_bf16_backward_forms[sorted-*]
  msda_bwd_d64_pk<kNone>     "                                value 4 bytes off 16-byte alignment         test_sorted_unaligned_value_takes_the_row_walk
  msda_bwd_value, parts = n  "                                parts = clamp(256 / (B M), 1, 8)            test_sorted_value_partitions[val_parts1 | 2 | 3 | 4 | 5 | 8]
    16 waves all own tiles   "                                S = 4160, parts = 1                         test_sorted_value_partitions[val_big]
    one tile, 128 waves      "                                S = 3, parts = 8                            test_sorted_value_partitions[val_s3]
    run of > 64 records      "                                every query samples the 1x1 level           test_sorted_value_partitions[val_hot]
    hi + mid + lo weights    "  (and staged, dense)           weights a + delta, off the lattice          test_value_weight_split_is_exact

xcd_logical_block and the image-interleaved order are bijections or rows go missing / are written twice: the row counts
1, 5, 15, 16, 17, 63, 65, 100 give workgroup counts below 8 and with nblk % 8 in {0, 1, 7} for 4-row and for 16-row
workgroups; outputs handed to the C ABI arrive full of NaN.

Expectations (none is a measured tolerance; tests/test_msda_lattice_cpu.py proves the oracle is bit-identical in f32 and f64 on
every configuration): f32 / f64 kernels equal the float64 oracle cast to their dtype; bf16 maps with f32 accumulation equal the
oracle rounded ONCE to bf16 (out, grad_value) and the oracle itself (grad_loc, grad_attn_w, f32); packed-bf16 atomics equal the
oracle on the coarse lattice, where every partial sum fits 8 bits.  Values are compared, so -0.0 == 0.0.  Only the two
dead-corner tests use random maps and a tolerance.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import msda as omsda
from tests import msda_lattice as ml

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib():
    from grit_amd import lib
    return lib.load(), lib.current_stream_ptr()


def _same(got, want, what):
    """got (device tensor) == want (float64 numpy or tensor, cast to got's dtype) element by element, by value."""
    got = got.detach().cpu()
    want = (want if torch.is_tensor(want) else torch.tensor(np.asarray(want))).to(got.dtype).reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, len(bad), got.numel(), i, float(got[i]), float(want[i])))


def _geometry(c):
    return _t(c.shapes, torch.int64), _t(c.lsi, torch.int64), _t(c.loc, torch.float32), _t(c.aw, torch.float32)


def _run_op(c, dtype):
    from grit_amd.ops.msda import MSDeformAttnFunction
    v, l, a = (_t(x, dtype).requires_grad_(True) for x in (c.value, c.loc, c.aw))
    out = MSDeformAttnFunction.apply(v, _t(c.shapes, torch.int64), _t(c.lsi, torch.int64), l, a, 64)
    out.backward(_t(c.cot, dtype))
    return out.detach(), v.grad, l.grad, a.grad


def _check_op(c, dtype):
    out, gv, gl, ga = _run_op(c, dtype)
    assert out.dtype == dtype and gv.dtype == dtype
    rgv, rgl, rga = c.ref_backward()
    _same(out, c.ref_forward(), "out")
    _same(gv, rgv, "grad_value")
    _same(gl, rgl, "grad_loc")
    _same(ga, rga, "grad_attn_w")


F32_CASES = [n for n in sorted(ml.CONFIGS) if n.startswith(("d64_", "d32_", "d1_", "d7_", "d130_"))]


@pytest.mark.parametrize("name", F32_CASES)
def test_f32_op_exact(name):
    _check_op(ml.case(name), torch.float32)


@pytest.mark.parametrize("name", ["d64_lp16", "d7_lp6"])
def test_f64_op_exact(name):
    _check_op(ml.case(name), torch.float64)


@pytest.mark.parametrize("name", ["d64_lp16", "d32_lp8"])
def test_f32_forward_unaligned_value(name):
    """A value map one float past a 16-byte boundary cannot take the float4 loads of msda_fwd_vec4: generic kernel, same numbers."""
    from grit_amd.ops.msda import ms_deform_attn_forward
    c = ml.case(name)
    buf = torch.full((c.value.size + 4,), float("nan"), dtype=torch.float32, device=DEV)
    value = buf[1:1 + c.value.size].view(c.value.shape)
    value.copy_(_t(c.value, torch.float32))
    assert value.is_contiguous() and value.data_ptr() % 16 == 4
    sh, lsi, loc, aw = _geometry(c)
    _same(ms_deform_attn_forward(value, sh, lsi, loc, aw, 64), c.ref_forward(), "out")


def _dead_corner_inputs(levels, B, Lq, M, P, seed):
    """Random map whose pixel (0, 0) of every level is NaN; points are well inside (never reach row / column 0) or entirely
    outside (dead: clamped address = pixel (0, 0)) -- as in test_msda_gpu.py::test_bf16_forward_kernels_layouts_and_dead_corners."""
    gen = torch.Generator().manual_seed(seed)
    shapes = torch.tensor(levels)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S, L = int(shapes.prod(1).sum()), len(levels)
    value = torch.randn(B, S, M, 64, generator=gen).bfloat16().float()
    value[:, lsi] = float("nan")
    hw = shapes.flip(1).float().view(1, 1, 1, L, 1, 2)
    inside = (1.6 + torch.rand(B, Lq, M, L, P, 2, generator=gen) * (hw - 2.7) + 0.5) / hw
    outside = -(1.5 + torch.rand(B, Lq, M, L, P, 2, generator=gen)) / hw
    dead = torch.rand(B, Lq, M, L, P, 1, generator=gen) < 0.25
    loc = torch.where(dead, outside, inside).contiguous()
    aw = torch.rand(B, Lq, M, L, P, generator=gen)
    ref = omsda.msda_forward(torch.nan_to_num(value).numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), aw.numpy())
    return value, shapes, lsi, loc, aw, ref


PYR = [(40, 40), (20, 20), (10, 10), (5, 5)]


@pytest.mark.parametrize("kind,levels,P", [("vec4", PYR, 4), ("vec4", PYR, 8), ("bf16", PYR[:1], 17), ("bf16", PYR, 5), ("bf16", PYR, 8)],
                         ids=["vec4-16", "vec4-32", "bf16-17", "bf16-20", "bf16-32"])
def test_dead_corners_do_not_leak(kind, levels, P):
    """msda_fwd_vec4 and msda_fwd_bf16_d64<3 | 4> load dead corners through a clamped address and claim 'select, not multiply':
    a NaN there must not reach the sum.  Random maps: the only comparisons with a tolerance in this file."""
    B, Lq, M = 2, 9, 3
    value, shapes, lsi, loc, aw, ref = _dead_corner_inputs(levels, B, Lq, M, P, seed=len(levels) * 100 + P)
    L, S = len(levels), value.shape[1]
    if kind == "vec4":
        from grit_amd.ops.msda import ms_deform_attn_forward
        out = ms_deform_attn_forward(value.to(DEV), shapes.to(DEV), lsi.to(DEV), loc.to(DEV), aw.to(DEV), 64)
        assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-4, atol=1e-5)
    else:
        lib, stream = _lib()
        v, sh, ls, lo, a = value.to(BF16).to(DEV), shapes.to(DEV), lsi.to(DEV), loc.to(DEV), aw.to(DEV)
        out = torch.full((B, Lq, M * 64), float("nan"), dtype=BF16, device=DEV)
        assert lib.grit_msda_fwd_bf16(_p(v), _p(sh), _p(ls), _p(lo), _p(a), B, S, M, 64, L, Lq, P, _p(out), stream) == 0
        assert bool(torch.isfinite(out.float()).all())
        np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=1e-2, atol=1e-2)  # bf16 output rounding


BF_ROWS4 = ["d64_lp4", "d64_lp6", "d64_lp8", "d64_lp9", "d64_lp12", "d64_lp16", "d64_lp16_1row", "d64_lp16_100"]


@pytest.mark.parametrize("name", BF_ROWS4)
def test_bf16_forward_op(name):
    from grit_amd.ops.msda import ms_deform_attn_forward
    c = ml.case(name)
    sh, lsi, loc, aw = _geometry(c)
    out = ms_deform_attn_forward(_t(c.value, BF16), sh, lsi, loc, aw, 64)
    assert out.dtype == BF16
    _same(out, ml.to_bf16(c.ref_forward()), "out")


@pytest.mark.parametrize("name", ["d64_lp17", "d64_lp20", "d64_lp25", "d64_lp29", "d64_lp32"])
def test_bf16_forward_row_per_wave(name):
    """msda_fwd_bf16_d64<3> and <4>: only the C ABI reaches them (the op keeps L*P > 16 on the f32 path)."""
    c = ml.case(name)
    B, S, M, D, L, Lq, P = c.dims
    lib, stream = _lib()
    sh, lsi, loc, aw = _geometry(c)
    value = _t(c.value, BF16)
    out = torch.full((B, Lq, M * D), float("nan"), dtype=BF16, device=DEV)
    assert lib.grit_msda_fwd_bf16(_p(value), _p(sh), _p(lsi), _p(loc), _p(aw), B, S, M, D, L, Lq, P, _p(out), stream) == 0
    _same(out, ml.to_bf16(c.ref_forward()), "out")


def _stacked(t, n, layer, fill=float("nan")):
    """t [B, S, M, D] as slice `layer` of a [B, S, n, M, D] tensor whose other slices hold `fill`; -> (stacked, pointer of the slice)."""
    B, S, M, D = t.shape
    st = torch.full((B, S, n, M, D), fill, dtype=t.dtype, device=DEV)
    st[:, :, layer] = t
    return st, ctypes.c_void_p(st.data_ptr() + layer * M * D * st.element_size())


def test_bf16_forward_strided_slice():
    """The map as slice 1 of 3 of a [B, S, 3, M, 64] tensor; the other slices are NaN, so a read from them shows."""
    c = ml.case("d64_lp16_100")
    B, S, M, D, L, Lq, P = c.dims
    lib, stream = _lib()
    sh, lsi, loc, aw = _geometry(c)
    st, vptr = _stacked(_t(c.value, BF16), 3, 1)
    out = torch.full((B, Lq, M * D), float("nan"), dtype=BF16, device=DEV)
    assert lib.grit_msda_fwd_bf16_strided(vptr, 3 * M * D, _p(sh), _p(lsi), _p(loc), _p(aw), B, S, M, D, L, Lq, P, _p(out), stream) == 0
    _same(out, ml.to_bf16(c.ref_forward()), "out")


_CHILD = """
import sys
sys.path.insert(0, %(root)r)
import torch
from tests import msda_lattice as ml
from grit_amd.ops.msda import ms_deform_attn_forward
ok = True
for name in ("d64_lp6", "d64_lp9", "d64_lp16_100"):
    c = ml.case(name)
    d = lambda a, dt: torch.from_numpy(a).to(dt).cuda()
    out = ms_deform_attn_forward(d(c.value, torch.bfloat16), d(c.shapes, torch.int64), d(c.lsi, torch.int64), d(c.loc, torch.float32),
                                 d(c.aw, torch.float32), 64)
    same = torch.equal(out.cpu(), ml.to_bf16(c.ref_forward()))
    print(name, "equal" if same else "DIFFERENT")
    ok = ok and same
sys.exit(0 if ok else 1)
"""
_child_failed = []


@pytest.mark.parametrize("batch", [0, 1, 4, 8])
def test_bf16_forward_batch_variants(batch):
    """GRIT_MSDA_FWD_BATCH is read once per process: 0 -> msda_fwd_bf16_d64<1 | 2>, 1 / 4 / 8 -> msda_fwd_bf16_rows4<1 | 4 | 8>.
    Each value gets a fresh child process, which runs the lattice forward at L*P = 6, 9 and 16 and exits 0 only on equality."""
    assert not _child_failed, "an earlier child failed (batch %s): nothing more is started" % _child_failed
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=dict(os.environ, GRIT_MSDA_FWD_BATCH=str(batch)),
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        _child_failed.append(batch)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.split() == ["d64_lp6", "equal", "d64_lp9", "equal", "d64_lp16_100", "equal"]


# ---- backward, bf16 maps: the four accumulation forms --------------------------------------------------------------------

def _bwd_bf16(form, c, value=None, pixel_stride=None, gv=None):
    """One C-ABI backward on bf16 maps.  value / gv: pointers into strided maps (sorted, staged), else dense tensors are made here.
    -> (grad_value tensor or None when gv was given, grad_loc, grad_attn_w); outputs arrive as NaN where the kernel must write
    every element and as zeros where it accumulates."""
    B, S, M, D, L, Lq, P = c.dims
    lib, stream = _lib()
    sh, lsi, loc, aw = _geometry(c)
    cot = _t(c.cot, BF16)
    keep = None
    if value is None:
        keep = _t(c.value, BF16)
        value, pixel_stride = _p(keep), M * D
    gl, ga = torch.full_like(loc, float("nan")), torch.full_like(aw, float("nan"))
    dims = (B, S, M, D, L, Lq, P)
    out = None
    if form == "dense":
        out = torch.zeros((B, S, M, D), dtype=torch.float32, device=DEV)
        st = lib.grit_msda_bwd_bf16(value, _p(sh), _p(lsi), _p(loc), _p(aw), _p(cot), *dims, _p(out), _p(gl), _p(ga), stream)
    elif form == "packed":
        out = torch.zeros((B, S, M, D), dtype=BF16, device=DEV)
        st = lib.grit_msda_bwd_bf16acc(value, _p(sh), _p(lsi), _p(loc), _p(aw), _p(cot), *dims, _p(out), _p(gl), _p(ga), stream)
    elif form == "staged":
        if gv is None:
            out = torch.zeros((B, S, M, D), dtype=BF16, device=DEV)
            gv = _p(out)
        stage = torch.zeros((B, S, M, 64), dtype=torch.float32, device=DEV)
        flags = torch.zeros((B, S, M), dtype=torch.uint8, device=DEV)
        st = lib.grit_msda_bwd_bf16_staged(value, pixel_stride, _p(sh), _p(lsi), _p(loc), _p(aw), _p(cot), *dims, _p(stage), _p(flags),
                                           gv, _p(gl), _p(ga), stream)
        assert int(stage.count_nonzero()) == 0 and int(flags.count_nonzero()) == 0  # scratch leaves the call zeroed
    else:
        assert form == "sorted" and lib.grit_msda_bwd_sorted_supported(B, S, M, L, Lq, P) == 0
        if gv is None:
            out = torch.full((B, S, M, D), float("nan"), dtype=BF16, device=DEV)
            gv = _p(out)
        st = lib.grit_msda_bwd_bf16_sorted(value, pixel_stride, _p(sh), _p(lsi), _p(loc), _p(aw), _p(cot), *dims, gv, _p(gl), _p(ga), stream)
    assert st == 0
    torch.cuda.synchronize()
    del keep
    return out, gl, ga


BF_BWD = ["d64_lp4", "d64_lp6", "d64_lp8", "d64_lp9", "d64_lp12", "d64_lp16", "d64_lp16_1row", "d64_lp16_100", "d64_lp8_p2", "d64_cluster"]
PK_BWD = ["pk_lp16", "pk_lp16_odd", "pk_cluster", "pk_lp8_p2", "pk_lp12"]


@pytest.mark.parametrize("form,name", [(f, n) for f in ("dense", "staged", "sorted") for n in BF_BWD + PK_BWD] +
                         [("packed", n) for n in PK_BWD])
def test_bf16_backward_forms(form, name):
    c = ml.case(name)
    gv, gl, ga = _bwd_bf16(form, c)
    rgv, rgl, rga = c.ref_backward()
    if form == "dense":  # f32 map: the oracle itself, before any rounding
        assert gv.dtype == torch.float32
        _same(gv, rgv, "grad_value")
    else:
        assert gv.dtype == BF16
        _same(gv, ml.to_bf16(rgv), "grad_value")
    _same(gl, rgl, "grad_loc")
    _same(ga, rga, "grad_attn_w")


@pytest.mark.parametrize("name", ["d64_lp16", "d64_lp8", "d64_lp12"])
def test_sorted_unaligned_value_takes_the_row_walk(name):
    """value 4 bytes past a 16-byte boundary (element 2 of an oversized buffer, same pixel stride): grit_msda_bwd_bf16_sorted
    cannot use the 16-byte gathers of msda_bwd_rows4 and takes msda_bwd_d64_pk<2> for grad_loc / grad_attn_w.  Same numbers as
    the aligned call and the oracle."""
    c = ml.case(name)
    B, S, M, D, L, Lq, P = c.dims
    buf = torch.full((c.value.size + 16,), float("nan"), dtype=BF16, device=DEV)
    buf[2:2 + c.value.size] = _t(c.value, BF16).reshape(-1)
    vptr = ctypes.c_void_p(buf.data_ptr() + 4)
    assert vptr.value % 16 == 4
    gv, gl, ga = _bwd_bf16("sorted", c, value=vptr, pixel_stride=M * D)
    gv2, gl2, ga2 = _bwd_bf16("sorted", c)
    rgv, rgl, rga = c.ref_backward()
    for got, want, what in ((gv, gv2, "grad_value"), (gl, gl2, "grad_loc"), (ga, ga2, "grad_attn_w")):
        _same(got, want.cpu(), what + " vs aligned call")
    _same(gv, ml.to_bf16(rgv), "grad_value")
    _same(gl, rgl, "grad_loc")
    _same(ga, rga, "grad_attn_w")


VALUE_CASES = [n for n in sorted(ml.CONFIGS) if n.startswith("val_")]


@pytest.mark.parametrize("name", VALUE_CASES)
def test_sorted_value_partitions(name):
    """msda_bwd_value over its workgroup partition (parts 1, 2, 3, 4, 5, 8), with all 16 waves owning tiles (S = 4160), with one
    tile for 128 waves (S = 3) and with a run of more than 64 records.  The gradient map is one slice of a strided buffer that
    arrives full of NaN: the other slices stay NaN, the written slice equals the oracle rounded to bf16, zeros included."""
    c = ml.case(name)
    B, S, M, D, L, Lq, P = c.dims
    parts = min(max(256 // (B * M), 1), 8)
    assert parts == {"val_parts1": 1, "val_parts2": 2, "val_parts3": 3, "val_parts4": 4, "val_parts5": 5, "val_parts8": 8,
                     "val_big": 1, "val_s3": 8, "val_hot": 8}[name]
    n = 2 if name == "val_big" else 3
    stv, vptr = _stacked(_t(c.value, BF16), n, 1)
    grad = torch.full((B, S, n, M, D), float("nan"), dtype=BF16, device=DEV)
    gptr = ctypes.c_void_p(grad.data_ptr() + 1 * M * D * 2)
    _, gl, ga = _bwd_bf16("sorted", c, value=vptr, pixel_stride=n * M * D, gv=gptr)
    for other in set(range(n)) - {1}:
        assert bool(torch.isnan(grad[:, :, other]).all()), "slice %d was written" % other
    rgv, rgl, rga = c.ref_backward()
    _same(grad[:, :, 1], ml.to_bf16(rgv), "grad_value")
    _same(gl, rgl, "grad_loc")
    _same(ga, rga, "grad_attn_w")


def test_value_weight_split_is_exact():
    """msda_bwd_value feeds each f32 weight to the matrix cores as three bf16 terms hi + mid + lo.  Pairs of queries on one pixel
    centre with weights a + delta, a and cotangents +g, -g leave exactly delta * g in the cell: 2^-9 .. 2^-23 relative to the
    terms, far below the final bf16 rounding, so a wrong mid or lo term shows as a wrong (or zero) cell.  The staged path and the
    dense f32 kernel rounded to bf16 give the same map."""
    c, want = ml.build_weight_split()
    want16 = ml.to_bf16(want)
    gv, _, _ = _bwd_bf16("sorted", c)
    _same(gv, want16, "sorted grad_value")
    gv, _, _ = _bwd_bf16("staged", c)
    _same(gv, want16, "staged grad_value")
    gv, _, _ = _bwd_bf16("dense", c)
    _same(gv, want, "dense grad_value (f32)")
    _same(gv.to(BF16), want16, "dense grad_value rounded")
