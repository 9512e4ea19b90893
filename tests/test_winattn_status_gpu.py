"""Status codes of the six window-attention entry points (grit_amd/csrc/winattn.hip) for arguments they reject.  Needs an MI355X,
but only for its buffers: every rejected call returns before any launch; the last test makes the valid calls.

All six check in the same order: a null pointer (GRIT_ERR_BAD_ARG), a non-positive dimension (BAD_ARG), window != 12, C != 32 *
num_heads or a shift outside 0 .. 11 (GRIT_ERR_UNSUPPORTED), a mask without mask windows (BAD_ARG); the fp32 pair then refuses more
than 2^31 - 1 (window, head) units (BAD_ARG).  mask and row_scale may be NULL.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
# the smallest geometry: one window, every tile row of it with padding
GEOM = dict(B=1, H=5, W=5, C=32, num_heads=1, window=12, shift=0, scale=32 ** -0.5, nmw=0)
GEOM_ORDER = ("B", "H", "W", "C", "num_heads", "window", "shift", "scale")

_FWD = ("qkv", "rel_bias", "pad", "mask", "nmw", "geom", "out", "lse")
_BWD = ("qkv", "rel_bias", "pad", "mask", "nmw", "out", "dout", "lse", "geom", "dqkv", "dbias", "dpad")
# entry point -> (argument order, pointers that must not be NULL, storage); "geom" stands for the eight values in GEOM_ORDER
ENTRIES = {
    "grit_winattn_fwd_bf16": (_FWD + ("stream",), ("qkv", "rel_bias", "pad", "out", "lse"), "bf16"),
    "grit_winattn_fwd_bf16_rows": (_FWD + ("row_scale", "stream"), ("qkv", "rel_bias", "pad", "out", "lse"), "bf16"),
    "grit_winattn_bwd_bf16": (_BWD + ("stream",), ("qkv", "rel_bias", "pad", "out", "dout", "lse", "dqkv", "dbias", "dpad"), "bf16"),
    "grit_winattn_bwd_bf16_rows": (_BWD + ("row_scale", "stream"),
                                   ("qkv", "rel_bias", "pad", "out", "dout", "lse", "dqkv", "dbias", "dpad"), "bf16"),
    "grit_winattn_fwd_f32": (_FWD + ("stream",), ("qkv", "rel_bias", "pad", "out", "lse"), "f32"),
    "grit_winattn_bwd_f32": (_BWD + ("stream",), ("qkv", "rel_bias", "pad", "out", "dout", "lse", "dqkv", "dbias", "dpad"), "f32"),
}
OUTPUTS = {"fwd": ("out", "lse"), "bwd": ("dqkv", "dbias", "dpad")}
SENTINEL = 7.0


def _buffers(dtype):
    T, C = GEOM["H"] * GEOM["W"], GEOM["C"]
    g = torch.Generator().manual_seed(5)
    f32 = torch.float32
    return {
        "qkv": torch.randn(1, T, 3 * C, generator=g).to(dtype).to(DEV),
        "rel_bias": (torch.randn(1, 144, 144, generator=g) * 0.5).bfloat16().float().to(DEV),
        "pad": (torch.randn(3 * C, generator=g) * 0.3).to(dtype).to(DEV),
        "mask": torch.zeros(1, 144, 144, dtype=f32, device=DEV),
        "row_scale": torch.ones(1, dtype=f32, device=DEV),
        "out": torch.full((1, T, C), SENTINEL, dtype=dtype, device=DEV),
        "dout": torch.randn(1, T, C, generator=g).to(dtype).to(DEV),
        "lse": torch.full((1, 1, 144), SENTINEL, dtype=f32, device=DEV),
        "dqkv": torch.full((1, T, 3 * C), SENTINEL, dtype=dtype, device=DEV),
        "dbias": torch.full((1, 144, 144), SENTINEL, dtype=f32, device=DEV),
        "dpad": torch.full((3 * C,), SENTINEL, dtype=f32, device=DEV),
    }


@pytest.fixture(scope="module")
def env():
    from grit_amd import lib
    return lib.load(), lib.current_stream_ptr(), {"bf16": _buffers(torch.bfloat16), "f32": _buffers(torch.float32)}


def _call(env, name, geom=None, null=(), mask=False, buf=None):
    """The entry point on the valid arguments with the values of `geom` overridden and the pointers in `null` passed as NULL; mask
    and row_scale are NULL unless `mask` / the entry point takes row_scale."""
    lib, stream, bufs = env
    order, _, storage = ENTRIES[name]
    buf = buf or bufs[storage]
    g = dict(GEOM, **(geom or {}))
    args = []
    for a in order:
        if a == "geom":
            args += [g[k] for k in GEOM_ORDER]
        elif a == "nmw":
            args.append(g["nmw"])
        elif a == "stream":
            args.append(stream)
        elif a == "mask":
            args.append(ctypes.c_void_p(buf["mask"].data_ptr() if mask else 0))
        else:
            args.append(ctypes.c_void_p(0 if a in null else buf[a].data_ptr()))
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_pointer_is_bad_arg(env, name):
    for p in ENTRIES[name][1]:
        assert _call(env, name, null=(p,)) == BAD_ARG, p


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_non_positive_dimension_is_bad_arg(env, name):
    for k in ("B", "H", "W", "C", "num_heads"):
        for v in (0, -1):
            assert _call(env, name, geom={k: v}) == BAD_ARG, (k, v)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_geometry_without_kernel_is_unsupported(env, name):
    assert _call(env, name, geom={"window": 7}) == UNSUPPORTED
    assert _call(env, name, geom={"C": 64}) == UNSUPPORTED  # C != 32 * num_heads
    assert _call(env, name, geom={"num_heads": 2}) == UNSUPPORTED
    assert _call(env, name, geom={"shift": -1}) == UNSUPPORTED
    assert _call(env, name, geom={"shift": 12}) == UNSUPPORTED


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_mask_without_windows_is_bad_arg(env, name):
    assert _call(env, name, mask=True, geom={"nmw": 0}) == BAD_ARG
    assert _call(env, name, mask=True, geom={"nmw": -1}) == BAD_ARG


@pytest.mark.parametrize("name", ["grit_winattn_fwd_f32", "grit_winattn_bwd_f32"])
def test_f32_unit_count_overflow_is_bad_arg(env, name):
    # 2^20 images of one window x 4096 heads = 2^32 (window, head) units; every earlier check passes: 3 * 2^37 elements < 2^40,
    # 2^20 windows < 2^21, C = 32 * num_heads
    assert _call(env, name, geom={"B": 1 << 20, "H": 1, "W": 1, "num_heads": 4096, "C": 32 * 4096}) == BAD_ARG


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_precedence(env, name):
    last = ENTRIES[name][1][-1]
    assert _call(env, name, null=(last,), geom={"window": 7}) == BAD_ARG  # null pointer before geometry
    assert _call(env, name, geom={"window": 7, "B": 0}) == BAD_ARG  # dimensions before window / heads / shift
    assert _call(env, name, geom={"shift": 12, "nmw": 0}, mask=True) == UNSUPPORTED  # geometry before the mask


def test_rejected_calls_write_nothing(env):
    _, _, bufs = env
    torch.cuda.synchronize()
    for storage, buf in bufs.items():
        for k in OUTPUTS["fwd"] + OUTPUTS["bwd"]:
            assert bool((buf[k].float() == SENTINEL).all()), (storage, k)


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_valid_call_is_ok(env, name, shift):
    storage = ENTRIES[name][2]
    buf = _buffers(torch.bfloat16 if storage == "bf16" else torch.float32)
    if "bwd" in name:  # a backward reads the forward's out and lse
        fwd = "grit_winattn_fwd_f32" if storage == "f32" else "grit_winattn_fwd_bf16"
        assert _call(env, fwd, geom={"shift": shift}, buf=buf) == OK
        for k in OUTPUTS["bwd"]:
            buf[k].zero_()  # d(bias) and d(pad) are accumulated into
    assert _call(env, name, geom={"shift": shift}, buf=buf) == OK
    torch.cuda.synchronize()
    for k in OUTPUTS["bwd" if "bwd" in name else "fwd"]:
        v = buf[k].float()
        assert bool(torch.isfinite(v).all()) and not bool((v == SENTINEL).all()), k
