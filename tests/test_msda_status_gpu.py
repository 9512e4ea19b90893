"""Status codes of the MSDA entry points (grit_amd/csrc/msda.hip) for arguments they reject.  Needs an MI355X, but only for
its buffers: every rejected call returns before any launch; the last test makes one valid call per entry point.

The table below is the argument check of each entry point as written in msda.hip: the pointers that must not be null, what the
pixel stride has to be a multiple of (None: the entry point takes no stride), the largest L*P of its D = 64 kernels (None: any D and
L*P) and the alignment it needs of which pointer.  GRIT_ERR_BAD_ARG (1) conditions -- a null pointer, a non-positive dimension, a
pixel stride below M*D, off its multiple or above 0x3fffffff -- win over GRIT_ERR_UNSUPPORTED (2) ones -- D != 64, L*P too large,
a misaligned pointer, a shape grit_msda_bwd_sorted_supported turns down.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, UNSUPPORTED = 1, 2
DIMS = dict(B=1, S=4, M=1, D=64, L=1, Lq=2, P=2)  # one 2x2 level
DIM_ORDER = ("B", "S", "M", "D", "L", "Lq", "P")

# entry point -> (argument order, pointers, stride multiple, max L*P, {pointer: alignment in bytes}); "dims" stands for the seven
# dimensions in DIM_ORDER, "stream" for the stream; value / grad_out / out / grad_value are f32 in the *_f32 entry points, else bf16
# (everything floating-point is f64 in the *_f64 entry points); the non-strided bf16 wrappers pass M*D as the stride
ENTRIES = {
    "grit_msda_fwd_f32": (("value32", "shapes", "lsi", "loc", "aw", "dims", "out32", "stream"),
                          ("value32", "shapes", "lsi", "loc", "aw", "out32"), None, None, {}),
    "grit_msda_bwd_f32": (("value32", "shapes", "lsi", "loc", "aw", "go32", "dims", "gv32", "gl", "ga", "stream"),
                          ("value32", "shapes", "lsi", "loc", "aw", "go32", "gv32", "gl", "ga"), None, None, {}),
    "grit_msda_fwd_f64": (("value64", "shapes", "lsi", "loc64", "aw64", "dims", "out64", "stream"),
                          ("value64", "shapes", "lsi", "loc64", "aw64", "out64"), None, None, {}),
    "grit_msda_bwd_f64": (("value64", "shapes", "lsi", "loc64", "aw64", "go64", "dims", "gv64", "gl64", "ga64", "stream"),
                          ("value64", "shapes", "lsi", "loc64", "aw64", "go64", "gv64", "gl64", "ga64"), None, None, {}),
    "grit_msda_fwd_bf16": (("value", "shapes", "lsi", "loc", "aw", "dims", "out", "stream"),
                           ("value", "shapes", "lsi", "loc", "aw", "out"), None, 32, {"value": 16, "out": 16}),
    "grit_msda_bwd_bf16acc": (("value", "shapes", "lsi", "loc", "aw", "go", "dims", "gv", "gl", "ga", "stream"),
                              ("value", "shapes", "lsi", "loc", "aw", "go", "gv", "gl", "ga"), None, 16,
                              {"value": 4, "go": 4, "gv": 4}),
    "grit_msda_fwd_bf16_strided": (("value", "stride", "shapes", "lsi", "loc", "aw", "dims", "out", "stream"),
                                   ("value", "shapes", "lsi", "loc", "aw", "out"), 8, 32, {"value": 16, "out": 16}),
    "grit_msda_bwd_bf16": (("value", "shapes", "lsi", "loc", "aw", "go", "dims", "gv32", "gl", "ga", "stream"),
                           ("value", "shapes", "lsi", "loc", "aw", "go", "gv32", "gl", "ga"), None, 16, {}),
    "grit_msda_bwd_bf16acc_strided": (("value", "stride", "shapes", "lsi", "loc", "aw", "go", "dims", "gv", "gl", "ga", "stream"),
                                      ("value", "shapes", "lsi", "loc", "aw", "go", "gv", "gl", "ga"), 2, 16,
                                      {"value": 4, "go": 4, "gv": 4}),
    "grit_msda_bwd_bf16_staged": (("value", "stride", "shapes", "lsi", "loc", "aw", "go", "dims", "stage", "flags", "gv", "gl",
                                   "ga", "stream"),
                                  ("value", "shapes", "lsi", "loc", "aw", "go", "gv", "gl", "ga", "stage", "flags"), 2, 16,
                                  {"value": 4, "go": 4, "stage": 4}),  # grad_value: 2 bytes, which every bf16 pointer has
    "grit_msda_bwd_bf16_sorted": (("value", "stride", "shapes", "lsi", "loc", "aw", "go", "dims", "gv", "gl", "ga", "stream"),
                                  ("value", "shapes", "lsi", "loc", "aw", "go", "gv", "gl", "ga"), 8, 16,
                                  {"value": 4, "go": 16, "gv": 16}),
}


@pytest.fixture(scope="module")
def env():
    from grit_amd import lib
    d = DIMS
    bf, f32 = torch.bfloat16, torch.float32
    rows = d["B"] * d["Lq"] * d["M"]
    buf = {
        "value": torch.ones((d["B"], d["S"], d["M"], d["D"]), dtype=bf, device=DEV),
        "value32": torch.ones((d["B"], d["S"], d["M"], d["D"]), dtype=f32, device=DEV),
        "shapes": torch.tensor([[2, 2]], dtype=torch.int64, device=DEV),
        "lsi": torch.zeros(1, dtype=torch.int64, device=DEV),
        "loc": torch.full((rows, d["L"], d["P"], 2), 0.5, dtype=f32, device=DEV),
        "aw": torch.full((rows, d["L"], d["P"]), 0.5, dtype=f32, device=DEV),
        "out": torch.zeros((rows, d["D"]), dtype=bf, device=DEV),
        "out32": torch.zeros((rows, d["D"]), dtype=f32, device=DEV),
        "go": torch.ones((rows, d["D"]), dtype=bf, device=DEV),
        "go32": torch.ones((rows, d["D"]), dtype=f32, device=DEV),
        "gv": torch.zeros((d["B"], d["S"], d["M"], d["D"]), dtype=bf, device=DEV),
        "gv32": torch.zeros((d["B"], d["S"], d["M"], d["D"]), dtype=f32, device=DEV),
        "gl": torch.zeros((rows, d["L"], d["P"], 2), dtype=f32, device=DEV),
        "ga": torch.zeros((rows, d["L"], d["P"]), dtype=f32, device=DEV),
        "value64": torch.ones((d["B"], d["S"], d["M"], d["D"]), dtype=torch.float64, device=DEV),
        "loc64": torch.full((rows, d["L"], d["P"], 2), 0.5, dtype=torch.float64, device=DEV),
        "aw64": torch.full((rows, d["L"], d["P"]), 0.5, dtype=torch.float64, device=DEV),
        "out64": torch.zeros((rows, d["D"]), dtype=torch.float64, device=DEV),
        "go64": torch.ones((rows, d["D"]), dtype=torch.float64, device=DEV),
        "gv64": torch.zeros((d["B"], d["S"], d["M"], d["D"]), dtype=torch.float64, device=DEV),
        "gl64": torch.zeros((rows, d["L"], d["P"], 2), dtype=torch.float64, device=DEV),
        "ga64": torch.zeros((rows, d["L"], d["P"]), dtype=torch.float64, device=DEV),
        "stage": torch.zeros((d["B"], d["S"], d["M"], 64), dtype=f32, device=DEV),
        "flags": torch.zeros((d["B"], d["S"], d["M"]), dtype=torch.uint8, device=DEV),
    }
    return lib.load(), lib.current_stream_ptr(), buf


def _call(env, name, dims=None, stride=None, null=(), offset=None):
    """The entry point on the valid arguments with `dims` overridden, pixel stride `stride` (default M*D), the pointers in `null`
    passed as NULL and those in `offset` moved by that many bytes (never dereferenced: the call has to return first)."""
    lib, stream, buf = env
    d = dict(DIMS, **(dims or {}))
    args = []
    for a in ENTRIES[name][0]:
        if a == "dims":
            args += [d[k] for k in DIM_ORDER]
        elif a == "stride":
            args.append(DIMS["M"] * DIMS["D"] if stride is None else stride)
        elif a == "stream":
            args.append(stream)
        else:
            addr = 0 if a in null else buf[a].data_ptr() + (offset or {}).get(a, 0)
            args.append(ctypes.c_void_p(addr))
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_pointer_is_bad_arg(env, name):
    for p in ENTRIES[name][1]:
        assert _call(env, name, null=(p,)) == BAD_ARG, p


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_non_positive_dimension_is_bad_arg(env, name):
    for k in DIM_ORDER:
        for v in (0, -1):
            assert _call(env, name, dims={k: v}) == BAD_ARG, (k, v)


@pytest.mark.parametrize("name", sorted(n for n in ENTRIES if ENTRIES[n][2]))
def test_pixel_stride_is_bad_arg(env, name):
    mult, md = ENTRIES[name][2], DIMS["M"] * DIMS["D"]
    assert _call(env, name, stride=md - mult) == BAD_ARG  # below M*D
    assert _call(env, name, stride=md + 1) == BAD_ARG  # odd
    if mult == 8:
        assert _call(env, name, stride=md + 2) == BAD_ARG and _call(env, name, stride=md + 4) == BAD_ARG
    assert _call(env, name, stride=0x40000000) == BAD_ARG  # a multiple of 8 above 0x3fffffff
    assert _call(env, name, stride=0) == BAD_ARG and _call(env, name, stride=-md) == BAD_ARG


def test_dense_wrappers_check_their_own_stride(env):
    """grit_msda_fwd_bf16 / grit_msda_bwd_bf16acc hand M*D to the strided entry points, whose stride rule then holds for M*D: a
    BAD_ARG, which wins over the UNSUPPORTED that D != 64 alone would give."""
    assert _call(env, "grit_msda_fwd_bf16", dims={"D": 4}) == BAD_ARG  # M*D = 4: no multiple of 8
    assert _call(env, "grit_msda_fwd_bf16", dims={"D": 8}) == UNSUPPORTED
    assert _call(env, "grit_msda_bwd_bf16acc", dims={"D": 1}) == BAD_ARG  # M*D odd
    assert _call(env, "grit_msda_bwd_bf16acc", dims={"D": 2}) == UNSUPPORTED


@pytest.mark.parametrize("name", sorted(n for n in ENTRIES if ENTRIES[n][3]))
def test_shape_without_kernel_is_unsupported(env, name):
    max_lp = ENTRIES[name][3]
    assert _call(env, name, dims={"D": 32}) == UNSUPPORTED
    assert _call(env, name, dims={"D": 128}, stride=128) == UNSUPPORTED
    assert _call(env, name, dims={"L": 1, "P": max_lp + 1}) == UNSUPPORTED  # L*P = 17 (backward), 33 (forward)


@pytest.mark.parametrize("name", sorted(n for n in ENTRIES if ENTRIES[n][4]))
def test_misaligned_pointer_is_unsupported(env, name):
    for p, align in ENTRIES[name][4].items():
        for off in (2, 4):
            if off % align:
                assert _call(env, name, offset={p: off}) == UNSUPPORTED, (p, off)


def test_sorted_supported(env):
    lib = env[0]
    assert lib.grit_msda_bwd_sorted_supported(1, 4, 1, 1, 2, 2) == 0
    assert lib.grit_msda_bwd_sorted_supported(1, 4, 1, 1, 4096, 2) == UNSUPPORTED  # Lq > 4095
    assert lib.grit_msda_bwd_sorted_supported(1, 4, 1, 4, 2048, 1) == UNSUPPORTED  # Lq*L*P > 4096
    assert lib.grit_msda_bwd_sorted_supported(1, 100000, 1, 1, 2, 2) == UNSUPPORTED  # S counters beyond the LDS
    for i in range(6):
        dims = [1, 4, 1, 1, 2, 2]
        dims[i] = 0
        assert lib.grit_msda_bwd_sorted_supported(*dims) == BAD_ARG
    assert _call(env, "grit_msda_bwd_bf16_sorted", dims={"Lq": 4096}) == UNSUPPORTED


@pytest.mark.parametrize("name", sorted(n for n in ENTRIES if ENTRIES[n][3]))
def test_bad_arg_wins_over_unsupported(env, name):
    _, ptrs, mult, _, align = ENTRIES[name]
    assert _call(env, name, dims={"D": 32}, null=(ptrs[-1],)) == BAD_ARG
    assert _call(env, name, dims={"D": 32, "B": 0}) == BAD_ARG
    assert _call(env, name, dims={"P": 40, "Lq": 0}) == BAD_ARG
    for p in align:
        if align[p] > 2:
            assert _call(env, name, offset={p: 2}, null=(ptrs[1],)) == BAD_ARG
            if mult:
                assert _call(env, name, offset={p: 2}, stride=DIMS["M"] * DIMS["D"] + 1) == BAD_ARG
    if name == "grit_msda_bwd_bf16_sorted":
        assert _call(env, name, dims={"Lq": 4096}, null=("gl",)) == BAD_ARG
        assert _call(env, name, dims={"Lq": 4096}, stride=60) == BAD_ARG


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_valid_call_is_ok(env, name):
    assert _call(env, name) == 0
    torch.cuda.synchronize()
    _, _, buf = env
    assert int(buf["stage"].count_nonzero()) == 0 and int(buf["flags"].count_nonzero()) == 0  # scratch leaves a call zeroed
