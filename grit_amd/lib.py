"""ctypes binding of libgrit_hip.so (C ABI in include/grit_hip.h).

There is no fallback: if the library is missing or a call fails this raises.  Tensors are handed over
as raw device pointers together with torch's *current* HIP stream, so launches are ordered with the
surrounding torch ops (same contract as the reference's at::cuda::getCurrentCUDAStream(),
models/ops/src/cuda/ms_deform_attn_cuda.cu:65).
"""
import ctypes
import os

from grit_amd import abi as _abi_reader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgrit_hip.so")

# Everything below the next blank line is include/grit_hip.h read by grit_amd/abi.py: a new entry point, job struct or constant is
# declared in the header and nowhere else.
_abi = _abi_reader.read()
ABI_VERSION = _abi.version  # load() checks it against the library: "this .so was built from this header"
SIGNATURES = {name: argtypes for name, (restype, argtypes) in _abi.functions.items()}  # name -> argument types
for _name, _value in _abi.constants.items():  # GRIT_SLAB_GROUP_MAX -> SLAB_GROUP_MAX, GRIT_OK -> OK, GRIT_ERR_BAD_ARG -> ERR_BAD_ARG
    globals()[_name[len("GRIT_"):]] = _value
for _cname, _fields in _abi.structs.items():  # grit_wgrad_job -> WgradJob, grit_cider_tables -> CiderTables
    _name = "".join(word.capitalize() for word in _cname[len("grit_"):].split("_"))
    globals()[_name] = type(_name, (ctypes.Structure,), {"_fields_": _fields, "__doc__": _cname + " of include/grit_hip.h."})

_lib = None


class GritHipError(RuntimeError):
    pass


def load():
    """Load (once) and type the library.  Raises GritHipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GritHipError(
            "libgrit_hip.so not found at %s -- run `python -m grit_amd.build` (there is no CPU or "
            "PyTorch fallback for the GRIT kernels)" % LIB_PATH)
    # The library resolves its HIP runtime to torch's copy by construction (grit_amd/build.py links libamdhip64.so.7 next to it
    # and sets the run path to $ORIGIN), so the import order of torch and this library does not matter.
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _abi.functions.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = restype, argtypes
    if lib.grit_abi_version() != ABI_VERSION:
        raise GritHipError("libgrit_hip.so ABI %d != binding ABI %d: rebuild" %
                           (lib.grit_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        raise GritHipError("%s failed: %s" % (what, load().grit_status_string(status).decode()))


class _NoGuard(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def device_guard(device):
    """`with device_guard(t.device):` = torch.cuda.device(t.device), but free when that device is already current (the
    one-process-per-GPU case): a training step enters this ~1 000 times and the generic context manager costs ~5 us each."""
    import torch
    index = device.index
    if index is None or index == torch._C._cuda_getDevice():
        return _NO_GUARD
    return torch.cuda.device(device)


def current_stream_ptr():
    """hipStream_t of torch's current stream on the current device (raw handle, no Stream object)."""
    import torch
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def ptr(t):
    """Device (or host) address of tensor `t` as a ctypes pointer argument; None -> NULL."""
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def require_device(*tensors):
    """Reference behaviour: CPU tensors -> error (ms_deform_attn.h:38 'Not implemented on the CPU')."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GritHipError("Not implemented on the CPU: the GRIT kernels need HIP device tensors")
