"""Shared test plumbing: build this repo's model with the name-keyed deterministic fill, run it on CPU with the
oracle ops injected (the ONLY way the modules run without a HIP device)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)

from fill import deterministic_fill_  # noqa: E402

from grit_amd.config import default_config  # noqa: E402
from grit_amd.ops.backend import use_reference_ops  # noqa: E402


def oracle_ops():
    from oracle import torch_ref
    return use_reference_ops(torch_ref)


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def build_model(n_layers=3, fill=True, **over):
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.detector import build_detector
    cfg = default_config(**{'model.cap_generator.n_layers': n_layers, **over})
    model = Transformer(build_detector(cfg), cfg)
    if fill:
        deterministic_fill_(model)
    return model, cfg


def disable_drop_path(model):
    from grit_amd.models.common.swin_model import DropPath
    for m in model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0


def result_manager():
    """multiprocessing Manager through which spawned workers hand results back.  Its server is a spawned process too: a forked
    one inherits the HIP state of a test process that already used the GPU, and its garbage collector can crash on freeing the
    inherited device tensors (the server then dies and the reading test sees EOFError)."""
    return torch.multiprocessing.get_context("spawn").Manager()


BEAM_STEP_OUTPUTS = ("sel_beam", "sel_word", "new_seq_logprob", "new_seq_mask", "picked_logprob", "new_met")


def beam_step_raw(**fields):
    """grit_beam_step as the C ABI states it: a zero-initialised grit_beam_step_args with `fields` set by name, the status back after
    a synchronise.  A tensor gives its address and None is NULL; `maps` (a list of tensors, n_maps = its length unless given) and
    `suppress` (a list of ids, n_suppress likewise) become the host arrays that the struct points to."""
    import ctypes
    from grit_amd import lib
    args, keep = lib.BeamStepArgs(), []
    names = {name for name, _ in lib.BeamStepArgs._fields_}
    for name, value in fields.items():
        assert name in names, name
        if name in ("maps", "suppress") and value is not None:
            items = [m.data_ptr() for m in value] if name == "maps" else list(value)
            keep.append(((ctypes.c_void_p if name == "maps" else ctypes.c_int) * max(1, len(items)))(*items))
            if "n_" + name not in fields:
                setattr(args, "n_" + name, len(items))
            value = ctypes.addressof(keep[-1])
        setattr(args, name, value.data_ptr() if torch.is_tensor(value) else value)
    status = lib.load().grit_beam_step(ctypes.byref(args), lib.current_stream_ptr())
    torch.cuda.synchronize()
    return status


def t(a, dtype=None, device="cpu"):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(device)
