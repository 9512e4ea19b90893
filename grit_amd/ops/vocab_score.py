"""The caption likelihood head: log-probability of one target word per decoder row and the row's log-sum-exp over the vocabulary.

`vocab_score` is grit_vocab_score_bf16 (include/grit_hip.h): the vocabulary projection, the log-softmax and the gather in two
launches, without the [rows, V] logit map.  `vocab_score_host` is the composed form: the logits and the log-softmax of
CaptionGenerator.forward (reference models/caption/cap_generator.py:157-167) as that function computes them (`head_logits` below is
its projection, shared with it), the gather, and torch.logsumexp.  It runs for every dtype and on the CPU.

Both follow the same rules for the target of a row: `pad_idx` gives +0.0, an index outside [0, V) that is not `pad_idx` gives NaN
(nothing is read out of bounds, nothing is checked on the host: no synchronisation)."""
import os

import torch
import torch.nn.functional as F

from grit_amd import lib as _lib
from grit_amd.ops import backend

# GRIT_VOCAB_HEAD=0: always the composed form (A/B knob, tools/bench_vocab_score.py)
VOCAB_HEAD = os.environ.get("GRIT_VOCAB_HEAD", "1") != "0"

_ptr = _lib.ptr


def head_logits(x, w):
    """float32 logits [..., V] of hidden states x [..., D] under the vocabulary weight w [V, D]: CaptionGenerator.forward's projection."""
    if x.is_cuda and x.dtype == w.dtype == torch.bfloat16 and not torch.is_grad_enabled() and backend.override() is None:
        # products of two bf16 values are exact in float32, so the bf16 GEMM with float32 accumulation and float32
        # output IS the float32 projection of the same operands (summation order aside) -- without up-casting the
        # [V, 512] weight on every step and at the bf16 matrix-core rate
        return torch.mm(x.reshape(-1, x.shape[-1]), w.t(), out_dtype=torch.float32).view(*x.shape[:-1], w.shape[0])
    return F.linear(x.float(), w.float())


def supported(x, w):
    """Does the kernel take x [R, D], w [V, D]?  (bf16 on a HIP device, D a multiple of 64 in [64, 512], no autograd.)"""
    if not (VOCAB_HEAD and backend.override() is None and x.is_cuda and w.is_cuda and x.device == w.device):
        return False
    if not (x.dtype == w.dtype == torch.bfloat16 and x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1]):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        return False
    D = x.shape[1]
    return D % 64 == 0 and 64 <= D <= 512 and x.shape[0] >= 1 and w.shape[0] >= 1


def _rows(t):
    """t [rows, D] with unit column stride, a row stride that is a multiple of 8 elements and a 16-byte aligned base."""
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def slice_width(V, D):
    """Columns per vocabulary slice of the kernel (0 outside its limits): a function of V and D only."""
    return int(_lib.load().grit_vocab_score_slice(int(V), int(D)))


def vocab_score(x, w, target, pad_idx):
    """x [R, D] bf16, w [V, D] bf16, target [R] int64 on the device -> (logp [R], lse [R]) float32.  Two launches on the current
    stream; no synchronisation, no host copy; capturable in a graph."""
    _lib.require_device(x, w, target)
    if not supported(x, w):
        raise _lib.GritHipError("vocab_score: needs bf16 x [R, D] and w [V, D] on one HIP device, D %% 64 == 0, 64 <= D <= 512, no "
                                "autograd (got %s %s, %s %s); vocab_score_host is the composed form"
                                % (tuple(x.shape), x.dtype, tuple(w.shape), w.dtype))
    if target.dtype != torch.int64 or target.dim() != 1 or target.shape[0] != x.shape[0] or target.device != x.device:
        raise _lib.GritHipError("vocab_score: target must be [R] int64 on the device of x")
    x, w = _rows(x), _rows(w)
    target = target if target.is_contiguous() else target.contiguous()
    R, D = x.shape
    V = w.shape[0]
    L = _lib.load()
    work = torch.empty(int(L.grit_vocab_score_workspace(R, V, D)), dtype=torch.uint8, device=x.device)
    out = torch.empty((2, R), dtype=torch.float32, device=x.device)
    with _lib.device_guard(x.device):
        st = L.grit_vocab_score_bf16(_ptr(x), x.stride(0), _ptr(w), w.stride(0), _ptr(target), int(pad_idx), R, V, D, _ptr(work),
                                     _ptr(out[0]), _ptr(out[1]), _lib.current_stream_ptr())
    _lib.check(st, "grit_vocab_score_bf16")
    return out[0], out[1]


def vocab_score_host(x, w, target, pad_idx):
    """The composed form, for every dtype and device: (logp [R], lse [R]) float32."""
    with torch.autocast(x.device.type, enabled=False):
        logits = head_logits(x, w)
        log_probs = F.log_softmax(logits, dim=-1)
        V = logits.shape[-1]
        target = target.reshape(-1)
        inside = (target >= 0) & (target < V)
        picked = torch.gather(log_probs, -1, target.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
        picked = torch.where(inside, picked, torch.full_like(picked, float('nan')))
        picked = torch.where(target == pad_idx, torch.zeros_like(picked), picked)
        return picked, torch.logsumexp(logits, dim=-1)


def score(x, w, target, pad_idx):
    """The kernel where it takes the call, the composed form otherwise (fp32 models, the CPU, GRIT_VOCAB_HEAD=0)."""
    if supported(x, w):
        return vocab_score(x, w, target, pad_idx)
    return vocab_score_host(x, w, target, pad_idx)
