"""One step of sampled decoding after the decoder as one launch (grit_sample_step_f32, include/grit_hip.h): a word per row from
softmax(word_logprob / temperature), restricted to the top_k most probable words and then to the smallest nucleus of mass top_p.

The choice is integer arithmetic on the stored bits, a device seed, the row and the step, so `sample_step_host` -- the same nine
steps in numpy and Python integers -- gives the kernel's words bit for bit.  The host form serves CPU tensors and runs under
`use_reference_ops`, where beam search uses its composed torch form; a device tensor the kernel cannot take raises."""
import numpy as np
import torch

from grit_amd import lib as _lib
from grit_amd.ops import backend

_ptr = _lib.ptr

MAX_V = _lib.SAMPLE_MAX_V
MAX_STEPS = 4096
_M64 = (1 << 64) - 1
_LOG2E = np.uint32(0x3FB8AA3B).view(np.float32)
# P(f) ~ 2^f on [0, 1], constant first: the bit patterns of include/grit_hip.h
_POLY = np.array([0x3F800000, 0x3F317216, 0x3E75FEAD, 0x3D634478, 0x3C1E8620, 0x3AA36993, 0x3962A320], np.uint32).view(np.float32)


def top_p_q32(top_p):
    """round(top_p * 2^32), the form in which the kernel takes the nucleus mass."""
    if not 0.0 < top_p <= 1.0:
        raise ValueError("top_p must be in (0, 1], got %r" % (top_p,))
    return min(max(int(round(top_p * 4294967296.0)), 1), 1 << 32)


def inv_temperature(temperature):
    if not temperature > 0.0:
        raise ValueError("temperature must be positive, got %r" % (temperature,))
    return float(np.float32(1.0 / temperature))


def supported(word_logprob):
    """The kernel takes this map: fp32 on a HIP device, rows of unit stride, a vocabulary within GRIT_SAMPLE_MAX_V."""
    return (word_logprob.is_cuda and word_logprob.dtype == torch.float32 and word_logprob.dim() == 2
            and 1 <= word_logprob.shape[1] <= MAX_V and word_logprob.stride(1) == 1 and backend.override() is None)


def weights_host(row, inv_t):
    """Steps 1-4 for one row of float32 log-probs: the uint64 weights."""
    row = np.asarray(row, np.float32)
    inv_t = np.float32(inv_t)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((row - row.max()) * inv_t) * _LOG2E
        live = t >= np.float32(-42.0)  # drops -inf and NaN, and keeps floor() convertible
        t = np.where(live, t, np.float32(0.0))
        k = np.floor(t)
        f = t - k
        p = np.full_like(f, _POLY[6])
        for c in _POLY[5::-1]:
            p = p * f
            p = p + c
        e = 40 + k.astype(np.int64)
        live &= e >= -1
        mant = (p * np.float32(8388608.0)).astype(np.uint64)
        sh = np.clip(e, -1, 40) - 23
        w = np.where(sh >= 0, mant << np.maximum(sh, 0).astype(np.uint64), mant >> np.maximum(-sh, 0).astype(np.uint64))
    return np.where(live, w, np.uint64(0)).astype(np.uint64)


def kept_host(row, w, top_k, q32):
    """Steps 5-6: the boolean mask of the kept words."""
    V = row.shape[0]
    order = np.argsort(-row.astype(np.float64), kind="stable")  # log-prob descending, equal ones by index
    K = min(top_k, V) if top_k > 0 else V
    cum = np.cumsum(w[order[:K]], dtype=np.uint64)
    need = max(1, (q32 * int(cum[-1])) >> 32)
    n = int(np.searchsorted(cum, np.uint64(need), side="left")) + 1  # the shortest prefix whose sum reaches `need`
    kept = np.zeros(V, bool)
    kept[order[:min(n, K)]] = True
    return kept


def draw(seed, r, step):
    """Step 7 up to the multiplication by S: splitmix64's finaliser of the counter of (row, step)."""
    x = (seed + 0x9E3779B97F4A7C15 * (r * 4096 + step + 1)) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def pick_host(w, kept, x):
    """Steps 7-8 for the kept weights and the 64-bit draw x."""
    cum = np.cumsum(np.where(kept, w, np.uint64(0)), dtype=np.uint64)
    target = (x * int(cum[-1])) >> 64
    return min(int(np.searchsorted(cum, np.uint64(target), side="right")), len(w) - 1)  # the clamp: rows without a finite entry


def sample_step_host(logp, rows, fan, prev_words, alive_in, eos, fill, inv_t, top_k, q32, seed, step):
    """grit_sample_step_f32 on the host.  logp [rows / fan, V] float32 (numpy), prev_words / alive_in [rows] or None together,
    seed a Python integer -> words int64, picked float32, alive float32, all [rows]."""
    logp = np.asarray(logp, np.float32)
    if (logp.ndim != 2 or rows <= 0 or fan <= 0 or rows % fan or logp.shape[0] * fan != rows or (prev_words is None) != (alive_in is None)
            or not 0 <= step < MAX_STEPS or top_k < 0 or not 1 <= q32 <= 1 << 32 or not (np.isfinite(inv_t) and inv_t > 0)):
        raise ValueError("sample_step_host: bad arguments")
    words = np.empty(rows, np.int64)
    picked = np.empty(rows, np.float32)
    alive = np.ones(rows, np.float32)
    if prev_words is not None:
        alive = (np.asarray(alive_in, np.float32) * (np.asarray(prev_words) != eos)).astype(np.float32)
        alive = (alive != 0).astype(np.float32)
    seed = int(seed) & _M64
    shared = {}  # source row -> (weights, kept): the `fan` samples of a row differ in the draw only
    for r in range(rows):
        if alive[r] == 0:
            words[r], picked[r] = fill, 0.0
            continue
        src = r // fan
        if src not in shared:
            shared.clear()
            w = weights_host(logp[src], inv_t)
            shared[src] = (w, kept_host(logp[src], w, top_k, q32))
        w, kept = shared[src]
        words[r] = pick_host(w, kept, draw(seed, r, step))
        picked[r] = logp[src, words[r]]
    return words, picked, alive


def sample_step(word_logprob, fan, prev_words, alive, eos_idx, temperature, top_k, top_p, seed, step, fill=0):
    """word_logprob [rows / fan, V] f32; prev_words [rows, 1] int64 and alive [rows] f32 (both None at the first step); seed a
    one-element int64 / uint64 tensor on word_logprob's device -> words [rows] int64, picked [rows] f32, alive [rows] f32."""
    lp = word_logprob.detach()
    rows = lp.shape[0] * fan
    inv_t, q32 = inv_temperature(temperature), top_p_q32(top_p)
    if not lp.is_cuda or backend.override() is not None:
        pw = None if prev_words is None else prev_words.reshape(-1).cpu().numpy()
        al = None if alive is None else alive.reshape(-1).float().cpu().numpy()
        out = sample_step_host(lp.float().cpu().numpy(), rows, fan, pw, al, int(eos_idx), fill, inv_t, int(top_k), q32,
                               int(seed.reshape(-1)[0].item()), int(step))
        return tuple(torch.from_numpy(o).to(lp.device) for o in out)
    if not supported(lp):
        raise _lib.GritHipError("grit_sample_step_f32 takes fp32 maps [rows, V <= %d] with unit column stride, got %s %s"
                                % (MAX_V, lp.dtype, tuple(lp.shape)))
    if seed.device != lp.device or seed.numel() != 1 or seed.element_size() != 8:
        raise _lib.GritHipError("sample_step: the seed is one 64-bit integer on the device of the log-probs")
    dev = lp.device
    words = torch.empty(rows, dtype=torch.int64, device=dev)
    picked = torch.empty(rows, dtype=torch.float32, device=dev)
    alive_out = torch.empty(rows, dtype=torch.float32, device=dev)
    pw = al = None
    if prev_words is not None:
        pw = prev_words.reshape(-1).contiguous()
        al = alive.reshape(-1).float().contiguous()
        if pw.numel() != rows or al.numel() != rows or pw.dtype != torch.int64:
            raise _lib.GritHipError("sample state does not match %d rows" % rows)
    with _lib.device_guard(dev):
        st = _lib.load().grit_sample_step_f32(_ptr(lp), lp.stride(0), rows, fan, lp.shape[1], _ptr(pw), _ptr(al), int(eos_idx),
                                              int(fill), inv_t, int(top_k), q32, _ptr(seed), int(step), _ptr(words), _ptr(picked),
                                              _ptr(alive_out), _lib.current_stream_ptr())
    _lib.check(st, "grit_sample_step_f32")
    return words, picked, alive_out
