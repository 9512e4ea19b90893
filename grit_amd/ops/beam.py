"""One beam-search step after the decoder as two launches (grit_beam_step_f32, include/grit_hip.h): the finished-beam masking,
candidate scores, top-k over beam x vocabulary, beam / word split and the score / mask / log-prob gathers of the reference's
Transformer.iter (models/caption/transformer.py:208-240), bit-identical to the composed torch form.  `beam_step_mean` is the same
step for an ensemble (models/caption/ensemble.py:128-214): the average of the members' maps (grit_beam_step_mean_f32)."""
import collections
import ctypes

import torch

from grit_amd import lib as _lib
from grit_amd.ops import backend


_ptr = _lib.ptr


def supported(word_logprob, cur_beam, beam_size):
    return (word_logprob.is_cuda and word_logprob.dtype == torch.float32 and not word_logprob.requires_grad
            and not torch.is_grad_enabled() and backend.override() is None and beam_size <= 8
            and cur_beam * beam_size * (8 if cur_beam == 1 else 2) <= 128 and word_logprob.shape[0] <= 65535)


def beam_step(word_logprob, seq_logprob, seq_mask, prev_words, eos_idx, beam_size):
    """word_logprob [B, cur_beam, V] f32, seq_logprob [B, cur_beam, 1], seq_mask [B, cur_beam, 1] and prev_words [B * cur_beam, 1]
    (both None at the first step) -> sel_beam, sel_word [B, beam] int64, seq_logprob, seq_mask, picked log-prob [B, beam, 1] f32."""
    B, cur, V = word_logprob.shape
    lp = word_logprob if word_logprob.is_contiguous() else word_logprob.contiguous()
    first = prev_words is None
    dev = lp.device
    L = _lib.load()
    nbytes = L.grit_beam_step_workspace(B, cur, beam_size)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sel_beam = torch.empty((B, beam_size), dtype=torch.int64, device=dev)
    sel_word = torch.empty((B, beam_size), dtype=torch.int64, device=dev)
    new_lp = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    new_mask = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    picked = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    slp = seq_logprob.reshape(-1).float().contiguous()
    if slp.numel() != B * cur:
        raise _lib.GritHipError("seq_logprob has %d entries for %d x %d beams" % (slp.numel(), B, cur))
    sm = pw = None
    if not first:
        sm = seq_mask.reshape(-1).float().contiguous()
        pw = prev_words.reshape(-1).contiguous()
        if sm.numel() != B * cur or pw.numel() != B * cur or pw.dtype != torch.int64:
            raise _lib.GritHipError("beam state does not match %d x %d beams" % (B, cur))
    with _lib.device_guard(dev):
        st = L.grit_beam_step_f32(_ptr(lp), lp.stride(1), _ptr(slp), _ptr(sm), _ptr(pw), int(eos_idx), int(first), B, cur, V,
                                  beam_size, _ptr(ws), nbytes, _ptr(sel_beam), _ptr(sel_word), _ptr(new_lp), _ptr(new_mask),
                                  _ptr(picked), _lib.current_stream_ptr())
    _lib.check(st, "grit_beam_step_f32")
    return sel_beam, sel_word, new_lp, new_mask, picked


MAX_MAPS = 8  # grit_beam_step_mean_f32


def supported_mean(word_logprobs, cur_beam, beam_size):
    """The ensemble step runs on the device kernel: up to 8 fp32 maps of one shape on one device, and what `supported` asks."""
    first = word_logprobs[0]
    return (0 < len(word_logprobs) <= MAX_MAPS and supported(first, cur_beam, beam_size)
            and all(m.shape == first.shape and m.dtype == first.dtype and m.device == first.device and not m.requires_grad
                    for m in word_logprobs))


def beam_step_mean(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size):
    """`beam_step` on the average of K <= 8 word log-probability maps ([B, cur_beam, V] f32 each, one per ensemble member), as
    torch.stack(word_logprobs).mean(0) computes it on the device, bit for bit (grit_beam_step_mean_f32).  The average is formed
    inside the kernel and never written; the returned picked log-prob is the averaged value."""
    B, cur, V = word_logprobs[0].shape
    maps = [m if m.is_contiguous() else m.contiguous() for m in word_logprobs]
    first = prev_words is None
    dev = maps[0].device
    L = _lib.load()
    nbytes = L.grit_beam_step_workspace(B, cur, beam_size)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sel_beam = torch.empty((B, beam_size), dtype=torch.int64, device=dev)
    sel_word = torch.empty((B, beam_size), dtype=torch.int64, device=dev)
    new_lp = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    new_mask = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    picked = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    slp = seq_logprob.reshape(-1).float().contiguous()
    if slp.numel() != B * cur:
        raise _lib.GritHipError("seq_logprob has %d entries for %d x %d beams" % (slp.numel(), B, cur))
    sm = pw = None
    if not first:
        sm = seq_mask.reshape(-1).float().contiguous()
        pw = prev_words.reshape(-1).contiguous()
        if sm.numel() != B * cur or pw.numel() != B * cur or pw.dtype != torch.int64:
            raise _lib.GritHipError("beam state does not match %d x %d beams" % (B, cur))
    table = (ctypes.c_void_p * len(maps))(*[m.data_ptr() for m in maps])  # host array: passed by value to the kernel
    with _lib.device_guard(dev):
        st = L.grit_beam_step_mean_f32(ctypes.cast(table, ctypes.c_void_p), len(maps), maps[0].stride(1), _ptr(slp), _ptr(sm),
                                       _ptr(pw), int(eos_idx), int(first), B, cur, V, beam_size, _ptr(ws), nbytes,
                                       _ptr(sel_beam), _ptr(sel_word), _ptr(new_lp), _ptr(new_mask), _ptr(picked),
                                       _lib.current_stream_ptr())
    _lib.check(st, "grit_beam_step_mean_f32")
    return sel_beam, sel_word, new_lp, new_mask, picked


# ------------------------------------------------------------------------------------------------------ constraints
# Step t chooses word position t; a LIVE source beam with the history h_0 .. h_{t-1} may not choose
#   <eos> while t < min_len; any id of `suppress`; h_{t-1} under no_repeat_word; and, for no_repeat_ngram = n >= 1, the word
#   h_{i+n-1} of every 0 <= i <= t - n with h_i .. h_{i+n-2} == h_{t-n+1} .. h_{t-1} (n = 1: every word used so far).
# A finished beam has no bans: it lives through vocabulary index 0 alone.  A banned candidate scores -inf and stays a candidate.
# `banned_words_host` states this in torch ops (CPU, wide beams, beam search with gradient); grit_beam_step_con_f32 is the same
# on the device inside the two launches of the step.
Constraints = collections.namedtuple("Constraints", "min_len no_repeat_ngram no_repeat_word suppress")
MAX_HISTORY, MAX_SUPPRESS, MAX_SLICE = _lib.BEAM_MAX_HISTORY, _lib.BEAM_MAX_SUPPRESS, _lib.BEAM_MAX_SLICE


def constraints(V, min_len=0, no_repeat_ngram=0, no_repeat_word=False, suppress=()):
    """The validated constraint tuple of one search over a vocabulary of V words (hashable: part of the decode-graph key), or
    None when every rule is off."""
    if isinstance(suppress, int):
        suppress = (suppress,)
    suppress = tuple(int(s) for s in (suppress if suppress is not None else ()))
    min_len, no_repeat_ngram = int(min_len or 0), int(no_repeat_ngram or 0)
    if min_len < 0:
        raise ValueError("min_len must be >= 0, not %d" % min_len)
    if no_repeat_ngram < 0:
        raise ValueError("no_repeat_ngram must be >= 0 (0: off), not %d" % no_repeat_ngram)
    for s in suppress:
        if not 0 <= s < V:
            raise ValueError("suppress id %d is outside the vocabulary [0, %d)" % (s, V))
    if not (min_len or no_repeat_ngram or no_repeat_word or suppress):
        return None
    return Constraints(min_len, no_repeat_ngram, bool(no_repeat_word), suppress)


def banned_words_host(history, alive, t, eos, V, min_len=0, suppress=(), no_repeat_word=False, no_repeat_ngram=0):
    """bool [B, cur_beam, V]: the words that step `t` may not choose.  history [B, cur_beam, t] int64 (any tensor with the two
    leading sizes when t == 0), alive [B, cur_beam] or [B, cur_beam, 1] (nonzero = live; None = every beam live)."""
    B, cur = history.shape[0], history.shape[1]
    banned = torch.zeros((B, cur, V + 1), dtype=torch.bool, device=history.device)  # column V takes what bans nothing

    def ban(words, on=None):  # words [B, cur, m] int64
        ok = (words >= 0) & (words < V)
        if on is not None:
            ok = ok & on
        banned.scatter_(2, torch.where(ok, words, torch.full_like(words, V)), True)

    if t < min_len and 0 <= eos < V:
        banned[:, :, eos] = True
    for s in suppress:
        banned[:, :, s] = True
    if t >= 1:
        hist = history[:, :, :t]
        n = int(no_repeat_ngram)
        if no_repeat_word:
            ban(hist[:, :, t - 1:])
        if n == 1:
            ban(hist)
        elif n > 1 and t >= n:
            # windows i = 0 .. t - n of n - 1 words against the last n - 1 words; a match bans the word that followed
            windows = hist.unfold(2, n - 1, 1)[:, :, :t - n + 1]
            match = (windows == hist[:, :, t - n + 1:].unsqueeze(2)).all(-1)
            ban(hist[:, :, n - 1:], match)
    banned = banned[:, :, :V]
    if alive is not None:
        banned = banned & (alive.reshape(B, cur, 1) != 0)
    return banned


def beam_step_con(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, history, t, con):
    """`beam_step` (one map) or `beam_step_mean` (several) under the constraint tuple `con` at step `t`, history [B, cur_beam, t]
    int64 (None at t == 0): grit_beam_step_con_f32, two launches, nothing uploaded.  Returns None when the call is outside the
    kernel's limits (t > 64, more than 16 suppress ids, a vocabulary slice above 65536 words): the caller uses the host form."""
    if t > MAX_HISTORY or len(con.suppress) > MAX_SUPPRESS:
        return None
    B, cur, V = word_logprobs[0].shape
    maps = [m if m.is_contiguous() else m.contiguous() for m in word_logprobs]
    first = prev_words is None
    dev = maps[0].device
    L = _lib.load()
    nbytes = L.grit_beam_step_workspace(B, cur, beam_size)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sel_beam = torch.empty((B, beam_size), dtype=torch.int64, device=dev)
    sel_word = torch.empty((B, beam_size), dtype=torch.int64, device=dev)
    new_lp = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    new_mask = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    picked = torch.empty((B, beam_size, 1), dtype=torch.float32, device=dev)
    slp = seq_logprob.reshape(-1).float().contiguous()
    if slp.numel() != B * cur:
        raise _lib.GritHipError("seq_logprob has %d entries for %d x %d beams" % (slp.numel(), B, cur))
    sm = pw = hist = None
    if not first:
        sm = seq_mask.reshape(-1).float().contiguous()
        pw = prev_words.reshape(-1).contiguous()
        if sm.numel() != B * cur or pw.numel() != B * cur or pw.dtype != torch.int64:
            raise _lib.GritHipError("beam state does not match %d x %d beams" % (B, cur))
    if t > 0:
        hist = history.reshape(B * cur, -1)
        if hist.shape[1] < t or hist.dtype != torch.int64 or hist.device != dev:
            raise _lib.GritHipError("history does not hold %d words for %d x %d beams" % (t, B, cur))
        hist = hist if hist.stride(1) == 1 else hist.contiguous()
    table = (ctypes.c_void_p * len(maps))(*[m.data_ptr() for m in maps])  # host arrays: passed by value to the kernel
    ids = (ctypes.c_int * max(1, len(con.suppress)))(*con.suppress)
    with _lib.device_guard(dev):
        st = L.grit_beam_step_con_f32(ctypes.cast(table, ctypes.c_void_p), len(maps), maps[0].stride(1), _ptr(slp), _ptr(sm),
                                      _ptr(pw), int(eos_idx), int(first), B, cur, V, beam_size, _ptr(hist),
                                      hist.stride(0) if hist is not None else 0, int(t), con.no_repeat_ngram,
                                      int(con.no_repeat_word), int(t < con.min_len), ctypes.cast(ids, ctypes.c_void_p),
                                      len(con.suppress), _ptr(ws), nbytes, _ptr(sel_beam), _ptr(sel_word), _ptr(new_lp),
                                      _ptr(new_mask), _ptr(picked), _lib.current_stream_ptr())
    if st == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(st, "grit_beam_step_con_f32")
    return sel_beam, sel_word, new_lp, new_mask, picked
