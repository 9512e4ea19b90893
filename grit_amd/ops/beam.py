"""One beam-search step after the decoder as two launches (grit_beam_step, include/grit_hip.h): the finished-beam masking,
candidate scores, top-k over beam x vocabulary, beam / word split and the score / mask / log-prob gathers of the reference's
Transformer.iter (models/caption/transformer.py:208-240), bit-identical to the composed torch form.  `beam_step_mean` is the same
step for an ensemble (models/caption/ensemble.py:128-214): the average of the members' maps.  Past the reference: the step under
constraints (`beam_step_con`), the step of a diverse search over beam groups (`beam_step_div`) and the step of a search with forced
words (`beam_step_forced`), each with its host form in torch ops.  All five are fronts over `_step`, the one place that fills
grit_beam_step_args and launches; `fused_step` chooses among them for the decoders."""
import collections
import ctypes

import torch

from grit_amd import lib as _lib
from grit_amd.ops import backend


def supported(word_logprob, cur_beam, beam_size):
    return (word_logprob.is_cuda and word_logprob.dtype == torch.float32 and not word_logprob.requires_grad
            and not torch.is_grad_enabled() and backend.override() is None and beam_size <= 8
            and cur_beam * beam_size * (8 if cur_beam == 1 else 2) <= 128 and word_logprob.shape[0] <= 65535)


MAX_MAPS = 8  # grit_beam_step: n_maps


def supported_mean(word_logprobs, cur_beam, beam_size):
    """The ensemble step runs on the device kernel: up to 8 fp32 maps of one shape on one device, and what `supported` asks."""
    first = word_logprobs[0]
    return (0 < len(word_logprobs) <= MAX_MAPS and supported(first, cur_beam, beam_size)
            and all(m.shape == first.shape and m.dtype == first.dtype and m.device == first.device and not m.requires_grad
                    for m in word_logprobs))


def _address(tensor):
    return None if tensor is None else tensor.data_ptr()


def _step(maps, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, con=None, history=None, t=0, groups=None, force_words=None,
          met=None, or_none=True):
    """grit_beam_step on one map or on the mean of several: the arguments of `beam_step`, and optionally the constraint tuple `con`
    with history [B, cur_beam, t] int64 (None at t == 0) and the step `t`, the `groups` tuple (num_groups, diversity), and
    force_words [B, C, W] int64 with met [B, cur_beam] int32 (None: the first step).  Returns the five outputs of `beam_step`, and
    new_met [B, beam] int32 behind them for forced words.  Outside the kernel's limits nothing is launched: None when `or_none`
    (the caller uses the host form), else GritHipError."""
    B, cur, V = maps[0].shape
    # the limits that the rules add, before the library is touched
    if con is not None and (t > MAX_HISTORY or len(con.suppress) > MAX_SUPPRESS):
        return None
    if (groups is not None or force_words is not None) and \
            (beam_size > 8 or V < beam_size or cur not in (1, beam_size) or len(maps) > MAX_MAPS):
        return None
    if groups is not None and beam_size % groups.num_groups != 0:
        return None
    if force_words is not None and not (1 <= force_words.shape[1] <= MAX_FORCED_SETS
                                        and 1 <= force_words.shape[2] <= MAX_FORCED_WORDS):
        return None
    # the kernel reads evenly spaced rows of adjacent words (any row stride >= V); every other layout is copied
    ld = {m.stride(0) if cur == 1 else m.stride(1) for m in maps}
    spaced = len(ld) == 1 and min(ld) >= V and all(m.stride(2) == 1 and (cur == 1 or m.stride(0) == cur * m.stride(1))
                                                   for m in maps)
    maps = list(maps) if spaced else [m.contiguous() for m in maps]
    ld = min(ld) if spaced else V
    first = prev_words is None
    dev = maps[0].device
    if force_words is not None:
        if force_words.shape[0] != B or force_words.dtype != torch.int64 or force_words.device != dev:
            raise _lib.GritHipError("force_words must be int64 [%d, sets, words] on %s" % (B, dev))
        force_words = force_words if force_words.is_contiguous() else force_words.contiguous()
        if met is not None:
            if met.numel() != B * cur or met.dtype != torch.int32 or met.device != dev:
                raise _lib.GritHipError("met must be int32 with %d x %d entries on %s" % (B, cur, dev))
            met = met.reshape(-1).contiguous()
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
    args = _lib.BeamStepArgs(
        maps=ctypes.addressof(table), n_maps=len(maps), ld=ld, seq_logprob=slp.data_ptr(), seq_mask=_address(sm),
        prev_words=_address(pw), eos=int(eos_idx), first_step=int(first), B=B, cur_beam=cur, V=V, k=beam_size,
        workspace=ws.data_ptr(), workspace_bytes=nbytes, sel_beam=sel_beam.data_ptr(), sel_word=sel_word.data_ptr(),
        new_seq_logprob=new_lp.data_ptr(), new_seq_mask=new_mask.data_ptr(), picked_logprob=picked.data_ptr())
    outputs = (sel_beam, sel_word, new_lp, new_mask, picked)
    if con is not None:
        hist = None
        if t > 0:
            hist = history.reshape(B * cur, -1)
            if hist.shape[1] < t or hist.dtype != torch.int64 or hist.device != dev:
                raise _lib.GritHipError("history does not hold %d words for %d x %d beams" % (t, B, cur))
            hist = hist if hist.stride(1) == 1 else hist.contiguous()
            args.history, args.history_ld = hist.data_ptr(), hist.stride(0)
        ids = (ctypes.c_int * len(con.suppress))(*con.suppress)  # host array as well
        args.t, args.no_repeat_ngram, args.no_repeat_word = int(t), con.no_repeat_ngram, int(con.no_repeat_word)
        args.ban_eos, args.suppress, args.n_suppress = int(t < con.min_len), ctypes.addressof(ids), len(ids)
    if groups is not None:
        args.groups, args.diversity = int(groups.num_groups), float(groups.diversity)
    if force_words is not None:
        new_met = torch.empty((B, beam_size), dtype=torch.int32, device=dev)
        args.force_words, args.n_sets, args.n_words = force_words.data_ptr(), force_words.shape[1], force_words.shape[2]
        args.met_in, args.new_met = _address(met), new_met.data_ptr()
        outputs += (new_met,)
    with _lib.device_guard(dev):
        st = L.grit_beam_step(ctypes.byref(args), _lib.current_stream_ptr())
    if st == _lib.ERR_UNSUPPORTED and or_none:
        return None
    _lib.check(st, "grit_beam_step")
    return outputs


def beam_step(word_logprob, seq_logprob, seq_mask, prev_words, eos_idx, beam_size):
    """word_logprob [B, cur_beam, V] f32, seq_logprob [B, cur_beam, 1], seq_mask [B, cur_beam, 1] and prev_words [B * cur_beam, 1]
    (both None at the first step) -> sel_beam, sel_word [B, beam] int64, seq_logprob, seq_mask, picked log-prob [B, beam, 1] f32."""
    return _step([word_logprob], seq_logprob, seq_mask, prev_words, eos_idx, beam_size, or_none=False)


def beam_step_mean(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size):
    """`beam_step` on the average of K <= 8 word log-probability maps ([B, cur_beam, V] f32 each, one per ensemble member), as
    torch.stack(word_logprobs).mean(0) computes it on the device, bit for bit.  The average is formed inside the kernel and never
    written; the returned picked log-prob is the averaged value."""
    return _step(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, or_none=False)



# ------------------------------------------------------------------------------------------------------ constraints
# Step t chooses word position t; a LIVE source beam with the history h_0 .. h_{t-1} may not choose
#   <eos> while t < min_len; any id of `suppress`; h_{t-1} under no_repeat_word; and, for no_repeat_ngram = n >= 1, the word
#   h_{i+n-1} of every 0 <= i <= t - n with h_i .. h_{i+n-2} == h_{t-n+1} .. h_{t-1} (n = 1: every word used so far).
# A finished beam has no bans: it lives through vocabulary index 0 alone.  A banned candidate scores -inf and stays a candidate.
# `banned_words_host` states this in torch ops (CPU, wide beams, beam search with gradient); grit_beam_step with its bans is the
# same on the device inside the two launches of the step.
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
    int64 (None at t == 0): two launches, nothing uploaded.  Returns None when the call is outside the kernel's limits (t > 64,
    more than 16 suppress ids, a vocabulary slice above 65536 words): the caller uses the host form."""
    return _step(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, con, history, t)


# ------------------------------------------------------------------------------------------------------ beam groups
# Diverse beam search (Vijayakumar et al. 2016, the num_beam_groups / diversity_penalty of the generation libraries): beam_size =
# G * g, group i owns the beam rows [i * g, (i + 1) * g) for the whole search, and within a step the groups are resolved in the order
# 0 .. G - 1 per image.  counts[w] = how many selections of the earlier groups in THIS step chose word w from a live source row
# (a finished row that survives through word 0 chose nothing; two beams choosing w count 2).  Group i scores
#   live row j, word w:  seq_logprob[j] + (word_logprob[j, w] - diversity * float(counts[w]))     three rounded fp32 operations
#   finished row j:      seq_logprob[j] at word 0, -999 elsewhere; no penalty
#   banned (j, w):       -inf
# and takes its g best of its g * V candidates, value descending, ties by ascending row * V + word.  At the first step every group
# reads row 0.  The running score that moves on is the PENALISED value (as the generation libraries keep it), `picked` the
# unpenalised word log-prob.  With counts == 0 the score is the plain step's bit for bit.  `beam_step_groups_host` states this in
# torch ops; grit_beam_step with groups >= 1 is the same on the device in the two launches of a step.
Groups = collections.namedtuple("Groups", "num_groups diversity")


def groups(beam_size, num_groups=1, diversity=0.0):
    """The validated (num_groups, diversity) of one search (hashable: part of the decode-graph key), or None for one group, which
    is the plain search whatever the penalty."""
    if isinstance(num_groups, bool) or int(num_groups) != num_groups:
        raise ValueError("num_groups must be an integer, not %r" % (num_groups,))
    num_groups, diversity = int(num_groups), float(diversity)
    if num_groups < 1:
        raise ValueError("num_groups must be >= 1, not %d" % num_groups)
    if beam_size % num_groups != 0:
        raise ValueError("num_groups = %d does not divide beam_size = %d" % (num_groups, beam_size))
    if not 0.0 <= diversity < float('inf'):  # refuses NaN as well
        raise ValueError("diversity must be finite and >= 0, not %r" % diversity)
    return None if num_groups == 1 else Groups(num_groups, diversity)


def beam_step_groups_host(word_logprob, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, num_groups, diversity, history=None,
                          t=0, con=None):
    """The grouped step in torch ops, on any device and with gradient: the arguments of `beam_step` (word_logprob is the mean
    already for an ensemble), the group count and penalty, and for a constraint tuple `con` the history [B, cur_beam, t] and the
    step.  Returns what `beam_step` returns.  Selection is a stable descending sort, so ties resolve by index."""
    B, cur, V = word_logprob.shape
    g = beam_size // num_groups
    if g * num_groups != beam_size or cur not in (1, beam_size):
        raise ValueError("%d groups over %d beams with %d source rows" % (num_groups, beam_size, cur))
    seq_logprob = seq_logprob.reshape(B, cur, 1)
    if prev_words is None:
        alive = torch.ones((B, cur, 1), dtype=torch.float32, device=word_logprob.device)
    else:
        alive = seq_mask.reshape(B, cur, 1) * (prev_words.reshape(B, cur, 1) != eos_idx).float()
    live = alive != 0
    frozen = seq_logprob.expand(B, cur, V).clone()
    frozen[:, :, 1:] = -999  # a finished beam survives only through vocabulary index 0
    banned = None
    if con is not None:
        if history is None:
            history = torch.zeros((B, cur, 0), dtype=torch.long, device=word_logprob.device)
        banned = banned_words_host(history, None if prev_words is None else alive, t, eos_idx, V, **con._asdict())
    penalty = torch.tensor(float(diversity), dtype=torch.float32, device=word_logprob.device)
    counts = torch.zeros((B, V), dtype=torch.float32, device=word_logprob.device)
    sel_beam, sel_word, new_lp = [], [], []
    for i in range(num_groups):
        lo, hi = (0, 1) if cur == 1 else (i * g, (i + 1) * g)
        cand = seq_logprob[:, lo:hi] + (word_logprob[:, lo:hi] - (penalty * counts).unsqueeze(1))
        cand = torch.where(live[:, lo:hi], cand, frozen[:, lo:hi])
        if banned is not None:
            cand = cand.masked_fill(banned[:, lo:hi], float('-inf'))
        value, index = torch.sort(cand.reshape(B, -1), dim=-1, descending=True, stable=True)
        value, index = value[:, :g], index[:, :g]
        local = torch.div(index, V, rounding_mode='floor')
        word = index - local * V
        source = local + lo
        counts = counts.scatter_add(1, word, (torch.gather(alive[:, :, 0], 1, source) != 0).float())
        sel_beam.append(source)
        sel_word.append(word)
        new_lp.append(value)
    sel_beam, sel_word = torch.cat(sel_beam, 1), torch.cat(sel_word, 1)
    col = sel_beam.unsqueeze(-1)
    new_mask = torch.gather(alive, 1, col)
    picked = torch.gather(torch.gather(word_logprob, 1, col.expand(B, beam_size, V)), 2, sel_word.unsqueeze(-1)) * new_mask
    return sel_beam, sel_word, torch.cat(new_lp, 1).unsqueeze(-1), new_mask, picked


def supported_div(word_logprobs, cur_beam, beam_size, num_groups):
    """The grouped step runs on the device kernel: what `supported_mean` asks of the maps, and a vocabulary of at least beam_size
    words (a group always finds its g candidates among stage 1's)."""
    return (supported_mean(word_logprobs, cur_beam, beam_size) and cur_beam in (1, beam_size) and beam_size % num_groups == 0
            and word_logprobs[0].shape[-1] >= beam_size)


def beam_step_div(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, num_groups, diversity, history=None, t=0,
                  con=None):
    """The grouped step of one map or of the mean of several on the device (two launches, nothing uploaded), under the constraint
    tuple `con` (None: unconstrained; history and t are then not read).  Returns None when the call is outside the kernel's limits
    (a beam above 8, fewer words than beams, and with constraints t > 64 or more than 16 suppress ids or a slice above 65536
    words): the caller uses `beam_step_groups_host`."""
    return _step(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, con, history, t,
                 groups=Groups(num_groups, diversity))


# ------------------------------------------------------------------------------------------------------ forced words
# Constrained beam search by dynamic beam allocation (Post & Vilar 2018; the force_words_ids of the generation libraries).
# force_words [B, C, W] int64 padded with -1: set c of image b is the ids >= 0 of force_words[b, c], a disjunction ("dog" or
# "dogs"); a set with no ids counts as met from the start.  Every beam carries `met`, an int32 bitmask of the sets that its words
# so far have hit; full = all C bits.  One step for an image with `cur` source rows and k = beam_size:
#   1. a live row has the bans of the constrained step, and <eos> is banned in addition while met != full;
#   2. candidates A: row j contributes its k best candidates under the constrained step's scoring (live: seq_logprob[j] +
#      logp[j][w], -inf where banned, ties to the ascending word); a finished row only its word-0 candidate, score seq_logprob[j];
#   3. candidates F: a live row also contributes (j, w) for every w of a set that it has not met and that is not banned for it,
#      same single add; duplicates of (j, w) are kept once;
#   4. met'(j, w) = met[j] | {c : w in set c} for a live row, met[j] for a finished one; bank = popcount(met'); a candidate that
#      scores -inf goes to bank -1;
#   5. inside a bank: score descending, then j * V + w ascending;
#   6. for round r = 0, 1, 2, ... and within a round for bank = C down to -1: a bank with more than r candidates gives its r-th,
#      until k are chosen;
#   7. outputs in the order of choice: sel_beam, sel_word, the candidate's score, the source row's liveness, the stored log-prob
#      times liveness, and new_met = met'.
# `beam_step_forced_host` states this in torch ops; grit_beam_step with force_words is the same on the device in two launches.
MAX_FORCED_SETS, MAX_FORCED_WORDS = _lib.BEAM_MAX_FORCED_SETS, _lib.BEAM_MAX_FORCED_WORDS


def forced(V, force_words, eos_idx, bos_idx=None, pad_idx=None):
    """The validated force_words of one search over a vocabulary of V words: an int64 tensor [B, C, W] padded with -1 (a tensor or
    nested lists of that shape), or None when there is nothing to force (None, C == 0 or W == 0).  ValueError for ids >= V, for
    <eos> / <bos> / <pad> in a set, for more than 8 sets or more than 4 words in a set."""
    if force_words is None:
        return None
    fw = torch.as_tensor(force_words)
    if fw.dim() != 3 or fw.dtype.is_floating_point or fw.dtype == torch.bool:
        raise ValueError("force_words must be an integer tensor [B, sets, words] padded with -1, not %s %s"
                         % (fw.dtype, tuple(fw.shape)))
    B, C, W = fw.shape
    if C > MAX_FORCED_SETS:
        raise ValueError("%d sets of forced words: at most %d" % (C, MAX_FORCED_SETS))
    if W > MAX_FORCED_WORDS:
        raise ValueError("%d words in a set of forced words: at most %d" % (W, MAX_FORCED_WORDS))
    if fw.numel() == 0:
        return None
    fw = fw.long().contiguous()
    special = [(name, i) for name, i in (("<eos>", eos_idx), ("<bos>", bos_idx), ("<pad>", pad_idx)) if i is not None and i >= 0]
    # one read of the device for all checks: the largest id, then how often every special id occurs
    top, *found = torch.stack([fw.max()] + [(fw == i).sum() for _, i in special]).tolist()
    if top >= V:
        raise ValueError("forced word %d is outside the vocabulary [0, %d)" % (top, V))
    for (name, i), bad in zip(special, found):
        if bad:
            raise ValueError("%s (%d) cannot be a forced word" % (name, i))
    return fw


def initial_met(force_words):
    """int32 [B]: the mask of the sets of every image that hold no id, which count as met from the start."""
    C = force_words.shape[1]
    bits = 1 << torch.arange(C, dtype=torch.int32, device=force_words.device)
    return ((force_words < 0).all(-1).int() * bits).sum(-1, dtype=torch.int32)


def beam_step_forced_host(word_logprob, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, force_words, met=None, history=None,
                          t=0, con=None):
    """The step with forced words in torch ops, on any device and with gradient: the arguments of `beam_step` (word_logprob is the
    mean already for an ensemble), force_words [B, C, W], met [B, cur_beam] int32 (None: the first step, the empty sets), and the
    history / step / constraint tuple of `beam_step_con`.  Returns what `beam_step` returns and new_met [B, beam] int32."""
    B, cur, V = word_logprob.shape
    k, dev = beam_size, word_logprob.device
    C, W = force_words.shape[1], force_words.shape[2]
    if cur not in (1, k) or V < k or force_words.shape[0] != B:
        raise ValueError("forced words over %d beams with %d source rows of %d words, %d images" % (k, cur, V, force_words.shape[0]))
    seq_logprob = seq_logprob.reshape(B, cur, 1)
    if prev_words is None:
        alive = torch.ones((B, cur, 1), dtype=torch.float32, device=dev)
    else:
        alive = seq_mask.reshape(B, cur, 1) * (prev_words.reshape(B, cur, 1) != eos_idx).float()
    live = alive != 0  # [B, cur, 1]
    full = (1 << C) - 1
    met = initial_met(force_words).view(B, 1).expand(B, cur) if met is None else met.reshape(B, cur).int()
    # 1. bans
    if con is not None:
        if history is None:
            history = torch.zeros((B, cur, 0), dtype=torch.long, device=dev)
        banned = banned_words_host(history, None if prev_words is None else alive, t, eos_idx, V, **con._asdict())
    else:
        banned = torch.zeros((B, cur, V), dtype=torch.bool, device=dev)
    if 0 <= eos_idx < V:
        banned[:, :, eos_idx] |= live[:, :, 0] & (met != full)
    cand = (seq_logprob + word_logprob).masked_fill(banned, float('-inf'))
    # 2. A: k per live row, the word-0 candidate of a finished row
    a_score, a_word = torch.sort(cand, dim=-1, descending=True, stable=True)
    a_score, a_word = a_score[:, :, :k], a_word[:, :, :k]
    a_valid = live | (torch.arange(k, device=dev) == 0)
    a_word = torch.where(live, a_word, torch.zeros_like(a_word))
    a_score = torch.where(live, a_score, seq_logprob.expand(B, cur, k))
    # 3. F: the words of the sets that a live row has not met, unless banned for it
    fw = force_words.reshape(B, 1, C * W).expand(B, cur, C * W)
    set_of = torch.arange(C, device=dev).repeat_interleave(W)
    unmet = ((met.unsqueeze(-1) >> set_of) & 1) == 0
    f_word = fw.clamp(min=0)
    f_valid = (fw >= 0) & unmet & live & ~torch.gather(banned, 2, f_word)
    f_score = seq_logprob + torch.gather(word_logprob, 2, f_word)
    n = k + C * W
    valid = torch.cat([a_valid, f_valid], -1).reshape(B, cur * n)
    word = torch.cat([a_word, f_word], -1)
    score = torch.cat([a_score, f_score], -1).reshape(B, cur * n)
    row = torch.arange(cur, device=dev).view(1, cur, 1).expand(B, cur, n)
    key = (row * V + word).reshape(B, cur * n)
    row, word = row.reshape(B, cur * n), word.reshape(B, cur * n)
    N = cur * n
    earlier = torch.ones((N, N), dtype=torch.bool, device=dev).tril(-1)  # [i, o]: o < i
    valid = valid & ~((key.unsqueeze(2) == key.unsqueeze(1)) & valid.unsqueeze(1) & earlier).any(-1)
    # 4. banks
    in_set = ((word.view(B, N, 1, 1) == force_words.view(B, 1, C, W)) & (force_words.view(B, 1, C, W) >= 0)).any(-1)  # [B, N, C]
    hits = (in_set.int() * (1 << torch.arange(C, dtype=torch.int32, device=dev))).sum(-1, dtype=torch.int32)
    row_met, row_live = torch.gather(met, 1, row), torch.gather(live[:, :, 0], 1, row)
    new_met = torch.where(row_live, row_met | hits, row_met)
    bank = sum((new_met >> c) & 1 for c in range(C))
    bank = torch.where(score == float('-inf'), torch.full_like(bank, -1), bank)
    bank = torch.where(valid, bank, torch.full_like(bank, -2))
    # 5. the candidates bank by bank (descending), inside a bank by score descending, then key ascending
    order = torch.sort(key, dim=1, stable=True)[1]
    order = torch.gather(order, 1, torch.sort(torch.gather(score.detach(), 1, order), dim=1, descending=True, stable=True)[1])
    order = torch.gather(order, 1, torch.sort(torch.gather(bank, 1, order), dim=1, descending=True, stable=True)[1])
    # 6. round r takes the r-th of every bank, high banks first: a stable sort by the rank inside the bank
    sorted_bank = torch.gather(bank, 1, order)
    at = torch.arange(N, device=dev).expand(B, N)
    starts = torch.ones((B, N), dtype=torch.bool, device=dev)
    starts[:, 1:] = sorted_bank[:, 1:] != sorted_bank[:, :-1]
    rank = at - torch.cummax(torch.where(starts, at, torch.zeros_like(at)), 1)[0]
    rank = torch.where(sorted_bank == -2, torch.full_like(rank, N), rank)
    chosen = torch.gather(order, 1, torch.sort(rank, dim=1, stable=True)[1][:, :k])
    # 7. outputs
    sel_beam, sel_word = torch.gather(row, 1, chosen), torch.gather(word, 1, chosen)
    col = sel_beam.unsqueeze(-1)
    new_mask = torch.gather(alive, 1, col)
    picked = torch.gather(torch.gather(word_logprob, 1, col.expand(B, k, V)), 2, sel_word.unsqueeze(-1)) * new_mask
    return sel_beam, sel_word, torch.gather(score, 1, chosen).unsqueeze(-1), new_mask, picked, torch.gather(new_met, 1, chosen)


def supported_forced(word_logprobs, cur_beam, beam_size):
    """The step with forced words runs on the device kernel: what `supported_mean` asks of the maps, one or beam_size source rows
    and a vocabulary of at least beam_size words."""
    return (supported_mean(word_logprobs, cur_beam, beam_size) and cur_beam in (1, beam_size)
            and word_logprobs[0].shape[-1] >= beam_size)


def beam_step_forced(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, force_words, met=None, history=None, t=0,
                     con=None):
    """The step with forced words of one map or of the mean of several on the device (two launches, nothing uploaded): force_words
    [B, C, W] int64 and met [B, cur_beam] int32 (None: the first step) are device tensors.  Returns the five outputs of `beam_step`
    and new_met [B, beam] int32, or None when the call is outside the kernel's limits (a beam above 8, fewer words than beams, more
    than 8 sets or 4 words a set, and the limits of `beam_step_con`): the caller uses `beam_step_forced_host`."""
    return _step(word_logprobs, seq_logprob, seq_mask, prev_words, eos_idx, beam_size, con, history, t, force_words=force_words,
                 met=met)


# ------------------------------------------------------------------------------------------------------ the decoders' choice
def fused_step(maps, state, constraints, groups, force_words, met, history, timestep):
    """The device step of a decoder, Transformer.iter (one map) and Ensemble.iter (one per member) alike: `state` is (seq_logprob,
    seq_mask, prev_words, eos_idx, beam_size) with mask and words None at the first step, `history` [B, cur_beam, t] or None.
    Returns what the chosen front returns, or None where the maps or the limits keep the step off the kernel: the caller then
    takes the composed form."""
    cur_beam, beam_size = maps[0].shape[1], state[-1]
    if force_words is not None:
        if supported_forced(maps, cur_beam, beam_size):
            return beam_step_forced(maps, *state, force_words, met, history, timestep, constraints)
    elif groups is not None:
        if supported_div(maps, cur_beam, beam_size, groups.num_groups):
            return beam_step_div(maps, *state, *groups, history, timestep, constraints)
    elif supported_mean(maps, cur_beam, beam_size):
        if constraints is not None:
            return beam_step_con(maps, *state, history, timestep, constraints)
        return beam_step_mean(maps, *state)
    return None
