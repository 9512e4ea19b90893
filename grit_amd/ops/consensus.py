"""Consensus (minimum-Bayes-risk) reranking of an image's candidate captions under CIDEr-D (Devlin et al. 2015): keep the candidate
that agrees most with the others.  The references of a candidate are the OTHER candidates of its image, and the result is an argmax.

    caption_i      the words of row i in front of the first <eos>; with `collapse` every word equal to its predecessor is dropped
                   (the evaluation's itertools.groupby); then tokenised by the project's tokenizer
    v_i            cider.cook([caption_i])[0]
    sim[b, i, j]   cider._similarity(v_i, v_j) for i != j (i the hypothesis, j the reference: the clipping min(w_h, w_r) * w_r makes
                   it asymmetric), 0.0 for i == j
    score[b, i]    (sum over j != i, j ascending, of sim[b, i, j]) / (n - 1) * 10.0, a sequential float64 sum; 0.0 for n == 1.  It is
                   cider.compute_score({0: [captions j != i]}, {0: [caption_i]})[1][0]
    best[b]        the smallest i whose score is maximal

`consensus_host` states this with the project's own `Cider` and tokenizer and is the yardstick of the device tests.
`device_consensus` (also `DeviceCider.consensus`) is grit_cider_consensus (include/grit_hip.h, grit_amd/csrc/consensus.hip): two
launches on the token ids where decoding left them, no copy to the host, no tokenisation, no synchronisation.  All candidates weigh
the same; there is no utility other than CIDEr-D."""
import collections
import ctypes
import itertools

import numpy as np
import torch

from grit_amd import lib as _lib
from grit_amd.datasets.caption.metrics import PTBTokenizer

MAX_CANDIDATES = _lib.CONSENSUS_MAX_CANDIDATES

Consensus = collections.namedtuple('Consensus', 'tokens log_probs score best bad score64 sim')
Consensus.__doc__ = """What `device_consensus` returns, all on the device: tokens [B, 1, T] and log_probs [B, 1, T] (None when none
were passed) = the rows best[b]; score [B, n] float32; best [B] int64; bad [B] int32 (1: a word id outside the vocabulary in front of
<eos> in some candidate of the image: its scores are NaN and best is 0); score64 [B, n] and sim [B, n, n] float64 when asked for."""


def candidate_captions(itos, tokens, eos_token='<eos>', collapse=True):
    """tokens [B, n, T] integers -> [B][n] strings: the words in front of the first <eos>, repeated words collapsed, joined by one
    space.  A word id outside the vocabulary in front of the cut raises ValueError."""
    rows = tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else np.asarray(tokens)
    if rows.ndim != 3:
        raise ValueError("consensus: tokens must be [B, n, T], not %r" % (tuple(rows.shape),))
    out = []
    for b, image in enumerate(rows.tolist()):
        captions = []
        for i, row in enumerate(image):
            words = []
            for w in row:
                if not 0 <= w < len(itos):
                    raise ValueError("consensus: word id %d of image %d, candidate %d is outside the vocabulary of %d words"
                                     % (w, b, i, len(itos)))
                if itos[w] == eos_token:
                    break
                words.append(itos[w])
            if collapse:
                words = [w for w, _ in itertools.groupby(words)]
            captions.append(' '.join(words))
        out.append(captions)
    return out


def consensus_host(cider, itos, tokens, eos_token='<eos>', collapse=True, tokenize=None):
    """tokens [B, n, T] -> (sim [B, n, n] float64, score [B, n] float64, best [B] int64) as numpy arrays: the definition of the
    module's docstring, composed of text decoding, `tokenize` (default PTBTokenizer.tokenize), Cider.cook and Cider._similarity."""
    if getattr(cider, 'doc_frequency', None) is None or cider.ref_len is None:
        raise ValueError("consensus needs a Cider built with corpus statistics (Cider(gts))")
    tokenize = PTBTokenizer.tokenize if tokenize is None else tokenize
    captions = candidate_captions(itos, tokens, eos_token, collapse)
    B, n = len(captions), len(captions[0]) if captions else 0
    sim = np.zeros((B, n, n), np.float64)
    score = np.zeros((B, n), np.float64)
    best = np.zeros(B, np.int64)
    for b in range(B):
        vecs = cider.cook(tokenize({0: captions[b]})[0])
        for i in range(n):
            total = 0.0
            for j in range(n):
                if j != i:
                    sim[b, i, j] = cider._similarity(vecs[i], vecs[j])
                    total += sim[b, i, j]
            score[b, i] = total / (n - 1) * 10.0 if n > 1 else 0.0
        for i in range(1, n):
            if score[b, i] > score[b, best[b]]:
                best[b] = i
    return sim, score, best


def _duplicated_words(itos):
    seen, twice = set(), []
    for w in itos:
        if w in seen:
            twice.append(w)
        seen.add(w)
    return twice


def device_consensus(tables, tokens, log_probs=None, collapse=True, return_matrix=False):
    """tables: a DeviceCider (it need not have cooked any reference); tokens [B, n, T] int64 and log_probs [B, n, T] (optional) on
    its device -> Consensus.  The kernel collapses repeated word IDS where the host form collapses repeated WORDS, so with `collapse`
    a vocabulary that holds a word twice is refused.  n > MAX_CANDIDATES or T beyond the reward's limit raises: there is no
    fall-back; `consensus_host` is public for a caller that wants one."""
    _lib.require_device(tokens, log_probs)
    if tokens.dim() != 3 or tokens.dtype != torch.int64:
        raise _lib.GritHipError("consensus: tokens must be [B, n, T] int64")
    if log_probs is not None and log_probs.shape != tokens.shape:
        raise _lib.GritHipError("consensus: log_probs %r for tokens %r" % (tuple(log_probs.shape), tuple(tokens.shape)))
    if tokens.device != tables.device:
        raise _lib.GritHipError("consensus: tokens on %s, tables on %s" % (tokens.device, tables.device))
    if collapse:
        twice = tables.__dict__.get('_duplicated')
        if twice is None:
            twice = tables.__dict__['_duplicated'] = _duplicated_words(tables.itos)
        if twice:
            raise ValueError("these words have more than one id, so collapsing repeated ids is not collapsing repeated words: %s"
                             % ', '.join(repr(w) for w in twice[:20]))
    B, n, T = tokens.shape
    dev = tables.device
    tok = tokens if tokens.is_contiguous() else tokens.contiguous()
    L = _lib.load()
    size = L.grit_cider_consensus_workspace(B, n, T) if B > 0 else 0
    workspace = torch.empty(max(size, 1), dtype=torch.uint8, device=dev)
    score64 = torch.empty((B, n), dtype=torch.float64, device=dev)
    score32 = torch.empty((B, n), dtype=torch.float32, device=dev)
    sim = torch.empty((B, n, n), dtype=torch.float64, device=dev) if return_matrix else None
    best = torch.empty(B, dtype=torch.int32, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    p = _lib.ptr
    with _lib.device_guard(dev):
        st = L.grit_cider_consensus(p(tok), B, n, T, 1 if collapse else 0, ctypes.c_void_p(ctypes.addressof(tables._table_struct())),
                                    p(sim), p(score64), p(score32), p(best), p(bad), p(workspace), _lib.current_stream_ptr())
    _lib.check(st, "grit_cider_consensus")
    best = best.long()
    index = best.view(B, 1, 1).expand(B, 1, T)
    return Consensus(torch.gather(tok, 1, index), None if log_probs is None else torch.gather(log_probs, 1, index), score32, best, bad,
                     score64 if return_matrix else None, sim)
