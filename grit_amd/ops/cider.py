"""The self-critical reward on the device (grit_cider_reward, include/grit_hip.h): generated token ids in, CIDEr-D out, with no
host round trip.  This module is the host-side packer: everything that does not depend on the hypothesis is computed once, with
the project's own tokenizer and `Cider`, and laid out for the kernel.

Why per-word tables are enough.  The host path tokenises the *joined string* of vocabulary words.  For the native tokenizer a
word's tokens do not depend on its neighbours; the one dependence on position is the sentence-final period rule.  So two tables
describe it: `mid[w]`, the tokens of w anywhere, and `fin[w]`, its tokens as the last word that is not whitespace-only.  The
constructor VERIFIES this for every word of the vocabulary (tokens of w in "w zz" equal those in "zz w zz", tokens of "w" alone
equal those in "zz w") and refuses a vocabulary for which it does not hold, naming the words.

Layout (all built here, read by grit_amd/csrc/cider.hip):
  * expansion [V, 2, E] int32 + word_meta [V]: mid / fin token ids, their counts, the blank and <eos> flags;
  * the corpus idf as a trie flattened order by order: for order k a sorted array of (index of the prefix in order k-1) << 32 | token
    keys with idf = log(corpus size) - log(max(1, df)) next to it -- exact (two n-grams never share an entry), found by one
    binary search per order;
  * the references of every image seen so far, cooked once by `Cider.cook`, CSR by slot / reference / order: token tuples
    padded to 4 with -1, tf-idf weights, the four norms and the length.  They are matched by token tuple, so a reference
    n-gram outside the corpus statistics still meets the same n-gram of a hypothesis.

With `score_tables=True` (the evaluation's scorer, grit_amd/ops/caption_scores.py) every reference additionally leaves what BLEU
and ROUGE-L need, in arrays beside the ones above (the layout grit_cider_reward reads is untouched): the raw term frequency next to
each `ent_tok` entry, the word count, and the token sequence split at single spaces (CSR; the empty string is ONE empty token).
"""
import ctypes
import math
import time

import numpy as np
import torch

from grit_amd import lib as _lib
from grit_amd.datasets.caption.metrics import cider as _cider
from grit_amd.datasets.caption.metrics import tokenizer as _tokenizer

E = _lib.CIDER_MAX_EXPANSION
_PROBE = 'zz'


def _tokens(text):
    drop = set(_tokenizer.PUNCTUATIONS)
    return [t for t in _tokenizer.ptb_tokens(text) if t not in drop]


def word_tables(itos):
    """(mid, fin, bad): per word its tokens anywhere / as the last non-blank word, and the words that break the two-table
    property or expand to more than E tokens."""
    mid, fin, bad = [], [], []
    for w in itos:
        a, b, c, d = (_tokens(s) for s in ('%s %s %s' % (_PROBE, w, _PROBE), '%s %s' % (w, _PROBE), '%s %s' % (_PROBE, w), w))
        ok = len(a) >= 2 and a[0] == _PROBE and a[-1] == _PROBE and b and b[-1] == _PROBE and c and c[0] == _PROBE
        m, f = (a[1:-1], c[1:]) if ok else ([], [])
        if not ok or b[:-1] != m or d != f or len(m) > E or len(f) > E:
            bad.append(w)
        mid.append(m)
        fin.append(f)
    return mid, fin, bad


class _Grow(object):
    """A device array that is appended to: capacity doubles, only the new part is uploaded."""

    def __init__(self, dtype, device, tail=(), first=None):
        self.dtype, self.device, self.tail, self.n = dtype, device, tuple(tail), 0
        self.t = torch.empty((1024,) + self.tail, dtype=dtype, device=device)
        if first is not None:
            self.append(first)

    def append(self, array):
        src = torch.as_tensor(np.ascontiguousarray(array)).to(self.dtype).reshape((-1,) + self.tail)
        need = self.n + src.shape[0]
        if need > self.t.shape[0]:
            grown = torch.empty((max(need, 2 * self.t.shape[0]),) + self.tail, dtype=self.dtype, device=self.device)
            grown[:self.n].copy_(self.t[:self.n])
            self.t = grown
        self.t[self.n:need].copy_(src)
        self.n = need

    def numpy(self):
        return self.t[:self.n].cpu().numpy()


class DeviceCider(object):
    """CIDEr-D of beam tokens against an image's references on the device.

    cider: a `Cider` built WITH corpus statistics (the call-local statistics form stays host-only); itos: the vocabulary;
    ids whose word equals `eos_token` end a row, as in the reference's TextField.decode.  `device` may be the CPU: the tables
    are then only packed (tests walk them), `reward` needs a HIP device."""

    def __init__(self, cider, itos, eos_token='<eos>', device='cuda', verbose=False, score_tables=False):
        if getattr(cider, 'doc_frequency', None) is None or cider.ref_len is None:
            raise ValueError("DeviceCider needs a Cider built with corpus statistics (Cider(gts)); the call-local form is host-only")
        if cider._n != 4:
            raise ValueError("DeviceCider implements n-grams of orders 1..4, this Cider has n = %d" % cider._n)
        self.cider, self.itos, self.eos_token = cider, list(itos), eos_token
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.sigma, self.log_corpus = float(cider._sigma), float(cider.ref_len)
        self._tok = {}
        t0 = time.time()
        self._build_words()
        t1 = time.time()
        self._build_idf()
        t2 = time.time()
        dev = self.device
        self._slots = {}
        self.slot_ref_start = _Grow(torch.int32, dev, first=[0])
        self.ref_ent_start = _Grow(torch.int32, dev, first=[0])
        self.ent_tok = _Grow(torch.int32, dev, tail=(4,))
        self.ent_w = _Grow(torch.float64, dev)
        self.ref_norm = _Grow(torch.float64, dev, tail=(4,))
        self.ref_len = _Grow(torch.int32, dev)
        self._n_ent = 0
        self._tables = None
        self.score_tables = bool(score_tables)
        if self.score_tables:
            self.ent_tf = _Grow(torch.int32, dev)
            self.ref_words = _Grow(torch.int32, dev)
            self.seq_start = _Grow(torch.int32, dev, first=[0])
            self.seq_tok = _Grow(torch.int32, dev)
            self._n_seq = 0
        self.stats = {'vocab': len(self.itos), 'expansion_bytes': int(self.expansion.numel() * 4 + self.word_meta.numel() * 4),
                      'idf_entries': [int(b - a) for a, b in zip(self.idf_start[:-1], self.idf_start[1:])],
                      'idf_bytes': int(self.idf_key.numel() * 16), 'tokens': len(self._tok),
                      'build_words_s': round(t1 - t0, 3), 'build_idf_s': round(t2 - t1, 3)}
        if verbose:
            print('DeviceCider: %d words, %d idf entries (%.1f MB), built in %.2f s + %.2f s' %
                  (len(self.itos), sum(self.stats['idf_entries']), self.stats['idf_bytes'] / 1e6, t1 - t0, t2 - t1))

    # ---- token ids -------------------------------------------------------------------------------------------------------
    def _tid(self, token):
        i = self._tok.get(token)
        if i is None:
            i = self._tok[token] = len(self._tok)
        return i

    def token_strings(self):
        out = [None] * len(self._tok)
        for s, i in self._tok.items():
            out[i] = s
        return out

    # ---- per-word expansion ----------------------------------------------------------------------------------------------
    def _build_words(self):
        mid, fin, bad = word_tables(self.itos)
        if bad:
            raise ValueError("the native tokenizer does not treat these vocabulary words independently of their neighbours, "
                             "or expands them to more than %d tokens: %s" % (E, ', '.join(repr(w) for w in bad[:20])))
        V = len(self.itos)
        exp = np.full((V, 2, E), -1, np.int32)
        meta = np.zeros(V, np.int32)
        for i, w in enumerate(self.itos):
            for j, toks in enumerate((mid[i], fin[i])):
                exp[i, j, :len(toks)] = [self._tid(t) for t in toks]
            meta[i] = len(mid[i]) | (len(fin[i]) << _lib.CIDER_META_FIN_SHIFT)
            if w.strip() == '':
                meta[i] |= _lib.CIDER_META_BLANK
            if w == self.eos_token:
                meta[i] |= _lib.CIDER_META_EOS
        self.final_words = [w for i, w in enumerate(self.itos) if mid[i] != fin[i]]
        self._exp_host, self._meta_host = exp, meta
        self.expansion = torch.from_numpy(exp).to(self.device)
        self.word_meta = torch.from_numpy(meta).to(self.device)

    def expand(self, ids):
        """Host mirror of the kernel's first step: word ids of one row -> token ids of the tokenised caption."""
        meta, exp = self._meta_host, self._exp_host
        cut = len(ids)
        for t, w in enumerate(ids):
            if meta[w] & _lib.CIDER_META_EOS:
                cut = t
                break
        last = -1
        for t in range(cut):
            if not meta[ids[t]] & _lib.CIDER_META_BLANK:
                last = t
        out = []
        for t in range(cut):
            m = int(meta[ids[t]])
            fin = t == last
            c = (m >> _lib.CIDER_META_FIN_SHIFT) & 15 if fin else m & 15
            out.extend(int(x) for x in exp[ids[t], 1 if fin else 0, :c])
        return out

    # ---- corpus idf ------------------------------------------------------------------------------------------------------
    def _build_idf(self):
        tid = self._tid
        flat, dfs = [[] for _ in range(4)], [[] for _ in range(4)]
        for ngram, df in self.cider.doc_frequency.items():
            k = len(ngram) - 1
            flat[k].extend([tid(t) for t in ngram])
            dfs[k].append(df)
        keys, vals, start = [], [], [0]
        for k in range(4):
            toks = np.asarray(flat[k], np.int64).reshape(-1, k + 1)
            node = np.zeros(len(toks), np.int64)
            for j in range(k):  # walk the prefix through the lower orders: doc_frequency is prefix-closed by construction
                key = (node << 32) | toks[:, j]
                pos = np.searchsorted(keys[j], key)
                found = pos < len(keys[j])
                found[found] = keys[j][pos[found]] == key[found]
                if not found.all():
                    raise ValueError("doc_frequency holds an n-gram whose prefix it does not hold")
                node = pos.astype(np.int64)
            key = (node << 32) | toks[:, k]
            order = np.argsort(key, kind='stable')
            key = key[order]
            if len(key) > 1 and not (key[1:] > key[:-1]).all():
                raise ValueError("doc_frequency holds an n-gram twice")
            # idf in float64 with _Vec's own expression; math.log per DISTINCT document frequency so that it is libm's value
            df = np.asarray(dfs[k], np.float64)[order]
            uniq, inv = np.unique(df, return_inverse=True)
            logs = np.asarray([math.log(max(1.0, float(u))) for u in uniq], np.float64)
            idf = np.asarray([self.log_corpus - v for v in logs], np.float64)[inv] if len(df) else np.zeros(0, np.float64)
            keys.append(key)
            vals.append(idf)
            start.append(start[-1] + len(key))
        self.idf_start = start
        allk = np.concatenate(keys) if start[-1] else np.zeros(0, np.int64)
        allv = np.concatenate(vals) if start[-1] else np.zeros(0, np.float64)
        pad = 1 if start[-1] == 0 else 0  # never hand the kernel a null pointer
        self.idf_key = torch.from_numpy(np.concatenate([allk, np.zeros(pad, np.int64)])).to(self.device)
        self.idf_val = torch.from_numpy(np.concatenate([allv, np.zeros(pad, np.float64)])).to(self.device)

    # ---- references ------------------------------------------------------------------------------------------------------
    def reference_slots(self, captions, sentences=None):
        """One slot per image of `captions` (a list of caption lists, batch['captions']).  An image seen before costs one
        dictionary lookup; a new one is tokenised and cooked on the host, once, and appended to the device arrays.
        `sentences`: the captions of every image already tokenised (PTBTokenizer.tokenize), for a caller that has them."""
        slots, new, given = [], {}, {}
        for i, caps in enumerate(captions):
            key = tuple(caps)
            s = self._slots.get(key)
            if s is None:
                s = new.get(key)
                if s is None:
                    s = new[key] = len(self._slots) + len(new)
                    if sentences is not None:
                        given[key] = sentences[i]
            slots.append(s)
        if new:
            self._cook(list(new), given)  # (in slot order; nothing is registered if cooking raises)
            self._slots.update(new)
        return slots

    def preload(self, caption_lists):
        for caps in caption_lists:
            self.reference_slots([caps])

    def _cook(self, images, tokenised=None):
        tid = self._tid
        ent_tok, ent_w, ent_start, norms, lens, ref_start = [], [], [], [], [], []
        ent_tf, words, seq_tok, seq_start = [], [], [], []
        n_ref = self.ref_len.n
        for caps in images:
            sentences = tokenised.get(tuple(caps)) if tokenised else None
            if sentences is None:
                sentences = _tokenizer.PTBTokenizer.tokenize([list(caps)])[0] if caps else []
            for sentence, vec in zip(sentences, self.cider.cook(sentences)):
                counts = _cider.ngram_counts(sentence) if self.score_tables else None
                for k in range(4):
                    for ngram, w in vec.weights[k].items():
                        ent_tok.append([tid(t) for t in ngram] + [-1] * (3 - k))
                        ent_w.append(w)
                        if counts is not None:
                            ent_tf.append(counts[ngram])
                    ent_start.append(self._n_ent + len(ent_w))
                norms.append(vec.norm)
                lens.append(vec.length)
                if counts is not None:
                    words.append(len(sentence.split()))
                    seq_tok.extend(tid(t) for t in sentence.split(' '))  # ROUGE's split: '' is one empty token
                    seq_start.append(self._n_seq + len(seq_tok))
            n_ref += len(sentences)
            ref_start.append(n_ref)
        self._n_ent += len(ent_w)
        if self._n_ent >= 2 ** 31:
            raise ValueError("more reference n-grams than 32-bit offsets hold")
        if lens:
            self.ent_tok.append(np.asarray(ent_tok, np.int32).reshape(-1, 4))
            self.ent_w.append(np.asarray(ent_w, np.float64))
            self.ref_ent_start.append(np.asarray(ent_start, np.int32))
            self.ref_norm.append(np.asarray(norms, np.float64))
            self.ref_len.append(np.asarray(lens, np.int32))
            if self.score_tables:
                self._n_seq += len(seq_tok)
                self.ent_tf.append(np.asarray(ent_tf, np.int32))
                self.ref_words.append(np.asarray(words, np.int32))
                self.seq_start.append(np.asarray(seq_start, np.int32))
                self.seq_tok.append(np.asarray(seq_tok, np.int32))
        self.slot_ref_start.append(np.asarray(ref_start, np.int32))
        self._tables = None

    @property
    def n_slots(self):
        return len(self._slots)

    def host_arrays(self):
        """The packed arrays as numpy (tests walk them)."""
        extra = {k: getattr(self, k).numpy() for k in ('ent_tf', 'ref_words', 'seq_start', 'seq_tok')} if self.score_tables else {}
        return {**extra, 'expansion': self._exp_host, 'word_meta': self._meta_host, 'idf_key': self.idf_key.cpu().numpy(),
                'idf_val': self.idf_val.cpu().numpy(), 'idf_start': list(self.idf_start),
                'slot_ref_start': self.slot_ref_start.numpy(), 'ref_ent_start': self.ref_ent_start.numpy(),
                'ent_tok': self.ent_tok.numpy(), 'ent_w': self.ent_w.numpy(), 'ref_norm': self.ref_norm.numpy(),
                'ref_len': self.ref_len.numpy(), 'sigma': self.sigma, 'log_corpus': self.log_corpus}

    # ---- the launch ------------------------------------------------------------------------------------------------------
    def _table_struct(self):
        if self._tables is None:
            p = lambda t: t.data_ptr()
            tab = _lib.CiderTables()
            tab.expansion, tab.word_meta, tab.vocab, tab.width = p(self.expansion), p(self.word_meta), len(self.itos), E
            tab.idf_key, tab.idf_val = p(self.idf_key), p(self.idf_val)
            tab.idf_start = (ctypes.c_long * 5)(*self.idf_start)
            tab.slot_ref_start, tab.n_slots = p(self.slot_ref_start.t), self.n_slots
            tab.ref_ent_start, tab.ent_tok, tab.ent_w = p(self.ref_ent_start.t), p(self.ent_tok.t), p(self.ent_w.t)
            tab.ref_norm, tab.ref_len = p(self.ref_norm.t), p(self.ref_len.t)
            tab.sigma, tab.log_corpus = self.sigma, self.log_corpus
            self._tables = tab
        return self._tables

    def reward(self, tokens, captions, return_float64=False):
        """tokens [B, beam, T] int64 on the device, captions = batch['captions'] (B lists) -> [B, beam] float32 on the device
        (and the float64 scores when asked).  No synchronisation once every image of the batch has been seen."""
        _lib.require_device(tokens)
        if tokens.dim() != 3 or tokens.dtype != torch.int64:
            raise _lib.GritHipError("cider reward: tokens must be [B, beam, T] int64")
        B, beam, T = tokens.shape
        if len(captions) != B:
            raise _lib.GritHipError("cider reward: %d caption lists for %d images" % (len(captions), B))
        if tokens.device != self.device:
            raise _lib.GritHipError("cider reward: tokens on %s, tables on %s" % (tokens.device, self.device))
        slots = self.reference_slots(captions)
        tok = tokens if tokens.is_contiguous() else tokens.contiguous()
        index = torch.tensor(slots, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        out32 = torch.empty((B, beam), dtype=torch.float32, device=self.device)
        out64 = torch.empty((B, beam), dtype=torch.float64, device=self.device) if return_float64 else None
        L = _lib.load()
        with _lib.device_guard(self.device):
            st = L.grit_cider_reward(ctypes.c_void_p(tok.data_ptr()), B * beam, T, ctypes.c_void_p(index.data_ptr()), beam,
                                     ctypes.c_void_p(ctypes.addressof(self._table_struct())), ctypes.c_void_p(out32.data_ptr()),
                                     ctypes.c_void_p(out64.data_ptr() if out64 is not None else 0), _lib.current_stream_ptr())
        _lib.check(st, "grit_cider_reward")
        return (out32, out64) if return_float64 else out32

    def consensus(self, tokens, log_probs=None, collapse=True, return_matrix=False):
        """Consensus reranking of the n candidates of every image under CIDEr-D (grit_amd/ops/consensus.py: device_consensus):
        tokens [B, n, T] int64 on the device -> Consensus(tokens [B, 1, T], log_probs, score [B, n] float32, best [B], bad [B],
        score64, sim).  It reads the word tables and the idf trie only, so no reference needs to have been cooked."""
        from grit_amd.ops.consensus import device_consensus
        return device_consensus(self, tokens, log_probs, collapse, return_matrix)
