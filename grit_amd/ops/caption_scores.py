"""The evaluation's caption scores on the device (grit_caption_scores, include/grit_hip.h): the token ids beam search left on the
device in, BLEU-1..4, ROUGE-L and CIDEr of the split out.  METEOR (a Java program outside the reference tree) is not computed.

`DeviceCaptionScorer` is built once per split from the references of every dataloader item in order.  It tokenises them once,
builds `Cider(tokenised)` over exactly those items -- which IS the call-local statistics of the reference's `Cider()` when the
call scores that split -- and reuses `DeviceCider` (grit_amd/ops/cider.py) for the word tables, the idf trie and the cooked
references, with `score_tables=True` for the per-reference term frequencies, word counts and token sequences.

Two calls, so that the device work carries no synchronisation:
  * `launch(tokens [N, T])` -> (comps int32 [N, 10], rouge float64 [N], cider float64 [N]) on the device;
  * `aggregate(comps, rouge, cider)` -> {'BLEU': [b1..b4], 'ROUGE': r, 'CIDEr': c}: one device-to-host copy, then the corpus
    formulas of the host oracles (datasets/caption/metrics/{bleu,rouge,cider}.py) in their order.

The evaluation collapses repeated WORDS before it tokenises; the kernel collapses repeated word IDS.  The two agree only if no
two ids share a word, so a vocabulary with a duplicated word is refused."""
import ctypes
import itertools

import numpy as np
import torch

from grit_amd import lib as _lib
from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
from grit_amd.datasets.caption.metrics.bleu import bleu_from_components
from grit_amd.datasets.caption.metrics.rouge import BETA
from grit_amd.ops.cider import DeviceCider

C = _lib.SCORE_COMPONENTS


class DeviceCaptionScorer(object):
    """caption_lists: the references of every item of one split, in dataloader order (item i of `launch`'s rows is scored
    against caption_lists[i]).  `device` may be the CPU: the tables are then only packed (tests walk them)."""

    def __init__(self, caption_lists, itos, eos_token='<eos>', device='cuda'):
        itos = list(itos)
        seen, twice = set(), []
        for w in itos:
            if w in seen:
                twice.append(w)
            seen.add(w)
        if twice:
            raise ValueError("these words have more than one id, so collapsing repeated ids is not collapsing repeated words: %s"
                             % ', '.join(repr(w) for w in twice[:20]))
        caption_lists = [list(caps) for caps in caption_lists]
        if not caption_lists or any(len(caps) == 0 for caps in caption_lists):
            raise ValueError("every item needs at least one reference caption")
        self.gts = PTBTokenizer.tokenize({i: caps for i, caps in enumerate(caption_lists)})
        self.tables = DeviceCider(Cider(self.gts), itos, eos_token=eos_token, device=device, score_tables=True)
        self.device = self.tables.device
        # (items with the same references share a slot; the references are not tokenised a second time)
        self.slots = self.tables.reference_slots(caption_lists, sentences=[self.gts[i] for i in range(len(caption_lists))])
        self.slot_index = torch.tensor(self.slots, dtype=torch.int32).to(self.device)
        self.empty_token = self.tables._tid('')
        self.eos_id = itos.index(eos_token) if eos_token in itos else None
        self.beta2 = BETA ** 2
        self._ext = None
        t = self.tables
        self.stats = dict(t.stats, items=len(self.slots), slots=t.n_slots, references=t.ref_len.n, entries=t.ent_w.n,
                          reference_bytes=int(t.ent_tok.n * 16 + t.ent_w.n * 8 + t.ent_tf.n * 4 + t.ref_norm.n * 32 + t.ref_len.n * 4 +
                                              t.ref_words.n * 4 + t.seq_start.n * 4 + t.seq_tok.n * 4))

    def __len__(self):
        return len(self.slots)

    # ---- host mirror of the kernel's first two steps ------------------------------------------------------------------------
    def expand(self, ids, collapse=True):
        """Word ids of one row -> token ids of the tokenised caption, with the evaluation's collapse of repeated words."""
        ids = [int(w) for w in ids]
        meta = self.tables._meta_host
        cut = next((t for t, w in enumerate(ids) if meta[w] & _lib.CIDER_META_EOS), len(ids))
        ids = ids[:cut]
        if collapse:
            ids = [w for w, _ in itertools.groupby(ids)]
        return self.tables.expand(ids)

    # ---- the launch ---------------------------------------------------------------------------------------------------------
    def _ext_struct(self):
        if self._ext is None:
            t, ext = self.tables, _lib.ScoreTables()
            ext.ent_tf, ext.ref_words = t.ent_tf.t.data_ptr(), t.ref_words.t.data_ptr()
            ext.seq_start, ext.seq_tok = t.seq_start.t.data_ptr(), t.seq_tok.t.data_ptr()
            ext.empty_tok, ext.beta2 = self.empty_token, self.beta2
            self._ext = ext
        return self._ext

    def launch(self, tokens, collapse=True, first=0):
        """tokens [N, T] int64 on the device, row i against the references of item first + i -> (comps [N, 10] int32,
        rouge [N] float64, cider [N] float64) on the device.  No synchronisation, no allocation on the host."""
        _lib.require_device(tokens)
        if tokens.dim() != 2 or tokens.dtype != torch.int64:
            raise _lib.GritHipError("caption scores: tokens must be [N, T] int64")
        N, T = tokens.shape
        if first < 0 or first + N > len(self.slots):
            raise _lib.GritHipError("caption scores: rows %d..%d of a split of %d items" % (first, first + N, len(self.slots)))
        if tokens.device != self.device:
            raise _lib.GritHipError("caption scores: tokens on %s, tables on %s" % (tokens.device, self.device))
        tok = tokens if tokens.is_contiguous() else tokens.contiguous()
        index = self.slot_index[first:first + N]
        comps = torch.empty((N, C), dtype=torch.int32, device=self.device)
        rouge = torch.empty(N, dtype=torch.float64, device=self.device)
        cider = torch.empty(N, dtype=torch.float64, device=self.device)
        L = _lib.load()
        p = _lib.ptr
        with _lib.device_guard(self.device):
            st = L.grit_caption_scores(p(tok), N, T, p(index), 1 if collapse else 0,
                                       ctypes.c_void_p(ctypes.addressof(self.tables._table_struct())),
                                       ctypes.c_void_p(ctypes.addressof(self._ext_struct())), p(comps), p(rouge), p(cider),
                                       _lib.current_stream_ptr())
        _lib.check(st, "grit_caption_scores")
        return comps, rouge, cider

    @staticmethod
    def aggregate(comps, rouge, cider):
        """One device-to-host copy, then the corpus formulas in the host oracles' order."""
        N = comps.shape[0]
        packed = torch.empty((N, C + 4), dtype=torch.int32, device=comps.device)  # 56 bytes per caption, one copy
        packed[:, :C] = comps
        packed[:, C:C + 2] = rouge.view(N, 1).view(torch.int32)
        packed[:, C + 2:] = cider.view(N, 1).view(torch.int32)
        host = packed.cpu().numpy()
        return aggregate_host(host[:, :C], np.ascontiguousarray(host[:, C:C + 2]).view(np.float64)[:, 0],
                              np.ascontiguousarray(host[:, C + 2:]).view(np.float64)[:, 0])

    def score(self, tokens, collapse=True):
        return self.aggregate(*self.launch(tokens, collapse))


def aggregate_host(comps, rouge, cider):
    """comps [N, 10] integers, rouge / cider [N] float64 (numpy) -> the scores dictionary."""
    if (comps < 0).any() or np.isnan(rouge).any() or np.isnan(cider).any():
        bad = np.nonzero((comps < 0).any(axis=1) | np.isnan(rouge) | np.isnan(cider))[0]
        raise ValueError("caption scores: rows %s hold a word id outside the vocabulary or an unknown reference slot" % bad[:10].tolist())
    sums = [int(x) for x in comps.astype(np.int64).sum(axis=0)]
    # plain Python floats: the dictionary goes into checkpoints that are read back with torch.load's weights-only default
    return {'BLEU': [float(b) for b in bleu_from_components(sums[0], sums[1], sums[2:6], sums[6:10])],
            'ROUGE': float(np.mean(np.array(rouge))), 'CIDEr': float(np.mean(np.array(cider)))}
