"""GRIT captioner: detector -> grid network -> caption decoder; teacher forcing and beam search.

Mirror of reference models/caption/transformer.py (Transformer.__init__ :14-51, forward :53-132, step :134-169,
select :184-188, _expand_state :190-202, iter :204-254).  The beam loop keeps the reference's observable
semantics to the token: always `max_len` steps, candidates = running score + word log-prob,
a finished beam keeps its score only at vocabulary index 0 (-999 elsewhere), selection = descending torch.sort of
the flattened [beam*V] candidates, beam = index // V, every registered state is re-gathered per step, final beams
re-sorted by score.
"""
import collections
import ctypes
import os
from contextlib import contextmanager

import torch
from torch import nn

from grit_amd import lib as _lib
from grit_amd.models.caption.base import BaseCaptioner
from grit_amd.ops import backend
from grit_amd.ops import beam as beam_ops
from grit_amd.ops import sample as sample_ops
from grit_amd.ops import vocab_score as vocab_score_ops
from grit_amd.models.caption.cap_generator import CaptionGenerator
from grit_amd.models.caption.grid_net import GridFeatureNetwork
from grit_amd.utils.misc import NestedTensor


# GRIT_GRAPH_DECODE=0: never replay beam search from a captured HIP graph (A/B knob, tools/bench_decode.py)
_GRAPH_DECODE = os.environ.get('GRIT_GRAPH_DECODE', '1') != '0'
# GRIT_FUSED_BEAM_STEP=0: the candidate / selection / gather arithmetic of a beam step as separate torch ops + grit_topk_rows_f32
_FUSED_BEAM_STEP = os.environ.get('GRIT_FUSED_BEAM_STEP', '1') != '0'


# What `score` returns: log_probs [B, N, T - 1] float32 (0 at pad targets), total [B, N] = their sum (divided by `length` under
# normalize='mean'), length [B, N] int64 = the number of targets that are not pad
CaptionScores = collections.namedtuple('CaptionScores', 'log_probs total length')


def check_score_call(module, captions, normalize):
    """The argument checks shared by Transformer.score and Ensemble.score -> captions as [B, N, T]."""
    if module.training or torch.is_grad_enabled():
        raise RuntimeError("score() measures a trained model: call model.eval() and run it under torch.no_grad() or "
                           "torch.inference_mode() (the training loss is model(samples, captions) + NLLLoss)")
    if normalize not in (None, 'mean'):
        raise ValueError("normalize must be None or 'mean', not %r" % (normalize,))
    if not isinstance(captions, torch.Tensor) or captions.dtype != torch.int64 or captions.dim() not in (2, 3):
        raise ValueError("captions must be an int64 tensor [B, T] or [B, N, T]: <bos>, words, <eos>, then pad")
    if captions.dim() == 2:
        captions = captions.unsqueeze(1)
    if captions.shape[-1] < 2 or captions.shape[1] < 1:
        raise ValueError("captions need at least <bos> and one target per row, got shape %s" % (tuple(captions.shape),))
    return captions


def finish_scores(log_probs, captions, pad_idx, normalize):
    """log_probs [B, N, T - 1] (0 at pad targets) -> CaptionScores."""
    length = (captions[..., 1:].to(log_probs.device) != pad_idx).sum(-1)
    total = log_probs.sum(-1)
    if normalize == 'mean':
        total = total / length
    return CaptionScores(log_probs, total, length)


class BeamSearchSteps(object):
    """Beam bookkeeping shared by Transformer and Ensemble (models/caption/ensemble.py): the search object keeps seq_mask,
    seq_logprob, log_probs, selected_words (and all_log_probs) of the running search; `members` are the captioners whose
    registered states follow the surviving beams (the Transformer itself, or every model of an ensemble)."""

    def _beam_result(self, outputs, batch_size, beam_size, max_len, out_size, return_probs, eos_idx=None, length_penalty=0.0,
                     met=None):
        outputs = torch.cat(outputs, -1)
        scores = self.seq_logprob
        if length_penalty != 0:
            # the final ranking only: score / L^alpha, L = words up to and including the first <eos> (max_len without one)
            is_eos = outputs == eos_idx
            length = torch.where(is_eos.any(-1), is_eos.long().argmax(-1) + 1, torch.full_like(outputs[..., 0], max_len))
            scores = scores / length.float().pow(float(length_penalty)).unsqueeze(-1)
        _, order = torch.sort(scores, 1, descending=True)
        if met is not None:
            # forced words: the hypotheses that met more sets first, inside a count by the score as before (met [B, beam] int32)
            count = ((met.unsqueeze(-1) >> torch.arange(beam_ops.MAX_FORCED_SETS, device=met.device)) & 1).sum(-1)
            _, by_count = torch.sort(torch.gather(count, 1, order.squeeze(-1)), dim=1, descending=True, stable=True)
            order = torch.gather(order, 1, by_count.unsqueeze(-1))
        idx = order.expand(batch_size, beam_size, max_len)
        outputs = torch.gather(outputs, 1, idx)
        log_probs = torch.gather(torch.cat(self.log_probs, -1), 1, idx)
        outputs, log_probs = outputs.contiguous()[:, :out_size], log_probs.contiguous()[:, :out_size]
        if out_size == 1:
            outputs, log_probs = outputs.squeeze(1), log_probs.squeeze(1)
        if not return_probs:
            return outputs, log_probs
        all_lp = torch.cat(self.all_log_probs, 2)
        all_lp = torch.gather(all_lp, 1, order.unsqueeze(-1).expand(batch_size, beam_size, max_len, all_lp.shape[-1]))
        return outputs, log_probs, all_lp

    def select(self, t, candidate_logprob, beam_size, **kwargs):
        """[B, Beam, V] -> the `beam_size` best of the flattened candidates, best first.  The reference takes the head of
        a full descending torch.sort over beam*V = 51 005 scores per image per step (transformer.py:184-188); the selection
        kernel (grit_topk_rows_f32: one workgroup per image, the row read once) returns the same values in the same order --
        the order among exactly tied scores is unspecified in the reference and is by ascending index here."""
        flat = candidate_logprob.reshape(candidate_logprob.shape[0], -1)
        if flat.is_cuda and flat.dtype == torch.float32 and beam_size <= 8 and not flat.requires_grad \
                and backend.override() is None:
            flat = flat if flat.stride(1) == 1 else flat.contiguous()
            idx = torch.empty((flat.shape[0], beam_size), dtype=torch.int64, device=flat.device)
            logprob = torch.empty((flat.shape[0], beam_size), dtype=torch.float32, device=flat.device)
            with _lib.device_guard(flat.device):
                st = _lib.load().grit_topk_rows_f32(ctypes.c_void_p(flat.data_ptr()), flat.stride(0), flat.shape[0],
                                                    flat.shape[1], beam_size, ctypes.c_void_p(idx.data_ptr()),
                                                    ctypes.c_void_p(logprob.data_ptr()), _lib.current_stream_ptr())
            _lib.check(st, "grit_topk_rows_f32")
            return idx, logprob
        # with gradient (self-critical training), on the CPU (oracle runs) and for wide beams: the library selection
        logprob, idx = torch.topk(flat, beam_size, dim=-1, largest=True, sorted=True)
        return idx, logprob

    def _expand_state(self, selected_beam, cur_beam_size, batch_size, beam_size):
        """state [B*cur_beam, ...] -> rows of the surviving beams [B*beam, ...]."""

        def fn(tensor):
            tail = [int(s) for s in tensor.shape[1:]]
            index = selected_beam.view(batch_size, beam_size, *([1] * len(tail))).expand(batch_size, beam_size, *tail)
            picked = torch.gather(tensor.view(batch_size, cur_beam_size, *tail), 1, index)
            return picked.view(-1, *tail)

        return fn

    def _beam_advance(self, members, timestep, word_logprob, fused, outputs, return_probs, batch_size, beam_size, eos_idx,
                      constraints=None, groups=None, force_words=None, **kwargs):
        """The body of `iter` after the word log-probabilities word_logprob [B, cur_beam, V]: `fused` holds what the fused step
        returned (sel_beam, sel_word, seq_logprob, seq_mask, picked), or is None for the composed torch form.  `constraints`
        (ops/beam.py) bans words per live beam; `outputs` then holds the history as one tensor (`_history`).  `groups`
        (ops/beam.py: Groups) makes it the step of a diverse search, whose composed form is beam_step_groups_host.  `force_words`
        [B, C, W] makes it the step of a search with forced words: `fused` then ends with the new mask of met sets, which the search
        object carries as `met` [B, beam] like seq_mask, and the composed form is beam_step_forced_host."""
        cur_beam = 1 if timestep == 0 else beam_size
        if force_words is not None:
            if fused is None:
                state = (self.seq_logprob, self.seq_mask if timestep > 0 else None, self.selected_words if timestep > 0 else None)
                fused = beam_ops.beam_step_forced_host(word_logprob, *state, eos_idx, beam_size, force_words,
                                                       self.met if timestep > 0 else None, outputs[0] if outputs else None, timestep,
                                                       constraints)
                if return_probs and timestep > 0:  # the plain composed form records the maps of finished beams as zeros
                    word_logprob = word_logprob * (self.seq_mask * (self.selected_words.view(batch_size, cur_beam, 1) != eos_idx).float())
            fused, self.met = fused[:5], fused[5]
        if fused is None and groups is not None:
            state = (self.seq_logprob, self.seq_mask if timestep > 0 else None, self.selected_words if timestep > 0 else None)
            fused = beam_ops.beam_step_groups_host(word_logprob, *state, eos_idx, beam_size, *groups,
                                                   outputs[0] if outputs else None, timestep, constraints)
            if return_probs and timestep > 0:  # the plain composed form records the maps of finished beams as zeros
                word_logprob = word_logprob * (self.seq_mask * (self.selected_words.view(batch_size, cur_beam, 1) != eos_idx).float())
        if fused is not None:
            selected_beam, selected_words, seq_logprob, seq_mask, picked = fused
        else:
            V = word_logprob.shape[-1]
            candidates = self.seq_logprob + word_logprob
            if timestep > 0:
                alive = (self.selected_words.view(batch_size, cur_beam) != eos_idx).float().unsqueeze(-1)
                self.seq_mask = self.seq_mask * alive
                word_logprob = word_logprob * self.seq_mask
                frozen = self.seq_logprob.expand_as(candidates).contiguous()
                frozen[:, :, 1:] = -999  # a finished beam survives only through vocabulary index 0
                candidates = self.seq_mask * candidates + frozen * (1 - self.seq_mask)
            if constraints is not None:
                history = outputs[0] if outputs else candidates.new_zeros(candidates.shape[:2] + (0,), dtype=torch.long)
                banned = beam_ops.banned_words_host(history, self.seq_mask if timestep > 0 else None, timestep, eos_idx, V,
                                                    **constraints._asdict())
                candidates = candidates.masked_fill(banned, float('-inf'))

            selected_idx, selected_logprob = self.select(timestep, candidates, beam_size, **kwargs)
            selected_beam = torch.div(selected_idx, V, rounding_mode='floor')
            selected_words = selected_idx - selected_beam * V

        for m in members:
            m._follow_beams(selected_beam, cur_beam, batch_size, beam_size)

        beam_col = selected_beam.unsqueeze(-1)
        if fused is not None:
            self.seq_logprob, self.seq_mask = seq_logprob, seq_mask
        else:
            self.seq_logprob = selected_logprob.unsqueeze(-1)
            self.seq_mask = torch.gather(self.seq_mask, 1, beam_col)
        # the history of every surviving beam moves with it: ONE gather of the concatenated columns instead of one per past
        # step (the lists hold a single [B, beam, t] tensor from step 1 on)
        if outputs:
            hist = outputs[0] if len(outputs) == 1 else torch.cat(outputs, -1)
            outputs = [torch.gather(hist, 1, beam_col.expand(batch_size, beam_size, hist.shape[-1]))]
        outputs.append(selected_words.unsqueeze(-1))
        if return_probs:
            lp = word_logprob.expand((batch_size, beam_size, -1)) if timestep == 0 else word_logprob
            self.all_log_probs.append(lp.unsqueeze(2))
        if fused is None:
            picked = torch.gather(word_logprob, 1, beam_col.expand(batch_size, beam_size, V))
            picked = torch.gather(picked, 2, selected_words.unsqueeze(-1))
        if self.log_probs:
            hist = self.log_probs[0] if len(self.log_probs) == 1 else torch.cat(self.log_probs, -1)
            self.log_probs = [torch.gather(hist, 1, beam_col.expand(batch_size, beam_size, hist.shape[-1]))]
        self.log_probs.append(picked)
        self.selected_words = selected_words.view(-1, 1)
        return outputs

    @staticmethod
    def _history(outputs):
        """The token history [B, cur_beam, t] as the one tensor that a constrained step reads: the concatenation that
        `_beam_advance` would do for its gather, done ahead of the step (and then not again)."""
        return [torch.cat(outputs, -1)] if len(outputs) > 1 else outputs


class Transformer(BeamSearchSteps, BaseCaptioner):

    def __init__(self, detector, config=None):
        super().__init__()
        self._decode_graphs = {}
        m = config.model
        # d_model 512 / 8 heads / d_ff 2048 are the constructor defaults on purpose: the reference never forwards
        # config.model.n_heads, grid_net.n_memories or cap_generator.decoder_name
        self.grid_net = GridFeatureNetwork(n_layers=m.grid_net.n_layers, d_in=m.grid_feat_dim, dropout=m.dropout)
        self.cap_generator = CaptionGenerator(n_layers=m.cap_generator.n_layers, vocab_size=m.vocab_size,
                                              max_len=m.max_len, pad_idx=m.pad_idx, dropout=m.dropout,
                                              cfg=m.cap_generator)
        self.config = config
        self.bos_idx = m.bos_idx
        self.use_reg_feat, self.use_gri_feat = m.use_reg_feat, m.use_gri_feat
        self.cached_features = False
        if self.use_gri_feat:
            self.register_state('gri_feat', None)
            self.register_state('gri_mask', None)
        if self.use_reg_feat:
            self.register_state('reg_feat', None)
            self.register_state('reg_mask', None)
        self.init_weights()
        self.detector = detector  # attached after init_weights: the detector keeps its own initialisation

    def init_weights(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    # ------------------------------------------------------------------ visual side
    def _visual_inputs(self, images):
        vis = images if self.cached_features else self.detector(images)
        vis = dict(vis)
        if self.config.model.use_gri_feat:
            if len(self.grid_net.layers) > 0 and type(self.grid_net).forward is GridFeatureNetwork.forward:
                vis['gri_feat'] = self.grid_net.last(vis['gri_feat'], vis['gri_mask'])  # == grid_net(...)[0][:, -1]
            else:
                grid, _ = self.grid_net(vis['gri_feat'], vis['gri_mask'])
                vis['gri_feat'] = grid[:, -1]
        return vis

    def forward(self, images, seq, use_beam_search=False, max_len=20, eos_idx=3, beam_size=5, out_size=1,
                return_probs=False, decode='beam', temperature=1.0, top_k=0, top_p=1.0, seed=None, min_len=0, no_repeat_ngram=0,
                no_repeat_word=False, suppress=(), length_penalty=0.0, num_groups=1, diversity=0.0, force_words=None, **kwargs):
        """Beam search under constraints (ops/beam.py): at least `min_len` words before <eos>, no n-gram of `no_repeat_ngram`
        words twice, no word twice in a row (`no_repeat_word`), the ids of `suppress` never; `length_penalty` = alpha ranks the
        final hypotheses by score / length^alpha.  All off by default.
        Diverse beam search: `num_groups` groups of beam_size / num_groups beams are searched in turn at every step, and a group
        pays `diversity` for every time a word was already chosen at this step by an earlier group; one group is the plain search.
        Forced words: `force_words` [B, C, W] int64 padded with -1 names C sets of up to W word ids per image (ops/beam.py); the
        beams are dealt out over banks by how many sets they have met, <eos> waits until a beam has met them all, and the final
        hypotheses are ranked by the sets met, then by score.
        decode='sample' (with use_beam_search=True): `beam_size` independent samples per image from the word distribution at
        `temperature`, truncated to the `top_k` most probable words (0: all) and to the nucleus of mass `top_p`; `seed` is an
        integer, or None for a seed from torch's device generator.  Returns tokens and log-probs [B, out_size, max_len]."""
        if not use_beam_search:
            return self.cap_generator(seq, self._visual_inputs(images))
        constraints = beam_ops.constraints(self.cap_generator.fc.weight.shape[0], min_len, no_repeat_ngram, no_repeat_word, suppress)
        length_penalty = float(length_penalty or 0.0)
        if length_penalty < 0:
            raise ValueError("length_penalty must be >= 0, not %g" % length_penalty)
        groups = beam_ops.groups(beam_size, num_groups, diversity)
        m = self.config.model
        force_words = beam_ops.forced(self.cap_generator.fc.weight.shape[0], force_words, eos_idx, self.bos_idx,
                                      getattr(m, 'pad_idx', None))
        if force_words is not None:
            if decode == 'sample':
                raise NotImplementedError("decode='sample' draws independent samples: forced words are for decode='beam'")
            if groups is not None:
                raise NotImplementedError("forced words with beam groups are not built: use num_groups=1")
            kwargs['force_words'] = force_words
        if decode == 'sample':
            if constraints is not None or length_penalty != 0:
                raise NotImplementedError("decode='sample' takes no beam-search constraints and no length penalty")
            if groups is not None:
                raise NotImplementedError("decode='sample' draws independent samples: beam groups are for decode='beam'")
            if return_probs or kwargs:
                raise NotImplementedError("decode='sample' returns the sampled words' log-probs only and takes no further arguments")
            return self.sample_decode(images, max_len, eos_idx, beam_size, out_size, temperature, top_k, top_p, seed)
        if decode != 'beam':
            raise ValueError("decode must be 'beam' or 'sample', not %r" % (decode,))
        return self.beam_search(images, max_len, eos_idx, beam_size, out_size, return_probs, constraints=constraints,
                                length_penalty=length_penalty, groups=groups, **kwargs)

    # ------------------------------------------------------------------ likelihood of given captions
    def score(self, images, captions, normalize=None):
        """How likely the model finds `captions` for `images`: int64 [B, T] or [B, N, T] (N captions per image), each row <bos>,
        words, <eos>, then pad.  The decoder runs teacher-forced on the B * N rows (the visual features are computed once per image
        and repeated per caption); the target of position t is token t + 1, the last position's is pad, so the hidden map goes to
        the likelihood head (ops/vocab_score.py) as it lies in memory.  Returns CaptionScores(log_probs [B, N, T - 1], total
        [B, N], length [B, N]); normalize='mean' divides `total` by `length`.  Eval mode without autograd only; `images` is what
        `forward` takes (a NestedTensor, or cached features with `cached_features` set)."""
        captions = check_score_call(self, captions, normalize)
        log_probs = self._score_log_probs(images, captions)
        return finish_scores(log_probs, captions, self.cap_generator.pad_idx, normalize)

    def _score_log_probs(self, images, captions):
        """captions [B, N, T] -> log-probability of every target [B, N, T - 1] float32, 0 where the target is pad."""
        gen = self.cap_generator
        B, N, T = captions.shape
        if T > gen.pos_emb.num_embeddings - 1:
            raise ValueError("captions of %d tokens (%d targets) exceed the position table: at most %d tokens (model.max_len)"
                             % (T, T - 1, gen.pos_emb.num_embeddings - 1))
        batch_size, device = self.get_bs_device(images)
        if batch_size != B:
            raise ValueError("captions name %d images, the batch has %d" % (B, batch_size))
        captions = captions.to(device)
        vis = self._visual_inputs(images)
        if N > 1:
            vis = {k: (v.repeat_interleave(N, 0) if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == B else v)
                   for k, v in vis.items()}
        rows = captions.reshape(B * N, T)
        hidden = gen.hidden(rows, vis)  # [B * N, T, D]
        target = torch.cat([rows[:, 1:], rows.new_full((B * N, 1), gen.pad_idx)], 1)
        logp, _ = vocab_score_ops.score(hidden.reshape(B * N * T, hidden.shape[-1]), gen.fc.weight, target.reshape(-1), gen.pad_idx)
        return logp.view(B, N, T)[..., :-1]

    # ------------------------------------------------------------------ beam search
    def beam_search(self, images, max_len, eos_idx, beam_size, out_size, return_probs, constraints=None, length_penalty=0.0,
                    groups=None, force_words=None, **kwargs):
        """Inference on a HIP device (no autograd, eval mode): the decode loop -- grid net + `max_len` decoder steps + beam
        bookkeeping, ~5 000 small kernels whose launches bound the loop at ~2.7 ms of host time per step -- is captured ONCE per
        (batch, beam, length, feature shapes) into a HIP graph and replayed from then on (next-row N1: the device-side beam
        loop).  Same kernels, same order, same data: tokens and log-probs are those of the eager loop bit for bit.  Training
        (self-critical: beam search with gradient), CPU runs and return_probs keep the eager loop."""
        if force_words is not None:
            batch_size, device = self.get_bs_device(images)
            if force_words.shape[0] != batch_size:
                raise ValueError("force_words names %d images, the batch has %d" % (force_words.shape[0], batch_size))
            force_words = force_words.to(device)
        if self._graph_eligible(images, return_probs, kwargs):
            vis = images if self.cached_features else self.detector(images)
            return self._beam_search_graphed(dict(vis), max_len, eos_idx, beam_size, out_size, constraints=constraints,
                                             length_penalty=length_penalty, groups=groups, force_words=force_words)
        from grit_amd.ops.linear import suspend_single_use
        with suspend_single_use():  # with gradient (self-critical training) the decoder's weights are used once per STEP
            return self._beam_search_eager(images, max_len, eos_idx, beam_size, out_size, return_probs, constraints=constraints,
                                           length_penalty=length_penalty, groups=groups, force_words=force_words, **kwargs)

    def _graph_eligible(self, images, return_probs, kwargs):
        if not _GRAPH_DECODE or return_probs or kwargs or self.training or torch.is_grad_enabled():
            return False
        _, device = self.get_bs_device(images)
        return device.type == 'cuda' and not torch.cuda.is_current_stream_capturing()

    def _decode_from_features(self, vis, decode, static_seed, static_force=None):
        was = self.cached_features
        self.cached_features = True
        try:
            return decode(vis, static_seed) if static_force is None else decode(vis, static_seed, static_force)
        finally:
            self.cached_features = was

    def _beam_search_graphed(self, vis, max_len, eos_idx, beam_size, out_size, sampling=None, seed=None, constraints=None,
                             length_penalty=0.0, groups=None, force_words=None):
        """sampling = (temperature, top_k, top_p) captures the sampled decode instead: part of the key, with the seed in a static
        device tensor that is rewritten from `seed` (a one-element device tensor) before every replay.  The constraint tuple, the
        length penalty and the beam groups of a beam search are part of the key as well: they are baked into the captured launches.
        Forced words are data like the seed: a static device tensor that is rewritten before every replay, its shape in the key."""
        def decode(feats, static_seed, static_force=None):
            if sampling is None:
                return self._beam_search_eager(feats, max_len, eos_idx, beam_size, out_size, False, constraints=constraints,
                                               length_penalty=length_penalty, groups=groups, force_words=static_force)
            return self._sample_eager(feats, max_len, eos_idx, beam_size, out_size, *sampling, static_seed)

        names = sorted(k for k, v in vis.items() if isinstance(v, torch.Tensor))
        # The graph reads every parameter from its storage at replay time (derived weights are rebuilt inside the capture), so
        # in-place writers -- optimizer steps, load_state_dict -- need no invalidation.  What does: parameter STORAGE being
        # replaced (module.to(dtype), Bf16Compute wrapping): the addresses of the first and last decoder parameters are in the key.
        probe = (self.grid_net.fc.weight, self.cap_generator.fc.weight)
        key = (max_len, eos_idx, beam_size, out_size, sampling, constraints, length_penalty, groups,
               torch.is_inference_mode_enabled(), vis[names[0]].device.index) + \
            tuple((p.data_ptr(), p.dtype) for p in probe) + \
            tuple((k, tuple(vis[k].shape), vis[k].dtype) for k in names)
        if force_words is not None:
            key += (('force_words', tuple(force_words.shape)),)
        entry = self._decode_graphs.pop(key, None)
        if entry is not None:
            self._decode_graphs[key] = entry  # most recently used last
        if entry is None:
            while len(self._decode_graphs) >= 8:  # a few live shapes at most (each graph keeps its activations): drop the
                self._decode_graphs.pop(next(iter(self._decode_graphs)))  # least recently used one, not all of them
            static_in = {k: vis[k].clone() for k in names}
            static_seed = None if sampling is None else seed.clone()
            static_force = None if force_words is None else force_words.clone()
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):  # warm-up on a side stream: library workspaces, lazily built caches
                self._decode_from_features(dict(static_in), decode, static_seed, static_force)
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = self._decode_from_features(dict(static_in), decode, static_seed, static_force)
            entry = self._decode_graphs[key] = (graph, static_in, static_out, static_seed, static_force)
        graph, static_in, static_out, static_seed, static_force = entry
        if static_seed is not None:
            static_seed.copy_(seed)
        if static_force is not None:
            static_force.copy_(force_words)
        for k in names:
            if vis[k].data_ptr() != static_in[k].data_ptr():
                static_in[k].copy_(vis[k])
        graph.replay()
        return tuple(o.clone() for o in static_out)

    def _beam_search_eager(self, images, max_len, eos_idx, beam_size, out_size, return_probs, constraints=None, length_penalty=0.0,
                           groups=None, force_words=None, **kwargs):
        batch_size, device = self.get_bs_device(images)
        self.seq_mask = torch.ones((batch_size, beam_size, 1), device=device)      # 1 while the beam is alive
        self.seq_logprob = torch.zeros((batch_size, 1, 1), device=device)          # running score per beam
        self.log_probs, self.selected_words = [], None
        if return_probs:
            self.all_log_probs = []
        outputs = []
        if force_words is not None:  # read by `iter` only when it is there: every other search passes what it always passed
            self.met = None
            kwargs['force_words'] = force_words
        with self._decode_session(batch_size):
            for t in range(max_len):
                images, outputs = self.iter(timestep=t, samples=images, outputs=outputs, return_probs=return_probs,
                                            batch_size=batch_size, beam_size=beam_size, eos_idx=eos_idx, constraints=constraints,
                                            groups=groups, **kwargs)
        return self._beam_result(outputs, batch_size, beam_size, max_len, out_size, return_probs, eos_idx, length_penalty,
                                 self.met if force_words is not None else None)

    # ------------------------------------------------------------------ sampled decoding
    def sample_decode(self, images, max_len, eos_idx, n_samples, out_size, temperature, top_k, top_p, seed):
        """`n_samples` captions per image, each word drawn by ops/sample.py (one launch per step on the device).  Without gradient
        on a HIP device the loop replays from a captured graph like beam search; with gradient (self-critical training) the
        kernel only picks the words and the log-probs are gathered from the decoder's output."""
        _, device = self.get_bs_device(images)
        if seed is None:
            seed_t = backend.dropout_seed(device) if device.type == 'cuda' else torch.empty(1, dtype=torch.int64).random_()
        else:
            seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            seed_t = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=device)
        sampling = (float(temperature), int(top_k), float(top_p))
        if self._graph_eligible(images, False, {}):
            vis = images if self.cached_features else self.detector(images)
            return self._beam_search_graphed(dict(vis), max_len, eos_idx, n_samples, out_size, sampling, seed_t)
        from grit_amd.ops.linear import suspend_single_use
        with suspend_single_use():
            return self._sample_eager(images, max_len, eos_idx, n_samples, out_size, *sampling, seed_t)

    def _sample_eager(self, images, max_len, eos_idx, n_samples, out_size, temperature, top_k, top_p, seed):
        batch_size, device = self.get_bs_device(images)
        with_grad = torch.is_grad_enabled()
        words = alive = None
        tokens, log_probs = [], []
        with self._decode_session(batch_size):
            for t in range(max_len):
                word_logprob = self.step(t, None if words is None else words.view(-1, 1), images, None, mode='feedback')
                word_logprob = word_logprob.view(word_logprob.shape[0], -1)  # [B, V] at step 0, then [B * n, V]
                words, picked, alive = sample_ops.sample_step(word_logprob, n_samples if t == 0 else 1, words, alive, eos_idx,
                                                              temperature, top_k, top_p, seed, t)
                if t == 0:  # the one fan-out: every sample continues row b; from step 1 on the rows stay where they are
                    self._follow_beams(torch.zeros((batch_size, n_samples), dtype=torch.int64, device=device), 1, batch_size,
                                       n_samples)
                if with_grad and word_logprob.requires_grad:
                    index = words.view(batch_size, n_samples) if t == 0 else words.view(-1, 1)
                    picked = torch.gather(word_logprob, 1, index).view(-1) * alive
                tokens.append(words.view(batch_size, n_samples, 1))
                log_probs.append(picked.view(batch_size, n_samples, 1))
        return torch.cat(tokens, -1)[:, :out_size].contiguous(), torch.cat(log_probs, -1)[:, :out_size].contiguous()

    @contextmanager
    def _decode_session(self, batch_size):
        """Stateful mode for one beam search of `batch_size` images, with the decoder's per-search caches armed (hoisted
        cross-attention K/V, fused self-attention K/V append) and disarmed again afterwards."""
        cross = [m.attention for layer in self.cap_generator.layers for m in (layer.vis_att1, layer.vis_att2)]
        try:
            for att in cross:  # N1: project the visual memory once per beam layout instead of once per step
                att.hoist_kv, att._kv = True, None
            for m in self._kv_cached_modules():
                m._kv_deferred, m._beam_src = False, None
            with self.statefulness(batch_size):
                yield
        finally:
            for att in cross:
                att.hoist_kv, att._kv = False, None

    def step(self, timestep, prev_output, samples, seq, mode='teacher_forcing', **kwargs):
        if mode != 'feedback':
            raise NotImplementedError
        if timestep == 0:
            vis = samples if self.cached_features else self.detector(samples)
            if self.config.model.use_gri_feat:
                grid, self.gri_mask = self.grid_net(vis['gri_feat'], vis['gri_mask'])
                self.gri_feat = grid[:, -1]
            if self.config.model.use_reg_feat:
                self.reg_feat, self.reg_mask = vis['reg_feat'], vis['reg_mask']
            feat = getattr(self, 'gri_feat', self.reg_feat)
            it = feat.data.new_full((feat.shape[0], 1), self.bos_idx).long()
        else:
            it = prev_output
        vis_inputs = {}
        if self.config.model.use_gri_feat:
            vis_inputs.update(gri_feat=self.gri_feat, gri_mask=self.gri_mask)
        if self.config.model.use_reg_feat:
            vis_inputs.update(reg_feat=self.reg_feat, reg_mask=self.reg_mask)
        return self.cap_generator(it, vis_inputs)

    def get_bs_device(self, samples):
        if isinstance(samples, dict):
            t = samples['gri_feat' if 'gri_feat' in samples else 'reg_feat']
        elif isinstance(samples, NestedTensor):
            t = samples.tensors
        else:
            raise TypeError("images must be a NestedTensor or a dict of cached features")
        return t.shape[0], t.device

    def init_state(self, batch_size, device):
        return [torch.zeros((batch_size, 0), dtype=torch.long, device=device), None, None]

    def _kv_cached_modules(self):
        return [layer.self_att for layer in self.cap_generator.layers]

    def iter(self, timestep, samples, outputs, return_probs, batch_size, beam_size=5, eos_idx=3, constraints=None, groups=None,
             force_words=None, **kwargs):
        cur_beam = 1 if timestep == 0 else beam_size
        word_logprob = self.step(timestep, self.selected_words, samples, None, mode='feedback', **kwargs)
        word_logprob = word_logprob.view(batch_size, cur_beam, -1)
        fused = None
        if constraints is not None:
            outputs = self._history(outputs)
        if _FUSED_BEAM_STEP and not return_probs and not kwargs:
            # masking, candidate scores, selection and the score / mask / log-prob gathers in two launches (ops/beam.py); None
            # where the step stays off the kernel: the composed form
            state = (self.seq_logprob, self.seq_mask if timestep > 0 else None, self.selected_words if timestep > 0 else None,
                     eos_idx, beam_size)
            met = self.met if force_words is not None and timestep > 0 else None
            fused = beam_ops.fused_step([word_logprob], state, constraints, groups, force_words, met, outputs[0] if outputs else None,
                                        timestep)
        outputs = self._beam_advance((self,), timestep, word_logprob, fused, outputs, return_probs, batch_size, beam_size,
                                     eos_idx, constraints=constraints, groups=groups, force_words=force_words, **kwargs)
        return samples, outputs

    def _follow_beams(self, selected_beam, cur_beam, batch_size, beam_size):
        """Re-gather the registered states by the surviving beams (reference transformer.py:229)."""
        expand = self._expand_state(selected_beam, cur_beam, batch_size, beam_size)
        # All beams of an image carry the SAME visual memory: re-gathering it by the surviving beam index (reference :229)
        # moves nothing, and replicating it per beam at step 0 only multiplies what every cross-attention reads.  The four
        # visual states stay [B, ...]; Attention.forward groups the beams of an image onto its one copy.  Leaving them
        # untouched also keeps their identity, which is what the hoisted K/V projections are keyed on.
        visual = {id(getattr(self, n, None)) for n in ('gri_feat', 'gri_mask', 'reg_feat', 'reg_mask')} - {id(None)}
        # Self-attention caches that update themselves (one launch: source beam's history + the new key / value, ops/kv_cache.py)
        # only need to be told which beam each survivor continues; everything else is re-gathered as in the reference.
        for m in self._kv_cached_modules():
            if m._kv_deferred:
                m._beam_src = selected_beam
                visual.update((id(m.running_keys), id(m.running_values)))
        self.apply_to_states(lambda tensor: tensor if id(tensor) in visual else expand(tensor))
