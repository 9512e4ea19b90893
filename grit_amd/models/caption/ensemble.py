"""Ensemble of GRIT captioners in one beam search (reference models/caption/ensemble.py, `Ensemble`).

Every step each member produces its word log-probabilities from its own visual features and its own decoder states; the
ensemble's word log-probability is their mean, torch.mean(torch.stack(per_model), 0) (reference :128-162), and the rest of
the step -- finished-beam masking, candidate scores, selection, the score / mask / log-prob gathers, every member's states
re-gathered by the surviving beams -- is `Transformer.iter`'s (reference :164-214).  On a HIP device the mean and the step are
one fused pair of launches (grit_beam_step with n_maps = K: the averaged map is never written) and the whole K-model decode from
features is captured once per shape into a HIP graph and replayed, with the policy of `Transformer._beam_search_graphed`.

The reference class reads `model.encoder`, `model.decoder`, `det_feat` and `config.model.decoder.decoder_name`, names left
over from another code base; here the members are this package's `Transformer`s and their own per-step pieces are reused
(visual inputs, the grid network, the hoisted cross-attention K/V, the fused K/V append, `_expand_state`).

`samples` is a NestedTensor (each member runs its own detector), a dict of cached features (every member uses them as they
are) or a list of such dicts, one per member (what `detect` returns: each member's own detector output)."""
from contextlib import ExitStack

import torch
from torch import nn

from grit_amd.models.caption import transformer as _tr
from grit_amd.models.caption.transformer import BeamSearchSteps
from grit_amd.ops import beam as beam_ops
from grit_amd.utils.misc import NestedTensor


class Ensemble(BeamSearchSteps, nn.Module):

    def __init__(self, models, bos_idx=2, use_vis_feat=True, use_reg_feat=False, config=None):
        super().__init__()
        models = list(models)
        if not models:
            raise ValueError("Ensemble needs at least one model")
        if len(models) > beam_ops.MAX_MAPS:
            raise ValueError("Ensemble takes at most %d models, got %d" % (beam_ops.MAX_MAPS, len(models)))
        for i, m in enumerate(models):
            if not hasattr(m, 'cap_generator') or not hasattr(m, '_decode_session'):
                raise TypeError("Ensemble member %d is a %s, not a captioning Transformer" % (i, type(m).__name__))
        vocab = [m.cap_generator.fc.weight.shape[0] for m in models]
        if len(set(vocab)) != 1:
            raise ValueError("Ensemble members have different vocabulary sizes: %s" % vocab)
        bos = [m.bos_idx for m in models]
        if len(set(bos)) != 1 or bos[0] != bos_idx:
            raise ValueError("Ensemble members' bos index %s does not match bos_idx=%d" % (bos, bos_idx))
        eos = [m.config.model.eos_idx for m in models]
        if len(set(eos)) != 1:
            raise ValueError("Ensemble members have different eos indices: %s" % eos)
        self.models = nn.ModuleList(models)
        self._check_placement()
        self.bos_idx = bos_idx
        self.eos_idx = eos[0]
        self.use_reg_feat = use_reg_feat
        self.use_vis_feat = use_vis_feat
        self.config = config
        # kept for the interface the engine drives (caption_stream sets it around a decode from features): the type of
        # `samples` decides here, a NestedTensor runs every member's detector, a dict is used as features
        self.cached_features = False
        self._decode_graphs = {}

    # ------------------------------------------------------------------ members
    @staticmethod
    def _probes(model):
        return (model.grid_net.fc.weight, model.cap_generator.fc.weight)

    def _check_placement(self):
        places = [(p.device, p.dtype) for m in self.models for p in self._probes(m)]
        if len(set(places)) != 1:
            raise ValueError("Ensemble members must sit on one device with one dtype, got %s" %
                             sorted({'%s/%s' % (d, str(t).replace('torch.', '')) for d, t in places}))

    def detect(self, samples):
        """Every member's own detector on one batch of images: a list of feature dicts, one per member."""
        return [dict(m.detector(samples)) for m in self.models]

    def _member_features(self, samples):
        if isinstance(samples, NestedTensor):
            return self.detect(samples)
        if isinstance(samples, dict):
            return [dict(samples) for _ in self.models]
        if isinstance(samples, (list, tuple)) and all(isinstance(s, dict) for s in samples):
            if len(samples) != len(self.models):
                raise ValueError("%d feature dicts for %d ensemble members" % (len(samples), len(self.models)))
            return [dict(s) for s in samples]
        raise TypeError("samples must be a NestedTensor, a dict of cached features or one such dict per member")

    def get_bs_device(self, samples):
        if isinstance(samples, (list, tuple)) and samples and isinstance(samples[0], dict):
            samples = samples[0]
        return self.models[0].get_bs_device(samples)

    def init_state(self, batch_size, device):
        return [torch.zeros((batch_size, 0), dtype=torch.long, device=device), None, None]

    # ------------------------------------------------------------------ decoding
    def forward(self, samples, seq, use_beam_search=False, max_len=20, eos_idx=3, beam_size=5, out_size=1, return_probs=False,
                **kwargs):
        if not use_beam_search:
            raise NotImplementedError("Ensemble only decodes by beam search (use_beam_search=True): the reference has no "
                                      "teacher-forcing ensemble")
        decode = kwargs.pop('decode', 'beam')  # Transformer.forward's switch; the signature here stays the reference's
        # Transformer.forward's constraints, validated before anything is refused or run
        constraints = beam_ops.constraints(self.models[0].cap_generator.fc.weight.shape[0], kwargs.pop('min_len', 0),
                                           kwargs.pop('no_repeat_ngram', 0), kwargs.pop('no_repeat_word', False),
                                           kwargs.pop('suppress', ()))
        length_penalty = float(kwargs.pop('length_penalty', 0.0) or 0.0)
        if length_penalty < 0:
            raise ValueError("length_penalty must be >= 0, not %g" % length_penalty)
        # Transformer.forward's diverse search: taken out of kwargs like the rest, so that the search can still replay from a graph
        groups = beam_ops.groups(beam_size, kwargs.pop('num_groups', 1), kwargs.pop('diversity', 0.0))
        # Transformer.forward's forced words: validated like the rest, refused with beam groups
        first = self.models[0]
        force_words = beam_ops.forced(first.cap_generator.fc.weight.shape[0], kwargs.pop('force_words', None), eos_idx, first.bos_idx,
                                      getattr(first.config.model, 'pad_idx', None))
        if force_words is not None and groups is not None:
            raise NotImplementedError("forced words with beam groups are not built: use num_groups=1")
        if decode != 'beam':
            raise NotImplementedError("Ensemble only decodes by beam search: decode=%r is for a single Transformer (sampling from "
                                      "an average of distributions is not built)" % (decode,))
        self._check_placement()
        feats = self._member_features(samples)
        if force_words is not None:
            batch_size, device = self.get_bs_device(feats)
            if force_words.shape[0] != batch_size:
                raise ValueError("force_words names %d images, the batch has %d" % (force_words.shape[0], batch_size))
            force_words = force_words.to(device)
        if self._graph_eligible(feats, return_probs, kwargs):
            return self._beam_search_graphed(feats, max_len, eos_idx, beam_size, out_size, constraints, length_penalty, groups,
                                             force_words)
        from grit_amd.ops.linear import suspend_single_use
        with suspend_single_use():
            return self._beam_search_eager(feats, max_len, eos_idx, beam_size, out_size, return_probs, constraints=constraints,
                                           length_penalty=length_penalty, groups=groups, force_words=force_words, **kwargs)

    # ------------------------------------------------------------------ likelihood of given captions
    def score(self, samples, captions, normalize=None):
        """`Transformer.score` for the ensemble: every member scores `captions` on its own features, and the ensemble's
        log-probability of a token is the mean of the members', torch.mean(torch.stack(per_member), 0) -- the rule of its beam step."""
        captions = _tr.check_score_call(self, captions, normalize)
        self._check_placement()
        feats = self._member_features(samples)
        per_member = []
        for m, f in zip(self.models, feats):
            with _features_mode(m):
                per_member.append(m._score_log_probs(f, captions))
        log_probs = torch.mean(torch.stack(per_member), 0)
        return _tr.finish_scores(log_probs, captions, self.models[0].cap_generator.pad_idx, normalize)

    def _graph_eligible(self, feats, return_probs, kwargs):
        if not _tr._GRAPH_DECODE or return_probs or kwargs or self.training or torch.is_grad_enabled():
            return False
        _, device = self.get_bs_device(feats)
        return device.type == 'cuda' and not torch.cuda.is_current_stream_capturing()

    def _beam_search_graphed(self, feats, max_len, eos_idx, beam_size, out_size, constraints=None, length_penalty=0.0, groups=None,
                             force_words=None):
        """`Transformer._beam_search_graphed` for K members: one graph per (every member's probe-parameter storage, batch, beam,
        length, constraints, beam groups, feature shapes), least recently used of 8 dropped, warm-up on a side stream.  The
        members' own graph caches are not touched.  Forced words are a static device tensor that is rewritten before every replay;
        only their shape is in the key."""
        def decode():
            return self._beam_search_eager([dict(s) for s in static_in], max_len, eos_idx, beam_size, out_size, False,
                                           constraints=constraints, length_penalty=length_penalty, groups=groups,
                                           force_words=static_force)

        names = [sorted(k for k, v in f.items() if isinstance(v, torch.Tensor)) for f in feats]
        key = (max_len, eos_idx, beam_size, out_size, constraints, length_penalty, groups, torch.is_inference_mode_enabled(),
               feats[0][names[0][0]].device.index) + \
            tuple((p.data_ptr(), p.dtype) for m in self.models for p in self._probes(m)) + \
            tuple(tuple((k, tuple(f[k].shape), f[k].dtype) for k in n) for f, n in zip(feats, names))
        if force_words is not None:
            key += (('force_words', tuple(force_words.shape)),)
        entry = self._decode_graphs.pop(key, None)
        if entry is not None:
            self._decode_graphs[key] = entry  # most recently used last
        if entry is None:
            while len(self._decode_graphs) >= 8:
                self._decode_graphs.pop(next(iter(self._decode_graphs)))
            # every member reads its OWN static copy, also when the call hands all members the same tensors (one dict): the
            # graph must not depend on which members shared their inputs at capture time, since the key does not say
            static_in = [{k: f[k].clone() for k in n} for f, n in zip(feats, names)]
            static_force = None if force_words is None else force_words.clone()
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):  # warm-up on a side stream: library workspaces, lazily built caches
                decode()
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = decode()
            entry = self._decode_graphs[key] = (graph, static_in, static_out, static_force)
        graph, static_in, static_out, static_force = entry
        if static_force is not None:
            static_force.copy_(force_words)
        for f, s, n in zip(feats, static_in, names):
            for k in n:
                if f[k].data_ptr() != s[k].data_ptr():
                    s[k].copy_(f[k])
        graph.replay()
        return tuple(o.clone() for o in static_out)

    def _beam_search_eager(self, feats, max_len, eos_idx, beam_size, out_size, return_probs, constraints=None, length_penalty=0.0,
                           groups=None, force_words=None, **kwargs):
        batch_size, device = self.get_bs_device(feats)
        self.seq_mask = torch.ones((batch_size, beam_size, 1), device=device)      # 1 while the beam is alive
        self.seq_logprob = torch.zeros((batch_size, 1, 1), device=device)          # running score per beam
        self.log_probs, self.selected_words = [], None
        if return_probs:
            self.all_log_probs = []
        outputs = []
        if force_words is not None:  # read by `iter` only when it is there
            self.met = None
            kwargs['force_words'] = force_words
        with ExitStack() as stack:
            for m in self.models:
                stack.enter_context(_features_mode(m))
                stack.enter_context(m._decode_session(batch_size))
            for t in range(max_len):
                feats, outputs = self.iter(timestep=t, samples=feats, outputs=outputs, return_probs=return_probs,
                                           batch_size=batch_size, beam_size=beam_size, eos_idx=eos_idx, constraints=constraints,
                                           groups=groups, **kwargs)
        return self._beam_result(outputs, batch_size, beam_size, max_len, out_size, return_probs, eos_idx, length_penalty,
                                 self.met if force_words is not None else None)

    def step(self, timestep, prev_output, samples, seq, mode='teacher_forcing', **kwargs):
        """Every member's word log-probabilities for this step (samples: one feature dict per member), [B * cur_beam, 1, V] each."""
        return [m.step(timestep, prev_output, f, seq, mode=mode, **kwargs) for m, f in zip(self.models, samples)]

    def iter(self, timestep, samples, outputs, return_probs, batch_size, beam_size=5, eos_idx=3, constraints=None, groups=None,
             force_words=None, **kwargs):
        cur_beam = 1 if timestep == 0 else beam_size
        maps = [lp.view(batch_size, cur_beam, -1)
                for lp in self.step(timestep, self.selected_words, samples, None, mode='feedback', **kwargs)]
        fused, word_logprob = None, None
        if constraints is not None:
            outputs = self._history(outputs)
        if _tr._FUSED_BEAM_STEP and not return_probs and not kwargs:  # None where the step stays off the kernel: the composed form
            state = (self.seq_logprob, self.seq_mask if timestep > 0 else None, self.selected_words if timestep > 0 else None,
                     eos_idx, beam_size)
            met = self.met if force_words is not None and timestep > 0 else None
            fused = beam_ops.fused_step(maps, state, constraints, groups, force_words, met, outputs[0] if outputs else None, timestep)
        if fused is None:
            word_logprob = torch.mean(torch.stack(maps), 0)
        outputs = self._beam_advance(self.models, timestep, word_logprob, fused, outputs, return_probs, batch_size, beam_size,
                                     eos_idx, constraints=constraints, groups=groups, force_words=force_words, **kwargs)
        return samples, outputs


class _features_mode(object):
    """A member reads `samples` as its visual features (cached_features) for the length of one ensemble decode."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was = self.model.cached_features
        self.model.cached_features = True

    def __exit__(self, *exc):
        self.model.cached_features = self.was
        return False
