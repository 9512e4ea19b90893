"""Configuration as a plain attribute namespace.

The reference drives everything through hydra/OmegaConf (configs/caption/coco_config.yaml, train_caption.py:207);
neither is installed here, and the model code only ever does attribute access (`config.model.d_model`,
`getattr(cfg, 'aux_loss', False)`), so a nested namespace with the same keys is a drop-in.  `default_config()`
returns the values of coco_config.yaml:1-93; `load_yaml()` reads a user yaml with the same layout (${...}
interpolations resolved for the two forms the reference uses: ${oc.env:NAME} and ${a.b}).
"""
import os
import re
from types import SimpleNamespace


class Config(SimpleNamespace):
    """Namespace that also supports `'key' in cfg` and dict-style get (OmegaConf habits used by the scripts)."""

    def __contains__(self, key):
        return key in self.__dict__

    def get(self, key, default=None):
        return self.__dict__.get(key, default)

    def to_dict(self):
        return {k: (v.to_dict() if isinstance(v, Config) else v) for k, v in self.__dict__.items()}


def to_config(obj):
    if isinstance(obj, dict):
        return Config(**{k: to_config(v) for k, v in obj.items()})
    if isinstance(obj, (list, tuple)):
        return [to_config(v) for v in obj]
    return obj


_DEFAULTS = {
    'exp': dict(seed=42, name='eval', rank=0, ngpus_per_node=8, world_size=8, checkpoint='', eval=False, resume=False,
                # the validation loss of every epoch (engine.caption_engine.evaluate_loss): 'torch' = model(samples, captions) + NLLLoss as in the reference; 'fused' = model.score (the likelihood head of grit_amd/ops/vocab_score.py: no [rows, V] map)
                eval_loss_head='torch',
                eval_scorer='device'),  # the per-epoch BLEU / ROUGE / CIDEr of train_caption.main: 'device' scores the beam tokens in one kernel launch (grit_amd/ops/caption_scores.py), 'host' decodes and scores in Python as the reference does (the choice for a run without a GPU: 'device' is refused there)
    'dataset': dict(overfit=False, ann_root='', img_root='', hdf5_path='', vocab_path='',
                    use_gri_feat=True, use_reg_feat=True,
                    transform_cfg=dict(size=[384, 640], resize_name='maxwh', randaug=False)),  # reference yaml: randaug true (host-side PIL); 'device' runs the same operations on the GPU
    'model': dict(
        use_gri_feat=True, use_reg_feat=True, grid_feat_dim=1024, frozen_stages=2, beam_size=5, beam_len=20,
        # beam-search constraints of evaluation and inference (Transformer.forward; all off, as in the reference): at least
        # beam_min_len words before <eos>, no n-gram of beam_no_repeat_ngram words twice, no word twice in a row, vocabulary ids that
        # are never chosen, final ranking by score / length^beam_length_penalty.  Self-critical training decodes unconstrained.
        beam_min_len=0, beam_no_repeat_ngram=0, beam_no_repeat_word=False, beam_suppress=[], beam_length_penalty=0.0,
        # diverse beam search of evaluation and inference: beam_groups groups of beam_size / beam_groups beams searched in turn, a
        # group paying beam_diversity per earlier choice of the same word at a step (1 group: the plain search, as in the reference)
        beam_groups=1, beam_diversity=0.0,
        # forced words of inference: every entry is one set, "dog|dogs" a set of two alternatives; the caption must hold a word of
        # every set (constrained beam search by dynamic beam allocation, grit_amd/ops/beam.py).  Empty: off
        beam_force_words=(),
        # consensus (minimum-Bayes-risk) reranking of evaluation under CIDEr-D (grit_amd/ops/consensus.py): of consensus_candidates
        # candidates per image the one that agrees most with the others is scored (0 or 1: off, hypothesis 0 as in the reference).
        # consensus_decode 'beam': the N best final hypotheses of the search configured above (N <= beam_size); 'sample': N samples
        # at consensus_temperature / consensus_top_k / consensus_top_p from consensus_seed (None: torch's device generator)
        consensus_candidates=0, consensus_decode='beam', consensus_temperature=1.0, consensus_top_k=0, consensus_top_p=1.0,
        consensus_seed=None,
        dropout=0.2, attn_dropout=0.2, vocab_size=10201, max_len=54, pad_idx=1, bos_idx=2, eos_idx=3, d_model=512,
        n_heads=8, grid_net=dict(n_memories=1, n_layers=3), cap_generator=dict(decoder_name='parallel', n_layers=3),
        detector=dict(checkpoint='', d_model=512, dim_feedforward=1024, num_heads=8, num_layers=6, num_levels=4,
                      num_points=4, num_queries=150, num_classes=1849, dropout=0.1, activation='relu',
                      return_intermediate=True, with_box_refine=True)),
    'optimizer': dict(warmup_init_lr=1e-5, min_lr=1e-4, xe_lr=1e-4, sc_lr=5e-6, xe_backbone_lr=1e-5,
                      sc_backbone_lr=5e-6, weight_decay=0.01, beta_1=0.9, beta_2=0.99, batch_size=16, num_workers=2,
                      freezing_xe_epochs=0, freezing_sc_epochs=0, finetune_xe_epochs=10, finetune_sc_epochs=10,
                      freeze_detector=False, freeze_backbone=False,
                      sc_reward='host',  # 'device': CIDEr-D of the beams in one kernel launch (grit_amd/ops/cider.py), no host round trip
                      # what the self-critical step decodes: 'beam' = the reference's beam search with gradient; 'sample' = sc_samples
                      # independent samples per image (None: model.beam_size) at sc_temperature, the mean reward of an image's samples
                      # as the baseline.  Only temperature 1 (and no truncation, which the step never applies) samples the policy
                      # itself, i.e. gives an unbiased policy gradient; any other temperature trains on a tempered proposal.
                      sc_decode='beam', sc_samples=None, sc_temperature=1.0),
}


def beam_constraints(config):
    """The model.beam_* constraint keys as keyword arguments of Transformer.forward / Ensemble.forward; a config written before
    they existed gives the defaults (all off)."""
    m = config.model
    return dict(min_len=getattr(m, 'beam_min_len', 0), no_repeat_ngram=getattr(m, 'beam_no_repeat_ngram', 0),
                no_repeat_word=getattr(m, 'beam_no_repeat_word', False), suppress=tuple(getattr(m, 'beam_suppress', None) or ()),
                length_penalty=getattr(m, 'beam_length_penalty', 0.0))


def beam_groups(config):
    """The model.beam_groups / model.beam_diversity keys as keyword arguments of Transformer.forward / Ensemble.forward; a config
    written before they existed gives the defaults (one group: the plain search)."""
    m = config.model
    return dict(num_groups=getattr(m, 'beam_groups', 1), diversity=getattr(m, 'beam_diversity', 0.0))


def force_words_ids(specs, stoi, batch_size=1):
    """The sets of forced words that `specs` names ("dog|dogs", "frisbee": one set per entry, alternatives separated by |) as the
    force_words tensor of Transformer.forward / Ensemble.forward, int64 [batch_size, sets, words] padded with -1 and the same for
    every image, or None without specs.  `stoi` maps a word to its id (a dict, or the list of words in id order); a word that the
    vocabulary does not hold is a ValueError that names it."""
    import torch
    specs = [specs] if isinstance(specs, str) else list(specs or ())
    if not specs:
        return None
    if not isinstance(stoi, dict):
        stoi = {word: i for i, word in enumerate(stoi)}
    sets = []
    for spec in specs:
        words = [w.strip() for w in str(spec).split('|') if w.strip()]
        if not words:
            raise ValueError("forced words: %r names no word" % (spec,))
        for w in words:
            if w not in stoi:
                raise ValueError("forced word %r is not in the vocabulary" % w)
        sets.append([int(stoi[w]) for w in words])
    width = max(len(ids) for ids in sets)
    table = torch.tensor([ids + [-1] * (width - len(ids)) for ids in sets], dtype=torch.int64)
    return table.unsqueeze(0).repeat(batch_size, 1, 1)


def consensus_options(config):
    """The model.consensus_* keys as a dictionary: candidates (0: off; 1 counts as off), decode ('beam' / 'sample') and the sampling
    keywords of Transformer.forward for 'sample'.  A config written before the keys existed is off."""
    m = config.model
    n = int(getattr(m, 'consensus_candidates', 0) or 0)
    decode = getattr(m, 'consensus_decode', 'beam')
    if n < 0:
        raise ValueError("model.consensus_candidates must be >= 0, not %r" % (n,))
    if decode not in ('beam', 'sample'):
        raise ValueError("model.consensus_decode must be 'beam' or 'sample', not %r" % (decode,))
    return dict(candidates=n if n > 1 else 0, decode=decode,
                sample=dict(temperature=getattr(m, 'consensus_temperature', 1.0), top_k=getattr(m, 'consensus_top_k', 0),
                            top_p=getattr(m, 'consensus_top_p', 1.0), seed=getattr(m, 'consensus_seed', None)))


def default_config(**overrides):
    """coco_config.yaml as a namespace.  Overrides use dotted keys: default_config(**{'model.dropout': 0.0})."""
    import copy
    raw = copy.deepcopy(_DEFAULTS)
    data_root = os.environ.get('DATA_ROOT', '')
    raw['dataset'].update(ann_root=os.path.join(data_root, 'annotations'), img_root=data_root,
                          hdf5_path=os.path.join(data_root, 'all_splits.h5'),
                          vocab_path=os.path.join(data_root, 'annotations', 'vocab.json'))
    for dotted, value in overrides.items():
        node = raw
        *path, leaf = dotted.split('.')
        for p in path:
            node = node.setdefault(p, {})
        node[leaf] = value
    return to_config(raw)


_DETECTION_DEFAULTS = {
    'exp': dict(seed=42, save_dir='', rank=0, ngpus_per_node=8, world_size=64, checkpoint='', eval=False, resume=False,
                eval_every_iters=-1),
    'model': dict(
        has_attr_head=False, num_attr_classes=400,
        backbone=dict(backbone_name='swin_base_win7_384_22k', pre_trained='imagenet'),
        det_module=dict(reduced_dim=512, dim_feedforward=1024, num_heads=8, num_layers=6, num_levels=4, num_points=4,
                        return_intermediate=True, num_queries=150, num_classes=1849, dropout=0.1, activation='relu',
                        with_box_refine=True, aux_loss=True,
                        loss=dict(dice_loss_coef=1., cls_loss_coef=2., bbox_loss_coef=5., giou_loss_coef=2., attr_loss_coef=0.,
                                  eos_coef=0.1, focal_alpha=0.25),
                        matcher=dict(set_cost_class=2.0, set_cost_bbox=5.0, set_cost_giou=2.0))),
    'optimizer': dict(lr=1e-5, lr_backbone=2e-5, batch_size=4, weight_decay=1e-4, lr_drop_epochs=[40], scheduler='step',
                      decay_rate=0.1, clip_max_norm=0.1, num_workers=4, num_epochs=50, sp_lr=1e-4, sp_lr_drop_epochs=[5]),
}


def detection_config(**overrides):
    """The detector pre-training configuration (the keys of configs/detection/train_config.yaml) as a namespace; dotted overrides
    as in default_config.  The dataset groups of the yaml are not part of it: the Visual Genome readers are out of scope."""
    import copy
    raw = copy.deepcopy(_DETECTION_DEFAULTS)
    for dotted, value in overrides.items():
        node = raw
        *path, leaf = dotted.split('.')
        for p in path:
            node = node.setdefault(p, {})
        node[leaf] = value
    return to_config(raw)


def load_yaml(path):
    import yaml
    with open(path) as f:
        raw = yaml.safe_load(f)

    def lookup(dotted):
        node = raw
        for p in dotted.split('.'):
            node = node[p]
        return node

    def resolve(v):
        if isinstance(v, dict):
            return {k: resolve(x) for k, x in v.items()}
        if isinstance(v, list):
            return [resolve(x) for x in v]
        if isinstance(v, str):
            whole = re.fullmatch(r"\$\{([\w.]+)\}", v)
            if whole:
                return resolve(lookup(whole.group(1)))
            return re.sub(r"\$\{oc\.env:(\w+)\}", lambda m: os.environ.get(m.group(1), ''), v)
        return v

    raw.pop('hydra', None)
    return to_config(resolve(raw))
