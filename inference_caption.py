"""Single-image captioning (reference inference_caption.py:34-69): build detector + Transformer, optional checkpoint
(`state_dict` key, strict=False), NestedTensor batch of one, beam search, token ids -> words through vocab.json.

    python inference_caption.py --img image.npy|image.png [--checkpoint ckpt.pth [ckpt2.pth ...]] [--vocab data/vocab.json] [--beam 5]
                                [--groups G --diversity X] [--n-best N] [--sample N] [--consensus --consensus-corpus captions.json]
                                [--force "dog|dogs" frisbee] [--score "a dog catches a frisbee" ["..." ...]]

Several checkpoints: one model per checkpoint, captioned together by models.caption.ensemble.Ensemble (their word
log-probabilities averaged at every beam step).

`caption_tokens()` is the plumbing the tests drive (BASELINE config 1: 224x224, beam 1 = greedy, CPU with the
oracle ops injected)."""
import argparse
import json
import os

import torch

from grit_amd.config import beam_constraints, beam_groups, default_config, force_words_ids
from grit_amd.tuning import load_tuned_gemms
from models.caption import Transformer
from models.caption.detector import build_detector
from engine.utils import nested_tensor_from_tensor_list


def build_model(config, device, checkpoint=''):
    if torch.device(device).type == 'cuda':
        load_tuned_gemms()  # library GEMM solutions tuned for this model's shapes (grit_amd/tuning.py)
    detector = build_detector(config).to(device)
    model = Transformer(detector=detector, config=config).to(device)
    if checkpoint and os.path.exists(checkpoint):
        state = torch.load(checkpoint, map_location='cpu')
        missing, unexpected = model.load_state_dict(state['state_dict'], strict=False)
        print(f"model missing:{len(missing)} model unexpected:{len(unexpected)}")
    model.cached_features = False
    return model.eval()


def build_captioner(config, device, checkpoints=('',)):
    """One checkpoint: build_model.  Several: one model per checkpoint, in one Ensemble."""
    checkpoints = list(checkpoints) or ['']
    if len(checkpoints) == 1:
        return build_model(config, device, checkpoints[0])
    from models.caption.ensemble import Ensemble
    return Ensemble([build_model(config, device, c) for c in checkpoints], bos_idx=config.model.bos_idx, config=config).eval()


@torch.inference_mode()
def caption_tokens(model, image, config, beam_size=None, n_best=1, force_words=None):
    """image [3,H,W] (already normalised) -> (tokens [1, beam_len] int64, log_probs [1, beam_len]); with n_best > 1 the n_best
    best final hypotheses, [1, n_best, beam_len] each.  force_words [1, sets, words] (config.force_words_ids): the caption holds a
    word of every set."""
    device = next(model.parameters()).device
    images = nested_tensor_from_tensor_list([image]).to(device)
    forced = {} if force_words is None else dict(force_words=force_words)
    return model(images, seq=None, use_beam_search=True, max_len=config.model.beam_len, eos_idx=config.model.eos_idx,
                 beam_size=beam_size or config.model.beam_size, out_size=n_best, return_probs=False, **beam_constraints(config),
                 **beam_groups(config), **forced)


def vocabulary(vocab_path):
    """The words of vocab.json in id order."""
    with open(vocab_path) as f:
        vocab = json.load(f)
    return vocab['itos'] if isinstance(vocab, dict) and 'itos' in vocab else vocab


@torch.inference_mode()
def sample_tokens(model, image, config, n, temperature=1.0, top_k=0, top_p=1.0, seed=None):
    """image [3,H,W] (already normalised) -> (tokens [n, beam_len] int64, log_probs [n, beam_len]): n captions drawn from the
    model's distribution (Transformer.forward(decode='sample')) instead of the best beam."""
    device = next(model.parameters()).device
    images = nested_tensor_from_tensor_list([image]).to(device)
    tokens, log_probs = model(images, seq=None, use_beam_search=True, max_len=config.model.beam_len, eos_idx=config.model.eos_idx,
                              beam_size=n, out_size=n, decode='sample', temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
    return tokens[0], log_probs[0]


@torch.inference_mode()
def caption_stream(model, batches, config, beam_size=None):
    """Caption a sequence of batches (NestedTensor each), yielding (tokens, log_probs) per batch in order -- the inner loop
    of evaluate_metrics (reference engine/caption_engine.py:156-175) arranged for the GPU: the detector of batch i+1 is
    enqueued on its own HIP stream BEFORE the beam search of batch i.  The beam-search loop is launch bound (~60 ms of
    host time for < 20 ms of GPU work at batch 64) while the detector is GPU bound (~48 ms), so the two overlap almost
    entirely.  Same kernels on the same data: the results are those of the sequential loop."""
    beam = beam_size or config.model.beam_size
    device = next(model.parameters()).device
    if device.type != 'cuda':
        for samples in batches:
            yield model(samples, seq=None, use_beam_search=True, max_len=config.model.beam_len, eos_idx=config.model.eos_idx,
                        beam_size=beam, out_size=1, return_probs=False, **beam_constraints(config), **beam_groups(config))
        return
    # The tuned GEMM table (grit_amd/tuning.py) is switched off while two streams issue library GEMMs side by side: with it, the
    # detector stream stalls for tens of ms every few batches next to the replayed decode graph (63-91 ms per batch instead of 51,
    # tools/micro/dbg_pipelined.py); the sequential path keeps it (detector 46.6 -> 40.5 ms).
    import torch.cuda.tunable as tunable
    tuned = tunable.is_enabled()
    tunable.enable(False)
    try:
        yield from _caption_stream_device(model, batches, config, beam, device)
    finally:
        tunable.enable(tuned)


def _caption_stream_device(model, batches, config, beam, device):
    det_stream, dec_stream = torch.cuda.Stream(device), torch.cuda.Stream(device)
    caller = torch.cuda.current_stream(device)
    det_stream.wait_stream(caller)
    dec_stream.wait_stream(caller)

    def beam_search(vis, ready):
        was = model.cached_features
        model.cached_features = True
        try:
            with torch.cuda.stream(dec_stream):
                dec_stream.wait_event(ready)
                for v in _feature_tensors(vis):
                    v.record_stream(dec_stream)
                out = model(vis, seq=None, use_beam_search=True, max_len=config.model.beam_len,
                            eos_idx=config.model.eos_idx, beam_size=beam, out_size=1, return_probs=False,
                            **beam_constraints(config), **beam_groups(config))
                done = torch.cuda.Event()
                done.record(dec_stream)
        finally:
            model.cached_features = was
        caller.wait_event(done)
        for o in out:
            o.record_stream(caller)
        return out

    pending = None
    for samples in batches:
        # `batches` may produce its items lazily on the caller's stream (device collator kernels, pinned-memory uploads):
        # order the detector after whatever has been enqueued there so far, and keep the batch's memory from being reused by
        # the caller-side allocator while the detector stream still reads it
        fetched = torch.cuda.Event()
        fetched.record(caller)
        det_stream.wait_event(fetched)
        for tns in (getattr(samples, 'tensors', None), getattr(samples, 'mask', None)):
            if isinstance(tns, torch.Tensor) and tns.is_cuda:
                tns.record_stream(det_stream)
        with torch.cuda.stream(det_stream):
            vis = _detect(model, samples)
            ready = torch.cuda.Event()
            ready.record(det_stream)
        if pending is not None:
            yield beam_search(*pending)
        pending = (vis, ready)
    if pending is not None:
        yield beam_search(*pending)


def _detect(model, samples):
    """Visual features of one batch: the detector's dict, or for an Ensemble one dict per member (each its own detector)."""
    detect = getattr(model, 'detect', None)
    return detect(samples) if detect is not None else dict(model.detector(samples))


def _feature_tensors(vis):
    for d in (vis if isinstance(vis, list) else [vis]):
        yield from d.values()


def decode(tokens, vocab_path, eos_idx=3):
    """ids -> words, cut at the first <eos> (reference datasets/caption/field.py:258-283)."""
    with open(vocab_path) as f:
        vocab = json.load(f)
    itos = vocab['itos'] if isinstance(vocab, dict) and 'itos' in vocab else vocab
    out = []
    for row in tokens.tolist():
        words = []
        for t in row:
            if t == eos_idx:
                break
            words.append(itos[t])
        out.append(' '.join(words))
    return out


def caption_ids(texts, stoi, bos_idx, eos_idx, pad_idx):
    """Captions as text -> int64 [N, T]: <bos>, the ids of the lower-cased, whitespace-split words, <eos>, then pad up to the longest.
    `stoi` maps a word to its id (a dict, or the list of words in id order); an unknown word is a ValueError that names it."""
    if not isinstance(stoi, dict):
        stoi = {word: i for i, word in enumerate(stoi)}
    rows = []
    for text in ([texts] if isinstance(texts, str) else list(texts)):
        words = str(text).lower().split()
        if not words:
            raise ValueError("caption %r holds no word" % (text,))
        for w in words:
            if w not in stoi:
                raise ValueError("word %r of caption %r is not in the vocabulary" % (w, text))
        rows.append([bos_idx] + [int(stoi[w]) for w in words] + [eos_idx])
    if not rows:
        raise ValueError("no caption to score")
    width = max(len(r) for r in rows)
    return torch.tensor([r + [pad_idx] * (width - len(r)) for r in rows], dtype=torch.int64)


@torch.inference_mode()
def score_texts(model, image, config, ids):
    """image [3,H,W] (already normalised), ids [N, T] (caption_ids) -> (total [N], length [N]) of the N captions for the image;
    `model` is a Transformer or an Ensemble."""
    device = next(model.parameters()).device
    images = nested_tensor_from_tensor_list([image]).to(device)
    scores = model.score(images, ids.unsqueeze(0).to(device))
    return scores.total[0], scores.length[0]


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--img', required=True)
    ap.add_argument('--checkpoint', nargs='+', default=[''], help="one checkpoint, or several for an ensemble")
    ap.add_argument('--vocab', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'vocab.json'))
    ap.add_argument('--beam', type=int, default=None)
    ap.add_argument('--min-len', type=int, default=0, help="at least this many words before <eos>")
    ap.add_argument('--no-repeat-ngram', type=int, default=0, metavar='N', help="no n-gram of N words twice in a caption (0: off)")
    ap.add_argument('--no-repeat-word', action='store_true', help="no word twice in a row")
    ap.add_argument('--suppress', type=int, nargs='*', default=[], metavar='ID', help="vocabulary ids that are never chosen")
    ap.add_argument('--length-penalty', type=float, default=0.0, help="rank the final beams by score / length^this (0: off)")
    ap.add_argument('--groups', type=int, default=1, metavar='G', help="diverse beam search: G groups of beam / G beams (1: off)")
    ap.add_argument('--diversity', type=float, default=0.0, metavar='X',
                    help="what a group pays per earlier choice of the same word at a step")
    ap.add_argument('--force', nargs='*', default=[], metavar='WORDS',
                    help='words that the caption must mention: one set per argument, alternatives separated by | ("dog|dogs" frisbee)')
    ap.add_argument('--n-best', type=int, default=1, metavar='N', help="print the N best final hypotheses instead of one")
    ap.add_argument('--sample', type=int, default=0, metavar='N', help="print N sampled captions instead of the best beam")
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--top-k', type=int, default=0, help="sample among the k most probable words only (0: all)")
    ap.add_argument('--top-p', type=float, default=1.0, help="sample inside the smallest nucleus of this mass")
    ap.add_argument('--seed', type=int, default=None, help="sampling seed (default: torch's device generator)")
    ap.add_argument('--score', nargs='+', default=[], metavar='CAPTION',
                    help="do not caption: print how likely the model finds each given caption (log-probability, per word, text), best first")
    ap.add_argument('--consensus', action='store_true',
                    help="rerank what --n-best N or --sample N produced by consensus under CIDEr-D: the chosen caption first, then "
                         "the candidates with their consensus scores (needs --consensus-corpus)")
    ap.add_argument('--consensus-corpus', default=None, metavar='FILE',
                    help="JSON list of caption lists, one list per image: the corpus of the CIDEr-D document frequencies")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.consensus and not a.consensus_corpus:
        ap.error("--consensus needs --consensus-corpus FILE (the captions the CIDEr-D document frequencies come from)")
    if a.consensus and max(a.n_best, a.sample) < 2:
        ap.error("--consensus reranks several candidates: give --n-best N or --sample N with N > 1")
    if a.force and a.sample > 0:
        ap.error("--force steers the beam search: it does not go with --sample")
    if a.force and a.groups > 1:
        ap.error("--force does not go with --groups")
    if a.score and (a.sample > 0 or a.force or a.consensus):
        ap.error("--score rates given captions, it decodes nothing: it does not go with --sample, --force or --consensus")
    return a


def consensus_cider(corpus_path):
    """The `Cider` of --consensus-corpus: a JSON list of caption lists, one per image, tokenised by the native tokenizer."""
    from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
    with open(corpus_path) as f:
        corpus = json.load(f)
    if not isinstance(corpus, list) or not corpus or not all(isinstance(c, list) and c and all(isinstance(s, str) for s in c) for c in corpus):
        raise ValueError("%s: expected a JSON list of non-empty lists of captions, one list per image" % corpus_path)
    return Cider(PTBTokenizer.tokenize({i: caps for i, caps in enumerate(corpus)}))


def print_consensus(tokens, cider, vocab_path, eos_idx=3):
    """tokens [n, T] on the device: the candidates of one image.  Prints the caption chosen by consensus, then every candidate
    with its consensus score."""
    from grit_amd.ops.cider import DeviceCider
    with open(vocab_path) as f:
        vocab = json.load(f)
    itos = vocab['itos'] if isinstance(vocab, dict) and 'itos' in vocab else vocab
    chosen = DeviceCider(cider, itos, eos_token=itos[eos_idx], device=tokens.device).consensus(tokens.unsqueeze(0))
    print(decode(chosen.tokens[0], vocab_path, eos_idx)[0])
    for score, line in zip(chosen.score[0].tolist(), decode(tokens, vocab_path, eos_idx)):
        print('%8.4f  %s' % (score, line))


def run_main():
    a = parse_args()
    config = default_config(**{'model.beam_min_len': a.min_len, 'model.beam_no_repeat_ngram': a.no_repeat_ngram,
                               'model.beam_no_repeat_word': a.no_repeat_word, 'model.beam_suppress': list(a.suppress),
                               'model.beam_length_penalty': a.length_penalty, 'model.beam_groups': a.groups,
                               'model.beam_diversity': a.diversity, 'model.beam_force_words': list(a.force)})
    # words -> ids before anything is built: an unknown word is an error that names it
    force_words = force_words_ids(config.model.beam_force_words, vocabulary(a.vocab)) if a.force else None
    m = config.model
    score_ids = caption_ids(a.score, vocabulary(a.vocab), m.bos_idx, m.eos_idx, m.pad_idx) if a.score else None
    device = torch.device('cuda:0')  # the kernels need a HIP device; there is no CPU path
    model = build_captioner(config, device, a.checkpoint)
    if a.img.endswith('.npy'):
        import numpy as np
        image = torch.from_numpy(np.load(a.img)).float()
    else:
        import numpy as np
        from PIL import Image
        rgb = np.asarray(Image.open(a.img).convert('RGB'), dtype=np.float32) / 255.0
        mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
        image = torch.from_numpy(((rgb - mean) / std).transpose(2, 0, 1))
    if a.score:
        total, length = score_texts(model, image, config, score_ids)
        total, length = total.tolist(), length.tolist()
        for i in sorted(range(len(a.score)), key=lambda i: -total[i]):  # best first
            print('%10.4f %8.4f  %s' % (total[i], total[i] / max(length[i], 1), a.score[i]))
        return
    if a.consensus:  # (the vocabulary is needed: consensus compares words, not ids)
        cider = consensus_cider(a.consensus_corpus)
        if a.sample > 0:
            tokens, _ = sample_tokens(model, image, config, a.sample, a.temperature, a.top_k, a.top_p, a.seed)
        else:
            tokens = caption_tokens(model, image, config, a.beam, a.n_best, force_words)[0][0]
        print_consensus(tokens, cider, a.vocab, config.model.eos_idx)
        return
    if a.sample > 0:
        tokens, _ = sample_tokens(model, image, config, a.sample, a.temperature, a.top_k, a.top_p, a.seed)
        for line in (decode(tokens, a.vocab, config.model.eos_idx) if os.path.exists(a.vocab) else tokens.tolist()):
            print(line)
        return
    tokens, _ = caption_tokens(model, image, config, a.beam, a.n_best, force_words)
    if a.n_best == 1:
        print(decode(tokens, a.vocab, config.model.eos_idx)[0] if os.path.exists(a.vocab) else tokens.tolist())
        return
    for line in (decode(tokens[0], a.vocab, config.model.eos_idx) if os.path.exists(a.vocab) else tokens[0].tolist()):  # best first
        print(line)


if __name__ == "__main__":
    run_main()
