"""The caption score kernel (grit_caption_scores, grit_amd/csrc/caption_scores.hip) on the device: against the reference-generated
fixture G18, against the host flow (decode -> collapse repeated words -> tokenise -> compute_scores) on adversarial rows over
the real vocabulary, against grit_cider_reward with the collapse off, its determinism and freedom from host synchronisation,
and inside evaluate_metrics.

Bounds.  BLEU integers: equal.  ROUGE-L rows: bit-equal to the in-process host Rouge -- only IEEE double + x / with contraction
off are involved, so a differing row is a defect in operation order, not noise -- and rtol 1e-14 to the fixture (written under
another libm's pow for beta ** 2).  CIDEr rows: rtol 1e-11, the bound derived for this arithmetic in
tests/test_cider_device_gpu.py.  Corpus numbers from `aggregate`: BLEU and ROUGE equal to the host oracles', CIDEr rtol 1e-11."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, build_model, load, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 3


class Field(object):
    """The slice of the reference's TextField that the evaluation needs (datasets/caption/field.py:258-283)."""
    eos_token = '<eos>'

    def __init__(self, itos):
        self.itos = list(itos)

    def decode(self, rows, join_words=True):
        out = []
        for r in rows.tolist():
            words = []
            for i in r:
                if self.itos[i] == self.eos_token:
                    break
                words.append(self.itos[i])
            out.append(' '.join(words) if join_words else words)
        return out


def _vocab():
    return json.load(open(os.path.join(GOLDEN, "vocab_g10.json")))["itos"]


def _host_flow(field, tokens, caption_lists, collapse=True):
    """The reference's evaluation after beam search (engine/caption_engine.py:194-207) -> the three oracles' outputs."""
    from grit_amd.datasets.caption.metrics import Bleu, Cider, PTBTokenizer, Rouge
    gen, gts = {}, {}
    for i, words in enumerate(field.decode(tokens.cpu(), join_words=False)):
        gen[i] = [' '.join(k for k, _ in itertools.groupby(words)) if collapse else ' '.join(words)]
        gts[i] = list(caption_lists[i])
    gts, gen = PTBTokenizer.tokenize(gts), PTBTokenizer.tokenize(gen)
    comps = np.asarray([[c[0], c[1]] + c[2] + c[3] for c in Bleu().compute_components(gts, gen)], np.int32)
    return comps, Bleu().compute_score(gts, gen)[0], Rouge().compute_score(gts, gen), Cider().compute_score(gts, gen)


def _assert_rows(what, dev, comps, rouge_rows, cider_rows):
    d_comps, d_rouge, d_cider = (x.cpu().numpy() for x in dev)
    nz = cider_rows != 0
    rel = np.abs(d_cider - cider_rows)[nz] / np.abs(cider_rows[nz])
    print("%s: %d rows; non-zero correct[0] %d, ROUGE %d, CIDEr %d; BLEU integers differ in %d rows, ROUGE bits in %d, CIDEr max rel err %.3g"
          % (what, len(comps), int((comps[:, 6] > 0).sum()), int((rouge_rows > 0).sum()), int(nz.sum()),
             int((d_comps != comps).any(axis=1).sum()), int((d_rouge != rouge_rows).sum()), rel.max() if nz.any() else 0.0))
    assert d_comps.dtype == np.int32 and d_rouge.dtype == np.float64 and d_cider.dtype == np.float64
    np.testing.assert_array_equal(d_comps, comps)
    np.testing.assert_array_equal(d_rouge, rouge_rows)
    assert np.isfinite(d_cider).all()
    np.testing.assert_allclose(d_cider, cider_rows, rtol=1e-11, atol=0)


def _assert_corpus(what, got, bleu, rouge, cider):
    print("%s corpus: BLEU %r ROUGE %r CIDEr %r (host %r %r %r)" % (what, got['BLEU'], got['ROUGE'], got['CIDEr'], bleu, rouge, cider))
    assert sorted(got) == ['BLEU', 'CIDEr', 'ROUGE']
    assert got['BLEU'] == bleu and got['ROUGE'] == rouge
    np.testing.assert_allclose(got['CIDEr'], cider, rtol=1e-11, atol=0)


def test_g18_through_the_kernel():
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    g = json.load(open(os.path.join(GOLDEN, "metrics_g18.json")))
    fix = lambda d: {int(k): v for k, v in d.items()}
    gts, res = fix(g["gts"]), fix(g["res"])
    words = sorted({w for caps in list(gts.values()) + list(res.values()) for c in caps for w in c.split()})
    itos = ['<unk>', '<pad>', '<bos>', '<eos>'] + words
    stoi = {w: i for i, w in enumerate(itos)}
    field = Field(itos)
    T = max(len(res[k][0].split()) for k in gts) + 3
    for keys, ref in ((sorted(gts), g["scores"]), ([int(k) for k in g["short_keys"]], g["short_scores"])):
        rng = np.random.RandomState(18)
        rows = []
        for k in keys:
            ids = [stoi[w] for w in res[k][0].split()] + [EOS]
            rows.append(ids + [int(x) for x in rng.randint(0, len(itos), T - len(ids))])  # what follows <eos> is ignored
        tokens = torch.tensor(rows, dtype=torch.int64, device=DEV)
        captions = [gts[k] for k in keys]
        sc = DeviceCaptionScorer(captions, itos, device=DEV)
        # the fixture scores the hypotheses as they are (some repeat a word): the collapse is off here
        dev = sc.launch(tokens, collapse=False)
        assert all(x.is_cuda for x in dev) and dev[0].shape == (len(keys), 10)
        want = np.asarray([[c["testlen"], c["reflen"]] + c["guess"] + c["correct"] for c in g["bleu_components"]], np.int32)[keys]
        assert torch.equal(dev[0].cpu(), torch.from_numpy(want))
        comps, bleu, (rouge, rouge_rows), (cider, cider_rows) = _host_flow(field, tokens, captions, collapse=False)
        _assert_rows("G18 (%d rows)" % len(keys), dev, comps, rouge_rows, cider_rows)
        np.testing.assert_allclose(dev[1].cpu().numpy(), ref["ROUGE_rows"], rtol=1e-14, atol=0)
        np.testing.assert_allclose(dev[2].cpu().numpy(), ref["CIDEr_rows"], rtol=1e-11, atol=0)
        got = sc.aggregate(*dev)
        _assert_corpus("G18", got, bleu, rouge, cider)
        np.testing.assert_allclose(got['BLEU'], ref["BLEU"], rtol=1e-14, atol=0)
        np.testing.assert_allclose(got['ROUGE'], ref["ROUGE"], rtol=1e-14, atol=0)
        np.testing.assert_allclose(got['CIDEr'], ref["CIDEr"], rtol=1e-11, atol=0)


def _rows():
    """The adversarial rows of the CIDEr reward test (real vocabulary, 10 images with 1..7 references, punctuation, clitics,
    unseen n-grams, final-form and blank words, <eos> first, no <eos>) plus rows with repeated words: plain, blank, final-form,
    and a repeat that straddles the cut.  One item per row."""
    from grit_amd.datasets.caption.metrics.tokenizer import PUNCTUATIONS, ptb_tokens
    from tests.test_cider_device_gpu import _adversarial
    itos, _, captions, tokens, tokens2 = _adversarial()
    drop = set(PUNCTUATIONS)
    tok = lambda s: [x for x in ptb_tokens(s) if x not in drop]
    final = [i for i, w in enumerate(itos) if tok('zz ' + w)[1:] != tok('zz ' + w + ' zz')[1:-1]]
    blank = [i for i, w in enumerate(itos) if w.strip() == '']
    B, beam, T = tokens.shape
    rng = np.random.RandomState(1810)
    rows, caps = [], []
    for b in range(B):
        for j in range(beam):
            rows.append(tokens[b, j].tolist())
            caps.append(captions[b])
        base = tokens[b, 0].tolist()
        base = base[:base.index(EOS)] if EOS in base else base
        assert len(base) >= 3
        fill = lambda ids: (ids + [EOS] + [int(x) for x in rng.randint(0, len(itos), T)])[:T]
        f, bl = final[b % len(final)], blank[b % len(blank)]
        rows.append(fill([w for w in base[:6] for _ in range(2)] + base[6:10]))                  # every word twice
        rows.append(fill(base[:3] + [bl, bl, bl] + [base[2]] + base[3:8]))           # a word, blanks, the same word again
        rows.append(fill(base[:5] + [f, f]))                                                     # the final-form word twice, last
        rows.append(fill(base[:2] + [f, f, f] + base[2:6] + [bl, bl]))                           # ... in the middle, blanks last
        rows.append((base[:6] + [EOS] + [base[5]] * T)[:T])                                      # the repeat straddles the cut
        rows.append(fill([base[0]] * 9))                                                         # one word only, after the collapse
        caps.extend([captions[b]] * 6)
    for j in range(tokens2.shape[0]):
        rows.append(tokens2[j, 0].tolist())
        caps.append(captions[j])
    return itos, torch.tensor(rows, dtype=torch.int64), caps


def test_adversarial_rows_against_the_host_flow():
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos, tokens, caps = _rows()
    field = Field(itos)
    assert sorted({len(c) for c in caps}) == [1, 2, 3, 4, 5, 6, 7]
    sc = DeviceCaptionScorer(caps, itos, device=DEV)
    dev_tokens = tokens.to(DEV)
    for collapse in (True, False):
        comps, bleu, (rouge, rouge_rows), (cider, cider_rows) = _host_flow(field, tokens, caps, collapse=collapse)
        dev = sc.launch(dev_tokens, collapse=collapse)
        _assert_rows("adversarial, collapse %s" % collapse, dev, comps, rouge_rows, cider_rows)
        n = len(caps)
        for name, count in (("BLEU", (comps[:, 6] > 0).sum()), ("ROUGE", (rouge_rows > 0).sum()), ("CIDEr", (cider_rows > 0).sum())):
            assert count > n // 2, (name, count, n)  # the comparison is not about zeros
        assert (comps[:, 9] > 0).sum() >= 20 and (comps[:, 6] < comps[:, 2]).sum() >= 20  # 4-grams found; unigrams clipped or missing
        _assert_corpus("adversarial, collapse %s" % collapse, sc.aggregate(*dev), bleu, rouge, cider)
    shorter = _host_flow(field, tokens, caps, collapse=True)[0][:, 0] < _host_flow(field, tokens, caps, collapse=False)[0][:, 0]
    assert shorter.sum() >= 30  # the collapse matters


def test_without_the_collapse_the_cider_column_is_the_reward_kernel():
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos, tokens, caps = _rows()
    sc = DeviceCaptionScorer(caps, itos, device=DEV)
    dev_tokens = tokens.to(DEV)
    _, _, cider = sc.launch(dev_tokens, collapse=False)
    out32, out64 = sc.tables.reward(dev_tokens.view(len(caps), 1, -1), caps, return_float64=True)
    assert torch.equal(cider, out64.view(-1)) and (out64 > 0).sum() > len(caps) // 2
    assert not torch.equal(sc.launch(dev_tokens, collapse=True)[2], cider)


def test_bad_rows_are_reported_not_scored():
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos, tokens, caps = _rows()
    sc = DeviceCaptionScorer(caps[:8], itos, device=DEV)
    rows = tokens[:8].clone()
    rows[2, 1] = len(itos)       # outside the vocabulary in front of the cut
    rows[5, 0] = -7
    first = int((rows[3] == EOS).nonzero()[0]) if (rows[3] == EOS).any() else None
    if first is not None and first + 1 < rows.shape[1]:
        rows[3, first + 1] = len(itos) + 5  # behind the cut: ignored
    comps, rouge, cider = (x.cpu() for x in sc.launch(rows.to(DEV)))
    good = sc.launch(tokens[:8].to(DEV))
    for r in range(8):
        if r in (2, 5):
            assert (comps[r] == -1).all() and torch.isnan(rouge[r]) and torch.isnan(cider[r])
        else:
            assert torch.equal(comps[r], good[0][r].cpu()) and rouge[r] == good[1][r].cpu() and cider[r] == good[2][r].cpu()
    with pytest.raises(ValueError, match=r"rows \[2, 5\]"):
        sc.aggregate(*sc.launch(rows.to(DEV)))
    from grit_amd.lib import GritHipError
    with pytest.raises(GritHipError, match="not supported"):
        sc.launch(torch.full((8, 40), EOS, dtype=torch.int64, device=DEV))  # 40 words x 8 tokens > GRIT_CIDER_MAX_TOKENS


def test_determinism_and_no_synchronisation():
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos, tokens, caps = _rows()
    sc = DeviceCaptionScorer(caps, itos, device=DEV)
    tk = tokens.to(DEV)
    first = sc.launch(tk)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        second = sc.launch(tk)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    third = sc.launch(tk)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)  # bit-identical (NaN-free: every row is valid)
    assert not torch.isnan(first[1]).any() and not torch.isnan(first[2]).any()


class Loader(object):
    """A dataloader object: the split's scorer is cached on it."""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def test_evaluate_metrics_on_the_device_against_the_host(tmp_path, monkeypatch):
    """The small test model on the images of fixture G9, invented captions built around what the model says: the device
    scorer against the host scorer inside evaluate_metrics, the best checkpoint written by both, and a second evaluation of
    the split without any tokenisation."""
    from grit_amd.datasets.caption.metrics import tokenizer
    from grit_amd.engine.caption_engine import build_optimizers, evaluate_metrics
    from grit_amd.utils.misc import NestedTensor
    monkeypatch.chdir(tmp_path)
    g = load("sc_g9.npz")
    itos = _vocab()
    field = Field(itos)
    model, cfg = build_model(3, **{'model.dropout': 0.0, 'model.detector.dropout': 0.0})
    model.to(DEV)
    cfg.model.beam_size, cfg.model.beam_len = 5, 20
    opts = build_optimizers(model, cfg, mode='xe')
    images = t(g["images"], device=DEV)
    B = images.shape[0]
    sample = lambda lo, hi: NestedTensor(images[lo:hi], torch.zeros(hi - lo, *images.shape[-2:], dtype=torch.bool, device=DEV))
    cut = max(1, B // 2)
    batches = [{'samples': sample(0, cut)}, {'samples': sample(cut, B)}] if B > 1 else [{'samples': sample(0, B)}]
    tokens, _ = evaluate_metrics(model, None, batches, None, config=cfg)
    decoded = [w for out in tokens for w in field.decode(out.cpu(), join_words=False)]
    captions = []
    for b, words in enumerate(decoded):  # invented: built around what the model says, so that the scores are not all zero
        words = [k for k, _ in itertools.groupby(words)] or ['a']
        other = decoded[(b + 1) % B] or ['a']
        captions.append([' '.join(words).capitalize() + '.', ' '.join(words[:4] + other[2:7]) + ", isn't it?",
                         'A ' + ' '.join(other[:5]) + ' "' + words[-1] + '"'][:b % 3 + 1])
    at = 0
    for batch in batches:
        n = batch['samples'].tensors.shape[0]
        batch['captions'] = captions[at:at + n]
        at += n
    loader = Loader(batches)
    results = {}
    for kind in ('host', 'device'):
        scores = {}
        out = evaluate_metrics(model, opts, loader, field, epoch=3, split='valid', config=cfg, best_cider=0.0, scorer=kind,
                               scores_out=scores)
        assert out == scores['CIDEr'] and os.path.exists('checkpoint_best_valid.pth')
        ckpt = torch.load('checkpoint_best_valid.pth', map_location='cpu')  # the weights-only default, as train_caption.main reads it
        assert ckpt['epoch'] == 3 and ckpt['scores']['BLEU'] == scores['BLEU']
        os.remove('checkpoint_best_valid.pth')
        results[kind] = scores
        print(kind, scores)
    h, d = results['host'], results['device']
    assert h['BLEU'] == d['BLEU'] and h['ROUGE'] == d['ROUGE'] and h['CIDEr'] > 0 and h['BLEU'][3] > 0 and h['ROUGE'] > 0
    np.testing.assert_allclose(d['CIDEr'], h['CIDEr'], rtol=1e-11, atol=0)
    again, _ = evaluate_metrics(model, None, batches, None, config=cfg)
    assert all(torch.equal(a, b) for a, b in zip(again, tokens))  # same tokens under both scorers' evaluations
    # the second evaluation of the split: the cached scorer, no tokenisation
    cached = loader._grit_caption_scorers
    assert len(cached) == 1
    calls = []
    real = tokenizer.ptb_tokens
    monkeypatch.setattr(tokenizer, 'ptb_tokens', lambda s: calls.append(s) or real(s))
    second = evaluate_metrics(model, None, loader, field, config=cfg, scorer='device')
    assert calls == [] and loader._grit_caption_scorers is cached and len(cached) == 1
    assert second['BLEU'] == d['BLEU'] and second['ROUGE'] == d['ROUGE'] and second['CIDEr'] == d['CIDEr']
