"""The CIDEr-D reward kernel (grit_cider_reward, grit_amd/csrc/cider.hip) on the device: against the reference-generated scores
of fixture G14, against the host reward_fn on adversarial rows over the real vocabulary, its determinism and freedom from host
synchronisation, and inside train_sc_step.

Bounds.  float64 output: rtol 1e-11 -- every score is a sum of non-negative terms (idf >= 0), fewer than 200 roundings of
1.1e-16 plus exp / sqrt / division at <= 1 ulp each give about 3e-14; 1e-11 leaves two orders for a different libm and is four
orders below float32 resolution.  float32 output: at most one float32 ulp from float32(reference) (double rounding)."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, build_model, disable_drop_path, load, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 3


class Field(object):
    """The slice of the reference's TextField that the reward needs: vocabulary and decode (datasets/caption/field.py:258-283)."""
    eos_token = '<eos>'

    def __init__(self, itos):
        self.itos = list(itos)

    def decode(self, rows):
        out = []
        for r in rows.tolist():
            words = []
            for i in r:
                if self.itos[i] == self.eos_token:
                    break
                words.append(self.itos[i])
            out.append(' '.join(words))
        return out


def _vocab():
    return json.load(open(os.path.join(GOLDEN, "vocab_g10.json")))["itos"]


def _host_float64(cider, field, tokens, captions):
    """cider_reward_fn's host pipeline (engine/caption_engine.py) without its final cast to float32."""
    from grit_amd.datasets.caption.metrics import PTBTokenizer
    B, beam, T = tokens.shape
    gen = PTBTokenizer.tokenize(field.decode(tokens.view(-1, T).cpu()))
    gts = PTBTokenizer.tokenize(list(itertools.chain(*([c] * beam for c in captions))))
    return cider.compute_score(gts, gen)[1].reshape(B, beam)


def _assert_scores(dev32, dev64, ref64, what):
    dev32, dev64 = dev32.cpu().numpy(), dev64.cpu().numpy()
    ref32 = ref64.astype(np.float32)
    rel = np.abs(dev64 - ref64) / np.maximum(np.abs(ref64), 1e-300)
    ulps = np.abs(dev32.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)
    print("%s: %d rows, %d non-zero, float64 max rel err %.3g, float32 max ulp %.3g" %
          (what, ref64.size, int((ref64 != 0).sum()), rel[ref64 != 0].max() if (ref64 != 0).any() else 0.0, ulps.max()))
    assert np.isfinite(dev64).all() and np.isfinite(dev32).all()
    np.testing.assert_allclose(dev64, ref64, rtol=1e-11, atol=0)
    assert (ulps <= 1.0).all(), (what, ulps.max())


def test_g14_through_the_kernel():
    from grit_amd.datasets.caption.metrics import Cider
    from grit_amd.ops.cider import DeviceCider
    g = json.load(open(os.path.join(GOLDEN, "cider_g14.json")))
    fix = lambda d: {int(k): v for k, v in d.items()}
    train, gts, res = fix(g["train"]), fix(g["gts"]), fix(g["res"])
    words = sorted({w for caps in list(train.values()) + list(gts.values()) + list(res.values()) for c in caps for w in c.split()})
    itos = ['<unk>', '<pad>', '<bos>', '<eos>'] + words
    stoi = {w: i for i, w in enumerate(itos)}
    keys = sorted(gts)
    T = max(len(res[k][0].split()) for k in keys) + 3
    rng = np.random.RandomState(14)
    rows = []
    for k in keys:
        ids = [stoi[w] for w in res[k][0].split()] + [EOS]
        rows.append(ids + [int(x) for x in rng.randint(0, len(itos), T - len(ids))])  # what follows <eos> is ignored
    tokens = torch.tensor(rows, dtype=torch.int64, device=DEV).view(len(keys), 1, T)
    dc = DeviceCider(Cider(train), itos, device=DEV)
    out32, out64 = dc.reward(tokens, [gts[k] for k in keys], return_float64=True)
    assert out32.shape == (len(keys), 1) and out32.dtype == torch.float32 and out32.is_cuda
    _assert_scores(out32, out64, np.asarray(g["scores"], np.float64).reshape(-1, 1), "G14")


def _adversarial():
    """Real vocabulary, a synthetic corpus, B = 10 images with 1..7 references, beam = 8 rows per image, T = 20."""
    from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
    from grit_amd.datasets.caption.metrics.tokenizer import PUNCTUATIONS, ptb_tokens
    itos = _vocab()
    stoi = {w: i for i, w in enumerate(itos)}
    rng = np.random.RandomState(355)
    drop = set(PUNCTUATIONS)
    tok = lambda s: [x for x in ptb_tokens(s) if x not in drop]
    plain = [i for i, w in enumerate(itos) if w.isalpha() and w.islower() and len(tok('zz ' + w + ' zz')) == 3]
    special = [i for i, w in enumerate(itos)
               if len(tok('zz ' + w + ' zz')) != 3 or tok('zz ' + w)[1:] != tok('zz ' + w + ' zz')[1:-1]]
    final = [i for i in special if tok('zz ' + itos[i])[1:] != tok('zz ' + itos[i] + ' zz')[1:-1]]
    blank = [i for i in special if itos[i].strip() == '' ]
    assert len(special) == 19 and final and blank
    common = [int(x) for x in rng.choice(plain, 60, replace=False)]  # a small pool, so that n-grams repeat across captions

    def sentence(n, pool=common):
        return [itos[int(rng.choice(pool))] for _ in range(n)]

    corpus = {i: [' '.join(sentence(int(rng.randint(5, 14)))) for _ in range(int(rng.randint(1, 8)))] for i in range(300)}
    cider = Cider(PTBTokenizer.tokenize(corpus))

    fresh = [int(x) for x in rng.choice([i for i in plain if i not in common], 12, replace=False)]  # never in the corpus
    B, beam, T = 10, 8, 20
    captions, rows, firsts = [], [], []
    for b in range(B):
        refs = []
        for r in range(b % 7 + 1):
            words = sentence(int(rng.randint(3, 16)))
            if r % 3 == 0:  # n-grams absent from the corpus statistics
                at = int(rng.randint(0, len(words)))
                words[at:at] = [itos[fresh[(b + j) % len(fresh)]] for j in range(3)]
            text = ' '.join(words)
            text = [text.capitalize() + '.', 'The ' + words[0] + "'s " + text + ", isn't it?", '"' + text + '" (they\'re ' + words[-1] + ')',
                    text + ' -- zyxwvq Qwertyuiop\'s ' + words[0] + '!', text][r % 5]
            refs.append(text)
        captions.append(refs)
        ref_ids = [stoi[w] for w in ' '.join(refs).lower().replace(',', ' ').replace('.', ' ').split() if w in stoi and stoi[w] != EOS]
        first = [stoi[w] for w in refs[0].lower().rstrip('.').split() if w in stoi and stoi[w] != EOS]
        firsts.append(first)
        fill = lambda ids: (ids + [EOS] + [int(x) for x in rng.randint(0, len(itos), T)])[:T]
        three = [itos[fresh[(b + j) % len(fresh)]] for j in range(3)]
        rows.append(fill(first[:T - 1]))                                                      # a reference itself
        rows.append(fill([stoi[w] for w in three] * 2 + ref_ids[:6]))                         # unseen n-grams, repeated
        rows.append(fill((ref_ids[:2] * 10)[:T - 4]))                                         # one bigram over and over: clipping
        rows.append(fill(ref_ids[:5] + [final[b % len(final)]]))                              # final-period word last
        rows.append(fill(ref_ids[:4] + [final[b % len(final)], blank[b % len(blank)], blank[(b + 1) % len(blank)]]))  # last but whitespace
        rows.append(fill([final[b % len(final)]] + ref_ids[:4] + [special[(b + j) % 19] for j in range(5)]))  # in the middle
        rows.append([EOS] + [int(x) for x in rng.randint(0, len(itos), T - 1)])               # <eos> first
        noeos = [int(x) for x in rng.choice(ref_ids + special, T)]                            # no <eos> at all
        rows.append([x if x != EOS else special[4] for x in noeos])
    # every special id appears in front of an <eos> somewhere
    extra = [fill(firsts[j // 2][:4] + [special[(j + s) % 19] for s in range(7)] + firsts[j // 2][4:8]) for j in range(0, 19, 2)]
    tokens = torch.tensor(rows, dtype=torch.int64).view(B, beam, T)
    tokens2 = torch.tensor(extra, dtype=torch.int64).view(len(extra), 1, T)
    return itos, cider, captions, tokens, tokens2


def test_adversarial_rows_against_the_host_reward_fn():
    from grit_amd.engine.caption_engine import cider_reward_fn
    from grit_amd.ops.cider import DeviceCider
    itos, cider, captions, tokens, tokens2 = _adversarial()
    field = Field(itos)
    dc = DeviceCider(cider, itos, device=DEV)
    host_fn = cider_reward_fn(cider, field)
    for what, tk, caps in (("adversarial", tokens, captions), ("specials", tokens2, captions[:tokens2.shape[0]])):
        assert sorted({len(c) for c in captions}) == [1, 2, 3, 4, 5, 6, 7]
        ref64 = _host_float64(cider, field, tk, caps)
        host32 = host_fn(tk, {'captions': caps}).numpy()
        np.testing.assert_array_equal(host32, ref64.astype(np.float32))  # the float64 reference IS the host reward before its cast
        out32, out64 = dc.reward(tk.to(DEV), caps, return_float64=True)
        _assert_scores(out32, out64, ref64, what)
        assert (ref64 > 0).sum() >= ref64.size // 2, what  # the comparison is not about zeros
        if what == "adversarial":
            assert (ref64[:, 6] == 0).all()  # <eos> first: an empty hypothesis scores 0


def test_determinism_no_synchronisation_no_tokenisation(monkeypatch):
    from grit_amd.datasets.caption.metrics import tokenizer
    from grit_amd.engine.caption_engine import cider_reward_fn
    itos, cider, captions, tokens, _ = _adversarial()
    fn = cider_reward_fn(cider, Field(itos), reward='device')
    tk = tokens.to(DEV)
    batch = {'captions': captions}
    first = fn(tk, batch)
    assert first.is_cuda and first.dtype == torch.float32 and first.shape == tokens.shape[:2]
    calls = []
    real = tokenizer.ptb_tokens
    monkeypatch.setattr(tokenizer, 'ptb_tokens', lambda s: calls.append(s) or real(s))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        second = fn(tk, batch)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert calls == []  # an image seen before is not tokenised again
    third = fn(tk, batch)
    assert torch.equal(first, second) and torch.equal(first, third)  # bit-identical
    assert calls == []


def test_device_reward_inside_the_self_critical_step():
    """The model and images of test_self_critical_step_on_hip_path_matches_reference (fixture G9, same tokens as the fixture,
    unconditionally), invented captions, a corpus Cider: train_sc_step with the device reward against the host reward."""
    from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
    from grit_amd.engine.caption_engine import build_optimizers, cider_reward_fn, train_sc_step
    from grit_amd.utils.misc import NestedTensor
    g = load("sc_g9.npz")
    itos = _vocab()
    field = Field(itos)
    B, beam, T = g["tokens"].shape
    rng = np.random.RandomState(9)
    decoded = field.decode(torch.from_numpy(g["tokens"]).view(-1, T))
    captions = []
    for b in range(B):  # invented: built around what the model says, so that the rewards are not all zero
        words = decoded[b * beam].split() or ['a']
        other = decoded[b * beam + beam - 1].split() or ['a']
        captions.append([' '.join(words).capitalize() + '.', ' '.join(words[:4] + other[2:7]) + ", isn't it?",
                         'A ' + ' '.join(other[:5]) + ' "' + words[-1] + '"'][:b % 3 + 1])
    corpus = {i: c for i, c in enumerate(captions)}
    for i in range(50):
        corpus[B + i] = [' '.join(itos[int(x)] for x in rng.randint(4, 400, int(rng.randint(4, 12))))]
    cider = Cider(PTBTokenizer.tokenize(corpus))
    results = {}
    for kind in ('host', 'device'):
        model, cfg = build_model(3, **{'model.dropout': 0.0, 'model.detector.dropout': 0.0})
        model.train().to(DEV)
        disable_drop_path(model)
        cfg.model.beam_size, cfg.model.beam_len = beam, T
        opts = build_optimizers(model, cfg, mode='sc')
        inner = cider_reward_fn(cider, field, reward=kind)
        seen = {}

        def reward_fn(tokens, batch, inner=inner, seen=seen):
            seen['tokens'] = tokens.cpu()
            seen['reward'] = inner(tokens, batch)
            return seen['reward']

        images = t(g["images"], device=DEV)
        batch = {'samples': NestedTensor(images, torch.zeros(images.shape[0], *images.shape[-2:], dtype=torch.bool, device=DEV)),
                 'captions': captions}
        loss, reward, baseline = train_sc_step(model, batch, opts, reward_fn, cfg)
        np.testing.assert_array_equal(seen['tokens'].numpy(), g["tokens"])
        results[kind] = (loss.item(), reward.item(), baseline.item(), seen['reward'].cpu().numpy())
        del model, opts
    assert results['device'][3].dtype == np.float32 and (results['host'][3] > 0).any()
    print("sc step host   loss %.9g reward %.9g baseline %.9g" % results['host'][:3])
    print("sc step device loss %.9g reward %.9g baseline %.9g" % results['device'][:3])
    ulp = 2.0 ** -23
    for i, name in ((1, 'reward'), (2, 'baseline')):
        h, d = results['host'][i], results['device'][i]
        assert abs(d - h) <= 2 * ulp * abs(h), (name, h, d)
    h, d = results['host'][0], results['device'][0]
    assert abs(d - h) < 2e-3 * abs(h) + 1e-7, (h, d)  # the loss bound of the fixture's own test
