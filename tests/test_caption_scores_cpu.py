"""The evaluation's caption scores without a GPU: the host scorers (datasets/caption/metrics/{bleu,rouge}.py, compute_scores)
against the reference-generated fixture G18 and on the edge rules; the host side of the device scorer
(grit_amd/ops/caption_scores.py: the collapse + expansion mirror against the tokenizer, the per-reference arrays); and the
public switches (evaluate_metrics(scorer=...), config.exp.eval_scorer, the evaluation inside train_caption.main).

Bound.  rtol 1e-14 against the fixture: it was written under one libm and is read under another; pow, exp and sqrt are within
1 ulp each and at most a handful compose, so 1e-14 (about 45 ulp) is margin, not fit.  The BLEU integers are equal."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN

EOS = 3
RTOL = 1e-14


def _vocab():
    return json.load(open(os.path.join(GOLDEN, "vocab_g10.json")))["itos"]


def _g18():
    g = json.load(open(os.path.join(GOLDEN, "metrics_g18.json")))
    fix = lambda d: {int(k): v for k, v in d.items()}
    return g, fix(g["gts"]), fix(g["res"])


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


# ---- host scorers against G18 ---------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases():
    g, gts, res = _g18()
    comps = g["bleu_components"]
    n = len(comps)
    assert n == 48 and {len(v) for v in gts.values()} == set(range(1, 8))
    assert sum(1 for v in res.values() if v[0] == '') >= 3
    for name in ("ROUGE_rows", "CIDEr_rows"):
        assert sum(1 for x in g["scores"][name] if x > 0) > n // 2
    assert sum(1 for c in comps if c["correct"][0] > 0) > n // 2 and any(c["correct"][3] > 0 for c in comps)
    sub = [comps[int(k)] for k in g["short_keys"]]
    assert sum(c["testlen"] for c in comps) > sum(c["reflen"] for c in comps)  # no corpus brevity penalty in the full set ...
    assert sub and sum(c["testlen"] for c in sub) < sum(c["reflen"] for c in sub)  # ... so the subset exercises it


def test_host_scorers_against_the_reference_scores():
    from grit_amd.datasets.caption.metrics import Bleu, Cider, Rouge, compute_scores
    g, gts, res = _g18()
    got = Bleu().compute_components(gts, res)
    want = [(c["testlen"], c["reflen"], c["guess"], c["correct"]) for c in g["bleu_components"]]
    assert [tuple(x) for x in got] == want
    for keys, ref in ((sorted(gts), g["scores"]), ([int(k) for k in g["short_keys"]], g["short_scores"])):
        sub_gts, sub_res = {k: gts[k] for k in keys}, {k: res[k] for k in keys}
        bleu, per_image = Bleu().compute_score(sub_gts, sub_res)
        rouge, rouge_rows = Rouge().compute_score(sub_gts, sub_res)
        cider, cider_rows = Cider().compute_score(sub_gts, sub_res)
        print("BLEU %r\n     %r\nROUGE %r %r CIDEr %r %r" % (bleu, ref["BLEU"], rouge, ref["ROUGE"], cider, ref["CIDEr"]))
        assert len(bleu) == 4 and len(per_image) == 4 and all(len(p) == len(keys) for p in per_image)
        np.testing.assert_allclose(bleu, ref["BLEU"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(rouge_rows, ref["ROUGE_rows"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(rouge, ref["ROUGE"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(cider_rows, ref["CIDEr_rows"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(cider, ref["CIDEr"], rtol=RTOL, atol=0)
        score, scores = compute_scores(sub_gts, sub_res)
        assert sorted(score) == ['BLEU', 'CIDEr', 'ROUGE'] and sorted(scores) == ['BLEU', 'CIDEr', 'ROUGE']  # no METEOR
        assert score['BLEU'] == bleu and score['ROUGE'] == rouge and score['CIDEr'] == cider


def test_edge_rules():
    from grit_amd.datasets.caption.metrics import Bleu, Rouge
    from grit_amd.datasets.caption.metrics.bleu import components
    # an empty hypothesis: no division by zero, every score 0
    bleu, rows = Bleu().compute_score({0: ['a dog runs']}, {0: ['']})
    assert components('', ['a dog runs']) == (0, 3, [0, 0, 0, 0], [0, 0, 0, 0])
    assert all(0 <= b < 1e-6 for b in bleu) and all(0 <= r[0] < 1e-6 for r in rows)
    assert Rouge().compute_score({0: ['a dog runs']}, {0: ['']})[0] == 0.0
    # split(" ") makes the empty string ONE empty token: empty against empty is a full match
    assert Rouge().compute_score({0: ['']}, {0: ['']})[0] == 1.0
    assert Rouge().compute_score({0: ['', 'a dog']}, {0: ['']})[1][0] == 1.0
    # closest reference length: a tie goes to the shorter reference
    six = 'a b c d e f'
    assert components(six, ['a b c d e f g', 'a b c d e'])[1] == 5
    assert components(six, ['a b c d e', 'a b c d e f g'])[1] == 5
    assert components(six, ['a b c d e f g h', 'a b c d e f g'])[1] == 7
    # clipping: the largest count in any ONE reference, not the sum over references
    assert components('a a a a', ['a a b', 'a c'])[3] == [2, 1, 0, 0]
    # a single-reference image: the hypothesis equal to it scores 1 in every metric that is a ratio
    bleu, _ = Bleu().compute_score({0: ['a dog runs in the park']}, {0: ['a dog runs in the park']})
    np.testing.assert_allclose(bleu, [1.0] * 4, rtol=1e-8)
    assert Rouge().compute_score({0: ['a dog runs in the park']}, {0: ['a dog runs in the park']})[0] == 1.0
    # ROUGE-L by hand: lcs('a b c d', 'a c d e f') = 3, p = 3/4, r = 3/5
    p, r, b2 = 3 / 4.0, 3 / 5.0, 1.2 ** 2
    assert Rouge().compute_score({0: ['a c d e f']}, {0: ['a b c d']})[0] == ((1 + b2) * p * r) / float(r + b2 * p)


# ---- the packer -----------------------------------------------------------------------------------------------------------------
def _special_ids(itos):
    from grit_amd.datasets.caption.metrics.tokenizer import PUNCTUATIONS, ptb_tokens
    drop = set(PUNCTUATIONS)
    tok = lambda s: [t for t in ptb_tokens(s) if t not in drop]
    final = [i for i, w in enumerate(itos) if tok('zz ' + w)[1:] != tok('zz ' + w + ' zz')[1:-1]]
    multi = [i for i, w in enumerate(itos) if len(tok('zz ' + w + ' zz')) != 3 or i in final]
    blank = [i for i, w in enumerate(itos) if w.strip() == '']
    return final, multi, blank


def test_collapse_and_expansion_equal_the_tokenizer_on_the_collapsed_string():
    from grit_amd.datasets.caption.metrics import PTBTokenizer
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos = _vocab()
    sc = DeviceCaptionScorer([["a dog sits.", "A dog runs"], ["a cat sits"]], itos, device='cpu')
    final, multi, blank = _special_ids(itos)
    assert final and blank and EOS in multi
    strings = None
    rng = np.random.RandomState(1818)
    mismatches, collapsed, blank_runs, final_runs = [], 0, 0, 0
    for r in range(6000):
        n = int(rng.randint(0, 21))
        row = []
        while len(row) < n:
            w = int(rng.choice(multi)) if rng.rand() < 0.25 else int(rng.randint(0, len(itos)))
            kind = rng.rand()
            if kind < 0.08:
                w = int(rng.choice(blank))
            elif kind < 0.16:
                w = int(rng.choice(final))
            row += [w] * (int(rng.randint(2, 4)) if rng.rand() < 0.3 else 1)  # runs of a word, blank and final-form words included
        row = row[:n]
        if n and rng.rand() < 0.6:
            row[int(rng.randint(0, n))] = EOS  # (a run may straddle the cut)
        cut = row.index(EOS) if EOS in row else len(row)
        words = [itos[t] for t in row[:cut]]
        runs = [(k, len(list(grp))) for k, grp in itertools.groupby(row[:cut])]
        collapsed += any(c > 1 for _, c in runs)
        blank_runs += any(c > 1 and k in blank for k, c in runs)
        final_runs += any(c > 1 and k in final for k, c in runs)
        want = PTBTokenizer.tokenize([' '.join(k for k, _ in itertools.groupby(words))])[0][0].split()
        strings = sc.tables.token_strings()
        got = [strings[t] for t in sc.expand(row)]
        if got != want:
            mismatches.append((row, got, want))
        plain = PTBTokenizer.tokenize([' '.join(words)])[0][0].split()
        assert [strings[t] for t in sc.expand(row, collapse=False)] == plain
    assert collapsed > 1000 and blank_runs > 50 and final_runs > 50
    assert not mismatches, "%d rows differ, e.g. %r" % (len(mismatches), mismatches[0])


def test_reference_arrays_hold_the_counts_lengths_and_sequences():
    from grit_amd.datasets.caption.metrics.cider import ngram_counts
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos = _vocab()
    captions = [["A man's dog, isn't it?", "the DOG runs the dog."], ["."], ['Two cats -- and "a dog" and a dog', "two cats"],
                ["A man's dog, isn't it?", "the DOG runs the dog."]]
    sc = DeviceCaptionScorer(captions, itos, device='cpu')
    assert sc.slots == [0, 1, 2, 0] and len(sc) == 4  # the same references share a slot
    a = sc.tables.host_arrays()
    strings = sc.tables.token_strings()
    assert strings[sc.empty_token] == ''
    flat = [s for slot in (0, 1, 2) for s in sc.gts[slot]]
    assert flat[2] == '' and len(flat) == len(a['ref_words'])
    for r, sentence in enumerate(flat):
        assert a['ref_words'][r] == len(sentence.split())
        seq = [strings[t] for t in a['seq_tok'][a['seq_start'][r]:a['seq_start'][r + 1]]]
        assert seq == sentence.split(' ')  # the empty reference is one empty token
        counts = ngram_counts(sentence)
        seen = {}
        for k in range(4):
            for e in range(a['ref_ent_start'][4 * r + k], a['ref_ent_start'][4 * r + k + 1]):
                ngram = tuple(strings[t] for t in a['ent_tok'][e][:k + 1])
                assert all(t == -1 for t in a['ent_tok'][e][k + 1:])
                seen[ngram] = int(a['ent_tf'][e])
        assert seen == dict(counts)
    assert a['ent_tf'].max() == 2 and len(a['ent_tf']) == len(a['ent_w'])


def test_a_vocabulary_with_a_duplicated_word_is_refused():
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    with pytest.raises(ValueError, match="more than one id.*'dog'"):
        DeviceCaptionScorer([["a dog"]], ['<unk>', '<pad>', '<bos>', '<eos>', 'a', 'dog', 'dog'], device='cpu')
    with pytest.raises(ValueError, match="at least one reference"):
        DeviceCaptionScorer([["a dog"], []], ['<unk>', '<pad>', '<bos>', '<eos>', 'a', 'dog'], device='cpu')


def test_aggregate_uses_the_host_formulas():
    from grit_amd.datasets.caption.metrics import Bleu, Cider, Rouge
    from grit_amd.ops.caption_scores import DeviceCaptionScorer, aggregate_host
    g, gts, res = _g18()
    comps = np.asarray([[c["testlen"], c["reflen"]] + c["guess"] + c["correct"] for c in g["bleu_components"]], np.int32)
    rouge, cider = Rouge().compute_score(gts, res)[1], Cider().compute_score(gts, res)[1]
    for how in ('numpy', 'torch'):
        if how == 'numpy':
            out = aggregate_host(comps, rouge, cider)
        else:
            out = DeviceCaptionScorer.aggregate(torch.from_numpy(comps), torch.from_numpy(rouge), torch.from_numpy(cider))
        assert out['BLEU'] == Bleu().compute_score(gts, res)[0]
        assert out['ROUGE'] == Rouge().compute_score(gts, res)[0] and out['CIDEr'] == Cider().compute_score(gts, res)[0]
    bad = comps.copy()
    bad[3] = -1
    with pytest.raises(ValueError, match=r"rows \[3\]"):
        aggregate_host(bad, rouge, cider)


def _lcs_by_diagonals(hyp, ref):
    """The kernel's sweep: cell (i, j) on diagonal i + j, three rotating diagonals, [i + 1] = hypothesis position i."""
    Lh, Lr = len(hyp), len(ref)
    diag = [[0] * (Lh + 1) for _ in range(3)]
    left = [0] * Lh
    for d in range(Lh + Lr - 1 if Lr else 0):
        cur, prev1, prev2 = diag[d % 3], diag[(d + 2) % 3], diag[(d + 1) % 3]
        for i in range(Lh):  # one thread each; they read only the two earlier diagonals
            j, v = d - i, 0
            if 0 <= j < Lr:
                v = prev2[i] + 1 if ref[j] == hyp[i] else max(prev1[i], left[i])
                left[i] = v
            cur[i + 1] = v
    return left[Lh - 1]


def _walk(sc, arrays, row, slot, collapse=True):
    """The kernel's steps 3 and 4 over the packed arrays in plain Python: the ten BLEU integers and ROUGE-L of one row."""
    from grit_amd.datasets.caption.metrics.rouge import BETA
    toks = sc.expand(row, collapse=collapse)
    L = len(toks)
    r0, r1 = arrays['slot_ref_start'][slot], arrays['slot_ref_start'][slot + 1]
    correct = [0] * 4
    for k in range(4):
        seen = set()
        for i in range(L - k):
            ngram = tuple(toks[i:i + k + 1])
            if ngram in seen:
                continue
            seen.add(ngram)
            tf = sum(1 for j in range(L - k) if tuple(toks[j:j + k + 1]) == ngram)
            best = 0
            for r in range(r0, r1):
                for e in range(arrays['ref_ent_start'][4 * r + k], arrays['ref_ent_start'][4 * r + k + 1]):
                    if tuple(arrays['ent_tok'][e]) == ngram + (-1,) * (3 - k):
                        best = max(best, int(arrays['ent_tf'][e]))
            correct[k] += min(tf, best)
    reflen, gap = 0, None
    prec, rec = 0.0, 0.0
    hyp = toks if L else [sc.empty_token]
    for r in range(r0, r1):
        words = int(arrays['ref_words'][r])
        if gap is None or abs(words - L) < gap or (abs(words - L) == gap and words < reflen):
            gap, reflen = abs(words - L), words
        ref = [int(x) for x in arrays['seq_tok'][arrays['seq_start'][r]:arrays['seq_start'][r + 1]]]
        lcs = _lcs_by_diagonals(hyp, ref)
        prec, rec = max(prec, lcs / float(len(hyp))), max(rec, lcs / float(len(ref)))
    b2 = BETA ** 2
    rouge = ((1 + b2) * prec * rec) / float(rec + b2 * prec) if prec != 0 and rec != 0 else 0.0
    return [L, reflen] + [max(0, L - k) for k in range(4)] + correct, rouge


def test_the_kernels_steps_over_the_packed_arrays_give_the_host_scores():
    from grit_amd.datasets.caption.metrics import Bleu, PTBTokenizer, Rouge
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos = _vocab()
    stoi = {w: i for i, w in enumerate(itos)}
    final, multi, blank = _special_ids(itos)
    rng = np.random.RandomState(418)
    pool = [w for w in itos if w.isalpha() and w.islower()][:25]
    captions, rows = [], []
    for b in range(42):
        refs = []
        for r in range(b % 7 + 1):
            words = [pool[int(x)] for x in rng.randint(0, len(pool), int(rng.randint(3, 13)))]
            text = ' '.join(words)
            refs.append([text.capitalize() + '.', 'The ' + words[0] + "'s " + text + ", isn't it?", text, '.', text + ' -- ' + words[0] + '!'][(b + r) % 5])
        captions.append(refs)
        ids = [stoi[w] for w in ' '.join(refs).lower().replace(',', ' ').replace('.', ' ').split() if w in stoi and stoi[w] != EOS]
        kind = b % 6
        hyp = [ids[:9], [w for w in ids[:5] for _ in range(2)], [], (ids[:2] * 8)[:14], ids[2:7] + [final[b % len(final)]] * 2,
               ids[:3] + [blank[b % len(blank)]] * 2 + ids[2:6]][kind]
        rows.append((hyp + [EOS] + [int(x) for x in rng.randint(0, len(itos), 20)])[:20])
    sc = DeviceCaptionScorer(captions, itos, device='cpu')
    arrays = sc.tables.host_arrays()
    field = Field(itos)
    for collapse in (True, False):
        gen = {}
        for i, words in enumerate(field.decode(torch.tensor(rows), join_words=False)):
            gen[i] = [' '.join(k for k, _ in itertools.groupby(words)) if collapse else ' '.join(words)]
        gen = PTBTokenizer.tokenize(gen)
        want = [[c[0], c[1]] + c[2] + c[3] for c in Bleu().compute_components(sc.gts, gen)]
        rouge = Rouge().compute_score(sc.gts, gen)[1]
        got = [_walk(sc, arrays, row, sc.slots[i], collapse) for i, row in enumerate(rows)]
        assert [g[0] for g in got] == want
        assert [g[1] for g in got] == list(rouge)  # bit-equal: the same IEEE operations in the same order
        assert sum(1 for w in want if w[6] > 0) > 21 and (rouge > 0).sum() > 21 and sum(1 for w in want if w[6] < w[2]) > 5
    assert any('' in sc.gts[i] for i in sc.gts) and sum(1 for r in rows if r[0] == EOS) == 7  # empty references and hypotheses


# ---- engine and training loop ---------------------------------------------------------------------------------------------------
ITOS = ['<unk>', '<pad>', '<bos>', '<eos>', 'a', 'dog', 'cat', 'sits', 'runs', 'on', 'the', 'mat', 'bench', 'red', "isn't"]
STOI = {w: i for i, w in enumerate(ITOS)}


def _ids(text, T=10):
    ids = [STOI[w] for w in text.split()] + [EOS]
    return ids + [STOI['mat']] * (T - len(ids))  # what follows <eos> is ignored


class StubModel(torch.nn.Module):
    """Returns, as the best beam of every image, the tokens the batch carries in batch['samples'][:, self.variant]."""

    def __init__(self, detector=None, config=None):
        super().__init__()
        self.fc = torch.nn.Linear(2, 2)
        self.detector = torch.nn.Linear(2, 2)
        self.variant = 0

    def forward(self, samples, seq=None, use_beam_search=True, **kw):
        assert use_beam_search and kw['out_size'] == 1 and not self.training
        return samples[:, self.variant].clone(), None


def _loader():
    captions = [["A dog sits on the mat.", "the dog sits on a red mat"], ["a cat runs on the bench", "A red cat runs!"],
                ["the dog runs", "a dog runs on the mat", "the red dog isn't on the bench"]]
    good = ["a dog sits sits on the the mat", "a red cat runs on the bench", "the dog isn't on the mat"]
    poor = ["a cat on the bench", "dog dog dog", "a a red mat"]
    samples = torch.tensor([[_ids(g), _ids(p)] for g, p in zip(good, poor)], dtype=torch.int64)
    return [{'samples': samples[:2], 'captions': captions[:2]}, {'samples': samples[2:], 'captions': captions[2:]}], captions, good, poor


def _optimizers(model):
    return {'model': torch.optim.Adam(model.fc.parameters()), 'backbone': torch.optim.Adam(model.detector.parameters()), 'mode': 'xe'}


def test_evaluate_metrics_host_scorer_and_the_best_checkpoint(tmp_path, monkeypatch):
    from grit_amd.config import default_config
    from grit_amd.datasets.caption.metrics import PTBTokenizer, compute_scores
    from grit_amd.engine.caption_engine import evaluate_metrics
    monkeypatch.chdir(tmp_path)
    cfg = default_config()
    assert cfg.exp.eval_scorer == 'device'
    loader, captions, good, poor = _loader()
    model, field = StubModel(), Field(ITOS)
    collapse = lambda s: ' '.join(k for k, _ in itertools.groupby(s.split()))
    assert collapse(good[0]) == "a dog sits on the mat" != good[0]
    keys = ['0_0', '0_1', '1_0']
    want = compute_scores(PTBTokenizer.tokenize(dict(zip(keys, captions))),
                          PTBTokenizer.tokenize({k: [collapse(s)] for k, s in zip(keys, good)}))[0]
    scores = evaluate_metrics(model.train(), None, loader, field, config=cfg, scorer='host')
    assert not model.training
    assert scores == want and scores['CIDEr'] > 0 and len(scores['BLEU']) == 4 and sorted(scores) == ['BLEU', 'CIDEr', 'ROUGE']
    # a callable and None behave as before
    seen = {}
    assert evaluate_metrics(model, None, loader, field, config=cfg, scorer=lambda gts, gen: seen.update(gts=gts, gen=gen) or {'x': 1}) == {'x': 1}
    assert seen['gen'] == {k: [collapse(s)] for k, s in zip(keys, good)} and seen['gts'] == dict(zip(keys, captions))
    tokens, avg = evaluate_metrics(model, None, loader, field, config=cfg)
    assert [t.shape for t in tokens] == [(2, 10), (1, 10)] and avg >= 0
    with pytest.raises(ValueError, match="'host' or 'device'"):
        evaluate_metrics(model, None, loader, field, config=cfg, scorer='java')
    with pytest.raises(ValueError, match="text_field"):
        evaluate_metrics(model, None, loader, None, config=cfg, scorer='host')
    # the best checkpoint: written when and only when CIDEr >= best_cider
    opts = _optimizers(model)
    out = evaluate_metrics(model, opts, loader, field, epoch=4, split='valid', config=cfg, best_cider=want['CIDEr'] + 1e-9, scorer='host')
    assert out == want and not os.path.exists('checkpoint_best_valid.pth')
    got = {}
    out = evaluate_metrics(model, opts, loader, field, epoch=5, split='valid', config=cfg, best_cider=want['CIDEr'], scorer='host',
                           scores_out=got)
    assert out == want['CIDEr'] and got == want
    ckpt = torch.load('checkpoint_best_valid.pth', map_location='cpu')  # as train_caption.main reads it: the weights-only default
    assert type(ckpt['scores']['ROUGE']) is float and type(ckpt['scores']['CIDEr']) is float and all(type(b) is float for b in ckpt['scores']['BLEU'])
    assert ckpt['epoch'] == 5 and ckpt['best_ciders'] == (want['CIDEr'], 0) and ckpt['scores'] == want
    out = evaluate_metrics(model, opts, loader, field, split='test', config=cfg, best_cider=0.0, scorer='host', log_and_save=False)
    assert out == want and not os.path.exists('checkpoint_best_test.pth')
    # the device scorer has no host fall-back: tokens on the CPU are an error
    from grit_amd.lib import GritHipError
    with pytest.raises(GritHipError):
        evaluate_metrics(model, None, loader, field, config=cfg, scorer='device')


def test_main_evaluates_every_epoch_and_carries_the_best_cider(tmp_path, monkeypatch):
    """Three XE epochs and one self-critical epoch on a stub model: the evaluation after every epoch, the best CIDEr carried, the
    best checkpoint read back at the XE -> SC boundary the way main reads it (torch.load's default), and a resume."""
    import train_caption
    from grit_amd.config import default_config
    monkeypatch.chdir(tmp_path)
    for k, v in (('MASTER_ADDR', '127.0.0.1'), ('MASTER_PORT', '29618'), ('RANK', '0'), ('WORLD_SIZE', '1')):
        monkeypatch.setenv(k, v)
    loader, captions, good, poor = _loader()
    made, at_sc = [], []

    def transformer(detector=None, config=None):
        made.append(StubModel())
        return made[-1]

    def train_xe(model, dataloaders, epoch=0, **kw):
        made[-1].variant = 0 if epoch == 0 else 1  # the first epoch's captions are the good ones, every later epoch's the poor ones
        with torch.no_grad():
            made[-1].fc.weight.fill_(float(epoch + 1))  # "training": the weights tell the epoch
        return {'loss': 1.0, 'reward': 0, 'reward_baseline': 0, 'val_loss': 0.0}

    def train_sc(model, dataloaders, epoch=0, **kw):
        at_sc.append(made[-1].fc.weight.detach().clone())
        made[-1].variant = 1
        return {'loss': 1.0, 'reward': 0, 'reward_baseline': 0, 'val_loss': 0.0}

    monkeypatch.setattr(train_caption, 'Transformer', transformer)
    monkeypatch.setattr(train_caption, 'build_detector', lambda config: torch.nn.Linear(2, 2))
    monkeypatch.setattr(train_caption, 'train_xe', train_xe)
    monkeypatch.setattr(train_caption, 'train_sc', train_sc)
    cfg = default_config(**{'optimizer.finetune_xe_epochs': 3, 'optimizer.finetune_sc_epochs': 1})
    cfg.exp.world_size, cfg.exp.bf16, cfg.exp.save, cfg.exp.eval_scorer = 1, False, True, 'host'
    loaders = {'train': [None] * 4, 'train_dict': [None] * 4, 'valid_dict': loader, 'test_dict': loader[:1]}
    results = train_caption.main(0, cfg, dataloaders=loaders, text_field=Field(ITOS), cider=object())
    assert len(results) == 4
    first, second, third, fourth = (r['valid_scores']['CIDEr'] for r in results)
    assert first > second == third == fourth > 0
    assert [r['best_cider_valid'] for r in results] == [first] * 4  # carried, not reset
    assert all(len(r['valid_scores']['BLEU']) == 4 and 'ROUGE' in r['valid_scores'] for r in results)
    assert results[0]['best_cider_test'] == results[0]['test_scores']['CIDEr'] == results[3]['best_cider_test']  # one rank: both splits
    # the self-critical epoch started from the best validation checkpoint -- epoch 0's weights, not epoch 2's
    assert len(at_sc) == 1 and bool((at_sc[0] == 1.0).all())
    for name in ('checkpoint_best_valid.pth', 'checkpoint_best_test.pth', 'checkpoint_ft_xe.pth', 'checkpoint_ft_sc.pth'):
        ckpt = torch.load(name, map_location='cpu')  # as main reads them: the weights-only default
        assert all(type(x) in (float, int) for x in ckpt['best_ciders'])  # plain numbers, no numpy scalars
    ckpt = torch.load('checkpoint_best_valid.pth', map_location='cpu')
    assert ckpt['epoch'] == 0 and ckpt['best_ciders'] == (first, 0)  # the later, poorer epochs did not overwrite it
    assert type(ckpt['scores']['CIDEr']) is float and type(ckpt['scores']['ROUGE']) is float and ckpt['scores'] == results[0]['valid_scores']
    ckpt = torch.load('checkpoint_ft_xe.pth', map_location='cpu')
    assert ckpt['epoch'] == 2 and list(ckpt['best_ciders']) == [first, results[0]['best_cider_test']]
    # a resume restores the two best values: the poorer self-critical epoch that follows does not overwrite the best checkpoint
    cfg.exp.resume_from = 'checkpoint_ft_xe.pth'
    resumed = train_caption.main(0, cfg, dataloaders=loaders, text_field=Field(ITOS), cider=object())
    assert len(resumed) == 1 and resumed[0]['valid_scores']['CIDEr'] == fourth and resumed[0]['best_cider_valid'] == first
    assert torch.load('checkpoint_best_valid.pth', map_location='cpu')['epoch'] == 0
    cfg.exp.resume_from = ''
    # the device scorer on a machine without a GPU is refused before the first epoch, not after it
    if not torch.cuda.is_available():
        cfg.exp.eval_scorer = 'device'
        calls = len(made)
        with pytest.raises(ValueError, match="eval_scorer='host'"):
            train_caption.main(0, cfg, dataloaders=loaders, text_field=Field(ITOS), cider=object())
        assert len(at_sc) == 2 and len(made) == calls + 1  # (the model was built, no epoch ran)
        cfg.exp.eval_scorer = 'host'
    # without the evaluation loaders main does what it did
    loaders = {'train': [None] * 4}
    results = train_caption.main(0, cfg, dataloaders=loaders, text_field=Field(ITOS))
    assert len(results) == 3 and all('valid_scores' not in r and 'best_cider_valid' not in r for r in results)
