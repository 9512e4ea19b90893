"""Fixture G18, tests/golden/metrics_g18.json: BLEU, ROUGE-L and CIDEr of the reference's own scorers (pure Python, loaded from
its files by path) on seeded synthetic captions.  A fixture generator, not a test:

    python tests/golden/make_metrics_golden.py /path/to/the/reference/checkout

48 images, `i % 7 + 1` references of 3..14 words from a 40-word Zipf pool, hypothesis kind `i % 8` (see `hypothesis`).  Only
data is written: the captions, the corpus scores, the per-image ROUGE and CIDEr, per image the BLEU integers read from
BleuScorer.ctest, and a second set of corpus scores over the rows with testlen < reflen (the full draw's length ratio is above
1, so only the subset exercises the corpus brevity penalty)."""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(ref):
    mods = {}
    for name in ('bleu', 'rouge', 'cider'):
        pkg = types.ModuleType('ref' + name)
        pkg.__path__ = [os.path.join(ref, 'datasets', 'caption', 'metrics', name)]
        sys.modules['ref' + name] = pkg
        mods[name] = importlib.import_module('ref%s.%s' % (name, name))
    return mods, importlib.import_module('refbleu.bleu_scorer')


def hypothesis(kind, refs, rng, pool, p):
    words = lambda n: [str(w) for w in rng.choice(pool, size=n, p=p)]
    first = refs[0].split()
    if kind == 0:
        return first                                   # a reference itself
    if kind == 1:
        return first[:2] * 6                           # one bigram repeated six times: clipping
    if kind == 2:
        return []                                      # empty
    if kind == 3:
        return first + words(12)                       # a reference plus twelve more words
    if kind == 4:
        return first[:1]                               # a single word
    if kind == 5:
        return first[::-1]                             # a reference reversed
    if kind == 6:
        return words(6)                                # six words (against references of five and seven, see main)
    out = []
    for w in first:                                    # a reference interleaved with noise
        out += [w] + words(1)
    return out


def main(ref):
    mods, scorer_mod = _load(ref)
    rng = np.random.default_rng(18)
    pool = ['w%02d' % i for i in range(40)]
    p = 1.0 / np.arange(1, 41)
    p /= p.sum()
    gts, res = {}, {}
    for i in range(48):
        lengths = [int(rng.integers(3, 15)) for _ in range(i % 7 + 1)]
        if i % 8 == 6 and len(lengths) >= 2:
            lengths[:2] = [5, 7]  # a six-word hypothesis between them: the closest length is a tie
        refs = [' '.join(str(w) for w in rng.choice(pool, size=n, p=p)) for n in lengths]
        gts[i] = refs
        res[i] = [' '.join(hypothesis(i % 8, refs, rng, pool, p))]

    def score(keys):
        g, r = {k: gts[k] for k in keys}, {k: res[k] for k in keys}
        bleu, _ = mods['bleu'].Bleu().compute_score(g, r)
        rouge, rouge_rows = mods['rouge'].Rouge().compute_score(g, r)
        cider, cider_rows = mods['cider'].Cider().compute_score(g, r)
        return {'BLEU': [float(b) for b in bleu], 'ROUGE': float(rouge), 'CIDEr': float(cider),
                'ROUGE_rows': [float(x) for x in rouge_rows], 'CIDEr_rows': [float(x) for x in cider_rows]}

    keys = sorted(gts)
    full = score(keys)
    scorer = scorer_mod.BleuScorer(n=4)
    for k in keys:
        scorer += (res[k][0], gts[k])
    comps = []
    for c in scorer.ctest:
        closest = min((abs(l - c['testlen']), l) for l in c['reflen'])[1]
        comps.append({'testlen': int(c['testlen']), 'reflen': int(closest), 'guess': [int(x) for x in c['guess']],
                      'correct': [int(x) for x in c['correct']]})
    short = [k for k, c in zip(keys, comps) if c['testlen'] < c['reflen']]
    sub = score(short)

    # coverage: the comparison is not about zeros and every case is present
    n = len(keys)
    assert {len(gts[k]) for k in keys} == set(range(1, 8))
    assert sum(1 for k in keys if res[k][0] == '') >= 3
    clipped = ties = 0
    for k, c in zip(keys, comps):
        hyp = scorer_mod.precook(res[k][0])[1]
        best = scorer_mod.cook_refs(gts[k])[1]
        clipped += any(0 < best.get(g, 0) < cnt for g, cnt in hyp.items())
        d = sorted({(abs(len(r.split()) - c['testlen']), len(r.split())) for r in gts[k]})
        ties += len(d) > 1 and d[0][0] == d[1][0]
    assert clipped >= 5 and ties >= 3, (clipped, ties)
    assert sum(1 for x in full['ROUGE_rows'] if x > 0) > n // 2 and sum(1 for x in full['CIDEr_rows'] if x > 0) > n // 2
    assert sum(1 for c in comps if c['correct'][0] > 0) > n // 2 and sum(1 for c in comps if c['correct'][3] > 0) >= 8
    ratio = sum(c['testlen'] for c in comps) / float(sum(c['reflen'] for c in comps))
    sub_comps = [c for c in comps if c['testlen'] < c['reflen']]
    sub_ratio = sum(c['testlen'] for c in sub_comps) / float(sum(c['reflen'] for c in sub_comps))
    assert sub_ratio < 1 and len(short) >= 8, (sub_ratio, len(short))

    out = {'gts': {str(k): gts[k] for k in keys}, 'res': {str(k): res[k] for k in keys}, 'scores': full, 'bleu_components': comps,
           'short_keys': [str(k) for k in short], 'short_scores': sub}
    with open(os.path.join(HERE, 'metrics_g18.json'), 'w') as f:
        json.dump(out, f)
    print('g18: %d images, %d empty, %d clipped, %d ties, ratio %.3f, subset of %d with ratio %.3f' %
          (n, sum(1 for k in keys if res[k][0] == ''), clipped, ties, ratio, len(short), sub_ratio))
    print('     BLEU', full['BLEU'], 'ROUGE', full['ROUGE'], 'CIDEr', full['CIDEr'])
    print('     subset BLEU', sub['BLEU'], 'ROUGE', sub['ROUGE'], 'CIDEr', sub['CIDEr'])


if __name__ == '__main__':
    main(sys.argv[1])
