"""BLEU-1..4 of the evaluation (reference datasets/caption/metrics/bleu/{bleu,bleu_scorer}.py, called with option='closest').

Same interface: `Bleu(n).compute_score(gts, res)` returns (the n corpus scores, n lists of per-image scores) for hypotheses
`res[k][0]` against references `gts[k]`.  Same definition (Papineni et al., 2002, as the COCO caption evaluation implements it):
per image the hypothesis length, the reference length closest to it (a tie goes to the shorter reference), the number of
hypothesis n-grams `guess[k]` and the number of them found in a reference, clipped by the largest count in any one reference
`correct[k]`; the corpus score is formed from the SUMS of those integers, not from the per-image scores.

Arranged differently from the reference: an image is reduced to ten integers (`components`) and the scalar expression is one
function (`bleu_from_components`) used for the per-image scores, for the corpus scores and by the device path
(grit_amd/ops/caption_scores.py), which produces the same ten integers in a kernel."""
import math

from .cider import ngram_counts

TINY, SMALL = 1e-15, 1e-9  # the reference's guards: a zero count still gives 0, a zero length does not divide by zero


def components(hypothesis, references, n=4):
    """(testlen, reflen, guess[n], correct[n]) of one image, all integers."""
    counts = ngram_counts(hypothesis, n)
    testlen = len(hypothesis.split())
    best = {}
    lengths = []
    for ref in references:
        lengths.append(len(ref.split()))
        for ngram, c in ngram_counts(ref, n).items():
            if c > best.get(ngram, 0):
                best[ngram] = c
    reflen = min((abs(l - testlen), l) for l in lengths)[1]
    guess = [max(0, testlen - k) for k in range(n)]
    correct = [0] * n
    for ngram, c in counts.items():
        correct[len(ngram) - 1] += min(best.get(ngram, 0), c)
    return testlen, reflen, guess, correct


def bleu_from_components(testlen, reflen, guess, correct):
    """The reference's scalar expression, in its order of operations (running product, root, brevity penalty last)."""
    scores = []
    bleu = 1.
    for k in range(len(guess)):
        bleu *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        scores.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        for k in range(len(guess)):
            scores[k] *= math.exp(1 - 1 / ratio)
    return scores


class Bleu(object):

    def __init__(self, n=4):
        self._n = n

    def compute_components(self, gts, res):
        """One (testlen, reflen, guess, correct) per image, in the order of `gts`."""
        assert gts.keys() == res.keys()
        out = []
        for k in gts.keys():
            assert type(res[k]) is list and len(res[k]) == 1 and type(gts[k]) is list and len(gts[k]) >= 1
            out.append(components(res[k][0], gts[k], self._n))
        return out

    def compute_score(self, gts, res):
        n = self._n
        per_image = [[] for _ in range(n)]
        testlen, reflen, guess, correct = 0, 0, [0] * n, [0] * n
        for tl, rl, g, c in self.compute_components(gts, res):
            testlen += tl
            reflen += rl
            for k in range(n):
                guess[k] += g[k]
                correct[k] += c[k]
            for k, s in enumerate(bleu_from_components(tl, rl, g, c)):
                per_image[k].append(s)
        return bleu_from_components(testlen, reflen, guess, correct), per_image

    def __str__(self):
        return 'BLEU'
