"""ROUGE-L of the evaluation (reference datasets/caption/metrics/rouge/rouge.py; Lin and Hovy, 2004).

Same interface: `Rouge().compute_score(gts, res)` returns (mean, per-image scores).  Per image: the longest common subsequence
of the hypothesis with every reference, precision = max lcs / len(hypothesis), recall = max lcs / len(reference), and
(1 + beta^2) p r / (r + beta^2 p) with beta = 1.2, or 0 when either maximum is 0.

Sentences are split at single spaces as the reference does, so the empty string is a sequence of ONE empty token: an empty
hypothesis has length 1 and scores 0 against any non-empty reference, and 1 against an empty one.

The subsequence length is computed with one rolling row instead of the reference's full table; the arithmetic on it
(`f_score`) is the reference's expression in its order and is shared with the device path's host mirror."""
import numpy as np

BETA = 1.2


def lcs_length(a, b):
    """Length of the longest common subsequence of two token lists."""
    if len(a) < len(b):
        a, b = b, a
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for j, y in enumerate(b):
            up = row[j + 1]
            row[j + 1] = diag + 1 if x == y else max(up, row[j])
            diag = up
    return row[len(b)]


def f_score(lcs, len_hyp, len_refs, beta=BETA):
    """lcs[r], len_refs[r] per reference -> the image's score."""
    prec_max = max(l / float(len_hyp) for l in lcs)
    rec_max = max(l / float(n) for l, n in zip(lcs, len_refs))
    if prec_max != 0 and rec_max != 0:
        return ((1 + beta ** 2) * prec_max * rec_max) / float(rec_max + beta ** 2 * prec_max)
    return 0.0


class Rouge(object):

    def __init__(self):
        self.beta = BETA

    def calc_score(self, candidate, refs):
        assert len(candidate) == 1 and len(refs) > 0
        hyp = candidate[0].split(" ")
        split = [r.split(" ") for r in refs]
        return f_score([lcs_length(r, hyp) for r in split], len(hyp), [len(r) for r in split], self.beta)

    def compute_score(self, gts, res):
        assert gts.keys() == res.keys()
        scores = []
        for k in gts.keys():
            assert type(res[k]) is list and len(res[k]) == 1 and type(gts[k]) is list and len(gts[k]) > 0
            scores.append(self.calc_score(res[k], gts[k]))
        scores = np.array(scores)
        return float(np.mean(scores)), scores

    def __str__(self):
        return 'ROUGE'
