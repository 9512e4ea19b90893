from .bleu import Bleu
from .cider import Cider
from .rouge import Rouge
from .tokenizer import PTBTokenizer

__all__ = ['Bleu', 'Cider', 'PTBTokenizer', 'Rouge', 'compute_scores']


def compute_scores(gts, gen):
    """The evaluation's scores (reference datasets/caption/metrics/__init__.py:7-16) of hypotheses `gen[k][0]` against references
    `gts[k]`, both tokenised: ({'BLEU': [b1..b4], 'ROUGE': r, 'CIDEr': c}, the per-image scores under the same keys).  METEOR,
    which the reference lists as well, is a Java program outside the reference tree and is not computed.  CIDEr takes its
    document frequencies from this call's own `gts`, as the reference's `Cider()` does.  The corpus scores are plain Python floats:
    the dictionary goes into checkpoints that are read back with torch.load's weights-only default."""
    all_score, all_scores = {}, {}
    for metric in (Bleu(), Rouge(), Cider()):
        score, scores = metric.compute_score(gts, gen)
        all_score[str(metric)] = [float(s) for s in score] if isinstance(score, (list, tuple)) else float(score)
        all_scores[str(metric)] = scores
    return all_score, all_scores
