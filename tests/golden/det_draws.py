"""Seeded inputs of fixture G19 (tests/golden/det_loss_g19.*), shared by its generator and the tests so that nothing logits-sized
is committed: every array is a numpy.random.default_rng draw that both sides repeat from the seeds stored in the fixture."""
import numpy as np

# the matcher cases: (Q, T).  Lane-count edges of the 64-lane column scan, the square case, T > Q, and a Q that is no multiple of 64
MATCH_CASES = [(150, t) for t in (0, 1, 7, 33, 64, 65, 100, 149, 150, 151, 180)] + [(20, 5), (20, 30)]
MATCH_LAYERS, MATCH_K = 2, 37
BIG_K = 1849
BIG_CASE_T = (7, 33)  # the one K = 1849 matcher case: L = 2, B = 2, Q = 150
COST_WEIGHTS = {'class': 2.0, 'bbox': 5.0, 'giou': 2.0}  # set_cost_* of the detection configuration
LOSS_WEIGHTS = {'loss_ce': 2.0, 'loss_bbox': 5.0, 'loss_giou': 2.0}
CRIT_L, CRIT_B, CRIT_Q = 3, 3, 150
CRIT_T = (0, 5, 40)
CRIT_KS = (37, 1849)
SAMPLE_STRIDE = 97


def boxes(rng, n):
    """[n, 4] cxcywh inside the unit square, sides in [0.05, 0.45)."""
    wh = 0.05 + 0.4 * rng.random((n, 2))
    centre = wh / 2 + (1 - wh) * rng.random((n, 2))
    return np.concatenate([centre, wh], 1).astype(np.float32)


def predictions(seed, Q, K):
    """logits [Q, K] ~ N(-2, 2) and boxes [Q, 4] of one (layer, image) problem."""
    rng = np.random.default_rng(seed)
    return (2.0 * rng.standard_normal((Q, K)) - 2.0).astype(np.float32), boxes(rng, Q)


def targets(seed, T, K):
    """labels [T] int64 and boxes [T, 4] of one image."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, K, T).astype(np.int64), boxes(rng, T)


SHARD_BYTES = 1000000  # the fixture is split into det_loss_g19.npz, det_loss_g19.1.npz, ... so that no file exceeds 1 MiB


def load_shards(directory, stem='det_loss_g19'):
    """Every array of the fixture, whichever shard holds it."""
    import glob
    import os
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, stem + '*.npz'))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def end_to_end_batch(seed, B=2, size=224, num_classes=11, counts=(3, 6)):
    """Images [B, 3, size, size] ~ N(0, 1) and per image labels / boxes for the tiny end-to-end detector step."""
    rng = np.random.default_rng(seed)
    images = rng.standard_normal((B, 3, size, size)).astype(np.float32)
    tg = []
    for n in counts:
        tg.append((rng.integers(0, num_classes, n).astype(np.int64), boxes(rng, n)))
    return images, tg
