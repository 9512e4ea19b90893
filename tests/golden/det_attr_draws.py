"""Seeded inputs of fixture G23 (tests/golden/det_attr_g23.*), shared by its generator and the tests so that nothing logits-sized
is committed: every array is a numpy.random.default_rng draw that both sides repeat from the seeds stored in the fixture."""
import numpy as np

HEAD_D, HEAD_B, HEAD_Q, HEAD_A = 256, 2, 150, 400
HEAD_KS = (37, 1849)
HEAD_MARGIN = 1e-3  # every row's gap between its best and second-best class logit
STRIDE = 29  # the large arrays are kept as every 29th element of their flat form

LOSS_B = 3
LOSS_AS, LOSS_QS = (37, 400), (19, 150)
LOSS_KINDS = ('mixed', 'none', 'zeros', 'ones', 'tq')
E2E_A = 23


def head_inputs(seed, K):
    """obj_h [B, Q, d] ~ N(0, 1), pred_logits [B, Q, K] ~ N(-2, 2) and the weights w [B, Q, A] of the scalar sum(attr_logits * w)."""
    rng = np.random.default_rng(seed)
    obj_h = rng.standard_normal((HEAD_B, HEAD_Q, HEAD_D)).astype(np.float32)
    logits = (2.0 * rng.standard_normal((HEAD_B, HEAD_Q, K)) - 2.0).astype(np.float32)
    w = rng.standard_normal((HEAD_B, HEAD_Q, HEAD_A)).astype(np.float32)
    return obj_h, logits, w


def top_gap(logits):
    """Smallest gap over the rows between the best and the second-best logit (float64)."""
    part = np.partition(logits.astype(np.float64), -2, axis=-1)
    return float((part[..., -1] - part[..., -2]).min())


def loss_counts(kind, Q):
    """Targets per image of a loss case."""
    return (0, 5, Q + 21) if kind == 'tq' else (0, 5, 40)


def loss_flags(kind):
    return (False, False, False) if kind == 'none' else ((True, False, True) if kind == 'mixed' else (True, True, True))


def loss_seed(kind, A, Q):
    return 23000 + LOSS_KINDS.index(kind) * 100 + LOSS_AS.index(A) * 10 + LOSS_QS.index(Q)


def loss_case(kind, A, Q):
    """attr_logits [B, Q, A] ~ N(0, 2) fp32; per image the attributes [T, A] uint8 (about 10 % ones; all 0 / all 1 for the kinds
    'zeros' / 'ones'), has_attr, and the given pairs (queries, targets): min(Q, T) distinct queries in increasing order, each with
    a distinct target."""
    rng = np.random.default_rng(loss_seed(kind, A, Q))
    x = (2.0 * rng.standard_normal((LOSS_B, Q, A))).astype(np.float32)
    attrs, pairs = [], []
    for T in loss_counts(kind, Q):
        a = (rng.random((T, A)) < 0.1).astype(np.uint8)
        if kind == 'zeros':
            a[:] = 0
        elif kind == 'ones':
            a[:] = 1
        n = min(Q, T)
        q = np.sort(rng.permutation(Q)[:n]).astype(np.int64)
        t = rng.permutation(T)[:n].astype(np.int64)
        attrs.append(a)
        pairs.append((q, t))
    return x, attrs, list(loss_flags(kind)), pairs


def match_t_of(pairs, Q):
    """[B, Q] int32: the target of each query, -1 for an unmatched one."""
    out = np.full((len(pairs), Q), -1, np.int32)
    for b, (q, t) in enumerate(pairs):
        out[b, q] = t
    return out


def e2e_attributes(seed, counts, A=E2E_A):
    """Per image of the end-to-end step: attributes [T, A] uint8 (about 15 % ones) and has_attr = (True, False)[image % 2]."""
    rng = np.random.default_rng(seed + 77)
    return [((rng.random((n, A)) < 0.15).astype(np.uint8), i % 2 == 0) for i, n in enumerate(counts)]
