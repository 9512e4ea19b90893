"""The device Hungarian matcher (grit_lsa_f32, grit_det_match_f32) against scipy's assignments of fixture G19
(tests/golden/make_det_loss_golden.py).  Every problem of the fixture has a uniqueness margin >= 1e-2, so index equality is demanded.
Needs an MI355X."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, t

import det_draws as D  # tests/golden, put on the path by tests.helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Largest |C_device - C_reference| measured on an MI355X over every stored cost matrix (K = 37 and K = 1849): MEASURED_COST_DEV.  The
# assertion allows 4x that (expf / logf differ by a few ulp between libraries) and never more than 1e-4, two orders under the margin.
MEASURED_COST_DEV = 4.06e-6  # the Q = 150, K = 37 group; 1.9e-6 at Q = 20 and 2.4e-6 at K = 1849
COST_TOL = min(4 * MEASURED_COST_DEV, 1e-4)


@pytest.fixture(scope="module")
def g19():
    return D.load_shards(GOLDEN), json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))


def check_problem(mq, mt, C, Q, T, ref_i, ref_j, demand_indices=True):
    """mq [>= T], mt [>= Q] numpy; C [Q, T] fp32; ref_i / ref_j scipy's pairs."""
    mq, mt = mq[:T], mt[:Q]
    n = min(Q, T)
    tq = [(int(q), k) for k, q in enumerate(mq) if q >= 0]
    assert len(tq) == n, "matching of size %d, expected %d" % (len(tq), n)
    assert all(0 <= q < Q for q, _ in tq)
    assert len({q for q, _ in tq}) == n, "a query is used twice"
    for q, k in tq:  # the two views agree
        assert mt[q] == k
    assert int((mt >= 0).sum()) == n
    if C is not None and n:
        C64 = C.astype(np.float64)
        got = sum(C64[q, k] for q, k in tq)
        opt = float(C64[ref_i, ref_j].sum())
        assert abs(got - opt) <= 1e-9 * max(1.0, abs(opt)), (got, opt)
    if demand_indices:
        assert sorted(tq) == sorted((int(a), int(b)) for a, b in zip(ref_i, ref_j))


def test_solver_alone_on_the_fixture_costs(g19):
    from grit_amd.ops.det_loss import linear_sum_assignment
    g, meta = g19
    cases = meta['match']  # both layers' matrices of every (Q, T) case
    assert [(p['Q'], p['T']) for p in cases if p['layer'] == 0] == D.MATCH_CASES and len(cases) == 2 * len(D.MATCH_CASES)
    Q, ld = max(p['Q'] for p in cases), max(p['T'] for p in cases)
    cost = np.full((len(cases), Q, ld), np.nan, np.float32)  # anything outside a problem's own block must not be read
    for n, p in enumerate(cases):
        assert p['margin'] is None or p['margin'] >= 1e-2
        cost[n, :p['Q'], :p['T']] = g['match/%d/%d/cost' % (p['case'], p['layer'])]
    counts = torch.tensor([p['T'] for p in cases], dtype=torch.int32, device=DEV)
    rows = torch.tensor([p['Q'] for p in cases], dtype=torch.int32, device=DEV)
    mq, mt = linear_sum_assignment(t(cost, device=DEV), counts, rows)  # ONE launch for all problems
    mq, mt = mq.cpu().numpy(), mt.cpu().numpy()
    for n, p in enumerate(cases):
        key = 'match/%d/%d' % (p['case'], p['layer'])
        check_problem(mq[n], mt[n], g[key + '/cost'], p['Q'], p['T'], g[key + '/i'], g[key + '/j'])
        assert (mq[n, p['T']:] == -1).all() and (mt[n, p['Q']:] == -1).all()


def _batch(problems, key, K, layers):
    """Problems of one Q grouped into logits [L, B, Q, K], boxes and the target list, from the fixture's seeds."""
    images = sorted({p[key] for p in problems})
    Q = problems[0]['Q']
    logits = np.zeros((layers, len(images), Q, K), np.float32)
    boxes = np.zeros((layers, len(images), Q, 4), np.float32)
    targets = [None] * len(images)
    for p in problems:
        b = images.index(p[key])
        logits[p['layer'], b], boxes[p['layer'], b] = D.predictions(p['seed'], Q, K)
        labels, tb = D.targets(p['target_seed'], p['T'], K)
        targets[b] = {'labels': t(labels, device=DEV), 'boxes': t(tb, device=DEV)}
    return images, t(logits, device=DEV), t(boxes, device=DEV), targets


@pytest.mark.parametrize("group", ["q150", "q20", "k1849"])
def test_fused_cost_and_assignment(g19, group):
    from grit_amd.ops.det_loss import match, pack_targets
    g, meta = g19
    if group == "k1849":
        problems, key, K, prefix = meta['bigmatch'], 'image', D.BIG_K, 'bigmatch'
    else:
        problems = [p for p in meta['match'] if p['Q'] == (150 if group == "q150" else 20)]
        key, K, prefix = 'case', D.MATCH_K, 'match'
    images, logits, boxes, targets = _batch(problems, key, K, 2)
    w = D.COST_WEIGHTS
    mq, mt, cost = match(logits, boxes, pack_targets(targets), w['class'], w['bbox'], w['giou'], return_cost=True)
    mq, mt, cost = mq.cpu().numpy(), mt.cpu().numpy(), cost.cpu().numpy()
    worst = 0.0
    for p in problems:
        b = images.index(p[key])
        name = '%s/%d/%d' % (prefix, p[key], p['layer'])
        C = g[name + '/cost']  # every problem's matrix is in the fixture: no cost_out goes uncompared
        if C.size:
            worst = max(worst, float(np.abs(cost[p['layer'], b, :, :p['T']] - C).max()))
        # optimality is judged on the DEVICE's own matrix (the solver's input); the indices against scipy's on the reference's
        own = cost[p['layer'], b, :, :p['T']]
        ref_i, ref_j = g[name + '/i'], g[name + '/j']
        check_problem(mq[p['layer'], b], mt[p['layer'], b], None, p['Q'], p['T'], ref_i, ref_j)
        if p['T']:
            got = sum(float(own[q, k]) for k, q in enumerate(mq[p['layer'], b, :p['T']]) if q >= 0)
            assert abs(got - float(own.astype(np.float64)[ref_i, ref_j].sum())) <= 1e-9 * max(1.0, abs(got))
        assert (mq[p['layer'], b, p['T']:] == -1).all()
    print("det match %s: largest |C_dev - C_ref| = %.3e (tolerance %.3e)" % (group, worst, COST_TOL))
    assert worst <= COST_TOL


def test_tied_costs_give_a_valid_optimal_matching():
    """Two identical queries (rows 1 and 2) and two identical targets: several optima, any of them is accepted."""
    from grit_amd.ops.det_loss import linear_sum_assignment
    C = np.array([[4, 1, 3, 1], [2, 0, 5, 0], [2, 0, 5, 0], [3, 2, 2, 2], [1, 1, 1, 1], [9, 9, 9, 9]], np.float32)  # Q = 6, T = 4
    best = min(sum(C[q, k] for k, q in enumerate(perm)) for perm in itertools.permutations(range(6), 4))
    for cost, Q, T in ((C, 6, 4), (np.ascontiguousarray(C.T), 4, 6)):
        mq, mt = linear_sum_assignment(t(cost[None], device=DEV), torch.tensor([T], dtype=torch.int32, device=DEV))
        mq, mt = mq.cpu().numpy()[0], mt.cpu().numpy()[0]
        check_problem(mq, mt, None, Q, T, None, None, demand_indices=False)
        assert sum(cost[q, k] for k, q in enumerate(mq[:T]) if q >= 0) == best


def test_bound_is_reported():
    from grit_amd import lib
    from grit_amd.ops.det_loss import linear_sum_assignment
    side = lib.DET_MAX_SIDE
    assert side >= 300
    with pytest.raises(lib.GritHipError, match="not supported"):
        linear_sum_assignment(torch.zeros(1, 4, side + 1, device=DEV), torch.tensor([2], dtype=torch.int32, device=DEV))
    # T = 300 with Q = 150 is inside the bound
    cost = torch.rand(1, 150, 300, generator=torch.Generator().manual_seed(3)).to(DEV)
    mq, mt = linear_sum_assignment(cost, torch.tensor([300], dtype=torch.int32, device=DEV))
    assert int((mq >= 0).sum()) == 150 and int((mt >= 0).sum()) == 150
    assert sorted(mq[0][mq[0] >= 0].tolist()) == list(range(150))
