"""tests/det_loss_model.py (the plain reference tests/test_det_loss_edges_gpu.py holds the matcher and the set criterion to) is
itself checked here, without a GPU: its cost matrix, its assignments and its criterion against fixture G19
(tests/golden/make_det_loss_golden.py), its solver against brute force on the tiny problems the GPU file runs, and the conditions
the GPU file relies on: the criterion is finite on the whole box lattice, and the problems whose indices it demands have one optimum."""
import json
import os

import numpy as np
import pytest
import torch

from tests import det_loss_model as M
from tests.helpers import GOLDEN
from tests.test_det_match_gpu import COST_TOL

import det_draws as D  # tests/golden, put on the path by tests.helpers


@pytest.fixture(scope="module")
def g19():
    return D.load_shards(GOLDEN), json.load(open(os.path.join(GOLDEN, "det_loss_g19.json")))


def _problems(meta):
    for p in meta['match']:
        yield 'match/%d/%d' % (p['case'], p['layer']), p, D.MATCH_K
    for p in meta['bigmatch']:
        yield 'bigmatch/%d/%d' % (p['image'], p['layer']), p, D.BIG_K


def test_fp32_costs_reproduce_the_stored_matrices(g19):
    g, meta = g19
    w = D.COST_WEIGHTS
    worst, seen = 0.0, 0
    for key, p, K in _problems(meta):
        logits, boxes = D.predictions(p['seed'], p['Q'], K)
        labels, tb = D.targets(p['target_seed'], p['T'], K)
        C = M.cost_matrix(logits, boxes, labels, tb, (w['class'], w['bbox'], w['giou']), torch.float32)
        ref = g[key + '/cost']
        assert C.shape == ref.shape == (p['Q'], p['T']) and C.dtype == np.float32
        if ref.size:
            worst = max(worst, float(np.abs(C.astype(np.float64) - ref).max()))
        seen += 1
    assert seen == 2 * len(D.MATCH_CASES) + 2 * len(D.BIG_CASE_T)
    print("det loss model: largest |C_model32 - C_stored| = %.3e (tolerance %.3e)" % (worst, COST_TOL))
    assert worst <= COST_TOL


def test_assign_reproduces_the_stored_pairs(g19):
    g, meta = g19
    for key, p, K in _problems(meta):
        i, j = M.assign(g[key + '/cost'])
        assert i.tolist() == g[key + '/i'].tolist() and j.tolist() == g[key + '/j'].tolist(), key


@pytest.mark.parametrize("K", D.CRIT_KS)
def test_criterion_reproduces_the_stored_float64_run(g19, K):
    """Both sides are float64 evaluations of the same composition; the difference is rounding order."""
    g, meta = g19
    meta = meta['crit'][str(K)]
    key = 'crit/%d' % K
    L, B, Q = D.CRIT_L, D.CRIT_B, D.CRIT_Q
    logits = np.zeros((L, B, Q, K), np.float32)
    boxes = np.zeros((L, B, Q, 4), np.float32)
    for l in range(L):
        for b in range(B):
            logits[l, b], boxes[l, b] = D.predictions(meta['seeds'][l][b], Q, K)
    tg = [D.targets(meta['target_seeds'][b], T, K) for b, T in enumerate(D.CRIT_T)]
    labels, tb = np.concatenate([a for a, _ in tg]), np.concatenate([b for _, b in tg])
    offsets = np.concatenate([[0], np.cumsum(D.CRIT_T)])
    rows = g[key + '/rows']
    match_t = np.full((L, B, Q), -1, np.int32)
    match_t[rows[:, 0], rows[:, 1], rows[:, 2]] = rows[:, 3]
    w = D.LOSS_WEIGHTS
    coef = np.tile([w['loss_ce'], w['loss_bbox'], w['loss_giou']], (L, 1))
    out, dl, db = M.criterion(logits, boxes, labels, tb, offsets, match_t, 0.25, float(max(sum(D.CRIT_T), 1)), coef)
    names = ('loss_ce', 'loss_bbox', 'loss_giou', 'cardinality_error', 'class_error')
    checked = 0
    for l in range(L):
        suffix = '' if l == L - 1 else '_%d' % l  # the last layer is the main output, the others the auxiliary ones
        for col, name in enumerate(names):
            if name + suffix not in meta['losses64']:
                assert name == 'class_error' and suffix
                continue
            ref = meta['losses64'][name + suffix]
            # the two counted outputs are the stored values that are no float64 results: the reference counts in fp32 whatever the
            # dtype of the logits (the fixture holds 88.88888549804688 for 100 - 100 / 9 and 130.6666717529297 for 392 / 3), so
            # they are held to one fp32 ulp of the exact quotient instead
            bound = float(np.spacing(np.float32(ref))) if col >= 3 else 1e-9 * abs(ref)
            assert abs(out[l, col] - ref) <= bound, (name + suffix, out[l, col], ref)
            checked += 1
    assert checked == len(meta['losses64'])
    gmax, bmax = float(g[key + '/dlogits_max']), float(g[key + '/dboxes_max'])
    ref_rows = np.concatenate([g[k] for k in sorted(g) if k.startswith(key + '/row_values/')])
    assert np.abs(dl[rows[:, 0], rows[:, 1], rows[:, 2]] - ref_rows).max() <= 1e-9 * gmax
    assert np.abs(dl.reshape(-1)[::D.SAMPLE_STRIDE] - g[key + '/sample']).max() <= 1e-9 * gmax
    assert abs(np.abs(dl).max() - gmax) <= 1e-9 * gmax and abs(np.abs(db).max() - bmax) <= 1e-9 * bmax
    assert abs(np.abs(dl).sum() - float(g[key + '/abs_sum'])) <= 1e-9 * float(g[key + '/abs_sum'])
    assert np.abs(db[rows[:, 0], rows[:, 1], rows[:, 2]] - g[key + '/dboxes']).max() <= 1e-9 * bmax
    mask = np.ones((L, B, Q), bool)
    mask[rows[:, 0], rows[:, 1], rows[:, 2]] = False
    assert not db[mask].any()


def test_assign_equals_brute_force_on_the_tiny_problems():
    problems = M.tiny_problems() + [('infeasible', M.infeasible_matrix(5)), ('infeasible T', M.infeasible_matrix(5).T)]
    assert len(problems) >= 12
    for name, C in problems:
        assert max(C.shape) <= 6
        best, pairs = M.brute_force_total(C), M.assign(C)
        if best is None:
            assert pairs is None, name
        else:
            assert len(pairs[0]) == min(C.shape) and float(C.astype(np.float64)[pairs[0], pairs[1]].sum()) == best, name
    assert M.brute_force_total(M.infeasible_matrix(5)) is None


@pytest.mark.parametrize("Q,T", [(65, 65), (64, 130), (130, 64), (129, 70), (70, 129)])
def test_product_matrix_has_the_reversed_pairing_as_its_only_optimum(Q, T):
    C = M.product_matrix(Q, T)
    i, j = M.assign(C)
    n = min(Q, T)
    want = [(q, n - 1 - q) for q in range(n)]
    assert list(zip(i.tolist(), j.tolist())) == (want if Q <= T else sorted((b, a) for a, b in want))
    assert M.margin(C) >= 1.0  # integers: any other matching costs at least 1 more


def test_band_matrices_are_feasible_and_the_nan_scatter_misses_the_band():
    plain, scattered = M.band_matrix(11), M.band_matrix(11, nan_every=7)
    assert np.isnan(scattered).sum() > 100 and not np.isnan(plain).any()
    finite = np.isfinite(plain)
    assert (finite.sum(1) == 3).all() and np.array_equal(finite, np.isfinite(scattered))
    assert np.array_equal(plain[finite], scattered[finite])
    a, b = M.assign(plain), M.assign(scattered)
    assert a is not None and plain[a].sum() == scattered[b].sum() and np.isfinite(plain[a].sum())


def test_cost_matrix_states_nan_where_the_kernel_does():
    boxes = np.array([[0.5, 0.5, 0.25, 0.25], [0.25, 0.25, 0.0, 0.0]], np.float32)
    tb = np.array([[0.5, 0.5, 0.25, 0.25], [0.75, 0.75, 0.0, 0.0]], np.float32)
    logits = np.zeros((2, 3), np.float32)
    for dtype in (torch.float32, torch.float64):
        C = M.cost_matrix(logits, boxes, [0, 2], tb, (2.0, 5.0, 2.0), dtype)
        assert np.isnan(C).tolist() == [[False, False], [False, True]]  # two empty boxes apart: union 0
        assert abs(C[0, 0] - (2.0 * (0.25 * 0.25 - 0.75 * 0.25) * -np.log(0.5 + 1e-8) - 2.0)) < 1e-6  # identical boxes: GIoU 1, L1 0
        for bad in (3, -1):
            C = M.cost_matrix(logits, boxes, [0, bad], tb, (2.0, 5.0, 2.0), dtype)
            assert np.isnan(C[:, 1]).all() and np.isfinite(C[:, 0]).all()


def test_criterion_is_finite_on_the_whole_box_lattice():
    """What lets the GPU test demand every one of the 256 box gradients: no pair of the lattice has an empty union or hull."""
    boxes = M.box_lattice()
    assert boxes.shape == (256, 4) and len({tuple(b) for b in boxes.tolist()}) == 256
    logits = np.zeros((1, 2, 256, 3), np.float32)
    both = np.stack([boxes, boxes])[None]
    for dtype in (torch.float64, torch.float32):
        out, dl, db = M.criterion(logits, both, [1, 2], np.array(M.LATTICE_TARGETS, np.float32), [0, 1, 2],
                                  np.zeros((1, 2, 256), np.int32), 0.25, 2.0, [[1.0, 1.0, 1.0]], dtype)
        assert np.isfinite(out).all() and np.isfinite(dl).all() and np.isfinite(db).all()
    # the lattice holds what it is for: a coincident box (L1 sign 0 everywhere), touching boxes, ties of an edge, empty boxes
    a0, a1 = boxes[:, :2] - boxes[:, 2:] / 2, boxes[:, :2] + boxes[:, 2:] / 2
    for tgt in M.LATTICE_TARGETS:
        g = np.array(tgt, np.float32)
        g0, g1 = g[:2] - g[2:] / 2, g[:2] + g[2:] / 2
        raw = np.minimum(a1, g1) - np.maximum(a0, g0)
        assert (boxes == g).all(1).sum() == 1 and (raw == 0).any() and (a0 == g0).any() and (a1 == g1).any()
    assert (boxes[:, 2:] == 0).all(1).sum() == 16


def test_criterion_counts_by_hand():
    """Cardinality with the lowest index winning a tie, class_error, and match_t entries >= T as unmatched."""
    x = np.zeros((1, 1, 4, 3), np.float32)
    x[0, 0, 0] = [1, 0, 1]  # tie of 0 and K - 1: argmax 0, counted
    x[0, 0, 1] = [0, 0, 2]  # K - 1: not counted
    x[0, 0, 2] = [0, 0, 0]  # all equal: argmax 0, counted
    x[0, 0, 3] = [0, 5, 0]
    boxes = np.full((1, 1, 4, 4), 0.25, np.float32)
    out, dl, db = M.criterion(x, boxes, [0, 1], np.full((2, 4), 0.25, np.float32), [0, 2], [[[0, 2, -1, 1]]], 0.25, 2.0, [[1, 1, 1]])
    assert out[0, 3] == 1.0 and out[0, 4] == 0.0  # 3 counted, T = 2; rows 0 and 3 are matched and right; the entry 2 = T is no match
    assert not db[0, 0, 1].any() and out[0, 1] == 0.0 and abs(out[0, 2]) < 1e-15
    none = M.criterion(x, boxes, [0, 1], np.full((2, 4), 0.25, np.float32), [0, 2], [[[-1, 2, -1, 9]]], 0.25, 2.0, [[1, 1, 1]])[0]
    assert none[0, 4] == 100.0
