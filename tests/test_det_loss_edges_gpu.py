"""Edges of the detector's matcher and set criterion (grit_amd/csrc/detloss.hip) that fixture G19 never reaches, against the plain
references of tests/det_loss_model.py (themselves checked by tests/test_det_loss_model_cpu.py).  Needs an MI355X.

a. The solver alone on integer costs: long augmenting paths, lane edges of the column side (63 .. 129 and the bound, 512), ties,
   forbidden (+inf, NaN) pairs, infeasible problems and invalid descriptors next to good problems.  Integer costs make every total
   exact in float64, so `device total == scipy total` is asserted with no tolerance, and indices where the optimum is unique.
b. Fused cost and assignment on a box lattice with saturated logits, K = 1, labels outside [0, K), empty boxes.
c. The criterion with hand-made match_t: exact ties and touching boxes of the GIoU gradient, focal terms in the tails, the loop
   edges of Q, K and B, every kind of match_t entry, cardinality and class_error where the answer is known, the workspaces.

Bounds of (c) follow tests/test_det_criterion_gpu.py: min(CAP, max(4 x MEASURED, 4 x |ref32 - ref64|)), relative to |reference| for a
loss and to the tensor's largest magnitude for a gradient, where ref32 is the same model evaluated in float32.  Costs -inf are
outside the kernels' contract (include/grit_hip.h) and are not run.
"""
import numpy as np
import pytest
import torch

from tests import det_loss_model as M
from tests.helpers import t
from tests.test_det_criterion_gpu import CAP
from tests.test_det_match_gpu import COST_TOL, check_problem

import det_draws as D  # tests/golden, put on the path by tests.helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Largest |C_device - C_model64| / max(1, |C_model64|) measured on an MI355X over the lattice problems of (b).  It is above
# COST_TOL because the stated composition forms 1 - p in fp32: at logits 8 and 30 that loses digits, in the float32 model as well.
MEASURED_LATTICE_COST_DEV = 3.03e-5

# Largest deviations from the float64 model seen on an MI355X, per group of (c): relative to |reference| (loss), to max |gradient|
# (dlogits, dboxes); for the focal tails dlogits is relative to each element's own reference.
MEASURED = {
    'lattice': {'loss': 3.84e-08, 'dlogits': 3.09e-07, 'dboxes': 2.57e-08},
    'tails': {'loss': 6.98e-08, 'dlogits': 2.13e-07, 'dboxes': 3.30e-08},
    'edges': {'loss': 1.21e-07, 'dlogits': 3.64e-07, 'dboxes': 5.43e-08},
    'b257': {'loss': 2.90e-08, 'dlogits': 3.89e-07, 'dboxes': 2.00e-08},
    'match_t': {'loss': 7.59e-08, 'dlogits': 2.38e-07, 'dboxes': 3.07e-08},
    'coef': {'loss': 5.26e-08, 'dlogits': 1.57e-07, 'dboxes': 4.88e-08},
}
W = (D.COST_WEIGHTS['class'], D.COST_WEIGHTS['bbox'], D.COST_WEIGHTS['giou'])


# =============================================================================================================== a. the solver

def _launch(problems):
    """problems: [(C [q, t], rows override or None, count override or None)] -> match_q [P, ld], match_t [P, Q] device tensors of
    ONE launch.  Whatever lies outside a problem's own block is NaN: it must not be read."""
    from grit_amd.ops.det_loss import linear_sum_assignment
    Q, ld = max(C.shape[0] for C, _, _ in problems), max(max(C.shape[1] for C, _, _ in problems), 1)
    cost = np.full((len(problems), Q, ld), np.nan, np.float32)
    for n, (C, _, _) in enumerate(problems):
        cost[n, :C.shape[0], :C.shape[1]] = C
    rows = [C.shape[0] if r is None else r for C, r, _ in problems]
    counts = [C.shape[1] if c is None else c for C, _, c in problems]
    return linear_sum_assignment(t(cost, device=DEV), torch.tensor(counts, dtype=torch.int32, device=DEV),
                                 torch.tensor(rows, dtype=torch.int32, device=DEV))


def _judge(mq, mt, C, unique=False):
    """One problem's rows of a launch against scipy on C [Q, T]: structure (check_problem), the tails, the total with NO
    tolerance, the indices where the optimum is unique; all -1 where scipy finds the problem infeasible."""
    Q, T = C.shape
    pairs = M.assign(C)
    if pairs is None:
        assert (mq == -1).all() and (mt == -1).all(), "an infeasible problem must come back unmatched"
        return
    check_problem(mq, mt, None, Q, T, pairs[0], pairs[1], demand_indices=unique)
    assert (mq[T:] == -1).all() and (mt[Q:] == -1).all()
    C64 = C.astype(np.float64)
    got = float(sum(C64[q, k] for k, q in enumerate(mq[:T]) if q >= 0))
    assert got == float(C64[pairs[0], pairs[1]].sum()), (got, float(C64[pairs[0], pairs[1]].sum()))


def _solve_and_judge(C, unique=False):
    mq, mt = _launch([(C, None, None)])
    _judge(mq.cpu().numpy()[0], mt.cpu().numpy()[0], C, unique)
    return mq, mt


@pytest.mark.parametrize("Q,T", [(65, 65), (64, 130), (130, 64), (129, 70), (70, 129)])
def test_product_matrices_need_full_length_searches(Q, T):
    """C[i, j] = (i + 1)(j + 1): one optimum, and each augmenting search walks through every column assigned so far."""
    _solve_and_judge(M.product_matrix(Q, T), unique=True)


@pytest.mark.parametrize("Q,T", [(64, 64), (128, 129), (129, 128), (63, 65), (65, 63), (512, 512)])
def test_square_random_integers(Q, T):
    """Integers in [0, min(Q, T)): searches tens of columns long, many equal reduced lengths; (512, 512) is the bound."""
    _solve_and_judge(M.integer_matrix(100 + Q + T, Q, T, 0, min(Q, T)))


@pytest.mark.parametrize("Q,T", [(65, 65), (20, 150), (150, 20)])
def test_small_ranges_are_solved_and_repeat_byte_for_byte(Q, T):
    """[-2, 2]: heavy in ties, mixed in sign.  The choice among equal lengths is a function of the data alone."""
    C = M.integer_matrix(7 + Q, Q, T, -2, 3)
    first = _solve_and_judge(C)
    again = _launch([(C, None, None)])
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def _mixed_problems():
    tiny = [C for _, C in M.tiny_problems()]
    return ([M.product_matrix(65, 65), M.integer_matrix(3, 63, 65, 0, 63), M.integer_matrix(4, 20, 150, -2, 3)] + tiny +
            [np.zeros((30, 0), np.float32),                # T = 0
             M.integer_matrix(5, 40, 1, -2, 3),            # T = 1
             M.integer_matrix(6, 1, 150, -2, 3),           # rows[p] = 1
             M.integer_matrix(8, 1, 1, 3, 4)])


def test_one_launch_of_many_problems():
    problems = _mixed_problems()
    mq, mt = _launch([(C, None, None) for C in problems])
    mq, mt = mq.cpu().numpy(), mt.cpu().numpy()
    assert mq.shape == (len(problems), 150) and mt.shape == (len(problems), 65)
    for n, C in enumerate(problems):
        _judge(mq[n], mt[n], C, unique=n == 0)


def test_forbidden_pairs_inf_and_nan():
    plain, scattered = M.band_matrix(11), M.band_matrix(11, nan_every=7)
    assert np.isnan(scattered).any() and np.array_equal(np.isfinite(plain), np.isfinite(scattered))
    mq, mt = _launch([(plain, None, None), (scattered, None, None), (plain.T.copy(), None, None)])
    mq, mt = mq.cpu().numpy(), mt.cpu().numpy()
    _judge(mq[0], mt[0], plain)
    _judge(mq[1], mt[1], scattered)
    _judge(mq[2], mt[2], plain.T.copy())
    assert np.array_equal(mq[0], mq[1]) and np.array_equal(mt[0], mt[1]), "NaN must forbid a pair exactly as +inf does"


def test_infeasible_problem_leaves_its_neighbours_alone():
    bad, good = M.infeasible_matrix(5), M.integer_matrix(9, 6, 6, 0, 5)
    assert M.assign(bad) is None and M.assign(bad.T) is None
    wide = np.concatenate([bad, np.full((6, 3), np.inf, np.float32)], 1)  # T > Q, still two rows with one finite column
    problems = [good, bad, bad.T.copy(), good.T.copy(), wide, M.integer_matrix(10, 6, 9, 0, 5)]
    mq, mt = _launch([(C, None, None) for C in problems])
    mq, mt = mq.cpu().numpy(), mt.cpu().numpy()
    for n, C in enumerate(problems):
        _judge(mq[n], mt[n], C)
    for n in (1, 2, 4):
        assert (mq[n] == -1).all() and (mt[n] == -1).all()


def test_invalid_descriptors_next_to_good_problems():
    """counts[p] of -1 and ld + 1, rows[p] of -1 and Q + 1: refused by the kernel's range check in front of any access."""
    good = [M.integer_matrix(20 + n, 9, 12, -2, 3) for n in range(6)]
    Q, ld = 9, 12
    problems = [(good[0], None, None), (good[1], None, -1), (good[2], None, ld + 1), (good[3], -1, None), (good[4], Q + 1, None),
                (good[5], None, None), (good[0].T.copy()[:9, :9], None, None)]
    mq, mt = _launch(problems)
    mq, mt = mq.cpu().numpy(), mt.cpu().numpy()
    assert mq.shape == (7, ld) and mt.shape == (7, Q)
    for n in (1, 2, 3, 4):
        assert (mq[n] == -1).all() and (mt[n] == -1).all()
    for n in (0, 5, 6):
        _judge(mq[n], mt[n], problems[n][0])


# ====================================================================================== b. fused cost and assignment (match)

def _targets(tg):
    return [{'labels': t(np.asarray(l, np.int64).reshape(-1), device=DEV), 'boxes': t(np.asarray(b, np.float32).reshape(-1, 4), device=DEV)}
            for l, b in tg]


def _match(logits, boxes, tg):
    from grit_amd.ops.det_loss import match, pack_targets
    mq, mt, cost = match(t(logits, device=DEV), t(boxes, device=DEV), pack_targets(_targets(tg)), *W, return_cost=True)
    return mq.cpu().numpy(), mt.cpu().numpy(), cost.cpu().numpy()


def _cost_deviation(dev, logits, boxes, labels, tb):
    """Largest |dev - C64| / max(1, |C64|) of one problem, after asserting the bound max(COST_TOL, 4 |C32 - C64|) per element."""
    C64 = M.cost_matrix(logits, boxes, labels, tb, W, torch.float64)
    C32 = M.cost_matrix(logits, boxes, labels, tb, W, torch.float32).astype(np.float64)
    assert np.isfinite(C64).all() and np.isfinite(dev).all()
    scaled = np.abs(dev.astype(np.float64) - C64) / np.maximum(1.0, np.abs(C64))
    bound = np.maximum(COST_TOL, 4 * np.abs(C32 - C64))
    worst = np.unravel_index(np.argmax(scaled - bound), scaled.shape)
    assert (scaled <= bound).all(), (worst, float(dev[worst]), float(C64[worst]), float(C32[worst]))
    return float(scaled.max())


def test_cost_values_on_the_box_lattice():
    """Identical, touching, nested and disjoint pairs, empty predicted boxes, logits out to +-30 (sigmoid saturates in fp32).  The
    targets come from the lattice's boxes with non-zero sides: two empty boxes have an empty union and a NaN cost, which is the
    degenerate-box test's subject, not this one's."""
    L, B, Q, K = 2, 3, 65, 5
    counts = (9, 65, 70)
    rng = np.random.default_rng(31)
    lattice, positive = M.box_lattice(), M.box_lattice(positive_sides=True)
    tg = []
    for T in counts:
        labels = rng.integers(0, K, T)
        labels[0], labels[1] = 0, K - 1
        tg.append((labels, positive[rng.integers(0, len(positive), T)]))
    boxes = np.stack([np.stack([lattice[rng.choice(256, Q, replace=False)] for _ in range(B)]) for _ in range(L)])
    for b in range(B):
        boxes[:, b, 0] = tg[b][1][0]  # an identical pair in every problem
    logits = rng.choice(np.array([-30, -8, 0, 8, 30], np.float32), (L, B, Q, K))
    mq, mt, cost = _match(logits, boxes, tg)
    assert cost.shape == (L, B, Q, max(counts))
    worst = 0.0
    for l in range(L):
        for b, T in enumerate(counts):
            own = cost[l, b, :, :T]
            worst = max(worst, _cost_deviation(own, logits[l, b], boxes[l, b], *tg[b]))
            # optimality is judged on the DEVICE's own matrix; on this lattice many matchings share the optimum
            check_problem(mq[l, b], mt[l, b], own, Q, T, *M.assign(own), demand_indices=False)
            assert (mq[l, b, T:] == -1).all()
    print("det edges lattice cost: largest scaled |C_dev - C_model64| = %.3e (recorded %.3e, COST_TOL %.3e)"
          % (worst, MEASURED_LATTICE_COST_DEV, COST_TOL))


def test_match_with_one_class():
    Q, T = 4, 2
    logits, boxes = D.predictions(41, Q, 1)
    labels, tb = np.zeros(T, np.int64), D.boxes(np.random.default_rng(42), T)
    mq, mt, cost = _match(logits[None, None], boxes[None, None], [(labels, tb)])
    _cost_deviation(cost[0, 0], logits, boxes, labels, tb)
    check_problem(mq[0, 0], mt[0, 0], cost[0, 0], Q, T, *M.assign(cost[0, 0]), demand_indices=False)
    C32 = M.cost_matrix(logits, boxes, labels, tb, W, torch.float32)
    assert M.margin(C32) >= 1e-2  # one optimum, by far more than fp32 rounding: the indices are demanded
    check_problem(mq[0, 0], mt[0, 0], None, Q, T, *M.assign(C32))


@pytest.mark.parametrize("bad", ["K", "-1"])
def test_label_outside_the_classes_poisons_its_problem_only(bad):
    L, B, Q, K = 2, 3, 8, 5
    counts = (3, 2, 3)
    logits = np.stack([np.stack([D.predictions(600 + l * B + b, Q, K)[0] for b in range(B)]) for l in range(L)])
    boxes = np.stack([np.stack([D.predictions(600 + l * B + b, Q, K)[1] for b in range(B)]) for l in range(L)])
    tg = [D.targets(650 + b, T, K) for b, T in enumerate(counts)]
    tg[1][0][1] = K if bad == "K" else -1
    mq, mt, cost = _match(logits, boxes, tg)
    for l in range(L):
        assert (mq[l, 1] == -1).all() and (mt[l, 1] == -1).all()
        assert np.isnan(cost[l, 1, :, 1]).all() and np.isfinite(cost[l, 1, :, 0]).all()
        for b in (0, 2):
            T = counts[b]
            _cost_deviation(cost[l, b, :, :T], logits[l, b], boxes[l, b], *tg[b])
            C32 = M.cost_matrix(logits[l, b], boxes[l, b], tg[b][0], tg[b][1], W, torch.float32)
            assert M.margin(C32) >= 1e-2  # one optimum, by far more than fp32 rounding: the indices are demanded
            check_problem(mq[l, b], mt[l, b], cost[l, b, :, :T], Q, T, *M.assign(C32))
            assert (mq[l, b, T:] == -1).all()


def test_empty_boxes_apart_give_a_nan_pair_that_is_never_matched():
    Q, K, T = 6, 3, 3
    rng = np.random.default_rng(77)
    for Q, T in ((6, 3), (3, 6), (4, 4)):
        logits, boxes = D.predictions(78 + Q, Q, K)
        labels, tb = D.targets(79 + T, T, K)
        boxes[2], tb[1] = (0.25, 0.25, 0.0, 0.0), (0.75, 0.75, 0.0, 0.0)
        other = (D.targets(80, 2, K)[0], D.boxes(rng, 2))  # an ordinary neighbour in the same launch
        lg = np.stack([logits, D.predictions(81, Q, K)[0]])[None]
        bx = np.stack([boxes, D.predictions(81, Q, K)[1]])[None]
        mq, mt, cost = _match(lg, bx, [(labels, tb), other])
        own = cost[0, 0, :, :T].copy()
        C64 = M.cost_matrix(logits, boxes, labels, tb, W, torch.float64)
        want = np.zeros((Q, T), bool)
        want[2, 1] = True
        assert np.array_equal(np.isnan(own), want) and np.array_equal(np.isnan(C64), want)
        assert mt[0, 0, 2] != 1 and mq[0, 0, 1] != 2
        own[2, 1] = np.inf  # the NaN pair excluded: scipy's optimum with that entry forbidden
        check_problem(mq[0, 0], mt[0, 0], own, Q, T, *M.assign(own), demand_indices=False)
        check_problem(mq[0, 1], mt[0, 1], cost[0, 1, :, :2], Q, 2, *M.assign(cost[0, 1, :, :2]), demand_indices=False)


# =========================================================================================================== c. the criterion

def _run(logits, boxes, tg, match_t, coef, alpha=0.25):
    """The op through autograd with the weighted sum sum(coef * out[:, :3]) -> (out, dlogits, dboxes) of the device in float64 numpy,
    then the same triple from the model in float64 and in float32."""
    from grit_amd.ops.det_loss import pack_targets, set_criterion
    coef = np.asarray(coef, np.float32)
    packed = pack_targets(_targets(tg))
    x = t(np.asarray(logits, np.float32), device=DEV).requires_grad_(True)
    bx = t(np.asarray(boxes, np.float32), device=DEV).requires_grad_(True)
    out = set_criterion(x, bx, t(np.asarray(match_t, np.int32), device=DEV), packed, alpha)
    (out[:, :3] * t(coef, device=DEV)).sum().backward()
    got = (out.detach().double().cpu().numpy(), x.grad.double().cpu().numpy(), bx.grad.double().cpu().numpy())
    labels = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l, _ in tg])
    tb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for _, b in tg])
    offsets = np.concatenate([[0], np.cumsum([len(np.asarray(l).reshape(-1)) for l, _ in tg])])
    args = (logits, boxes, labels, tb, offsets, match_t, alpha, float(max(len(labels), 1)), coef.astype(np.float64))
    return got, M.criterion(*args), M.criterion(*args, dtype=torch.float32)


def _hold(group, got, ref, ref32, seen, failures, what=""):
    """The bounds of the module docstring on the three losses and both gradients; cardinality_error must be equal, class_error
    within two fp32 ulps of 100 (the kernel rounds 100 / matched and its product with the correct rows once each, both below
    100; the subtraction from 100 is then exact).  Columns 5.. of the device's out are zero."""
    out, dl, db = got
    assert out.shape[1] == 8 and not out[:, 5:].any()
    measured = MEASURED[group]
    for l in range(out.shape[0]):
        for col in range(3):
            r = ref[0][l, col]
            if r == 0.0:
                dev, bound = abs(out[l, col]), 0.0
            else:
                dev = abs(out[l, col] - r) / abs(r)
                bound = min(CAP, max(4 * measured['loss'], 4 * abs(ref32[0][l, col] - r) / abs(r)))
                seen['loss'] = max(seen['loss'], dev)
            if not dev <= bound:
                failures.append((what, 'out[%d, %d]' % (l, col), out[l, col], r, dev, bound))
    if not np.array_equal(out[:, 3], ref[0][:, 3].astype(np.float32).astype(np.float64)):
        failures.append((what, 'cardinality_error', out[:, 3].tolist(), ref[0][:, 3].tolist()))
    if not (np.abs(out[:, 4] - ref[0][:, 4]) <= 2 * float(np.spacing(np.float32(100.0)))).all():
        failures.append((what, 'class_error', out[:, 4].tolist(), ref[0][:, 4].tolist()))
    for name, g, r, r32 in (('dlogits', dl, ref[1], ref32[1]), ('dboxes', db, ref[2], ref32[2])):
        assert g.shape == r.shape and np.isfinite(r).all()
        scale = float(np.abs(r).max())
        if scale == 0.0:
            dev, bound = float(np.abs(g).max()), 0.0
        else:
            dev = float(np.abs(g - r).max()) / scale
            bound = min(CAP, max(4 * measured[name], 4 * float(np.abs(r32 - r).max()) / scale))
            seen[name] = max(seen[name], dev)
        if not dev <= bound:
            failures.append((what, name, dev, bound))


def _report(group, seen, failures, what=""):
    print("det edges %s %s: deviations %s (recorded %s)" % (group, what, {k: float('%.3e' % v) for k, v in seen.items()}, MEASURED[group]))
    assert not failures, failures


def _new_seen():
    return {'loss': 0.0, 'dlogits': 0.0, 'dboxes': 0.0}


def test_giou_gradient_on_the_box_lattice():
    """All 256 lattice boxes matched to one target per image: exact ties of every edge (the 0.5 branches), touching boxes (the
    clamp at exactly zero), containment both ways, the coincident box (an L1 sign of 0) and empty predictions.  Layer 1 matches
    every other row only.  No matched row is skipped (the model is finite on all of them, tests/test_det_loss_model_cpu.py), and
    an unmatched row's box gradient is exactly zero."""
    L, B, Q, K = 2, 2, 256, 3
    lattice = M.box_lattice()
    boxes = np.broadcast_to(lattice, (L, B, Q, 4)).copy()
    logits = (2 * np.random.default_rng(5).standard_normal((L, B, Q, K))).astype(np.float32)
    tg = [([1], [M.LATTICE_TARGETS[0]]), ([2], [M.LATTICE_TARGETS[1]])]
    match_t = np.zeros((L, B, Q), np.int32)
    match_t[1, :, 1::2] = -1
    got, ref, ref32 = _run(logits, boxes, tg, match_t, [[2.0, 5.0, 2.0], [1.0, 0.5, 3.0]])
    seen, failures = _new_seen(), []
    _hold('lattice', got, ref, ref32, seen, failures)
    db = got[2]
    assert np.isfinite(db).all() and not db[1, :, 1::2].any()
    # row by row as well, held to CAP of the row's largest magnitude (the kernel's formula evaluates in double and rounds once, so
    # 2^-24 is what to expect), so that one wrong branch of one box cannot hide under the tensor's largest magnitude; the
    # box that coincides with its target has L1 sign 0 and sits at GIoU's maximum: its row is zero and is held absolutely
    scale = np.abs(ref[2]).max(-1, keepdims=True)
    row_dev = np.abs(db - ref[2]) / np.where(scale > 0, scale, 1.0)
    seen['dboxes_row'] = float(row_dev.max())
    if not row_dev.max() <= CAP:
        failures.append(('row', np.unravel_index(np.argmax(row_dev), row_dev.shape), float(row_dev.max())))
    _report('lattice', seen, failures)


TAIL_VALUES = (-80.0, -30.0, -17.0, -8.0, -1.0, 0.0, 1.0, 8.0, 17.0, 30.0, 80.0)
TINY = 2.0 ** -100  # below it a reference gradient is the fp32 underflow of p^2: the device only has to stay below it too


def test_focal_terms_in_the_tails():
    """Each tail value once as the matched class (column 0) and once as a negative (column 1); dlogits element by element relative
    to ITS OWN float64 value, held to CAP: what `none of them by cancellation` claims."""
    n = len(TAIL_VALUES)
    logits = np.zeros((1, 1, n, 2), np.float32)
    logits[0, 0, :, 0] = TAIL_VALUES
    logits[0, 0, :, 1] = np.roll(TAIL_VALUES, 3)
    boxes = D.boxes(np.random.default_rng(3), n)[None, None]
    tg = [([0], D.boxes(np.random.default_rng(4), 1))]
    got, ref, ref32 = _run(logits, boxes, tg, np.zeros((1, 1, n), np.int32), [[1.0, 1.0, 1.0]])
    seen, failures = _new_seen(), []
    _hold('tails', got, ref, ref32, seen, failures)
    dl, r, r32 = got[1].reshape(-1), ref[1].reshape(-1), ref32[1].reshape(-1)
    big = np.abs(r) >= TINY
    assert big.sum() >= 14 and (~big).sum() >= 2  # both kinds exist
    assert (np.abs(dl[~big]) <= TINY).all()
    rel = np.abs(dl[big] - r[big]) / np.abs(r[big])
    rel32 = np.abs(r32[big] - r[big]) / np.abs(r[big])
    seen['dlogits'] = float(rel.max())  # per element here, not per tensor
    for i in np.nonzero(rel > CAP)[0]:
        failures.append(('element', float(logits.reshape(-1)[np.nonzero(big)[0][i]]), float(rel[i]), 'float32 model: %.3e' % rel32[i]))
    _report('tails', seen, failures)


def _random_case(seed, L, B, Q, K, counts):
    rng = np.random.default_rng(seed)
    logits = (3 * rng.standard_normal((L, B, Q, K))).astype(np.float32)
    boxes = D.boxes(rng, L * B * Q).reshape(L, B, Q, 4)
    tg = [(rng.integers(0, K, T), D.boxes(rng, T)) for T in counts]
    match_t = np.full((L, B, Q), -1, np.int32)
    for l in range(L):
        for b, T in enumerate(counts):
            n = min(Q, T)
            match_t[l, b, rng.permutation(Q)[:n]] = rng.permutation(T)[:n]
    return logits, boxes, tg, match_t


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("Q", [1, 19, 20, 21, 41])
def test_loop_edges_of_rows_and_classes(Q, K):
    """Chunks of 20 rows on four waves, classes strided by 64 lanes: one row, a chunk short of one, a full one, one more, two and
    one; fewer classes than lanes, as many, one more, two strides and one."""
    logits, boxes, tg, match_t = _random_case(1000 * Q + K, 2, 2, Q, K, (3, 1))
    got, ref, ref32 = _run(logits, boxes, tg, match_t, [[2.0, 5.0, 2.0], [1.0, 3.0, 0.5]])
    seen, failures = _new_seen(), []
    _hold('edges', got, ref, ref32, seen, failures)
    _report('edges', seen, failures, "Q %d K %d" % (Q, K))


def test_more_images_than_the_finalising_block_has_threads():
    """B = 257: the finalising block strides the images by 256.  Image 256 alone has a target and a matched row, so that its
    share shows in every column: the two box losses and class_error come from it alone."""
    L, B, Q, K = 1, 257, 2, 2
    logits, boxes, _, _ = _random_case(257, L, B, Q, K, ())
    logits[0, 256] = [[5.0, -2.0], [6.0, 4.0]]  # both rows argmax 0, counted; row 1 is matched to label 0: right
    tg = [([], [])] * 256 + [([0], [(0.5, 0.5, 0.25, 0.5)])]
    match_t = np.full((L, B, Q), -1, np.int32)
    match_t[0, 256, 1] = 0
    got, ref, ref32 = _run(logits, boxes, tg, match_t, [[2.0, 5.0, 2.0]])
    assert ref[0][0, 1] > 0 and ref[0][0, 2] > 0 and ref[0][0, 4] == 0.0
    without = M.criterion(logits[:, :256], boxes[:, :256], [], np.zeros((0, 4)), np.zeros(257, np.int64), match_t[:, :256], 0.25, 1.0, [[2.0, 5.0, 2.0]])[0]
    assert abs(without[0, 0] - ref[0][0, 0]) > 10 * CAP * ref[0][0, 0] and without[0, 3] * 256 != ref[0][0, 3] * 257
    seen, failures = _new_seen(), []
    _hold('b257', got, ref, ref32, seen, failures)
    assert got[0][0, 4] == 0.0 and got[2][0, 256, 1].any() and not got[2][0, :256].any()
    _report('b257', seen, failures)


def _match_t_cases():
    L, B, Q, K = 2, 2, 5, 4
    logits, boxes, tg, match_t = _random_case(11, L, B, Q, K, (2, 3))
    yield "all -1", logits, boxes, tg, np.full_like(match_t, -1)
    logits, boxes, tg, match_t = _random_case(12, L, B, 3, K, (5, 5))
    assert (match_t >= 0).all() and match_t.max() == 4
    yield "T 5 > Q 3, every query matched", logits, boxes, tg, match_t
    logits, boxes, tg, match_t = _random_case(13, L, B, Q, K, (2, 3))
    free = np.argwhere(match_t < 0)
    match_t[tuple(free[0])] = (2, 3)[free[0][1]]       # T of its image
    match_t[tuple(free[1])] = (2, 3)[free[1][1]] + 7   # T + 7
    match_t[tuple(free[2])] = -5
    yield "entries T, T + 7 and -5 are unmatched", logits, boxes, tg, match_t
    logits, boxes, tg, match_t = _random_case(14, L, 3, Q, K, (2, 0, 3))
    assert (match_t[:, 1] == -1).all()
    yield "an image without targets between two with", logits, boxes, tg, match_t


def test_match_t_contents():
    seen, failures = _new_seen(), []
    for what, logits, boxes, tg, match_t in _match_t_cases():
        got, ref, ref32 = _run(logits, boxes, tg, match_t, [[2.0, 5.0, 2.0], [0.5, 1.0, 3.0]])
        _hold('match_t', got, ref, ref32, seen, failures, what)
        counts = np.array([len(l) for l, _ in tg])
        unmatched = (match_t < 0) | (match_t >= counts[None, :, None])
        assert not got[2][unmatched].any(), what
        if what == "all -1":
            assert (got[0][:, 4] == 100.0).all() and not got[0][:, 1:3].any()
    _report('match_t', seen, failures)


def _counting_cases():
    """(name, logits [Q, K], labels, match_t [Q]) -> cardinality_error and class_error known exactly."""
    row = lambda *v: list(v)
    yield "argmax at K - 1", [row(0, 1, 2, 3, 9)] * 4, [4, 0], [0, 1, -1, -1], 2.0, 50.0
    yield "tie of 0 and K - 1: the lowest index wins, the row counts", [row(7, 1, 2, 3, 7)] * 4, [0], [-1, -1, 0, -1], 3.0, 0.0
    yield "all-equal rows", [row(2.5, 2.5, 2.5, 2.5, 2.5)] * 4, [4], [0, -1, -1, -1], 3.0, 100.0
    yield "K = 1", [[-3.0], [0.0], [2.0], [80.0]], [0, 0], [-1, 0, -1, 1], 2.0, 0.0
    labels = [0, 1, 2, 3, 0, 1, 2]
    top = [0, 1, 2, 0, 1, 2, 3, 3, 3]  # rows 0..2 right, rows 3..6 one class on, rows 7 and 8 unmatched at K - 1
    logits = [[5.0 if k == a else float(k) - 4 for k in range(4)] for a in top]
    yield "three of seven matched rows right", logits, labels, [0, 1, 2, 3, 4, 5, 6, -1, -1], 1.0, 100.0 - 300.0 / 7.0
    yield "no matched row", [row(1, 0, 0), row(0, 0, 1), row(0, 2, 0), row(0, 0, 0)], [1, 2], [-1, -1, -1, -1], 1.0, 100.0


def test_cardinality_and_class_error_where_the_answer_is_known():
    """Equality, not a tolerance: cardinality_error exactly, class_error to one fp32 ulp of the exact quotient.  The argmax tie
    order (lowest index) is the kernel's documented choice and is pinned here."""
    for what, logits, labels, match_t, cardinality, class_error in _counting_cases():
        logits = np.asarray(logits, np.float32)[None, None]
        Q = logits.shape[2]
        boxes = D.boxes(np.random.default_rng(Q), Q)[None, None]
        tg = [(labels, D.boxes(np.random.default_rng(50), len(labels)))]
        got, ref, _ = _run(logits, boxes, tg, np.asarray(match_t, np.int32)[None, None], [[1.0, 1.0, 1.0]])
        assert ref[0][0, 3] == cardinality and abs(ref[0][0, 4] - class_error) < 1e-12, what  # the model agrees with the hand count
        assert got[0][0, 3] == cardinality, (what, got[0][0, 3])
        assert abs(got[0][0, 4] - class_error) <= float(np.spacing(np.float32(class_error))), (what, got[0][0, 4], class_error)


def test_upstream_coefficients_scale_per_layer_and_per_term():
    """The weighted sum's coefficients reach the backward through autograd: distinct everywhere, zero for one layer's loss_giou."""
    L, B, Q, K = 3, 2, 5, 4
    logits, boxes, tg, match_t = _random_case(21, L, B, Q, K, (3, 1))
    coef = [[1.5, 0.5, 2.0], [0.25, 3.0, 0.0], [2.0, 1.0, 0.75]]
    got, ref, ref32 = _run(logits, boxes, tg, match_t, coef)
    seen, failures = _new_seen(), []
    _hold('coef', got, ref, ref32, seen, failures)
    # layer 1 has no GIoU term: its box gradient is the L1 sign times 3 / num_boxes, exactly (num_boxes = 4)
    hit = match_t[1] >= 0
    assert hit.sum() == 4 and np.array_equal(np.abs(got[2][1][hit]), np.full((4, 4), 0.75))
    assert not np.array_equal(np.abs(got[2][0][match_t[0] >= 0]), np.full((4, 4), 0.125))
    _report('coef', seen, failures)


def test_forward_entry_point_on_poisoned_workspaces():
    """grit_det_loss_fwd_f32 itself: partials and out full of NaN, the ticket at 0xFFFFFFFF.  The entry point zeroes the ticket
    and the kernel writes every value it later reads."""
    from grit_amd import lib
    from grit_amd.ops.det_loss import pack_targets, set_criterion
    L, B, Q, K = 2, 3, 41, 5
    logits, boxes, tg, match_t = _random_case(31, L, B, Q, K, (3, 0, 4))
    packed = pack_targets(_targets(tg))
    x, bx, mt = t(logits, device=DEV), t(boxes, device=DEV), t(match_t, device=DEV)
    want = set_criterion(x, bx, mt, packed, 0.25)
    chunks = (Q + lib.DET_LOSS_ROWS - 1) // lib.DET_LOSS_ROWS
    assert chunks == 3
    p, outs = lib.ptr, []
    for _ in range(2):
        partials = torch.full((L * B * chunks, 8), float('nan'), dtype=torch.float64, device=DEV)
        ticket = torch.full((1,), -1, dtype=torch.int32, device=DEV)  # 0xFFFFFFFF
        out = torch.full((L, lib.DET_LOSS_FIELDS), float('nan'), device=DEV)
        lib.check(lib.load().grit_det_loss_fwd_f32(p(x), p(bx), p(packed.labels), p(packed.boxes), p(packed.offsets), p(mt), L, B, Q, K, 0.25,
                                                   p(packed.num_boxes), p(partials), p(ticket), p(out), lib.current_stream_ptr()), "fwd")
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and not bool(outs[0][:, 5:].any())
    assert outs[0].cpu().numpy().tobytes() == want.detach().cpu().numpy().tobytes() == outs[1].cpu().numpy().tobytes()
