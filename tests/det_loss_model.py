"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  Plain references of the detector's matcher and set criterion
(grit_amd/csrc/detloss.hip: grit_lsa_f32, grit_det_match_f32, grit_det_loss_{fwd,bwd}_f32), written from the comment block
"Detector set criterion" of include/grit_hip.h, and builders of the inputs on which such kernels go wrong.

cost_matrix is the matcher's elementwise composition in a dtype of the caller's choice, assign is scipy's solver, criterion is the
set criterion in torch with autograd (float64 unless asked otherwise).  No kernel of this project is called.
tests/test_det_loss_model_cpu.py checks all three against fixture G19 and brute force; tests/test_det_loss_edges_gpu.py then holds
the kernels to them.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------------- matcher

def cost_matrix(logits, boxes, labels, tgt_boxes, w, dtype):
    """logits [Q, K], boxes [Q, 4], labels [T] int, tgt_boxes [T, 4] (numpy or torch), w = (class, bbox, giou) -> C [Q, T] numpy of
    `dtype` (torch.float32 / torch.float64): w_bbox * L1 + w_class * (pos - neg) - w_giou * GIoU, every operation in `dtype` and in
    the order the header states.  A label outside [0, K) gives a NaN column; a pair of boxes whose union is empty gives NaN, as
    0 / 0 does."""
    from utils.box_ops import box_cxcywh_to_xyxy, generalized_box_iou
    x = torch.as_tensor(logits).to(dtype)
    qb, tb = torch.as_tensor(boxes).to(dtype), torch.as_tensor(tgt_boxes).to(dtype).reshape(-1, 4)
    labels = torch.as_tensor(labels).to(torch.int64).reshape(-1)
    K = x.shape[1]
    valid = (labels >= 0) & (labels < K)
    p = 1.0 / (1.0 + torch.exp(-x[:, labels.clamp(0, K - 1)]))  # [Q, T]
    neg = 0.75 * (p * p) * (-torch.log(1.0 - p + 1e-8))
    pos = 0.25 * ((1.0 - p) * (1.0 - p)) * (-torch.log(p + 1e-8))
    cls = pos - neg
    d = (qb[:, None, :] - tb[None, :, :]).abs()
    l1 = d[..., 0] + d[..., 1] + d[..., 2] + d[..., 3]
    giou = generalized_box_iou(box_cxcywh_to_xyxy(qb), box_cxcywh_to_xyxy(tb))
    C = w[1] * l1 + w[0] * cls + w[2] * (-giou)
    C = torch.where(valid[None, :], C, torch.full_like(C, float('nan')))
    return C.numpy()


def assign(C):
    """scipy.optimize.linear_sum_assignment on C [Q, T] -> (i, j), or None for an infeasible problem.  +inf forbids a pair; so
    does NaN here (the kernel never takes an entry that does not compare below a finite length), which scipy itself refuses."""
    from scipy.optimize import linear_sum_assignment
    C = np.asarray(C, np.float64)
    try:
        return linear_sum_assignment(np.where(np.isnan(C), np.inf, C))
    except ValueError:
        return None


def brute_force_total(C):
    """The optimum of a tiny problem by trying every injection of the smaller side into the larger; None when none is finite."""
    C = np.asarray(C, np.float64)
    C = np.where(np.isnan(C), np.inf, C)
    if C.shape[0] > C.shape[1]:
        C = C.T
    n, m = C.shape
    best = min((sum(C[i, j] for i, j in enumerate(perm)) for perm in itertools.permutations(range(m), n)), default=0.0)
    return None if np.isinf(best) else float(best)


def margin(C):
    """Smallest increase of the optimum when one matched pair is forbidden (inf when no other matching exists)."""
    C = np.asarray(C, np.float64)
    i, j = assign(C)
    opt, best = C[i, j].sum(), np.inf
    for a, b in zip(i, j):
        Cf = C.copy()
        Cf[a, b] = np.inf
        alt = assign(Cf)
        if alt is not None:
            best = min(best, Cf[alt[0], alt[1]].sum() - opt)
    return best


# ---- solver inputs: integers in fp32, so that every total is exact in float64

def product_matrix(Q, T):
    """C[i, j] = (i + 1)(j + 1): the unique optimum pairs the smaller side, reversed, with the first indices of the larger
    (rearrangement inequality, all products distinct along it), and every augmenting search runs through all assigned columns."""
    return np.outer(np.arange(1, Q + 1), np.arange(1, T + 1)).astype(np.float32)


def integer_matrix(seed, Q, T, lo, hi):
    """Uniform integers in [lo, hi)."""
    return np.random.default_rng(seed).integers(lo, hi, (Q, T)).astype(np.float32)


def band_matrix(seed, n=65, nan_every=0):
    """+inf except three finite integers per row on a wrapping band (the diagonal is always finite, so the problem is feasible);
    with nan_every, every nan_every-th forbidden entry is NaN instead."""
    rng = np.random.default_rng(seed)
    C = np.full((n, n), np.inf, np.float32)
    if nan_every:
        flat = C.reshape(-1)
        flat[::nan_every] = np.nan
    for i in range(n):
        for d in range(3):
            C[i, (i + d) % n] = rng.integers(0, 5)
    return C


def infeasible_matrix(seed, n=6):
    """Rows 0 and 1 have their only finite entry in column 0."""
    C = integer_matrix(seed, n, n, 0, 5)
    C[0, 1:] = np.inf
    C[1, 1:] = np.inf
    return C


def tiny_problems():
    """Tie-heavy integer problems with Q, T <= 6, brute force is their judge: [(name, C [Q, T])]."""
    rng = np.random.default_rng(2024)
    out = [('tied 6x4', np.array([[4, 1, 3, 1], [2, 0, 5, 0], [2, 0, 5, 0], [3, 2, 2, 2], [1, 1, 1, 1], [9, 9, 9, 9]], np.float32))]
    for n, (Q, T) in enumerate(((6, 6), (6, 6), (5, 6), (6, 5), (1, 6), (6, 1), (3, 4), (2, 2))):
        out.append(('ints %dx%d #%d' % (Q, T, n), rng.integers(-1, 2, (Q, T)).astype(np.float32)))
    out.append(('zeros 6x6', np.zeros((6, 6), np.float32)))
    C = rng.integers(0, 3, (6, 6)).astype(np.float32)
    C[rng.random((6, 6)) < 0.3] = np.inf
    C[np.arange(6), np.arange(6)] = 1  # feasible
    out.append(('forbidden 6x6', C))
    return out


# ---- boxes on a dyadic lattice: corners, sides, areas and their sums are exact in fp32, and edges tie, touch and coincide

LATTICE_CENTRES = (4 / 16, 6 / 16, 8 / 16, 10 / 16)
LATTICE_SIDES = (0.0, 2 / 16, 4 / 16, 8 / 16)
LATTICE_TARGETS = ((0.5, 0.5, 0.25, 0.25), (6 / 16, 10 / 16, 4 / 16, 8 / 16))


def box_lattice(positive_sides=False):
    """[256, 4] cxcywh fp32: every (cx, cy, w, h) of LATTICE_CENTRES^2 x LATTICE_SIDES^2; with positive_sides the 144 of them whose
    sides are both non-zero."""
    sides = LATTICE_SIDES[1:] if positive_sides else LATTICE_SIDES
    return np.array(list(itertools.product(LATTICE_CENTRES, LATTICE_CENTRES, sides, sides)), np.float32)


# ----------------------------------------------------------------------------------------------------------------- criterion

def _pair_losses(a, g):
    """L1 and 1 - GIoU of matched cxcywh pairs a, g [n, 4] with torch.max / torch.min / clamp(min=0): autograd splits the
    derivative evenly at a tie and passes the clamp at zero."""
    l1 = (a - g).abs().sum(-1)
    a0, a1 = a[:, :2] - 0.5 * a[:, 2:], a[:, :2] + 0.5 * a[:, 2:]
    g0, g1 = g[:, :2] - 0.5 * g[:, 2:], g[:, :2] + 0.5 * g[:, 2:]
    area_a = (a1[:, 0] - a0[:, 0]) * (a1[:, 1] - a0[:, 1])
    area_g = (g1[:, 0] - g0[:, 0]) * (g1[:, 1] - g0[:, 1])
    iw = (torch.min(a1, g1) - torch.max(a0, g0)).clamp(min=0)
    ew = (torch.max(a1, g1) - torch.min(a0, g0)).clamp(min=0)
    inter, hull = iw[:, 0] * iw[:, 1], ew[:, 0] * ew[:, 1]
    union = area_a + area_g - inter
    return l1, 1.0 - (inter / union - (hull - union) / hull)


def criterion(logits, boxes, labels, tgt_boxes, offsets, match_t, alpha, num_boxes, coef, dtype=torch.float64):
    """The set criterion of all layers.  logits [L, B, Q, K], boxes [L, B, Q, 4], labels [sum T] int, tgt_boxes [sum T, 4], offsets
    [B + 1], match_t [L, B, Q] int (an entry outside [0, T_b) is an unmatched query), num_boxes a float, coef [L, 3] the weights of
    loss_ce, loss_bbox, loss_giou in the total whose gradient is returned.

    -> out [L, 5] float64 numpy (loss_ce, loss_bbox, loss_giou, cardinality_error, class_error), dlogits [L, B, Q, K], dboxes
    [L, B, Q, 4] float64 numpy.  The focal loss is stated through log-sigmoids only (softplus(x) = -logsigmoid(-x), sigmoid(x) =
    exp(logsigmoid(x))): nothing is formed as 1 - p.  An argmax tie goes to the lowest index; class_error is 100 with no match."""
    x = torch.as_tensor(logits).to(dtype).clone().requires_grad_(True)
    bx = torch.as_tensor(boxes).to(dtype).clone().requires_grad_(True)
    labels = torch.as_tensor(labels).to(torch.int64).reshape(-1)
    tb = torch.as_tensor(tgt_boxes).to(dtype).reshape(-1, 4)
    offsets = torch.as_tensor(offsets).to(torch.int64)
    mt = torch.as_tensor(match_t).to(torch.int64)
    coef = torch.as_tensor(coef).to(dtype)
    L, B, Q, K = x.shape
    counts = offsets[1:] - offsets[:-1]
    hit = (mt >= 0) & (mt < counts[None, :, None])
    flat = torch.where(hit, offsets[:-1][None, :, None] + mt, torch.zeros_like(mt))  # row of the packed targets
    label = torch.where(hit, labels[flat] if labels.numel() else torch.zeros_like(mt), torch.full_like(mt, -1))
    positive = torch.arange(K)[None, None, None, :] == label[..., None]
    ls_pos, ls_neg = F.logsigmoid(x), F.logsigmoid(-x)  # log p, log (1 - p)
    on_positive = alpha * (-ls_pos) * torch.exp(2.0 * ls_neg)
    on_negative = (1.0 - alpha) * (-ls_neg) * torch.exp(2.0 * ls_pos)
    loss_ce = torch.where(positive, on_positive, on_negative).sum((1, 2, 3)) / num_boxes
    l1, gl = _pair_losses(bx[hit], tb[flat[hit]])
    layer = torch.arange(L)[:, None, None].expand(L, B, Q)[hit]
    loss_bbox = torch.zeros(L, dtype=dtype).index_add(0, layer, l1) / num_boxes
    loss_giou = torch.zeros(L, dtype=dtype).index_add(0, layer, gl) / num_boxes
    (coef[:, 0] * loss_ce + coef[:, 1] * loss_bbox + coef[:, 2] * loss_giou).sum().backward()
    xd = x.detach()
    top = xd.max(-1, keepdim=True).values
    arg = torch.where(xd == top, torch.arange(K).expand_as(xd), torch.full_like(xd, K, dtype=torch.int64)).min(-1).values
    count = (arg != K - 1).sum(-1).double()  # [L, B]
    cardinality = (count - counts[None, :].double()).abs().mean(1)
    matched = hit.sum((1, 2)).double()
    correct = (hit & (arg == label)).sum((1, 2)).double()
    class_error = torch.where(matched > 0, 100.0 - 100.0 * correct / matched.clamp(min=1), torch.full_like(matched, 100.0))
    out = torch.stack([loss_ce.detach().double(), loss_bbox.detach().double(), loss_giou.detach().double(), cardinality, class_error], 1)
    dboxes = bx.grad if bx.grad is not None else torch.zeros_like(bx)
    return out.numpy(), x.grad.double().numpy(), dboxes.double().numpy()
