"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  Inputs on which multi-scale deformable attention is EXACT.

On a lattice case every product and every partial sum of the forward pass and of all three gradients is a dyadic rational
with far fewer than 24 significant bits, so the float32 result does not depend on the order of the sums, on the order in
which atomics arrive, on fma contraction or on how the lanes split the work: a kernel can be compared with `==` against the
float64 oracle (tests/test_msda_lattice_cpu.py shows the oracle itself is bit-identical in float32 and float64 on every
configuration below).

  levels      power-of-two sides, non-square and degenerate ones included;
  locations   loc = (k / step + 0.5) / side with integer k, i.e. pixel coordinate k / step: step = 4 (fine lattice, bilinear
              weights are multiples of 1/16) or step = 2 (coarse lattice, multiples of 1/4).  Per level and axis at least one
              point sits on every special coordinate of `specials()`; the other axis of such a point is live, so the special
              coordinate alone decides what happens.  The rest comes from a seeded generator;
  weights     multiples of 1/2 in [-2, 2] (fine) or {-1, 0, 1} (coarse): not restricted to softmax output;
  value       integers in [-4, 4];  cotangent: integers in [-2, 2] (fine) or {-1, 0, 1} (coarse) -- exact in bf16.

The coarse lattice is for the packed-bf16 atomics (grit_msda_bwd_bf16acc), where every partial sum must fit bf16's 8
significant bits: all terms are multiples of 1/4, and the builder asserts that the sum of their magnitudes per element is at
most 32 (so any partial sum, in any order, is a multiple of 1/4 below 64).
"""
import numpy as np
import torch

from oracle import msda as omsda

LEVELS4 = ((8, 4), (4, 8), (2, 2), (1, 1))
LEVELS3 = ((8, 4), (2, 2), (1, 1))
LEVELS2 = ((16, 8), (1, 2))
LEVELS1 = ((4, 8),)
PYRAMID = ((8, 8), (4, 4), (2, 2), (1, 1))  # S = 85: the last 16-cell tile of msda_bwd_value is partial


def specials(side, coarse=False):
    """Pixel coordinates with their own rule, for one axis of a level with `side` cells:
    fine:   -1.25, -1 dead (the strict > -1 test sits at -1); -0.75 live, low corner dead; -0.5 live; 0 and side - 1 kinks
            (at side - 1 the high corner has index side, weight 0 and is dead); side - 0.25 live, high corner dead; side dead
            (the strict < side test sits here); side + 0.25 dead.
    coarse: the same roles on the half lattice: -1.5, -1, -0.5, 0, side - 1, side - 0.5, side, side + 0.5."""
    if coarse:
        return sorted({-1.5, -1.0, -0.5, 0.0, side - 1.0, side - 0.5, float(side), side + 0.5})
    return sorted({-1.25, -1.0, -0.75, -0.5, 0.0, side - 1.0, side - 0.25, float(side), side + 0.25})


class Case(object):
    """float64 numpy inputs of one configuration + lazily computed float64 references (computed once, never modified)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._fwd = self._bwd = None

    @property
    def dims(self):
        B, S, M, D = self.value.shape
        _, Lq, _, L, P, _ = self.loc.shape
        return B, S, M, D, L, Lq, P

    @property
    def nrows(self):
        B, S, M, D, L, Lq, P = self.dims
        return B * Lq * M

    def inputs(self, dtype=np.float64):
        return (self.value.astype(dtype), self.shapes, self.lsi, self.loc.astype(dtype), self.aw.astype(dtype))

    def ref_forward(self):
        if self._fwd is None:
            self._fwd = omsda.msda_forward(*self.inputs())
            self._fwd.setflags(write=False)
        return self._fwd

    def ref_backward(self):
        if self._bwd is None:
            self._bwd = omsda.msda_backward(*self.inputs(), self.cot)
            for a in self._bwd:
                a.setflags(write=False)
        return self._bwd


def to_bf16(a):
    """float64 array -> bf16 tensor, ONE rounding to nearest even (the values here are exact in float32 on the way)."""
    a = np.asarray(a, dtype=np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return torch.tensor(a).to(torch.bfloat16)


def pixel_coords(case, l):
    """(x, y) pixel coordinates of level l's points, [B, Lq, M, P] each -- exact: side is a power of two."""
    H, W = (int(v) for v in case.shapes[l])
    return case.loc[:, :, :, l, :, 0] * W - 0.5, case.loc[:, :, :, l, :, 1] * H - 0.5


def special_counts(case):
    """{(level, axis, coordinate): number of points whose OTHER axis is live} for every special coordinate."""
    out = {}
    for l, (H, W) in enumerate(case.shapes.tolist()):
        x, y = pixel_coords(case, l)
        live_x, live_y = (x > -1) & (x < W), (y > -1) & (y < H)
        for s in specials(W, case.coarse):
            out[(l, "x", s)] = int(((x == s) & live_y).sum())
        for s in specials(H, case.coarse):
            out[(l, "y", s)] = int(((y == s) & live_x).sum())
    return out


def corner_geometry(case):
    """Clamped corner cells and validity flags per point, by the rule of make_corners in grit_amd/csrc/msda.hip:
    cells [B, Lq, M, L, P, 4] (index into the S cells of an image), flags [B, Lq, M, L, P, 4] (corner inside the map and the
    point live)."""
    B, S, M, D, L, Lq, P = case.dims
    cells = np.zeros((B, Lq, M, L, P, 4), dtype=np.int64)
    flags = np.zeros((B, Lq, M, L, P, 4), dtype=bool)
    for l, (H, W) in enumerate(case.shapes.tolist()):
        x, y = pixel_coords(case, l)
        live = (y > -1) & (x > -1) & (y < H) & (x < W)
        hl = np.clip(np.floor(y), -2, H).astype(np.int64)
        wl = np.clip(np.floor(x), -2, W).astype(np.int64)
        for k, (dh, dw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            h, w = hl + dh, wl + dw
            flags[:, :, :, l, :, k] = live & (h >= 0) & (h <= H - 1) & (w >= 0) & (w <= W - 1)
            cells[:, :, :, l, :, k] = int(case.lsi[l]) + np.clip(h, 0, H - 1) * W + np.clip(w, 0, W - 1)
    return cells, flags


def merge_branches(case):
    """(levels whose four points share corner cells and flags: the merged branch of msda_bwd_d64_pk,
        point pairs (2i, 2i + 1) that share them inside a level that is not merged: the pair branch).  P = 4, L*P = 16 only."""
    B, S, M, D, L, Lq, P = case.dims
    if P != 4 or L * P != 16:
        return 0, 0
    cells, flags = corner_geometry(case)
    key = np.concatenate([cells, flags.astype(np.int64)], -1)  # [B, Lq, M, L, 4, 8]
    same = lambda a, b: (key[:, :, :, :, a] == key[:, :, :, :, b]).all(-1)
    merged = same(0, 1) & same(0, 2) & same(0, 3)
    pairs = (same(0, 1) & ~merged).sum() + (same(2, 3) & ~merged).sum()
    return int(merged.sum()), int(pairs)


def max_records_per_cell(case):
    """Largest number of (query, point, corner) records one cell of one (image, head) collects in msda_bwd_value."""
    B, S, M, D, L, Lq, P = case.dims
    cells, flags = corner_geometry(case)
    best = 0
    for b in range(B):
        for m in range(M):
            c = cells[b, :, m][flags[b, :, m]]
            if c.size:
                best = max(best, int(np.bincount(c, minlength=S).max()))
    return best


def build(levels, B, Lq, M, D, P, seed=0, coarse=False, cluster=False, live_levels=()):
    """One lattice case.  cluster: rows 0, 1 (mod 3) put the four points of every level into ONE cell (row 0 mod 3) or points
    (0, 1) and (2, 3) into two different cells (row 1 mod 3), border cells with dead corners included; the special coordinates
    then go to the remaining rows.  live_levels: levels whose generated points are all live (hot cells)."""
    rng = np.random.default_rng(seed)
    step = 2 if coarse else 4
    shapes = np.asarray(levels, dtype=np.int64)
    for side in shapes.ravel():
        assert side & (side - 1) == 0, "power-of-two sides only: (k / step + 0.5) / side must be exact"
    L = len(levels)
    lsi = np.concatenate([[0], np.cumsum(shapes[:, 0] * shapes[:, 1])[:-1]]).astype(np.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    rows = np.arange(B * Lq * M).reshape(B, Lq, M, 1)
    loc = np.zeros((B, Lq, M, L, P, 2))
    all_disjoint = True
    for l, (H, W) in enumerate(levels):
        k = np.zeros((B, Lq, M, P, 2), dtype=np.int64)  # lattice units: pixel coordinate = k / step, axis 0 = x, 1 = y
        for ax, side in ((0, W), (1, H)):
            lo, hi = (-step + 1, side * step - 1) if l in live_levels else (-3 * step // 2, side * step + (5 * step) // 4)
            k[..., ax] = rng.integers(lo, hi + 1, size=(B, Lq, M, P))
            if cluster:
                assert P == 4
                cell = rng.integers(-1, side, size=(B, Lq, M, 1))
                frac = rng.integers(0, step, size=(B, Lq, M, P))
                one = cell * step + frac
                other = np.where(cell + 1 > side - 1, -1, cell + 1)  # a different cell of the same range
                two = np.concatenate([np.broadcast_to(cell, (B, Lq, M, 2)), np.broadcast_to(other, (B, Lq, M, 2))], -1) * step + frac
                k[..., ax] = np.where(rows % 3 == 0, one, np.where(rows % 3 == 1, two, k[..., ax]))
        # special coordinates on a seeded choice of the free points; the other axis of such a point is live
        eligible = rows % 3 == 2 if cluster else np.ones_like(rows, dtype=bool)
        free = rng.permutation(np.flatnonzero(np.broadcast_to(eligible, (B, Lq, M, P)).ravel()))
        sx, sy = specials(W, coarse), specials(H, coarse)
        assert len(free) >= max(len(sx), len(sy)), "too few points per level for the special coordinates"
        kf = k.reshape(-1, 2)
        disjoint = len(free) >= len(sx) + len(sy)
        all_disjoint = all_disjoint and disjoint
        for j, s in enumerate(sx):
            kf[free[j], 0] = int(round(s * step))
            if disjoint:
                kf[free[j], 1] = rng.integers(-step + 1, H * step)
        for j, s in enumerate(sy):
            i = free[len(sx) + j] if disjoint else free[(j + len(sy) // 2) % len(sy)]
            kf[i, 1] = int(round(s * step))
            if disjoint:
                kf[i, 0] = rng.integers(-step + 1, W * step)
        loc[:, :, :, l, :, 0] = (k[..., 0] / step + 0.5) / W
        loc[:, :, :, l, :, 1] = (k[..., 1] / step + 0.5) / H
    if coarse:
        aw = rng.integers(-1, 2, size=(B, Lq, M, L, P)).astype(np.float64)
        cot = rng.integers(-1, 2, size=(B, Lq, M * D)).astype(np.float64)
    else:
        aw = rng.integers(-4, 5, size=(B, Lq, M, L, P)) / 2.0
        cot = rng.integers(-2, 3, size=(B, Lq, M * D)).astype(np.float64)
    value = rng.integers(-4, 5, size=(B, S, M, D)).astype(np.float64)
    case = Case(value=value, shapes=shapes, lsi=lsi, loc=loc, aw=aw, cot=cot, coarse=coarse, cluster=cluster, abs_sum_max=None)
    assert np.array_equal(loc.astype(np.float32).astype(np.float64), loc)
    if all_disjoint:
        missing = [key for key, n in special_counts(case).items() if n == 0]
        assert not missing, missing
    else:  # tiny cases share points between the two axes: the coordinate occurs, its partner may be anything
        for l, (H, W) in enumerate(levels):
            x, y = pixel_coords(case, l)
            assert all((x == s).any() for s in specials(W, coarse)) and all((y == s).any() for s in specials(H, coarse))
    if coarse:
        # every term of grad_value is a multiple of 1/4; with sum of |terms| <= 32 every partial sum fits 8 significant bits
        case.abs_sum_max = float(omsda.msda_backward(value, shapes, lsi, loc, np.abs(aw), np.abs(cot))[0].max())
        assert case.abs_sum_max <= 32.0, case.abs_sum_max
    return case


# Every configuration the GPU file uses, by name: levels, B, Lq, M, D, P (+ options).  Row counts B*Lq*M go over
# {1, 5, 15, 16, 17, 63, 65, 100}: 4-row and 16-row workgroups with a tail, fewer than 8 workgroups, nblk % 8 in {0, 1, 7}.
CONFIGS = {
    # ---- D = 64, by L*P
    "d64_lp4":      dict(levels=LEVELS1, B=1, Lq=5, M=1, D=64, P=4),                 # 5 rows
    "d64_lp6":      dict(levels=LEVELS2, B=1, Lq=5, M=3, D=64, P=3),                 # 15 rows
    "d64_lp8":      dict(levels=LEVELS2, B=2, Lq=2, M=4, D=64, P=4),                 # 16 rows, (Lq*M) % 4 == 0
    "d64_lp12":     dict(levels=LEVELS3, B=1, Lq=17, M=1, D=64, P=4),                # 17 rows
    "d64_lp16":     dict(levels=LEVELS4, B=3, Lq=7, M=3, D=64, P=4),                 # 63 rows, (Lq*M) % 4 != 0
    "d64_lp16_1row": dict(levels=LEVELS1, B=1, Lq=1, M=1, D=64, P=16),               # 1 row
    "d64_lp16_100": dict(levels=LEVELS4, B=5, Lq=5, M=4, D=64, P=4),                 # 100 rows: 25 workgroups of 4, 7 of 16
    "d64_lp17":     dict(levels=LEVELS1, B=1, Lq=5, M=3, D=64, P=17),
    "d64_lp20":     dict(levels=LEVELS4, B=1, Lq=17, M=1, D=64, P=5),
    "d64_lp24":     dict(levels=LEVELS3, B=5, Lq=13, M=1, D=64, P=8),                # 65 rows
    "d64_lp28":     dict(levels=LEVELS4, B=3, Lq=7, M=3, D=64, P=7),
    "d64_lp32":     dict(levels=LEVELS4, B=5, Lq=5, M=4, D=64, P=8),                 # 100 rows
    # L*P = 8 n + 1 (D = 32 and bf16 maps: 8 points per round) or 4 n + 1 (D = 64, f32): the last round has ONE point, handled by
    # the first lane group alone while the lane that read the point's attention weight sits in another group
    "d64_lp9":      dict(levels=LEVELS3, B=1, Lq=5, M=3, D=64, P=3),
    "d64_lp21":     dict(levels=LEVELS3, B=1, Lq=17, M=1, D=64, P=7),
    "d64_lp25":     dict(levels=LEVELS1, B=1, Lq=5, M=1, D=64, P=25),
    "d64_lp29":     dict(levels=LEVELS1, B=2, Lq=2, M=4, D=64, P=29),
    "d64_lp8_p2":   dict(levels=LEVELS4, B=2, Lq=6, M=2, D=64, P=2),                 # P = 2: neither merge branch applies
    "d64_cluster":  dict(levels=LEVELS4, B=2, Lq=6, M=2, D=64, P=4, cluster=True),   # merged and pair branches, interleaved
    # ---- D = 32
    "d32_lp5":      dict(levels=LEVELS1, B=1, Lq=5, M=3, D=32, P=5),
    "d32_lp8":      dict(levels=LEVELS2, B=1, Lq=17, M=1, D=32, P=4),
    "d32_lp16":     dict(levels=LEVELS4, B=5, Lq=13, M=1, D=32, P=4),
    "d32_lp24":     dict(levels=LEVELS3, B=2, Lq=2, M=4, D=32, P=8),
    "d32_lp32":     dict(levels=LEVELS4, B=3, Lq=7, M=3, D=32, P=8),
    "d32_lp9":      dict(levels=LEVELS3, B=1, Lq=5, M=3, D=32, P=3),
    "d32_lp17":     dict(levels=LEVELS1, B=1, Lq=5, M=1, D=32, P=17),
    "d32_lp25":     dict(levels=LEVELS1, B=1, Lq=17, M=1, D=32, P=25),
    # ---- any D
    "d1_lp6":       dict(levels=LEVELS2, B=1, Lq=5, M=3, D=1, P=3),
    "d7_lp6":       dict(levels=LEVELS2, B=3, Lq=7, M=3, D=7, P=3),
    "d130_lp5":     dict(levels=LEVELS1, B=1, Lq=17, M=1, D=130, P=5),
    # ---- coarse lattice (packed-bf16 atomics)
    "pk_lp16":      dict(levels=LEVELS4, B=2, Lq=48, M=2, D=64, P=4, coarse=True),   # a few dozen terms in the small levels' cells
    "pk_lp16_odd":  dict(levels=LEVELS4, B=3, Lq=7, M=3, D=64, P=4, coarse=True),    # 63 rows, not interleaved
    "pk_cluster":   dict(levels=LEVELS4, B=2, Lq=6, M=2, D=64, P=4, coarse=True, cluster=True),
    "pk_lp8_p2":    dict(levels=LEVELS4, B=2, Lq=6, M=2, D=64, P=2, coarse=True),
    "pk_lp12":      dict(levels=LEVELS3, B=1, Lq=5, M=3, D=64, P=4, coarse=True),    # 15 rows
    # ---- msda_bwd_value: parts = clamp(256 / (B*M), 1, 8) workgroups per (image, head)
    "val_parts1":   dict(levels=PYRAMID, B=32, Lq=2, M=8, D=64, P=4),
    "val_parts2":   dict(levels=PYRAMID, B=16, Lq=3, M=8, D=64, P=4),
    "val_parts3":   dict(levels=PYRAMID, B=17, Lq=3, M=5, D=64, P=4),
    "val_parts4":   dict(levels=PYRAMID, B=8, Lq=5, M=8, D=64, P=4),
    "val_parts5":   dict(levels=PYRAMID, B=17, Lq=4, M=3, D=64, P=4),
    "val_parts8":   dict(levels=PYRAMID, B=2, Lq=8, M=8, D=64, P=4),
    "val_big":      dict(levels=((64, 64), (8, 8)), B=33, Lq=2, M=4, D=64, P=8),     # S = 4160, parts = 1: all 16 waves own tiles
    "val_s3":       dict(levels=((1, 2), (1, 1)), B=2, Lq=5, M=8, D=64, P=8),        # S = 3: one tile, 128 waves
    "val_hot":      dict(levels=((2, 2), (1, 1)), B=2, Lq=24, M=2, D=64, P=4, live_levels=(1,)),  # > 64 records in one cell
}

_CASES = {}


def case(name):
    """The (cached) case of CONFIGS[name]; the seed is derived from the name's position, so every case differs."""
    if name not in _CASES:
        _CASES[name] = build(seed=1000 + sorted(CONFIGS).index(name), **CONFIGS[name])
    return _CASES[name]


# ---- weight split of msda_bwd_value: off the lattice, and still exact ------------------------------------------------------

SPLIT_DELTAS = (2.0 ** -9, 2.0 ** -12, 2.0 ** -17, 2.0 ** -20, 2.0 ** -23)
SPLIT_BASES = (0.5, 0.75, 1.0)
# With a in SPLIT_BASES the weight a + delta splits as hi = a, mid = delta, lo = 0 for EVERY delta (a power of two is a bf16
# number however small), so those pairs need the mid term only.  These bases carry a bit below bf16's 8 of their own: hi = 0.5
# or 0.75, mid = the base's low bit, and a delta of 2^-20 or 2^-23 is left for the lo term.
SPLIT_BASES_LO = (0.5 + 2.0 ** -10, 0.75 + 2.0 ** -11)


def bf16_split3(w):
    """hi, mid, lo of a float32 weight as msda_bwd_value step 3 forms them (three bf16 terms whose sum is w exactly)."""
    r = lambda x: float(torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).float())
    w = float(np.float32(w))
    hi = r(w)
    mid = r(float(np.float32(w - hi)))
    lo = r(float(np.float32(np.float32(w - hi) - np.float32(mid))))
    return hi, mid, lo


def split_pairs():
    """(a, delta) of every query pair; a + delta and every partial sum of the pair's terms fit 24 bits (1 + 2^-23 does not)."""
    pairs = [(a, d) for a in SPLIT_BASES for d in SPLIT_DELTAS if not (a == 1.0 and d == 2.0 ** -23)]
    pairs += [(a, d) for a in SPLIT_BASES_LO for d in SPLIT_DELTAS]
    return pairs


def build_weight_split(seed=7):
    """One 4x4 level, L = P = 1, D = 64.  Queries come in pairs on the same pixel centre (corner weight exactly 1): the first
    has attention weight a + delta and cotangent +g, the second a and -g, with g in {+-1, +-2, +-4} per channel.  The cell's
    gradient is exactly delta * g.  One pair per cell and head (two pairs in a cell could mix scales beyond 24 bits), 12 pairs
    per head: 24 queries and, with the zero-weight corners that lie inside the map, well over 32 records in the one tile.
    -> case, expected grad_value [B, S, M, D] (float64)."""
    rng = np.random.default_rng(seed)
    pairs = split_pairs()
    M = 2
    per_head = (len(pairs) + M - 1) // M
    assert per_head <= 16
    B, S, D, L, P, Lq = 1, 16, 64, 1, 1, 2 * per_head
    shapes = np.asarray([[4, 4]], dtype=np.int64)
    lsi = np.zeros(1, dtype=np.int64)
    loc = np.zeros((B, Lq, M, L, P, 2))
    aw = np.zeros((B, Lq, M, L, P))
    cot = np.zeros((B, Lq, M, D))
    want = np.zeros((B, S, M, D))
    for m in range(M):
        cells = rng.permutation(16)
        for i in range(per_head):
            a, d = pairs[(m * per_head + i) % len(pairs)]
            cy, cx = divmod(int(cells[i]), 4)
            g = rng.choice([1.0, 2.0, 4.0], size=D) * rng.choice([-1.0, 1.0], size=D)
            loc[0, 2 * i:2 * i + 2, m, 0, 0] = ((cx + 0.5) / 4, (cy + 0.5) / 4)
            aw[0, 2 * i, m, 0, 0], aw[0, 2 * i + 1, m, 0, 0] = a + d, a
            cot[0, 2 * i, m], cot[0, 2 * i + 1, m] = g, -g
            want[0, cells[i], m] = d * g
    assert np.array_equal(aw.astype(np.float32).astype(np.float64), aw)
    value = rng.integers(-4, 5, size=(B, S, M, D)).astype(np.float64)
    c = Case(value=value, shapes=shapes, lsi=lsi, loc=loc, aw=aw, cot=cot.reshape(B, Lq, M * D), coarse=False, cluster=False,
             abs_sum_max=None)
    return c, want
