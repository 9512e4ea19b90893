"""Backward half of the Linear layers -- wgrad_tn.hip (four- and eight-wave kernels, single and grouped, drop-path row skipping),
wgrad.hip (short maps, single and grouped), colsum.hip (column sums, the three slab-sum shapes) and transpose.hip -- at the step,
slice and job edges the workload-sized shapes of test_gemm_gpu.py and the self-recorded digests of test_wgrad_plan_gpu.py do not
reach: one, two and three steps per slice, last slices shorter than the others, the eight-wave kernel inside a grouped launch
(some job with M % 64 == 32), jobs whose first block is no multiple of 8, row skipping with one step per sample, 64 samples,
slices that begin in the middle of a sample, and every refusal.

EXACT method, no tolerance anywhere.  dY and X are integers in [-LIMIT, LIMIT] = [-3, 3]: exact in bf16, every product at most 9 in
magnitude, every sum over at most MAX_ROWS = 16 384 rows below 9 * 2^14 < 2^18 -- far inside the 2^24 up to which fp32 holds every
integer, so fp32 accumulation is exact in ANY order and the float64 reference of the same contraction is the one right answer.  Every
comparison is torch.equal: each slice's partial against the contraction over THAT slice's rows, each slice's column sums likewise,
bf16 outputs against reference.float().bfloat16() (one round-to-nearest-even of an exactly known value).
test_inputs_stay_in_the_exact_regime keeps a later edit from leaving that regime unnoticed.

Fences.  Every operand is a view into a larger NaN-filled buffer: FENCE = 64 NaN rows before row 0 and after row M - 1 and, where
the leading dimension exceeds the width, NaN columns left and right.  Every output is the middle of a NaN-filled buffer with one
guard slab on either side and is itself pre-filled with NaN.  After a launch the guards are still all NaN and the output is all
finite and exact: a tile computed twice by a wrong block-to-job mapping leaves another tile NaN, a read of row M or of a padding
column puts a NaN into the result, a store outside the output shows in a guard.

Row skipping: which live 64-row step belongs to which slice is MEASURED by a census launch (dY[m, n] = 1 where n is the step of row
m, X = 1: partial[s][n][:] is 64 exactly where step n belongs to slice s) whose result must be a fair share (every live step owned
once, dropped steps by nobody, contiguous runs in order, sizes within one of each other); the exact comparison then uses that
ownership.  The formula of the kernel is not repeated here."""
import pytest
import torch

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LIMIT = 3          # |dY|, |X| <= LIMIT
MAX_ROWS = 16384   # no contraction in this file is longer
FENCE = 64         # NaN rows before and after every operand
NAN = float("nan")
NK_TN = [(256, 256), (512, 256), (256, 512), (512, 768)]
# (M, S, steps per slice): grit_wgrad_tn_grouped with every M % 64 == 0 (64-row steps) ...
FOUR_WAVE = [(64, 1, (1,)), (128, 1, (2,)), (128, 2, (1, 1)), (192, 1, (3,)), (192, 2, (2, 1)), (320, 2, (3, 2)),
             (320, 3, (2, 2, 1)), (640, 1, (10,)), (640, 4, (3, 3, 3, 1))]
# ... and with M % 64 == 32 (32-row steps; 7 and 13 steps wrap the four-stage ring)
EIGHT_WAVE = [(32, 1, (1,)), (96, 1, (3,)), (96, 2, (2, 1)), (96, 3, (1, 1, 1)), (160, 2, (3, 2)), (224, 1, (7,)),
              (224, 3, (3, 3, 1)), (416, 1, (13,)), (416, 5, (3, 3, 3, 3, 1))]
SMALL_NK = [(64, 64), (128, 64), (64, 192)]
SMALL_M = [1, 31, 32, 33, 64, 65, 416, 417, 833]


def _L():
    from grit_amd import lib
    return lib


def _ints(shape, seed, device=DEV, dtype=BF16):
    """Random integers in [-LIMIT, LIMIT], the same on every device (drawn on the host)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-LIMIT, LIMIT + 1, tuple(shape), generator=g).to(device=device, dtype=dtype)


def _ceil(a, b):
    return -(-a // b)


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------------
# CPU: the exact regime, and the slice normalisation of ops/linear.py against the kernel's and the library's
# ---------------------------------------------------------------------------------------------------------------
def test_inputs_stay_in_the_exact_regime():
    """What `torch.equal` rests on: |values| <= 3 (and 3 occurs), integers, exact in bf16; the longest contraction sums
    MAX_ROWS products of at most 9 and stays below 2^18 (fp32 holds every integer up to 2^24); every shape of this file is within
    MAX_ROWS (asserted again where an operand is built)."""
    for seed in (0, 1, 2):
        v = _ints((64, 256), seed, device="cpu", dtype=F32)
        assert float(v.abs().max()) == LIMIT == 3 and torch.equal(v, v.round())
        assert torch.equal(v.bfloat16().float(), v)
    assert LIMIT * LIMIT * MAX_ROWS < 2 ** 18 <= 2 ** 24
    rows = [m for m, _, _ in FOUR_WAVE + EIGHT_WAVE] + SMALL_M + [2080, 4096, 4160]
    assert max(rows) <= MAX_ROWS
    # slab sums: up to 1 024 slabs of |v| <= 3 plus one extra term
    assert LIMIT * (1024 + 1) < 2 ** 24


def test_tn_slices_is_accepted_by_the_kernel_and_agrees_with_the_library():
    """ops.linear.tn_slices for every M = 32 i, i = 1..400, want = 1..80: the answer is a slice count tn_fill (wgrad_tn.hip)
    accepts -- at most `want`, at most the number of steps, and no slice empty when every slice takes ceil(steps / S) steps -- and
    tn_slices(M, 256 // tiles) is what grit_wgrad_tn_splits (host code of the library) answers for the same shape."""
    from grit_amd.ops.linear import tn_slices
    lib = _L().load()
    shapes = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (4, 4), (8, 2), (8, 8), (16, 16)]  # (N / 256, K / 256): 1 .. 256 tiles
    for i in range(1, 401):
        M = 32 * i
        steps = M // (64 if M % 64 == 0 else 32)
        for want in range(1, 81):
            S = tn_slices(M, want)
            per = _ceil(steps, S)
            assert 1 <= S <= want and S <= steps and _ceil(steps, per) == S, (M, want, S)
        for tn, tk in shapes:
            assert tn_slices(M, 256 // (tn * tk)) == lib.grit_wgrad_tn_splits(M, 256 * tn, 256 * tk), (M, tn, tk)


# ---------------------------------------------------------------------------------------------------------------
# fences
# ---------------------------------------------------------------------------------------------------------------
class _Operand(object):
    """view = rows [FENCE, FENCE + M), columns [pad, pad + W) of a NaN-filled buffer of leading dimension W + 2 pad."""

    def __init__(self, data, pad=0):
        M, W = data.shape
        assert M <= MAX_ROWS and pad % 8 == 0
        self.buf = torch.full((FENCE + M + FENCE, W + 2 * pad), NAN, dtype=data.dtype, device=DEV)
        self.view = self.buf[FENCE:FENCE + M, pad:pad + W]
        self.view.copy_(data)
        self.ld = W + 2 * pad
        assert self.view.data_ptr() % 16 == 0 and self.ld % 8 == 0 and self.view.stride(0) == self.ld

    @property
    def ptr(self):
        return self.view.data_ptr()


class _Out(object):
    """out = slabs [guard, guard + shape[0]) of a NaN-filled buffer with `guard` more slabs on either side."""

    def __init__(self, shape, dtype=F32, guard=1):
        self.guard, self.n = guard, shape[0]
        self.buf = torch.full((shape[0] + 2 * guard,) + tuple(shape[1:]), NAN, dtype=dtype, device=DEV)
        self.out = self.buf[guard:guard + shape[0]]
        assert self.out.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.out.data_ptr()

    def reset(self):
        self.buf.fill_(NAN)

    def untouched(self):
        return _all_nan(self.buf)

    def check(self, ref, what=""):
        """guards still NaN, output finite and exactly the (float64, integer-valued) reference in the output's type"""
        assert _all_nan(self.buf[:self.guard]) and _all_nan(self.buf[self.guard + self.n:]), "guard slab written " + what
        assert bool(torch.isfinite(self.out).all()), "NaN left in / read into the output " + what
        want = ref.to(F32) if self.out.dtype == F32 else ref.to(F32).to(BF16)
        assert want.shape == self.out.shape
        assert torch.equal(self.out, want), "not exact " + what


def _rows(ranges):
    return torch.cat([torch.arange(lo, hi, device=DEV) for lo, hi in ranges]) if ranges else torch.zeros(0, dtype=torch.long, device=DEV)


def _refs(dy, x, slices):
    """float64 [S, N, K] and [S, N]: the contraction and the column sums over each slice's own rows"""
    dw, db = [], []
    for ranges in slices:
        idx = _rows(ranges)
        ys = dy[idx].to(F64)
        dw.append(ys.t() @ x[idx].to(F64))
        db.append(ys.sum(0))
    return torch.stack(dw), torch.stack(db)


def _tn_slices_of(M, S):
    """The fixed row ranges of grit_wgrad_tn / grit_wgrad_tn_grouped (include/grit_hip.h): slice s = rows
    [s ceil(steps / S) g, ...) with g = 64 when M % 64 == 0, else 32; also the steps per slice."""
    g = 64 if M % 64 == 0 else 32
    steps = M // g
    per = _ceil(steps, S)
    slices = [[(s * per * g, min(M, (s + 1) * per * g))] for s in range(S)]
    return slices, tuple((hi - lo) // g for [(lo, hi)] in slices)


class _Problem(object):
    """One weight-gradient problem: integer operands behind fences, fenced fp32 outputs [S, N, K] and (with_db) [S, N].
    drop = sample indices whose rows (rows_per_sample each) are zero in dY; nan_dropped puts NaN into X there."""

    def __init__(self, M, N, K, S, seed, pad_y=0, pad_x=0, with_db=True, drop=(), rows_per_sample=0, nan_dropped=False):
        self.M, self.N, self.K, self.S = M, N, K, S
        self.dy, self.x = _ints((M, N), 2 * seed + 1), _ints((M, K), 2 * seed + 2)
        self.rows_per_sample, self.scale = rows_per_sample, None
        x_in = self.x
        if rows_per_sample:
            self.scale = torch.full((M // rows_per_sample,), 1.25, device=DEV)
            x_in = self.x.clone()
            for b in drop:
                self.scale[b] = 0.0
                self.dy[b * rows_per_sample:(b + 1) * rows_per_sample] = 0
                if nan_dropped:
                    x_in[b * rows_per_sample:(b + 1) * rows_per_sample] = NAN
        self.Y, self.X = _Operand(self.dy, pad_y), _Operand(x_in, pad_x)
        self.part = _Out((S, N, K))
        self.db = _Out((S, N)) if with_db else None
        self._ref = {}

    def job(self, with_db=None, with_rows=True):
        use_db = self.db is not None if with_db is None else with_db
        self.used_db = use_db
        rows = self.scale is not None and with_rows
        return _L().WgradJob(self.Y.ptr, self.Y.ld, self.X.ptr, self.X.ld, self.M, self.N, self.K, self.S, self.part.ptr,
                             self.db.ptr if use_db else None, self.scale.data_ptr() if rows else None,
                             self.rows_per_sample if rows else 0)

    def reset(self):
        self.part.reset()
        if self.db is not None:
            self.db.reset()

    def untouched(self):
        return self.part.untouched() and (self.db is None or self.db.untouched())

    def check(self, slices, what=""):
        key = repr(slices)
        if key not in self._ref:
            self._ref[key] = _refs(self.dy, self.x, slices)
        dw, db = self._ref[key]
        what = "%s (M %d N %d K %d S %d)" % (what, self.M, self.N, self.K, self.S)
        self.part.check(dw, "dW " + what)
        if self.db is not None:
            if self.used_db:
                self.db.check(db, "db " + what)
            else:
                assert self.db.untouched(), "db written though NULL was passed " + what


def _table(jobs):
    return (_L().WgradJob * len(jobs))(*jobs)


def _tn_grouped(structs):
    st = _L().load().grit_wgrad_tn_grouped(_table(structs), len(structs), _L().current_stream_ptr())
    torch.cuda.synchronize()
    return st


# ---------------------------------------------------------------------------------------------------------------
# 1, 2: grit_wgrad_tn_grouped -- the four-wave kernel (every M % 64 == 0) and the eight-wave one (M % 64 == 32)
# ---------------------------------------------------------------------------------------------------------------
def _grouped_table_case(table, N, K, seed):
    probs = []
    for t, (M, S, steps) in enumerate(table):
        slices, got_steps = _tn_slices_of(M, S)
        assert got_steps == steps, (M, S, got_steps)
        probs.append((_Problem(M, N, K, S, seed + t, pad_y=8 * (t % 3), pad_x=8 * ((t + 1) % 3)), slices))
    for parity in (0, 1):  # db_partial set on every other job, then on the others
        for p, _ in probs:
            p.reset()
        assert _tn_grouped([p.job(with_db=(t % 2 == parity)) for t, (p, _) in enumerate(probs)]) == 0
        for p, slices in probs:
            p.check(slices, "parity %d" % parity)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", NK_TN)
def test_tn_grouped_four_wave_small_step_counts(N, K):
    """Nine jobs of 1 .. 10 steps of 64 rows in 1 .. 4 slices (per slice 1, 2, 3 and 10 steps: the prologue that has two steps in
    flight re-fetches the last rows past the end) in one launch; k-tile 0 with and without the bias by-product, the other k-tiles,
    jobs whose first block is no multiple of 8.  Each slice exact over its own rows."""
    _grouped_table_case(FOUR_WAVE, N, K, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", NK_TN)
def test_tn_grouped_eight_wave_small_step_counts(N, K):
    """The same with M % 64 == 32 on every job: the launch runs wgrad_tn_256_grouped with 32-row steps; 1, 2, 3 steps per slice
    (fewer than the four-stage ring), 7 and 13 (the ring wraps)."""
    _grouped_table_case(EIGHT_WAVE, N, K, 200)


@pytest.mark.gpu
def test_tn_grouped_refuses_an_empty_slice():
    """M = 320 is five 64-row steps; four slices of ceil(5 / 4) = 2 steps leave the fourth without a step."""
    p = _Problem(320, 256, 256, 4, 300)
    assert _tn_grouped([p.job()]) != 0
    assert p.untouched()
    q = _Problem(320, 256, 256, 3, 300)
    assert _tn_grouped([q.job()]) == 0
    q.check(_tn_slices_of(320, 3)[0])


@pytest.mark.gpu
def test_tn_grouped_mixed_jobs_block_to_job_mapping():
    """Jobs of 2, 4, 6 and 18 workgroups in orders that put first blocks at 2, 6, 12 and at 18, 24, 28: tn_group_logical must be a
    permutation of each job's (slice, tile) pairs -- a pair taken twice leaves another one NaN.  With the M = 96 job the launch runs
    the eight-wave kernel for all four, without it the four-wave kernel for the other three."""
    spec = [(128, 256, 256, 2), (96, 512, 256, 2), (320, 256, 512, 3), (640, 512, 768, 3)]
    probs = [_Problem(M, N, K, S, 400 + t, pad_y=8 * (t % 2), pad_x=8 * ((t + 1) % 2)) for t, (M, N, K, S) in enumerate(spec)]
    wgs = [(p.N // 256) * (p.K // 256) * p.S for p in probs]
    assert wgs == [2, 4, 6, 18]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1], [0, 2, 3], [3, 2, 0], [2, 0, 3]):
        firsts = [sum(wgs[j] for j in order[:i]) for i in range(len(order))]
        assert any(f % 8 for f in firsts)
        for p in probs:
            p.reset()
        assert _tn_grouped([probs[t].job(with_db=(t + len(order)) % 2 == 0) for t in order]) == 0
        for t in order:
            probs[t].check(_tn_slices_of(probs[t].M, probs[t].S)[0], "order %r first blocks %r" % (order, firsts))
        if 1 not in order:
            assert probs[1].untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [(64, 128, 192), (32, 64, 96)], ids=["four_wave", "eight_wave"])
def test_tn_grouped_job_limit(rows):
    """GRIT_WGRAD_GROUP_MAX = 32 jobs of one workgroup each are exact; a table of 33 is refused and nothing is written."""
    assert _L().WGRAD_GROUP_MAX == 32
    probs = [_Problem(rows[t % 3], 256, 256, 1, 500 + t, with_db=t % 2 == 0) for t in range(33)]
    assert _tn_grouped([p.job() for p in probs]) != 0
    assert all(p.untouched() for p in probs)
    assert _tn_grouped([p.job() for p in probs[:32]]) == 0
    for p in probs[:32]:
        p.check(_tn_slices_of(p.M, 1)[0])
    assert probs[32].untouched()


# ---------------------------------------------------------------------------------------------------------------
# 3: grit_wgrad_tn and grit_wgrad_tn_rows, one problem per launch, the library's own slice count
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,S,steps", [(64, 256, 256, 1, (1,)), (128, 256, 256, 2, (1, 1)), (224, 2048, 2048, 4, (2, 2, 2, 1)),
                                           (2080, 256, 256, 65, (1,) * 65), (4096, 1024, 1024, 16, (4,) * 16)])
def test_tn_single_launch_per_slice(M, N, K, S, steps):
    """One and two steps in all, the eight-wave kernel with a short last slice, 65 one-step slices of 32 rows, 16 slices of four
    64-row steps; fenced operands with padded leading dimensions; through both entry points (no factors)."""
    lib, L = _L().load(), _L()
    assert lib.grit_wgrad_tn_splits(M, N, K) == S
    slices, got = _tn_slices_of(M, S)
    assert got == steps
    p = _Problem(M, N, K, S, 600, pad_y=8, pad_x=16)
    st = lib.grit_wgrad_tn(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, M, N, K, S, p.part.ptr, p.db.ptr, L.current_stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    p.used_db = True
    p.check(slices, "grit_wgrad_tn")
    p.reset()
    st = lib.grit_wgrad_tn_rows(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, M, N, K, S, p.part.ptr, None, None, 0, L.current_stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    p.used_db = False
    p.check(slices, "grit_wgrad_tn_rows without factors")


# ---------------------------------------------------------------------------------------------------------------
# 4: row skipping
# ---------------------------------------------------------------------------------------------------------------
def _launch_rows(p, entry):
    """`entry` "grouped": a one-job grit_wgrad_tn_grouped with the factors in the job; "rows": grit_wgrad_tn_rows."""
    lib, L = _L().load(), _L()
    if entry == "grouped":
        return _tn_grouped([p.job()])
    assert lib.grit_wgrad_tn_splits(p.M, p.N, p.K) == p.S
    st = lib.grit_wgrad_tn_rows(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, p.M, p.N, p.K, p.S, p.part.ptr, p.db.ptr if p.db else None,
                                p.scale.data_ptr(), p.rows_per_sample, L.current_stream_ptr())
    torch.cuda.synchronize()
    p.used_db = p.db is not None
    return st


def _census(B, sps, drop, S, N, K, pad, entry):
    """Ownership of the 64-row steps under skipping, measured: list (per slice) of the step indices it summed; asserts the fair
    share.  X is NaN in the dropped samples, so a slice that loads a dropped step shows."""
    M, steps = B * sps * 64, B * sps
    assert steps <= N
    p = _Problem(M, N, K, S, 0, pad_y=pad, pad_x=pad, drop=drop, rows_per_sample=sps * 64, nan_dropped=True)
    dy = torch.zeros((M, N), dtype=BF16, device=DEV)
    m = torch.arange(M, device=DEV)
    dy[m, m // 64] = 1
    for b in drop:
        dy[b * sps * 64:(b + 1) * sps * 64] = 0
    p.Y.view.copy_(dy)
    x = torch.ones((M, K), dtype=BF16, device=DEV)
    for b in drop:
        x[b * sps * 64:(b + 1) * sps * 64] = NAN
    p.X.view.copy_(x)
    assert _launch_rows(p, entry) == 0
    part, db = p.part.out, p.db.out
    assert p.part.untouched() is False and _all_nan(p.part.buf[:1]) and _all_nan(p.part.buf[-1:])
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(db).all())
    assert bool((part == part[:, :, :1]).all())          # a row n of a slice is one number: 64 x (step n is mine)
    own = part[:, :, 0]
    assert torch.equal(db, own)                          # the column sums count the same rows
    assert bool(((own == 0) | (own == 64)).all()) and bool((own[:, steps:] == 0).all())
    own = (own[:, :steps] == 64).cpu()
    live = [t for t in range(steps) if t // sps not in drop]
    owned = [[t for t in range(steps) if own[s, t]] for s in range(S)]
    owners = own.sum(0).tolist()
    assert [t for t in range(steps) if owners[t] == 1] == live and all(owners[t] == 0 for t in range(steps) if t not in live)
    assert sum(owned, []) == live                        # contiguous runs of the live steps, in slice order
    sizes = [len(o) for o in owned]
    assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 1, sizes
    return owned


_KEEP5, _KEEP1 = (0, 5, 6, 62, 63), (63,)
SKIP_CASES = [
    # B, steps per sample, dropped samples, S, N, K, pad, entry
    (2, 1, (0,), 1, 256, 256, 0, "grouped"),
    (2, 1, (1,), 1, 256, 256, 0, "grouped"),
    (4, 2, (1, 2), 1, 256, 256, 0, "grouped"),   # a two-sample gap inside one slice
    (4, 2, (1, 2), 3, 256, 256, 0, "grouped"),
    (4, 2, (1, 2), 4, 256, 256, 0, "grouped"),   # live == S
    (5, 3, (0, 2, 4), 4, 256, 256, 0, "grouped"),  # 6 live steps over 4 slices: slices begin in the middle of a sample
    (5, 3, (0, 2, 4), 4, 256, 256, 8, "grouped"),  # ... with ldy > N, ldx > K: the gap between samples comes from the leading dimensions
    (5, 3, (1, 3), 2, 256, 256, 0, "grouped"),     # 9 live steps: the second slice begins in the middle of a sample AND crosses a gap
    (64, 1, tuple(b for b in range(64) if b not in _KEEP5), 2, 256, 256, 0, "grouped"),  # bit 63 of the keep mask
    (64, 1, tuple(b for b in range(64) if b not in _KEEP1), 1, 256, 256, 0, "grouped"),
    (4, 2, (1, 2), 3, 256, 512, 0, "grouped"),   # two k-tiles, the bias by-product on k-tile 0 only
    (4, 2, (1, 2), 3, 512, 256, 8, "grouped"),
    (64, 1, tuple(b for b in range(64) if b % 3 == 2), 16, 1024, 1024, 0, "rows"),  # 43 live steps over 16 slices
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,sps,drop,S,N,K,pad,entry", SKIP_CASES)
def test_row_skip_census_and_exact_slices(B, sps, drop, S, N, K, pad, entry):
    """Skipping applies (four-wave kernel, whole 64-row steps per sample, 2..64 samples, some sample dropped, at least S live
    steps): the live steps are shared fairly (census), dropped rows of X -- NaN here -- are never read, and every slice's partial
    and column sums are exact over the steps it owns."""
    live = (B - len(drop)) * sps
    assert S <= live < B * sps
    if entry == "rows":
        assert live == 43
    owned = _census(B, sps, drop, S, N, K, pad, entry)
    slices = [[(64 * t, 64 * t + 64) for t in steps] for steps in owned]
    p = _Problem(B * sps * 64, N, K, S, 700 + B + S, pad_y=pad, pad_x=pad, drop=drop, rows_per_sample=sps * 64, nan_dropped=True)
    assert _launch_rows(p, entry) == 0
    p.check(slices, "skipping")


NO_SKIP_CASES = [
    # B, rows per sample, dropped samples, S (grouped launch)
    (4, 128, (), 3),            # nothing dropped
    (4, 128, (0, 1, 2, 3), 3),  # everything dropped: exact zeros
    (4, 96, (1,), 3),           # rows_per_sample % 64 != 0
    (65, 64, (1, 7), 5),        # more than 64 samples
    (4, 128, (0, 1, 3), 4),     # 2 live steps, 4 slices
]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["grouped", "rows"])
@pytest.mark.parametrize("B,per,drop,S", NO_SKIP_CASES)
def test_row_skip_does_not_apply(B, per, drop, S, entry):
    """Where skipping does not apply the factors change nothing: the slices are the fixed row ranges and the result equals the plain
    launch of the same (finite) operands bit for bit.  That includes FEWER LIVE STEPS THAN SLICES: the kernel then reads every row,
    those of dropped samples too, so X must be finite there -- `never read` (include/grit_hip.h) holds only where skipping applies."""
    lib, L = _L().load(), _L()
    M, N, K = B * per, 256, 256
    if entry == "rows":
        S = lib.grit_wgrad_tn_splits(M, N, K)
    live = (B - len(drop)) * (per // 64)
    applies = per % 64 == 0 and 2 <= B <= 64 and len(drop) > 0 and live >= S
    assert not applies
    slices, _ = _tn_slices_of(M, S)
    p = _Problem(M, N, K, S, 800 + B, pad_y=8, pad_x=8, drop=drop, rows_per_sample=per)
    plain = (_Out((S, N, K)), _Out((S, N)))
    if entry == "grouped":
        twin = L.WgradJob(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, M, N, K, S, plain[0].ptr, plain[1].ptr, None, 0)
        assert _tn_grouped([p.job(), twin]) == 0
    else:
        assert _launch_rows(p, "rows") == 0
        assert lib.grit_wgrad_tn(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, M, N, K, S, plain[0].ptr, plain[1].ptr, L.current_stream_ptr()) == 0
        torch.cuda.synchronize()
    p.check(slices, "factors given, skipping not applicable")
    dw, db = p._ref[repr(slices)]
    plain[0].check(dw, "plain dW")
    plain[1].check(db, "plain db")
    assert torch.equal(p.part.out, plain[0].out) and torch.equal(p.db.out, plain[1].out)
    if len(drop) == B:
        assert int(p.part.out.count_nonzero()) == 0 and int(p.db.out.count_nonzero()) == 0


@pytest.mark.gpu
def test_row_skip_next_to_an_eight_wave_job():
    """A grouped launch with an M % 64 == 32 job runs the eight-wave kernel for every job: the factors of the other job are not used,
    its slices stay the fixed row ranges."""
    a = _Problem(512, 256, 256, 3, 900, drop=(1, 2), rows_per_sample=128)
    b = _Problem(96, 256, 256, 2, 901)
    assert _tn_grouped([a.job(), b.job()]) == 0
    a.check(_tn_slices_of(512, 3)[0])
    b.check(_tn_slices_of(96, 2)[0])


# ---------------------------------------------------------------------------------------------------------------
# 5: grit_wgrad_small, grit_wgrad_small_grouped
# ---------------------------------------------------------------------------------------------------------------
def _small_slices(M, S):
    rows = _ceil(_ceil(M, S), 32) * 32
    assert _ceil(M, rows) == S
    return [[(s * rows, min(M, (s + 1) * rows))] for s in range(S)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(M, N, K) for M in SMALL_M for N, K in SMALL_NK] +
                         [(33, 2048, 2048), (416, 2048, 2048), (417, 2048, 2048)])  # 13 steps in one split; two splits of 7 steps
def test_small_single_launch(M, N, K):
    """Row counts around the 32-row step, the 64-row split and the 13-step register ring (416 rows).  One split: finished bf16
    gradients = the bf16 cast of the exact sums; several: fp32 partials, each exact over its split's rows.  With and without db."""
    lib, L = _L().load(), _L()
    S = lib.grit_wgrad_small_splits(M, N, K)
    assert S >= 1
    if M <= 64 or (N == 2048 and M <= 416):
        assert S == 1
    slices = _small_slices(M, S)
    p = _Problem(M, N, K, S, 1000 + M, pad_y=8, pad_x=16)
    dw, db = _refs(p.dy, p.x, slices)
    dtype = BF16 if S == 1 else F32
    for with_db in (True, False):
        o_w, o_b = _Out((S, N, K), dtype), _Out((S, N), dtype)
        st = lib.grit_wgrad_small(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, M, N, K, S, o_w.ptr, o_b.ptr if with_db else None, L.current_stream_ptr())
        torch.cuda.synchronize()
        assert st == 0
        o_w.check(dw, "dW S %d" % S)
        if with_db:
            o_b.check(db, "db S %d" % S)
        else:
            assert o_b.untouched()
    assert lib.grit_wgrad_small(p.Y.ptr, p.Y.ld, p.X.ptr, p.X.ld, M, N, K, S + 1, o_w.ptr, None, L.current_stream_ptr()) != 0


def _small_grouped(structs):
    st = _L().load().grit_wgrad_small_grouped(_table(structs), len(structs), _L().current_stream_ptr())
    torch.cuda.synchronize()
    return st


@pytest.mark.gpu
def test_small_grouped_launch():
    """27 jobs of different M, N, K and leading dimensions in one launch, db_partial on every other one."""
    lib = _L().load()
    probs = []
    for t, (M, (N, K)) in enumerate((M, nk) for M in SMALL_M for nk in SMALL_NK):
        S = lib.grit_wgrad_group_splits(M)
        assert S == _ceil(M, 416)
        probs.append(_Problem(M, N, K, S, 1100 + t, pad_y=8 * (t % 3), pad_x=8 * ((t + 2) % 3)))
    assert len(probs) == 27
    for parity in (0, 1):
        for p in probs:
            p.reset()
        assert _small_grouped([p.job(with_db=t % 2 == parity) for t, p in enumerate(probs)]) == 0
        for p in probs:
            p.check(_small_slices(p.M, p.S), "parity %d" % parity)


@pytest.mark.gpu
def test_small_grouped_job_limit():
    probs = [_Problem(SMALL_M[t % 6], 64, 64, 1, 1200 + t, with_db=t % 2 == 1) for t in range(33)]
    assert _small_grouped([p.job() for p in probs]) != 0
    assert all(p.untouched() for p in probs)
    assert _small_grouped([p.job() for p in probs[:32]]) == 0
    for p in probs[:32]:
        p.check(_small_slices(p.M, 1))
    assert probs[32].untouched()


# ---------------------------------------------------------------------------------------------------------------
# 6: grit_colsum, grit_colsum_grouped, grit_slab_sum, grit_slab_sum_grouped
# ---------------------------------------------------------------------------------------------------------------
def _colsum_ref(x, M, slabs):
    rows = _ceil(M, slabs)
    return torch.stack([x[min(M, s * rows):min(M, (s + 1) * rows)].to(F64).sum(0) for s in range(slabs)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 13, 16, 17, 29, 32, 33, 45, 61])
def test_colsum_loop_edges(rows, dtype):
    """Rows per slab across the boundaries of a wave's 8-, 4- and 1-row loops (a wave takes every fourth row: 8 rows in flight from
    29 + wave rows on, 4 from 13 + wave); widths of one lane, an almost full strip, a full one and a second strip of one lane; a last
    slab one row short."""
    lib, L = _L().load(), _L()
    for N in (8, 504, 512, 520):
        for M, slabs in ((3 * rows, 3), (max(1, 3 * rows - 1), 3 if rows > 1 else 2)):
            assert _ceil(M, slabs) == rows
            x = _ints((M, N), 1300 + rows + N, dtype=dtype)
            X, out = _Operand(x), _Out((slabs, N))
            st = lib.grit_colsum(X.ptr, M, N, int(dtype == BF16), slabs, out.ptr, L.current_stream_ptr())
            torch.cuda.synchronize()
            assert st == 0
            out.check(_colsum_ref(x, M, slabs), "N %d M %d" % (N, M))


@pytest.mark.gpu
def test_colsum_empty_slabs_and_slab_limit():
    """M smaller than the slab count: the slabs without a row come back as exact zeros (`fully overwritten`); 256 slabs are
    accepted, 257 refused, in both forms."""
    lib, L = _L().load(), _L()
    for M, slabs in ((2, 5), (1, 4), (100, 256)):
        x = _ints((M, 520), 1400 + M)
        X, out = _Operand(x), _Out((slabs, 520))
        assert lib.grit_colsum(X.ptr, M, 520, 1, slabs, out.ptr, L.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        ref = _colsum_ref(x, M, slabs)
        assert int(ref[M:].count_nonzero()) == 0
        out.check(ref)
    assert L.COLSUM_MAX_SLABS == 256
    out.reset()
    assert lib.grit_colsum(X.ptr, 100, 520, 1, 257, out.ptr, L.current_stream_ptr()) != 0
    job = L.ColsumJob(X.ptr, X.ld, 100, 520, 257, out.ptr)
    assert lib.grit_colsum_grouped((L.ColsumJob * 1)(job), 1, L.current_stream_ptr()) != 0
    torch.cuda.synchronize()
    assert out.untouched()
    job = L.ColsumJob(X.ptr, X.ld, 100, 520, 256, out.ptr)
    assert lib.grit_colsum_grouped((L.ColsumJob * 1)(job), 1, L.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    out.check(_colsum_ref(x, 100, 256))


@pytest.mark.gpu
def test_colsum_grouped_padded_jobs_and_job_limit():
    """32 jobs of different M, N, slab counts and leading dimensions (NaN in the padding columns) in one launch; 33 are refused."""
    lib, L = _L().load(), _L()
    assert L.COLSUM_GROUP_MAX == 32
    rows, widths = [1, 3, 4, 5, 13, 16, 17, 29, 32, 33, 45, 61], [8, 504, 512, 520]
    keep = []
    for t in range(33):
        r, N, slabs = rows[t % 12], widths[t % 4], 1 + t % 5
        M = max(1, r * slabs - (t % 2))
        x = _ints((M, N), 1500 + t)
        keep.append((x, _Operand(x, pad=8 * (1 + t % 3)), _Out((slabs, N)), M, N, slabs))
    table = (L.ColsumJob * 33)(*[L.ColsumJob(X.ptr, X.ld, M, N, slabs, out.ptr) for _, X, out, M, N, slabs in keep])
    assert lib.grit_colsum_grouped(table, 33, L.current_stream_ptr()) != 0
    torch.cuda.synchronize()
    assert all(k[2].untouched() for k in keep)
    assert lib.grit_colsum_grouped(table, 32, L.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    for x, _, out, M, N, slabs in keep[:32]:
        out.check(_colsum_ref(x, M, slabs), "M %d N %d slabs %d" % (M, N, slabs))
    assert keep[32][2].untouched()


class _Slabs(object):
    """groups x slabs x n integer partials; group g at g * stride with stride > slabs * n; NaN in the gap and around."""

    def __init__(self, groups, slabs, n, seed, gap=8):
        self.groups, self.slabs, self.n, self.stride = groups, slabs, n, slabs * n + gap
        self.buf = torch.full((64 + groups * self.stride + 64,), NAN, dtype=F32, device=DEV)
        self.view = self.buf[64:64 + groups * self.stride].view(groups, self.stride)[:, :slabs * n]
        self.data = _ints((groups, slabs, n), seed, dtype=F32)
        self.view.copy_(self.data.view(groups, slabs * n))
        self.extra = _ints((groups, n), seed + 1, dtype=F32)
        self.ref = self.data.to(F64).sum(1)
        self.ref_extra = self.ref + self.extra.to(F64)
        assert self.view.data_ptr() % 16 == 0 and self.stride % 4 == 0 and self.extra.data_ptr() % 16 == 0

    def job(self, out, bf16, extra):
        return _L().SlabJob(self.view.data_ptr(), self.stride, self.groups, self.slabs, self.n, out.ptr, int(bf16),
                            self.extra.data_ptr() if extra else None)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 252, 260, 65536, 65540])
@pytest.mark.parametrize("slabs", [1, 7, 8, 9, 15, 16, 17])
def test_slab_sum_paths(slabs, n):
    """The wide shape (n >= 65 536: a thread walks all slabs, eight in flight; at 65 540 the last workgroup holds one column group)
    and the narrow one (one, 63 and 65 column groups) around the 8- and 4-slab loop boundaries; three groups with NaN between them;
    fp32 and bf16 outputs; the grouped form with and without `extra`."""
    lib, L = _L().load(), _L()
    src = _Slabs(3, slabs, n, 1600 + slabs)
    for bf16 in (False, True):
        out = _Out((3, n), BF16 if bf16 else F32, guard=2)
        st = lib.grit_slab_sum(src.view.data_ptr(), 3, src.stride, slabs, n, out.ptr, int(bf16), L.current_stream_ptr())
        torch.cuda.synchronize()
        assert st == 0
        out.check(src.ref, "single bf16=%d" % bf16)
    combos = [(False, True), (True, False), (False, False), (True, True)]
    outs = [_Out((3, n), BF16 if bf16 else F32, guard=2) for bf16, _ in combos]
    table = (L.SlabJob * 4)(*[src.job(o, bf16, extra) for o, (bf16, extra) in zip(outs, combos)])
    assert lib.grit_slab_sum_grouped(table, 4, L.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    for o, (bf16, extra) in zip(outs, combos):
        o.check(src.ref_extra if extra else src.ref, "grouped bf16=%d extra=%d" % (bf16, extra))


@pytest.mark.gpu
def test_slab_sum_narrowed_for_tall_partials():
    """1 024 slabs of 512 columns (the LayerNorm partials): the column width is narrowed to 8 column groups and 32 slab lanes."""
    lib, L = _L().load(), _L()
    src = _Slabs(3, 1024, 512, 1700)
    for bf16 in (False, True):
        out, gout = _Out((3, 512), BF16 if bf16 else F32, guard=2), _Out((3, 512), BF16 if bf16 else F32, guard=2)
        assert lib.grit_slab_sum(src.view.data_ptr(), 3, src.stride, 1024, 512, out.ptr, int(bf16), L.current_stream_ptr()) == 0
        assert lib.grit_slab_sum_grouped((L.SlabJob * 1)(src.job(gout, bf16, True)), 1, L.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        out.check(src.ref)
        gout.check(src.ref_extra)


@pytest.mark.gpu
def test_slab_sum_grouped_output_alignment():
    """Grouped form: a bf16 output on an 8-byte boundary that is no 16-byte boundary is accepted (and exact, its neighbours
    untouched); an fp32 output there is refused."""
    lib, L = _L().load(), _L()
    for n in (252, 65540):
        src = _Slabs(3, 9, n, 1800)
        buf = torch.full((8 + 3 * n + 8,), NAN, dtype=BF16, device=DEV)
        out = buf[4:4 + 3 * n]
        assert out.data_ptr() % 16 == 8
        job = L.SlabJob(src.view.data_ptr(), src.stride, 3, 9, n, out.data_ptr(), 1, None)
        assert lib.grit_slab_sum_grouped((L.SlabJob * 1)(job), 1, L.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        assert _all_nan(buf[:4]) and _all_nan(buf[4 + 3 * n:])
        assert torch.equal(out.view(3, n), src.ref.to(F32).to(BF16))
        fbuf = torch.full((4 + 3 * n + 4,), NAN, dtype=F32, device=DEV)
        fout = fbuf[2:2 + 3 * n]
        assert fout.data_ptr() % 16 == 8
        job = L.SlabJob(src.view.data_ptr(), src.stride, 3, 9, n, fout.data_ptr(), 0, None)
        assert lib.grit_slab_sum_grouped((L.SlabJob * 1)(job), 1, L.current_stream_ptr()) != 0
        torch.cuda.synchronize()
        assert _all_nan(fbuf)


# ---------------------------------------------------------------------------------------------------------------
# 7: grit_transpose_bf16_grouped
# ---------------------------------------------------------------------------------------------------------------
CANARY = 0x7FE5


def _transpose_case(rows, cols, start):
    """src: consecutive 16-bit patterns (every element of a matrix differs from every other); dst between canaries"""
    src = ((torch.arange(rows * cols, dtype=torch.int32, device=DEV) + start) & 0xFFFF).to(torch.int16).view(rows, cols)
    buf = torch.full((64 + rows * cols + 64,), CANARY, dtype=torch.int16, device=DEV)
    return src, buf, buf[64:64 + rows * cols].view(cols, rows)


def _transpose_run(cases):
    L = _L()
    table = (L.TransposeJob * len(cases))(*[L.TransposeJob(s.data_ptr(), d.data_ptr(), s.shape[0], s.shape[1]) for s, _, d in cases])
    st = L.load().grit_transpose_bf16_grouped(table, len(cases), L.current_stream_ptr())
    torch.cuda.synchronize()
    return st


@pytest.mark.gpu
def test_transpose_grouped_bit_patterns_between_canaries():
    assert 192 * 320 <= 65536
    cases = [_transpose_case(r, c, 7 * t) for t, (r, c) in enumerate([(64, 64), (64, 128), (128, 64), (192, 320)])]
    for order in (cases, cases[::-1]):
        for _, buf, _ in cases:
            buf.fill_(CANARY)
        assert _transpose_run(order) == 0
        for src, buf, dst in cases:
            assert torch.equal(dst, src.t())
            assert bool((buf[:64] == CANARY).all()) and bool((buf[-64:] == CANARY).all())


@pytest.mark.gpu
def test_transpose_grouped_limits():
    """32 jobs are accepted and exact, 33 refused; rows or columns that are no multiple of 64 are refused; nothing is written then."""
    assert _L().TRANSPOSE_GROUP_MAX == 32
    shapes = [(64, 64), (64, 128), (128, 64)]
    cases = [_transpose_case(*shapes[t % 3], start=11 * t) for t in range(33)]
    assert _transpose_run(cases) != 0
    assert all(bool((buf == CANARY).all()) for _, buf, _ in cases)
    assert _transpose_run(cases[:32]) == 0
    for src, buf, dst in cases[:32]:
        assert torch.equal(dst, src.t()) and bool((buf[:64] == CANARY).all()) and bool((buf[-64:] == CANARY).all())
    assert bool((cases[32][1] == CANARY).all())
    for rows, cols in ((96, 64), (64, 96), (32, 64)):
        bad = _transpose_case(rows, cols, 0)
        assert _transpose_run([bad]) != 0
        assert bool((bad[1] == CANARY).all())
