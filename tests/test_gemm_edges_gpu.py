"""Forward / input-gradient GEMM family (grit_gemm_bf16_nt, _res, _relu, _rows; gemm.hip, gemm_w4.hip, ops/gemm.py) at the places
the workload-sized shapes of test_gemm_gpu.py do not reach: leading dimensions larger than the width on every operand at once,
bases inside an allocation, guard rows and columns around every output, every tile edge of every variant at the smallest shapes,
the smallest legal K (one step against a 3- or 4-slot ring), several tiles per workgroup with one or two K steps each in the
persistent kernels, the drop-path skip at eight and nine row panels, the locality of a non-finite operand, and every refusal.

Every reference is float64 (torch, on the device) on the same bf16-rounded inputs.

EXACT inputs (A in {-1, 0, 1}, B integers in [-2, 2], bias in [-8, 8]): every product and partial sum is an integer fp32 holds
exactly and the result stays within |.| <= 256 (asserted on the reference: a condition on the inputs, ten standard deviations
away at K <= 1 024), so the bf16 output is exact too: NONE / BIAS / BIAS_RES are compared with torch.equal -- a swapped row, column
or k chunk, a dropped step or a row counted twice cannot hide.  GELU' with aux = +16 everywhere: s = rcp(1 + exp2(-large)) = 1, the
derivative s * fma(x q, 1 - s, 1) is exactly 1 (confirmed on the device by test_gelu_derivative_at_16_is_exactly_one), so C is the
plain product and every column-sum slab an exact integer sum over the rows that slab owns.

RANDOM inputs (randn, weights times K^-1/2), per element:   |got - ref| <= U |ref| + 2 K 2^-24 S,   S = |x| |w|^T (+ |b|)
  * U |ref|: the one bf16 rounding.  U = 2^-8: bf16 carries 8 significant bits, so round-to-nearest errs by up to half a spacing
    2^(e-8) of a value in [2^e, 2^(e+1)), i.e. 2^-8 relative (1 + 2^-8 rounds to 1).  The issue text asked for 2^-9 here; that is
    half the format's unit roundoff and a correctly rounding kernel exceeds it (worst err / bound of the linear group below is 0.99
    with 2^-8, i.e. ~2 with 2^-9).  Only this term (and the same rounding where it re-appears below) was changed.
  * 2 K 2^-24 S: the standard fp32 accumulation bound, times 2 because MFMA's internal summation order is not specified.
  * BIAS_GELU adds the fit error (3e-5, as test_fused_gelu_epilogues_against_erf_gelu_over_the_whole_range), |GELU'| <= 1.13 times the
    pre-activation's own error and, for variants 7 / 9, 1.13 U |pre| for the bf16-rounded pre-activation they start from.  Where aux is
    kept the activation is checked against GELU of the STORED pre-activation: for variants 7 / 9 that drops both extra terms (they
    compute GELU of exactly that value); the eight-wave variants compute GELU of the unrounded fp32 sum, which differs from the stored
    value by its rounding, so there the term 1.13 U |pre| stays (it moves from the four-wave kernels to the eight-wave ones).
  * GELU' (C = acc * gelu'(aux)): U |ref| + 1.13 x (accumulation bound) + 1.5e-4 |acc| (fit error of the derivative) and, variants
    7 / 9, 1.13 U |acc| for the bf16-rounded gradient; column sums: the sum of the per-element bounds without the final rounding
    (sums are taken before it) + rows x 2^-24 x sum |ref| for the fp32 summation.
  * BIAS_RES with real factors f: U |ref| + f (U |branch| + accumulation bound) + 2^-22 (|residual| + f |branch|).

Worst observed err / bound per group on an MI355X (fence / tile-edge / short-stream shapes; test_zz_report prints a run's figures):
  linear (NONE, BIAS)            0.987 / 0.993 / --       kept pre-activation        0.986 / 0.993 / 0.995
  GELU of the stored pre         0.964 / 0.964 / 0.964    GELU without aux           0.984 / 0.986 / 0.993
  GELU'                          0.974 / 0.978 / 0.985    GELU' column sums          0.288 / 0.880 / 0.395
  residual with real factors     0.989
(the values next to 1 are the bf16 rounding itself: half a spacing just above a power of two.)  GELU'(16) is exactly 1 there.

Guards: every output (and every operand) is a view [r0 : r0 + M, c0 : c0 + width] of a larger buffer pre-filled with a NaN bit
pattern that no kernel produces; at least one tile height of guard rows lies below, so a missing row test is seen in the guards
instead of landing in the allocator's slack.  After each call every guard element still holds its fill, bit for bit."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -8             # unit roundoff of bf16 (8 significant bits)
FIT, DFIT = 3e-5, 1.5e-4  # sigmoid-form GELU against erf GELU, value and derivative (gemm_math.h: 2.6e-5 / 1.1e-4 + margin of the existing test)
DG = 1.13                 # max |GELU'|
NAN16, NAN32 = 0x7FE5, 0x7FC00A5A  # quiet NaNs with a payload: not what an arithmetic instruction writes
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
# variant -> (BM, BN, BK, ring slots, wave tile height); 9: the 224-row form (asserted where it runs)
TILES = {1: (256, 128, 32, 3, 128), 2: (256, 128, 64, 2, 128), 3: (256, 128, 32, 4, 128), 4: (256, 256, 64, 2, 128),
         5: (256, 256, 32, 4, 128), 10: (64, 128, 64, 3, 32), 11: (128, 128, 64, 2, 64), 12: (64, 64, 64, 3, 16),
         13: (64, 128, 32, 4, 32), 7: (256, 256, 64, 2, 128), 9: (224, 256, 64, 2, 112)}
VARIANTS = sorted(TILES)
# extra elements per row of each operand (leading dimension = width + extra); colliding strides are moved apart by _extras
LAYOUTS = ({"A": 8, "B": 72, "C": 8, "aux": 72, "res": 136}, {"A": 72, "B": 8, "C": 72, "aux": 8, "res": 24})
_WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _at_most_16_reference_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _G():
    from grit_amd.ops import gemm as G
    return G


def _lib():
    from grit_amd import lib
    return lib.load()


def _stream():
    from grit_amd import lib
    return lib.current_stream_ptr()


def _p(t, byte_off=0):
    return ctypes.c_void_p(t.data_ptr() + byte_off) if t is not None else None


# ---------------------------------------------------------------------------------------------------------------
# fences, inputs, references
# ---------------------------------------------------------------------------------------------------------------
class _Fence(object):
    """view = buf[above : above + rows, c0 : c0 + width] of a buffer filled with a NaN bit pattern; leading dimension width + extra.
    c0 is a multiple of 8 that is no multiple of 64 (0 only for extra == 0: guard rows alone); with extra == 8 the right-hand guard of
    a row is the left-hand guard of the next one."""

    def __init__(self, rows, width, extra=0, dtype=BF16, above=8, below=264):
        self.bits = torch.int16 if dtype == BF16 else torch.int32
        self.fill = NAN16 if dtype == BF16 else NAN32
        self.c0 = 0 if extra == 0 else (8 if extra <= 40 else 40)
        assert self.c0 % 8 == 0 and (extra == 0 or self.c0 % 64) and self.c0 <= extra and extra % 8 == 0
        self.buf = torch.empty((above + rows + below, width + extra), dtype=dtype, device=DEV)
        self.buf.view(self.bits).fill_(self.fill)
        self.r0, self.rows, self.width = above, rows, width
        self.view = self.buf[above:above + rows, self.c0:self.c0 + width]

    def guards_intact(self):
        b = self.buf.view(self.bits).clone()
        b[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.width] = self.fill
        return bool((b == self.fill).all())

    def untouched(self):
        return bool((self.buf.view(self.bits) == self.fill).all())


def _place(t, extra):
    """`t` ([rows, width] or [width]) copied into a fenced view with leading dimension width + extra."""
    t2 = t if t.dim() == 2 else t.unsqueeze(0)
    f = _Fence(t2.shape[0], t2.shape[1], extra, dtype=t.dtype, below=8)
    f.view.copy_(t2)
    return f.view if t.dim() == 2 else f.view[0]


def _extras(lay, N, K):
    if lay is None:
        return dict.fromkeys(("A", "B", "C", "aux", "res"), 0)
    e, width, seen = dict(LAYOUTS[lay]), {"A": K, "B": K, "C": N, "aux": N, "res": N}, set()
    for k in ("A", "B", "C", "aux", "res"):
        while width[k] + e[k] in seen:
            e[k] += 16
        seen.add(width[k] + e[k])
    assert len(seen) == 5
    return e


def _exact_inputs(M, N, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed * 7919 + M * 31 + N + K)
    nz = torch.rand(M, K, device=DEV, generator=g) < 0.25
    sign = torch.randint(0, 2, (M, K), device=DEV, generator=g) * 2 - 1
    a = (nz * sign).to(BF16)
    b = torch.randint(-2, 3, (N, K), device=DEV, generator=g).to(BF16)
    bias = torch.randint(-8, 9, (N,), device=DEV, generator=g).to(BF16)
    return a, b, bias


def _random_inputs(M, N, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed * 104729 + M * 31 + N + K)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, device=DEV, generator=g).bfloat16()
    return x, w, b


def _products(a, b):
    a64, b64 = a.double(), b.double()
    return a64 @ b64.t(), a64.abs() @ b64.abs().t()


def _dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _check(group, got, ref, bound):
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    _WORST[group] = max(_WORST.get(group, 0.0), ratio) if ratio == ratio else float("nan")
    print("%s: err / bound = %.4f" % (group, ratio))
    assert ratio <= 1.0, (group, ratio)


def _height(variant, M, N):
    """Tile height of the four-wave kernel for a shape (None for the other variants)."""
    if variant == 7:
        return 256
    return _G().w4_tile_rows(M, N) if variant == 9 else None


def _slab_ranges(variant, M, height=None):
    """Rows [lo, hi) that each row of the GELU' column sums owns."""
    if variant in (7, 9):
        H, out = height, []
        for tm in range(-(-M // H)):
            m_tile = tm * H
            m0 = min(m_tile, M - H)  # the last tile is shifted back to end at row M; the rows it shares are its neighbour's
            for wm in (0, 1):
                lo, hi = max(m0 + wm * (H // 2), m_tile), m0 + (wm + 1) * (H // 2)
                out.append((lo, max(lo, hi)))
        return out
    return [(s * 128, min(s * 128 + 128, M)) for s in range(-(-M // 128))]


def _slab_matrix(ranges, M):
    own = torch.zeros((len(ranges), M), dtype=torch.float64, device=DEV)
    for s, (lo, hi) in enumerate(ranges):
        own[s, lo:hi] = 1.0
    return own


_DGELU16 = []


def _dgelu16_exact():
    """GELU'(16) == 1.0f on the device, through an identity GEMM on each of the three kernels (dgelu2, dgelu_f, the four-wave epilogue)."""
    if not _DGELU16:
        G, N, ok = _G(), 256, True
        ones, eye = torch.ones(256, N, device=DEV, dtype=BF16), torch.eye(N, device=DEV, dtype=BF16)
        aux = torch.full((256, N), 16.0, device=DEV, dtype=BF16)
        for v in (1, 5, 7):
            part = torch.empty((2, N), device=DEV)
            d = G.gemm_nt(ones, eye, G.DGELU, aux=aux, colsum=part, variant=v)
            ok = ok and bool((d.float() == 1.0).all()) and bool((part == 128.0).all())  # (ones . I = ones; 128 rows per slab)
        _DGELU16.append(ok)
    return _DGELU16[0]


def _run_nt(variant, epi, a, b, e, bias=None, aux=None, keep_aux=False, slabs=0):
    """One grit_gemm_bf16_nt call through the plain wrapper with fenced outputs -> (C, aux-out or None, colsum or None) fences."""
    G = _G()
    M, N = a.shape[0], b.shape[0]
    c = _Fence(M, N, e["C"])
    auxf = _Fence(M, N, e["aux"]) if (epi == G.BIAS_GELU and keep_aux) else None
    cs = _Fence(slabs, N, 0, dtype=F32, below=8) if epi == G.DGELU else None
    G.gemm_nt(a, b, epi, bias=bias, aux=auxf.view if auxf is not None else aux, colsum=cs.view if cs is not None else None,
              out=c.view, variant=variant)
    return c, auxf, cs


def _exact_checks(variant, M, N, K, lay, seed, dgelu=True):
    """NONE, BIAS and GELU' (aux = +16) on exact inputs: torch.equal against float64, guards intact."""
    G = _G()
    a, b, bias = _exact_inputs(M, N, K, seed)
    prod, _ = _products(a, b)
    with_bias = prod + bias.double()
    assert float(prod.abs().max()) <= 256 and float(with_bias.abs().max()) <= 256  # (condition on the inputs: see the module docstring)
    e = _extras(lay, N, K)
    av, bv, biasv = _place(a, e["A"]), _place(b, e["B"]), _place(bias, 8)
    c, _, _ = _run_nt(variant, G.NONE, av, bv, e)
    assert torch.equal(c.view.double(), prod), (variant, M, N, K, "NONE")
    assert c.guards_intact(), (variant, M, N, K, "NONE guards")
    c, _, _ = _run_nt(variant, G.BIAS, av, bv, e, bias=biasv)
    assert torch.equal(c.view.double(), with_bias), (variant, M, N, K, "BIAS")
    assert c.guards_intact(), (variant, M, N, K, "BIAS guards")
    if variant >= 10 or not dgelu:
        return
    ranges = _slab_ranges(variant, M, _height(variant, M, N))
    aux16 = _place(torch.full((M, N), 16.0, device=DEV, dtype=BF16), e["aux"])
    c, _, cs = _run_nt(variant, G.DGELU, av, bv, e, aux=aux16, slabs=len(ranges))
    sums = _slab_matrix(ranges, M) @ prod
    if _dgelu16_exact():
        assert torch.equal(c.view.double(), prod), (variant, M, N, K, "DGELU")
        assert torch.equal(cs.view.double(), sums), (variant, M, N, K, "DGELU column sums")
    else:  # (not taken on gfx950: kept so that a different rcp / exp2 still has a test, under the random-input bound)
        elem = (DFIT + (DG * U if variant in (7, 9) else 0.0)) * prod.abs()
        _check("dgelu16", c.view, prod, U * prod.abs() + elem)
        _check("dgelu16_colsum", cs.view, sums, _slab_matrix(ranges, M) @ (elem + 2.0 ** -17 * prod.abs()) + 1e-30)
    assert c.guards_intact() and cs.guards_intact(), (variant, M, N, K, "DGELU guards")


def _random_checks(variant, M, N, K, lay, seed, linear=False, tag=""):
    """BIAS_GELU with and without the kept pre-activation and GELU' on random inputs under the bounds of the module docstring
    (linear: also one NONE / BIAS pass)."""
    G = _G()
    w4 = variant in (7, 9)
    x, w, bias = _random_inputs(M, N, K, seed)
    prod, S = _products(x, w)
    pre = prod + bias.double()
    acc_nb = 2.0 * K * 2.0 ** -24 * S
    acc_b = 2.0 * K * 2.0 ** -24 * (S + bias.double().abs())
    e = _extras(lay, N, K)
    xv, wv, biasv = _place(x, e["A"]), _place(w, e["B"]), _place(bias, 8)
    if linear:
        c, _, _ = _run_nt(variant, G.NONE, xv, wv, e)
        _check("linear" + tag, c.view, prod, U * prod.abs() + acc_nb)
        assert c.guards_intact()
        c, _, _ = _run_nt(variant, G.BIAS, xv, wv, e, bias=biasv)
        _check("linear" + tag, c.view, pre, U * pre.abs() + acc_b)
        assert c.guards_intact()
    c, auxf, _ = _run_nt(variant, G.BIAS_GELU, xv, wv, e, bias=biasv, keep_aux=True)
    _check("gelu_pre" + tag, auxf.view, pre, U * pre.abs() + acc_b)
    stored = auxf.view.double()
    ref = F.gelu(stored)
    _check("gelu_of_stored_pre" + tag, c.view, ref, U * ref.abs() + FIT + (0.0 if w4 else DG * U * stored.abs()))
    assert c.guards_intact() and auxf.guards_intact(), (variant, M, N, K, "BIAS_GELU guards")
    c, _, _ = _run_nt(variant, G.BIAS_GELU, xv, wv, e, bias=biasv)
    ref = F.gelu(pre)
    _check("gelu_no_aux" + tag, c.view, ref, U * ref.abs() + FIT + DG * acc_b + (DG * U * pre.abs() if w4 else 0.0))
    assert c.guards_intact(), (variant, M, N, K, "BIAS_GELU (no aux) guards")
    if variant >= 10:
        return
    g = torch.Generator(device=DEV).manual_seed(seed + M + N)
    aux = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    ranges = _slab_ranges(variant, M, _height(variant, M, N))
    c, _, cs = _run_nt(variant, G.DGELU, xv, wv, e, aux=_place(aux, e["aux"]), slabs=len(ranges))
    ref = prod * _dgelu64(aux.double())
    elem = DG * acc_nb + DFIT * prod.abs() + (DG * U * prod.abs() if w4 else 0.0)
    _check("dgelu" + tag, c.view, ref, U * ref.abs() + elem)
    own = _slab_matrix(ranges, M)
    _check("dgelu_colsum" + tag, cs.view, own @ ref, own @ (elem + 2.0 ** -23 * ref.abs()) + 128 * 2.0 ** -24 * (own @ ref.abs()) + 1e-30)
    assert c.guards_intact() and cs.guards_intact(), (variant, M, N, K, "DGELU guards")


# ---------------------------------------------------------------------------------------------------------------
# 7. rejections (cheapest first: a fault further down ends the run)
# ---------------------------------------------------------------------------------------------------------------
def _filled(shape, dtype=BF16):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16 if dtype == BF16 else torch.int32).fill_(NAN16 if dtype == BF16 else NAN32)
    return t


def _is_untouched(t):
    return bool((t.view(torch.int16 if t.dtype == BF16 else torch.int32) == (NAN16 if t.dtype == BF16 else NAN32)).all())


class _Args(object):
    """Operands large enough for every call of the rejection tests (M <= 512, N <= 384, K <= 128), outputs filled with the NaN pattern."""

    def __init__(self):
        g = torch.Generator(device=DEV).manual_seed(1)
        self.a = torch.randn(520, 160, device=DEV, generator=g).bfloat16()
        self.b = torch.randn(392, 160, device=DEV, generator=g).bfloat16()
        self.bias = torch.randn(400, device=DEV, generator=g).bfloat16()
        self.aux_in = torch.randn(520, 400, device=DEV, generator=g).bfloat16()
        self.c, self.aux_out, self.colsum = _filled((520, 400)), _filled((520, 400)), _filled((16, 400), F32)
        self.scale = torch.ones(8, device=DEV)
        self.seed = torch.tensor([1234567], dtype=torch.int64, device=DEV)

    def clean(self):
        return _is_untouched(self.c) and _is_untouched(self.aux_out) and _is_untouched(self.colsum)


def _nt(r, M=300, N=256, K=128, epi=None, variant=1, lda=160, ldb=160, ldc=400, ldaux=400, off=()):
    """grit_gemm_bf16_nt on the operands of `r`; off: names of pointers moved 8 bytes off their 16-byte alignment."""
    G = _G()
    epi = G.NONE if epi is None else epi
    o = lambda name: 8 if name in off else 0  # noqa: E731
    aux = r.aux_in if epi == G.DGELU else (r.aux_out if epi == G.BIAS_GELU else None)
    return _lib().grit_gemm_bf16_nt(_p(r.a, o("A")), lda, _p(r.b, o("B")), ldb, _p(r.c, o("C")), ldc, M, N, K, epi,
                                    _p(r.bias, o("bias")) if epi in (G.BIAS, G.BIAS_GELU) else None, _p(aux, o("aux")), ldaux,
                                    _p(r.colsum) if epi == G.DGELU else None, variant, _stream())


def test_rejected_leading_dimensions_alignment_shapes_and_variants():
    """grit_gemm_bf16_nt: every refused call returns its code and writes nothing -- a leading dimension that is no multiple of 8, a
    base 8 bytes off 16-byte alignment, the shape limits of each tile configuration, GELU' on the short-map tiles, an unknown variant."""
    G = _G()
    r = _Args()
    assert _nt(r) == OK and not _is_untouched(r.c)  # (the base call of this list is a legal one)
    r = _Args()
    for kw in ({"lda": 164}, {"ldb": 164}, {"ldc": 404}, {"ldaux": 404, "epi": G.BIAS_GELU}, {"ldaux": 404, "epi": G.DGELU}):
        assert _nt(r, **kw) == UNSUPPORTED, kw
    for name in ("A", "B", "C", "aux", "bias"):
        assert _nt(r, epi=G.BIAS_GELU, off=(name,)) == UNSUPPORTED, name
    assert _nt(r, epi=G.DGELU, off=("aux",)) == UNSUPPORTED
    for v in (7, 9):
        for kw in ({"M": 255}, {"K": 96}, {"N": 384}):
            assert _nt(r, variant=v, **kw) == UNSUPPORTED, (v, kw)
    for v in (4, 5):
        assert _nt(r, variant=v, N=384) == UNSUPPORTED, v
    for v in (2, 4, 10, 11, 12):
        assert _nt(r, variant=v, K=96) == UNSUPPORTED, v
    for v in (10, 11, 12, 13):
        assert _nt(r, variant=v, epi=G.DGELU) == UNSUPPORTED, v
    for v in (6, 8, 14, -1):
        assert _nt(r, variant=v) == BAD_ARG, v
    assert _nt(r, N=96) == UNSUPPORTED and _nt(r, K=48) == UNSUPPORTED
    torch.cuda.synchronize()
    assert r.clean()


def test_rejected_relu_residual_and_row_skip_calls():
    """grit_gemm_bf16_nt_relu / _res / _rows: the refusals of their own contracts, nothing written."""
    from grit_amd import lib as L
    G = _G()
    lib, r = _lib(), _Args()
    M, N, K = 200, 128, 64

    def relu(epi, N=N, ldc=N, p=0.1, seed=True, ldaux=400, lda=160, off=()):
        o = lambda name: 8 if name in off else 0  # noqa: E731
        return lib.grit_gemm_bf16_nt_relu(_p(r.a, o("A")), lda, _p(r.b), 160, _p(r.c, o("C")), ldc, M, N, K, epi, _p(r.bias),
                                          _p(r.aux_in, o("aux")) if epi == G.DRELU else None, ldaux, p, _p(r.seed) if seed else None, _stream())
    assert relu(G.BIAS_RELU_DROP, ldc=N + 8) == UNSUPPORTED       # the dropout hash runs over m * N + n
    assert relu(G.BIAS_RELU_DROP, N=96, ldc=96) == UNSUPPORTED
    assert relu(G.DRELU, N=96) == UNSUPPORTED
    assert relu(G.BIAS_RELU_DROP, seed=False) == BAD_ARG
    assert relu(G.BIAS_RELU_DROP, p=1.0) == BAD_ARG and relu(G.DRELU, p=1.0) == BAD_ARG
    assert relu(G.DRELU, ldaux=404) == UNSUPPORTED and relu(G.DRELU, lda=164) == UNSUPPORTED and relu(G.DRELU, ldc=132) == UNSUPPORTED
    assert relu(G.DRELU, off=("aux",)) == UNSUPPORTED and relu(G.DRELU, off=("C",)) == UNSUPPORTED and relu(G.DRELU, off=("A",)) == UNSUPPORTED
    assert relu(G.NONE) == BAD_ARG

    def res(M=512, N=256, K=64, per=256, scale=True, ldres=400, ldc=400, off=()):
        o = lambda name: 8 if name in off else 0  # noqa: E731
        return lib.grit_gemm_bf16_nt_res(_p(r.a), 160, _p(r.b), 160, _p(r.c, o("C")), ldc, M, N, K, _p(r.bias, o("bias")),
                                         _p(r.aux_in, o("res")), ldres, _p(r.scale) if scale else None, per, _stream())
    for kw in ({"N": 256, "K": 64}, {"N": 128, "K": 32}):  # the four-wave kernel / the 256 x 128 per-tile kernel
        assert res(ldres=404, **kw) == UNSUPPORTED and res(ldc=404, **kw) == UNSUPPORTED
        assert res(off=("res",), **kw) == UNSUPPORTED and res(off=("C",), **kw) == UNSUPPORTED and res(off=("bias",), **kw) == UNSUPPORTED
        assert res(per=0, **kw) == BAD_ARG
    assert res(per=128) == UNSUPPORTED    # a sample shorter than the tile on the four-wave path: a tile would span three samples
    assert res(per=223) == UNSUPPORTED
    assert res(M=255, scale=False) == UNSUPPORTED
    assert res(N=192, scale=False) == UNSUPPORTED and res(K=48, scale=False) == UNSUPPORTED

    def rows(epi, variant=0, per=256, scale=True):
        return lib.grit_gemm_bf16_nt_rows(_p(r.a), 160, _p(r.b), 160, _p(r.c), 400, 512, 256, 64, epi, _p(r.bias),
                                          _p(r.aux_in if epi == G.DGELU else r.aux_out), 400, _p(r.colsum), _p(r.scale) if scale else None,
                                          per, variant, _stream())
    for v in (5, 7, 9, 10):
        assert rows(G.DGELU, variant=v) == BAD_ARG, v
    assert rows(G.NONE) == BAD_ARG and rows(G.BIAS) == BAD_ARG and rows(L.GEMM_BIAS_RES) == BAD_ARG
    assert rows(G.NONE, scale=False) == BAD_ARG
    assert rows(G.DGELU, per=0) == BAD_ARG
    torch.cuda.synchronize()
    assert r.clean()


def test_residual_output_must_not_alias_the_residual():
    """ops.gemm.gemm_nt_residual(out=...): the four-wave kernel stores the rows of its shifted last tile twice, so `out` sharing
    storage with `residual` would add the branch twice there -- refused before any launch."""
    G = _G()
    a, b, bias = _exact_inputs(300, 256, 64, 3)
    buf = torch.zeros(600, 256, device=DEV, dtype=BF16)
    res = buf[:300]
    with pytest.raises(ValueError):
        G.gemm_nt_residual(a, b, bias, res, out=res)
    with pytest.raises(ValueError):
        G.gemm_nt_residual(a, b, bias, res, out=buf[300:])
    assert float(buf.abs().max()) == 0.0
    out = G.gemm_nt_residual(a, b, bias, res, out=torch.empty_like(res))
    assert torch.equal(out.double(), _products(a, b)[0] + bias.double())


def test_gelu_derivative_at_16_is_exactly_one():
    """What the exact GELU' checks of this module rest on: s = rcp(1 + exp2(-large)) = 1 and s * fma(x q, 1 - s, 1) = 1 at x = 16."""
    assert _dgelu16_exact()


# ---------------------------------------------------------------------------------------------------------------
# 3. leading dimensions and fences together
# ---------------------------------------------------------------------------------------------------------------
def _fence_rows(variant):
    BM = TILES[variant][0]
    return {7: (300, 512), 9: (300, 448)}.get(variant, (BM + 17, 2 * BM))  # one ragged M, one full-tile M (more than one tile each)


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_strided_operands_inside_fences(variant, lay):
    """Every variant with A, B, C, aux on four different leading dimensions (width + 8 / + 72 among them) and bases inside their
    allocations: NONE, BIAS and GELU' (aux = +16) bit for bit against float64, BIAS_GELU with and without aux and GELU' on random
    inputs under the bound, every guard element untouched."""
    BM, BN, BK, slots, _ = TILES[variant]
    for M in _fence_rows(variant):
        N, K = 2 * BN, 3 * BK if BK == 32 else 2 * BK
        if variant == 9:
            assert _G().w4_tile_rows(M, N) == 224
        _exact_checks(variant, M, N, K, lay, seed=variant)
        _random_checks(variant, M, N, K, lay, seed=variant, linear=True)


def _check_res(M, N, K, lay, per, seed):
    """grit_gemm_bf16_nt_res: exact inputs without factors and with factors in {0, 1, 2} (torch.equal), random inputs with the real
    drop-path factors 1 / 0.9 and zeros (bound); C and the residual on different leading dimensions inside fences."""
    G = _G()
    e = _extras(lay, N, K)
    nb = -(-M // per)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = torch.arange(M, device=DEV) // per
    a, b, bias = _exact_inputs(M, N, K, seed)
    res = torch.randint(-8, 9, (M, N), device=DEV, generator=g).to(BF16)
    branch = _products(a, b)[0] + bias.double()
    av, bv, biasv, resv = _place(a, e["A"]), _place(b, e["B"]), _place(bias, 8), _place(res, e["res"])
    for factors in (None, torch.tensor([(0.0, 1.0, 2.0, 1.0)[i % 4] for i in range(nb)], device=DEV),
                    torch.tensor([(2.0, 0.0, 1.0)[i % 3] for i in range(nb)], device=DEV)):
        f = 1.0 if factors is None else factors.double()[rows][:, None]
        ref = res.double() + f * branch
        assert float(branch.abs().max()) <= 256 and float(ref.abs().max()) <= 256
        c = _Fence(M, N, e["C"])
        G.gemm_nt_residual(av, bv, biasv, resv, factors, per if factors is not None else 0, out=c.view)
        assert torch.equal(c.view.double(), ref), (M, N, K, per, "BIAS_RES exact")
        assert c.guards_intact(), (M, N, K, per, "BIAS_RES guards")
    x, w, bias = _random_inputs(M, N, K, seed)
    res = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    prod, S = _products(x, w)
    branch = prod + bias.double()
    factors = torch.full((nb,), 1.0 / 0.9, device=DEV)
    factors[0] = 0.0
    factors[nb - 1] = 0.0 if nb > 2 else factors[nb - 1]
    f = factors.double()[rows][:, None]
    ref = res.double() + f * branch
    c = _Fence(M, N, e["C"])
    G.gemm_nt_residual(_place(x, e["A"]), _place(w, e["B"]), _place(bias, 8), _place(res, e["res"]), factors, per, out=c.view)
    bound = U * ref.abs() + f * (U * branch.abs() + 2.0 * K * 2.0 ** -24 * (S + bias.double().abs())) \
        + 2.0 ** -22 * (res.double().abs() + f * branch.abs())
    _check("residual", c.view, ref, bound)
    dropped = (factors == 0)[rows]
    assert torch.equal(c.view[dropped], res[dropped]) and c.guards_intact()


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("per", [256, 320])
@pytest.mark.parametrize("N,K", [(256, 64), (512, 128), (128, 32), (128, 96)])
def test_residual_epilogue_strided_with_samples_straddling_tiles(N, K, per, lay):
    """grit_gemm_bf16_nt_res on both of its kernels (N % 256 == 0: the four-wave kernel, tile height by shape; N = 128: the 256 x 128
    per-tile kernel), at their smallest K, ragged and full-tile M, samples of 256 and 320 rows so that tiles straddle samples."""
    for M in (2 * per + 57, 768):
        _check_res(M, N, K, lay, per, seed=N + K + per)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("M,N,K", [(81, 64, 64), (128, 128, 192), (64 + 17, 192, 128), (1, 64, 64)])
def test_relu_dropout_epilogues_strided(M, N, K, p):
    """grit_gemm_bf16_nt_relu on exact inputs: BIAS_RELU_DROP = the bf16 Linear result (here exactly the float64 one) followed by
    grit_relu_dropout_fwd with the same seed, DRELU = the bf16 product followed by grit_relu_dropout_bwd, bit for bit; p = 0 also
    against plain torch.  A, B, aux strided; C contiguous for BIAS_RELU_DROP (the contract), strided for DRELU; guards untouched."""
    G = _G()
    lib = _lib()
    seed = torch.tensor([987654321 + M], dtype=torch.int64, device=DEV)
    sp = _p(seed) if p > 0 else None
    for lay in (0, 1):
        e = _extras(lay, N, K)
        a, b, bias = _exact_inputs(M, N, K, seed=lay + 11)
        prod, _ = _products(a, b)
        lin = prod + bias.double()
        assert float(prod.abs().max()) <= 256 and float(lin.abs().max()) <= 256
        av, bv, biasv = _place(a, e["A"]), _place(b, e["B"]), _place(bias, 8)
        # forward
        lin16 = lin.to(BF16).contiguous()
        want = torch.empty_like(lin16)
        assert lib.grit_relu_dropout_fwd(_p(lin16), lin16.numel(), p, sp, 1, _p(want), _stream()) == OK
        c = _Fence(M, N, 0)
        assert lib.grit_gemm_bf16_nt_relu(_p(av), av.stride(0), _p(bv), bv.stride(0), _p(c.view), N, M, N, K, G.BIAS_RELU_DROP, _p(biasv),
                                          None, 0, p, sp, _stream()) == OK
        assert torch.equal(c.view, want) and c.guards_intact(), (M, N, K, p, lay, "BIAS_RELU_DROP")
        if p == 0:
            assert torch.equal(c.view.double(), lin.clamp_min(0.0))
        else:
            kept = (want != 0).sum().item() / max(1, (lin16 > 0).sum().item())
            assert M * N < 4096 or 0.6 < kept < 0.9  # the mask is a mask
        # backward of the following Linear: aux = the forward's output
        fwd = _place(want, e["aux"])
        dy16 = prod.to(BF16).contiguous()
        want_d = torch.empty_like(dy16)
        assert lib.grit_relu_dropout_bwd(_p(want), _p(dy16), dy16.numel(), p, sp, 1, _p(want_d), _stream()) == OK
        c = _Fence(M, N, e["C"])
        assert lib.grit_gemm_bf16_nt_relu(_p(av), av.stride(0), _p(bv), bv.stride(0), _p(c.view), c.view.stride(0), M, N, K, G.DRELU, None,
                                          _p(fwd), fwd.stride(0), p, None, _stream()) == OK
        assert torch.equal(c.view, want_d) and c.guards_intact(), (M, N, K, p, lay, "DRELU")
        if p == 0:
            assert torch.equal(c.view.double(), torch.where(want.double() > 0, prod, torch.zeros_like(prod)))


# ---------------------------------------------------------------------------------------------------------------
# 5. drop-path skip at a small shape
# ---------------------------------------------------------------------------------------------------------------
def _rows_call(a, b, c, epi, bias, aux, colsum, scale, per, variant):
    return _lib().grit_gemm_bf16_nt_rows(_p(a), a.stride(0), _p(b), b.stride(0), _p(c), c.stride(0), a.shape[0], b.shape[0], a.shape[1], epi,
                                         _p(bias), _p(aux), aux.stride(0) if aux is not None else 0, _p(colsum), _p(scale), per, variant, _stream())


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,per,zeros", [(2048, 512, (0, 3)), (2031, 512, (0, 2, 3)), (2304, 384, (0, 2, 5)), (2200, 512, (1, 4))])
def test_drop_path_skip_at_eight_and_nine_row_panels(M, per, zeros, variant):
    """grit_gemm_bf16_nt_rows, both epilogues, variants 0..4: eight row panels (round-robin panel mapping, tiles_m % 8 == 0) and nine
    (banded mapping), factors with zeros for the first and the last sample among others, samples that tiles straddle (384 rows).
    GELU': bit-equal to the dense call on the same zeroed rows, a NaN planted in the aux rows of a wholly skipped tile is never read.
    BIAS_GELU: zeros in C and aux for the skipped tiles, the dense values elsewhere.  Outputs inside fences; row_scale = NULL equals
    grit_gemm_bf16_nt."""
    G = _G()
    N, lay = 256, M % 2
    K = 128 if M != 2031 else (64 if variant == 0 else TILES[variant][2])  # (the ragged shape at the variant's smallest K: one step)
    e = _extras(lay, N, K)
    nb = -(-M // per)
    scale = torch.full((nb,), 1.25, device=DEV)
    scale[list(zeros)] = 0.0
    sample = torch.arange(M, device=DEV) // per
    x, w, bias = _random_inputs(M, N, K, seed=variant)
    x = (x.float() * scale[sample][:, None]).bfloat16()  # the backward's operand: exact zero rows for dropped samples
    skipped = torch.zeros(M, dtype=torch.bool, device=DEV)
    for m0 in range(0, M, 256):
        s_lo, s_hi = m0 // per, (min(m0 + 256, M) - 1) // per
        if s_lo == s_hi and float(scale[s_lo]) == 0.0:
            skipped[m0:m0 + 256] = True
    assert bool(skipped.any()) and not bool(skipped.all())
    xv, wv, biasv = _place(x, e["A"]), _place(w, e["B"]), _place(bias, 8)
    g = torch.Generator(device=DEV).manual_seed(M)
    aux = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    aux_nan = aux.clone()
    aux_nan[skipped] = float("nan")
    auxv, auxnv = _place(aux, e["aux"]), _place(aux_nan, e["aux"])
    slabs = -(-M // 128)
    # GELU'
    dense, _, dense_cs = _run_nt(variant, G.DGELU, xv, wv, e, aux=auxv, slabs=slabs)
    c, cs = _Fence(M, N, e["C"]), _Fence(slabs, N, 0, dtype=F32, below=8)
    assert _rows_call(xv, wv, c.view, G.DGELU, None, auxnv, cs.view, scale, per, variant) == OK
    assert torch.equal(c.view, dense.view) and torch.equal(cs.view, dense_cs.view), (M, per, variant, "DGELU")
    assert float(c.view[skipped].abs().max()) == 0.0 and c.guards_intact() and cs.guards_intact()
    c, cs = _Fence(M, N, e["C"]), _Fence(slabs, N, 0, dtype=F32, below=8)
    assert _rows_call(xv, wv, c.view, G.DGELU, None, auxv, cs.view, None, 0, variant) == OK
    assert torch.equal(c.view, dense.view) and torch.equal(cs.view, dense_cs.view) and c.guards_intact() and cs.guards_intact()
    # BIAS_GELU (forward operand: the rows of dropped samples are ordinary values)
    x2 = _random_inputs(M, N, K, seed=variant + 50)[0]
    x2v = _place(x2, e["A"])
    for keep_aux in (True, False):
        dense, dense_aux, _ = _run_nt(variant, G.BIAS_GELU, x2v, wv, e, bias=biasv, keep_aux=keep_aux)
        c, auxo = _Fence(M, N, e["C"]), (_Fence(M, N, e["aux"]) if keep_aux else None)
        assert _rows_call(x2v, wv, c.view, G.BIAS_GELU, biasv, auxo.view if keep_aux else None, None, scale, per, variant) == OK
        want = dense.view.clone()
        want[skipped] = 0
        assert torch.equal(c.view, want) and c.guards_intact(), (M, per, variant, "BIAS_GELU")
        if keep_aux:
            want = dense_aux.view.clone()
            want[skipped] = 0
            assert torch.equal(auxo.view, want) and auxo.guards_intact(), (M, per, variant, "BIAS_GELU aux")
        c, auxo = _Fence(M, N, e["C"]), (_Fence(M, N, e["aux"]) if keep_aux else None)
        assert _rows_call(x2v, wv, c.view, G.BIAS_GELU, biasv, auxo.view if keep_aux else None, None, None, 0, variant) == OK
        assert torch.equal(c.view, dense.view) and c.guards_intact()
        assert not keep_aux or (torch.equal(auxo.view, dense_aux.view) and auxo.guards_intact())


# ---------------------------------------------------------------------------------------------------------------
# 6. locality of a non-finite operand
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_nan_poisons_exactly_its_row_or_column(variant):
    """One NaN in A at (m*, k*) -- m* on a tile edge, on a wave edge, in the rows a shifted last tile shares with its neighbour and at
    M - 1 of a ragged M (the row the per-tile kernels replicate into the rows past M): exactly row m* of C is NaN, every other element
    equals the clean float64 product, no guard row is touched; in GELU' only the column-sum slab that owns m* is NaN.  One NaN in B at
    (n*, k*): exactly column n*."""
    G = _G()
    BM, BN, BK, slots, WTM = TILES[variant]
    lay = variant % 2
    if variant in (7, 9):
        M, N, K = 600, 512, 128
        H = _height(variant, M, N)
        assert H == BM
        # last tile shifted back to [M - H, M): shared rows [M - H, 2 H)
        rows = (H - 1, H, H // 2, M - H, M - H + H // 2, 2 * H - 1, 2 * H, M - 1)
    else:
        M, N, K = 2 * BM + 9, 2 * BN, 2 * BK
        rows = (0, WTM - 1, WTM, BM - 1, BM, 2 * BM, M - 1)
    e = _extras(lay, N, K)
    a, b, _ = _exact_inputs(M, N, K, seed=variant + 100)
    prod, _ = _products(a, b)
    assert float(prod.abs().max()) <= 256
    bv = _place(b, e["B"])
    ranges = _slab_ranges(variant, M, _height(variant, M, N))
    own = _slab_matrix(ranges, M)
    aux16 = _place(torch.full((M, N), 16.0, device=DEV, dtype=BF16), e["aux"])
    assert _dgelu16_exact()
    for i, m in enumerate(rows):
        an = a.clone()
        an[m, (i * 37 + 5) % K] = float("nan")
        av = _place(an, e["A"])
        clean = torch.ones(M, dtype=torch.bool, device=DEV)
        clean[m] = False
        runs = [(G.NONE, None)] + ([(G.DGELU, aux16)] if variant < 10 else [])
        for epi, aux in runs:
            c, _, cs = _run_nt(variant, epi, av, bv, e, aux=aux, slabs=len(ranges))
            got = c.view.double()
            assert bool(torch.isnan(got[m]).all()), (variant, m, epi)
            assert torch.equal(got[clean], prod[clean]), (variant, m, epi)
            assert c.guards_intact(), (variant, m, epi)
            if cs is not None:
                owner = [s for s, (lo, hi) in enumerate(ranges) if lo <= m < hi]
                assert len(owner) == 1
                sums = cs.view.double()
                good = torch.ones(len(ranges), dtype=torch.bool, device=DEV)
                good[owner[0]] = False
                assert bool(torch.isnan(sums[owner[0]]).all()), (variant, m, "slab")
                assert torch.equal(sums[good], (own @ prod)[good]), (variant, m, "other slabs")
                assert cs.guards_intact()
    av = _place(a, e["A"])
    for i, n in enumerate((0, BN - 1, BN, N - 1)):
        bn = b.clone()
        bn[n, (i * 53 + 3) % K] = float("nan")
        c, _, _ = _run_nt(variant, G.NONE, av, _place(bn, e["B"]), e)
        got = c.view.double()
        clean = torch.ones(N, dtype=torch.bool, device=DEV)
        clean[n] = False
        assert bool(torch.isnan(got[:, n]).all()) and torch.equal(got[:, clean], prod[:, clean]) and c.guards_intact(), (variant, n)


# ---------------------------------------------------------------------------------------------------------------
# 2. tile edges at the smallest shapes
# ---------------------------------------------------------------------------------------------------------------
def _m_edges(variant):
    BM, _, _, _, WTM = TILES[variant]
    if variant == 7:
        return (256, 257, 511, 512, 513)
    if variant == 9:
        return (256, 447, 448, 449, 671)
    return tuple(sorted({1, 15, 17, WTM - 1, WTM, WTM + 1, BM - 1, BM, BM + 1, 2 * BM + 9}))


def _n_edges(variant):
    BN = TILES[variant][1]
    return (BN, 2 * BN)  # (variant 12: 64 and 128)


def _k_edges(variant):
    _, _, BK, slots, _ = TILES[variant]
    return tuple(sorted({BK, 2 * BK, (slots - 1) * BK, slots * BK, (slots + 1) * BK}))


@pytest.mark.parametrize("variant", VARIANTS)
def test_row_edges_of_every_tile(variant):
    """Every M around the wave tile and the tile (the last tile of variants 7 / 9 shifted back by 1 .. height - 1 rows), at one and two
    tile widths and one mid K: every epilogue the variant carries."""
    K = _k_edges(variant)[-1]
    for N in _n_edges(variant):
        for M in _m_edges(variant):
            if variant == 9:
                assert _G().w4_tile_rows(M, N) == 224
            _exact_checks(variant, M, N, K, None, seed=M)
            _random_checks(variant, M, N, K, None, seed=M, tag="_edges")


@pytest.mark.parametrize("variant", VARIANTS)
def test_depth_edges_of_every_ring(variant):
    """K of one step (32 for variants 1, 3, 13 and 5), two, slots - 1, slots and slots + 1 steps at M = tile height + 1."""
    M = {7: 257, 9: 449}.get(variant, TILES[variant][0] + 1)
    assert _k_edges(variant)[0] == TILES[variant][2] == (32 if variant in (1, 3, 13, 5) else 64)
    for N in _n_edges(variant):
        for K in _k_edges(variant):
            if variant == 9:
                assert _G().w4_tile_rows(M, N) == 224
            _exact_checks(variant, M, N, K, None, seed=K)
            _random_checks(variant, M, N, K, None, seed=K, linear=(N == TILES[variant][1]), tag="_edges")


# ---------------------------------------------------------------------------------------------------------------
# 4. one stream over several tiles with one or two K steps
# ---------------------------------------------------------------------------------------------------------------
def _stream_rows():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, 256 * (-(-(cus + 1) // 8)) + 17


@pytest.mark.parametrize("N", [2048, 4096])
@pytest.mark.parametrize("variant,K", [(7, 64), (7, 128), (7, 192), (9, 64), (9, 128), (9, 192), (5, 32), (5, 64), (5, 96), (5, 128)])
def test_several_tiles_per_workgroup_with_short_k(variant, K, N):
    """The persistent kernels with more tiles than CUs (N = 2 048: two per workgroup for some; N = 4 096: three) and 1, 2 or 3 K steps
    per tile (variant 5: 1 .. 4 of its 32-deep steps): the prologue's transfers belong to two tiles, the epilogue's loads are issued
    before the tile's only step.  Variant 9 runs the 256-row kernels' M: with 224 ceil((CUs + 1) / 8) + 17 rows (and with 3
    ceil((CUs + 1) / 16) + 1 row tiles at N = 4 096) the 256-row tiling fits one round less and grit_gemm_w4_tile_rows answers 256;
    at this M both tilings need the same number of rounds, 224 wins and its tile count is just above one / two rounds."""
    cus, M = _stream_rows()
    if variant == 9:
        assert _G().w4_tile_rows(M, N) == 224
    H = 224 if variant == 9 else 256
    tiles = -(-M // H) * (N // 256)
    assert tiles > cus * (N // 2048) and tiles <= cus * (N // 2048 + 1)
    _exact_checks(variant, M, N, K, None, seed=K + N)
    _random_checks(variant, M, N, K, None, seed=K + N, linear=False, tag="_stream")


@pytest.mark.parametrize("N", [2048, 4096])
@pytest.mark.parametrize("K", [64, 128, 192])
def test_residual_epilogue_over_several_tiles_with_short_k(K, N):
    """grit_gemm_bf16_nt_res on the four-wave kernel at the same shapes (its loads of the residual tile run ahead of the K step too)."""
    cus, M = _stream_rows()
    assert -(-M // _G().w4_tile_rows(M, N)) * (N // 256) > cus
    _check_res(M, N, K, None, 1024, seed=K + N)


def test_variant_9_at_the_row_count_of_one_round_of_256_row_tiles():
    """224 ceil((CUs + 1) / 8) + 17 rows at N = 2 048: whichever height grit_gemm_w4_tile_rows answers runs, bit for bit the float64 result."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 224 * (-(-(cus + 1) // 8)) + 17
    assert _G().w4_tile_rows(M, 2048) in (224, 256)
    for K in (64, 128):
        _exact_checks(9, M, 2048, K, None, seed=K)


def test_zz_report():
    """Prints the worst err / bound per group of this run (pytest -s)."""
    for k in sorted(_WORST):
        print("WORST %s %.4f" % (k, _WORST[k]))
    assert all(v <= 1.0 for v in _WORST.values())
