"""The ten small kernels that hold the two decoders together (grit_amd/csrc/decoder.hip, grit_amd/csrc/glue.hip), at the places where
such kernels go wrong unnoticed: every template instantiation (the G = 64 geometry kernels), grid-stride loops that wrap, the copy
loop of the key mask over several passes, one-vector rows and odd vector counts, index arithmetic with cur != beam, saturated gates,
rounding ties, one-hot softmax rows, clamped and NaN reference points, and the dropout hash bit for bit.  References are the float64
/ exact models of tests/decoder_glue_model.py (checked on the CPU by tests/test_decoder_glue_model_cpu.py).

Which test reaches what:
  G = 64 geometry kernels (L*P in 33..64)       test_sampling_geometry_edges[3-11-*], [4-9-*], [4-16-*] (forward and backward)
  gate_pack loop wrap                           test_gate_pack_is_the_two_concatenations[1027-8200-*]
  gate_fuse loop wrap                           test_gate_fuse_bf16_is_the_composed_form_bit_for_bit[1027-8200],
                                                test_gate_fuse_fp32_against_float64[1027-8200]
  gate_bwd_a / gate_bwd_b loop wrap             test_gate_backward_stages[2051-520-*]
  relu_dropout forward / backward loop wrap     test_relu_dropout_mask_is_the_counter_hash[1048833-*]
  key-mask copy over several passes             test_decode_step_inputs_edges[*] (t_old = 65 and 130; 63 and 64 are the last one-pass sizes)

Bounds that carry a term of their own reasoning (everything else is the figure of the kernels' first tests or bit equality):
  UNDERFLOW   sigmoid(g) for g below about -87.3 lies under the smallest normal float (and bf16 shares float's exponent range): neither
              format holds it with any relative precision, and 1 + exp(-g) overflows for g < -88.7, where the device returns 0 and
              float64 does not.  Every gate bound therefore allows 2^-120 (64 smallest normals: gate inputs here are below 64 in
              magnitude) on top of its relative part.
  dG          t e s (1 - s) is NOT a pure product: s is rounded to float before 1 - s, an absolute error of up to a few 2^-24 in
              (1 - s) that is all of it once s rounds to 1 (g >= 17).  Its bound is the relative term on |dG| plus the same float
              term as the second stage on |t e s|.
  K_MIN       the fp32 bounds are four times torch's measured constant, but never under a fixed minimum of 8 units: on a handful
              of elements torch's largest error can come out as a fraction of a unit (or 0) by luck, while a correctly rounded
              float chain of the merge (sigmoid, product, sum, scale: half a unit each) already has a worst case of 2.
"""
import functools

import numpy as np
import pytest
import torch

from grit_amd import lib as binding
from tests import decoder_glue_model as dm

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, BAD_ARG, UNSUPPORTED = binding.OK, binding.ERR_BAD_ARG, binding.ERR_UNSUPPORTED
BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = -12345.0  # exactly representable in bf16 and fp32
PAD = 64             # canary elements behind every output
UNDERFLOW = 2.0 ** -120
K_MIN = 8.0
K_MAX = 32.0
DIV = float(np.float32(np.sqrt(2)))  # the divisor ops/gate.py and ops/glue.py pass
_ptr = binding.ptr


def _lib():
    return binding.load(), binding.current_stream_ptr()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _out(shape, dtype, fill=SENTINEL):
    """A sentinel-filled buffer and its leading view of `shape`; what lies behind the view is the canary."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _canary_intact(*bufs):
    for buf in bufs:
        assert bool((buf[-PAD:] == SENTINEL).all()), "canary overwritten"


def _untouched(*bufs):
    for buf in bufs:
        assert bool((buf == SENTINEL).all()), "a refused call wrote to its output"


def _ratio(got, want, unit, floor=UNDERFLOW):
    """Largest (|got - want| - floor) / unit over the elements with unit > 0; where unit is 0 the error must be within floor."""
    err = (got.double() - want).abs()
    assert bool(err.isfinite().all())
    dead = unit == 0
    assert bool((err[dead] <= floor).all())
    if bool(dead.all()):
        return 0.0
    return float(((err[~dead] - floor).clamp(min=0) / unit[~dead]).max())


# ------------------------------------------------------------------------------------------------------ gate_pack / gate_fuse

GATE_SHAPES = [(1, 8), (37, 24), (1027, 8200)]  # one vector; odd vector count per row in bf16; 1 052 675 bf16 vectors: the loop wraps


@pytest.fixture(scope="module")
def device_cases():
    """Device inputs shared by the tests of this module (built once per key, never modified) and freed when the module ends: the
    loop-wrap cases are a few hundred megabytes that the rest of the suite should not carry."""
    cache = {}

    def get(build, *key):
        if (build, key) not in cache:
            cache[(build, key)] = build(*key)
        return cache[(build, key)]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _gate_case(rows, d, dtype):
    case = dm.gate_case(rows, d, dtype, torch.Generator().manual_seed(rows * 7 + d))
    return {k: v.to(DEV) for k, v in case.items()}


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("rows,d", GATE_SHAPES)
def test_gate_pack_is_the_two_concatenations(rows, d, dtype, device_cases):
    c = device_cases(_gate_case, rows, d, dtype)
    lib, stream = _lib()
    buf, X = _out((2 * rows, 2 * d), dtype)
    st = lib.grit_gate_pack(_ptr(c["self_att"]), _ptr(c["enc1"]), _ptr(c["enc2"]), _ptr(c["mask"]), rows, d, int(dtype == BF16), _ptr(X),
                            stream)
    assert st == OK
    want = dm.gate_pack(c["self_att"], c["enc1"], c["enc2"], c["mask"])
    assert torch.equal(_bits(X), _bits(want))  # signed zeros included
    _canary_intact(buf)


def _fuse(c, rows, d, dtype):
    lib, stream = _lib()
    buf, out = _out((rows, d), dtype)
    st = lib.grit_gate_fuse(_ptr(c["enc1"]), _ptr(c["enc2"]), _ptr(c["G"]), _ptr(c["mask"]), rows, d, DIV, int(dtype == BF16), _ptr(out),
                            stream)
    assert st == OK
    _canary_intact(buf)
    return out


def _fuse_composed(c, rows):
    m = c["mask"].view(-1, 1)
    e1, e2 = c["enc1"] * m, c["enc2"] * m
    return ((e1 * torch.sigmoid(c["G"][:rows]) + e2 * torch.sigmoid(c["G"][rows:])) / np.sqrt(2)) * m


@pytest.mark.parametrize("rows,d", GATE_SHAPES)
def test_gate_fuse_bf16_is_the_composed_form_bit_for_bit(rows, d, device_cases):
    """Saturated gates (+-20, +-88, +-100, +-inf), +-0 in enc, products that cancel, masked rows: the project's stated contract."""
    c = device_cases(_gate_case, rows, d, BF16)
    out = _fuse(c, rows, d, BF16)
    want = _fuse_composed(c, rows)
    assert not bool(out.isnan().any())
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("rows,d", GATE_SHAPES)
def test_gate_fuse_fp32_against_float64(rows, d, device_cases):
    """|out - float64 chain| <= max(4 k, K_MIN) 2^-24 (|p1| + |p2|) + UNDERFLOW, k = torch's own fp32 composed form measured the same
    way on the same inputs, k < 32.
    Measured on gfx950, k of torch / of the kernel: (1, 8) 0.563 / 0.563; (37, 24) 1.456 / 1.456; (1027, 8200) 2.072 / 2.072 (the
    kernel's error is torch's own, element for element, on these inputs)."""
    c = device_cases(_gate_case, rows, d, F32)
    out = _fuse(c, rows, d, F32)
    want = dm.gate_fuse(c["enc1"], c["enc2"], c["G"], c["mask"], c=dm.C_F32)
    p1, p2 = dm.gate_products(c["enc1"], c["enc2"], c["G"], c["mask"])
    unit = 2.0 ** -24 * (p1.abs() + p2.abs())
    k_torch = _ratio(_fuse_composed(c, rows), want, unit)
    k_kernel = _ratio(out, want, unit)
    print("gate_fuse fp32 (%d, %d): k torch %.3f  kernel %.3f" % (rows, d, k_torch, k_kernel))
    assert k_torch < K_MAX
    assert k_kernel <= max(4 * k_torch, K_MIN)
    assert bool((out[c["mask"] == 0] == 0).all())


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_gate_kernels_refuse_what_they_cannot_load(dtype):
    """d = 12 (rows that are no whole 16-byte vectors) and operands one element off a 16-byte boundary: ERR_UNSUPPORTED, nothing written."""
    from grit_amd.ops import gate
    lib, stream = _lib()
    bf = int(dtype == BF16)
    rows = 4
    for d in (12, 16):
        mk = lambda n=rows * d: torch.randn(n + 8, device=DEV).to(dtype)
        s, a, b, g = mk(), mk(), mk(), mk(2 * rows * d)
        m = torch.ones(rows, device=DEV, dtype=dtype)
        xbuf = torch.full((4 * rows * d + 8,), SENTINEL, dtype=dtype, device=DEV)
        obuf = torch.full((rows * d + 8,), SENTINEL, dtype=dtype, device=DEV)
        if d == 12:
            fc = torch.nn.Linear(2 * d, d).to(DEV, dtype)
            with torch.no_grad():
                assert not gate.supported(s[:rows * d].view(rows, 1, d), a[:rows * d].view(rows, 1, d), b[:rows * d].view(rows, 1, d),
                                          m.view(rows, 1, 1), fc)
            assert lib.grit_gate_pack(_ptr(s), _ptr(a), _ptr(b), _ptr(m), rows, d, bf, _ptr(xbuf), stream) == UNSUPPORTED
            assert lib.grit_gate_fuse(_ptr(a), _ptr(b), _ptr(g), _ptr(m), rows, d, DIV, bf, _ptr(obuf), stream) == UNSUPPORTED
        else:  # each operand in turn at element offset 1
            fc = torch.nn.Linear(2 * d, d).to(DEV, dtype)
            with torch.no_grad():  # the same call at d = 16 is supported: above it is d = 12 that is refused
                assert gate.supported(s[:rows * d].view(rows, 1, d), a[:rows * d].view(rows, 1, d), b[:rows * d].view(rows, 1, d),
                                      m.view(rows, 1, 1), fc)
            for off in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
                st = lib.grit_gate_pack(_ptr(s[off[0]:]), _ptr(a[off[1]:]), _ptr(b[off[2]:]), _ptr(m), rows, d, bf, _ptr(xbuf[off[3]:]), stream)
                assert st == UNSUPPORTED, off
                st = lib.grit_gate_fuse(_ptr(a[off[0]:]), _ptr(b[off[1]:]), _ptr(g[off[2]:]), _ptr(m), rows, d, DIV, bf, _ptr(obuf[off[3]:]),
                                        stream)
                assert st == UNSUPPORTED, off
        torch.cuda.synchronize()
        _untouched(xbuf, obuf)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_gated_merge_takes_operands_off_a_16_byte_boundary(dtype):
    """Contiguous views at element offset 1 of a larger buffer (what a slice of a flat workspace is) give the aligned copy's result."""
    from grit_amd.ops import gate
    rows, T, d = 5, 1, 24
    g = torch.Generator().manual_seed(11)
    fc = torch.nn.Linear(2 * d, d).to(DEV, dtype)
    flat = [torch.randn(rows * T * d + 8, generator=g).to(DEV, dtype) for _ in range(3)]
    odd = [f[1:1 + rows * T * d].view(rows, T, d) for f in flat]
    assert all(t.is_contiguous() and t.data_ptr() % 16 for t in odd)
    mask = torch.tensor([1, 0, 1, 1, 1.0], device=DEV).to(dtype).view(rows, T, 1)
    with torch.no_grad():
        assert gate.supported(*odd, mask, fc)
        want = gate.gated_merge(*[t.clone() for t in odd], mask, fc)
        for which in range(3):
            ops = [t if i == which else t.clone() for i, t in enumerate(odd)]
            assert torch.equal(_bits(gate.gated_merge(*ops, mask, fc)), _bits(want)), which
        assert torch.equal(_bits(gate.gated_merge(*odd, mask, fc)), _bits(want))
        G = torch.randn(2 * rows * T * d + 8, generator=g).to(DEV, dtype)
        assert torch.equal(_bits(gate.fuse(odd[1], odd[2], G[1:1 + 2 * rows * T * d].view(-1, d), mask)),
                           _bits(gate.fuse(odd[1].clone(), odd[2].clone(), G[1:1 + 2 * rows * T * d].clone().view(-1, d), mask)))


# ------------------------------------------------------------------------------------------------------------------ kv_append

KV_CASES = [(3, 5, 2, 6, 8), (3, 3, 5, 6, 8), (2, 4, 4, 53, 64), (1, 1, 1, 1, 8)]  # (B, cur, beam, t_old, d), bf16: d = 8 is ONE vector


def _kv_codes(B, cur, beam, t_old, d):
    """Caches whose every element names its (tensor, row, t, col) as a 16-bit code (all codes distinct, asserted), viewed as bf16."""
    n_old, n_new = B * cur * t_old * d, B * beam * d
    assert 2 * (n_old + n_new) <= 65536
    code = lambda lo, n, shape: (torch.arange(lo, lo + n, dtype=torch.int32) - 32768).to(torch.int16).view(shape).view(BF16).to(DEV)
    return (code(0, n_old, (B * cur, t_old, d)), code(n_old, n_old, (B * cur, t_old, d)),
            code(2 * n_old, n_new, (B * beam, 1, d)), code(2 * n_old + n_new, n_new, (B * beam, 1, d)))


def _kv_src(pattern, B, cur, beam):
    if pattern == "first":
        return torch.zeros(B, beam, dtype=torch.int64, device=DEV)
    if pattern == "last":
        return torch.full((B, beam), cur - 1, dtype=torch.int64, device=DEV)
    b, j = torch.arange(B).view(B, 1), torch.arange(beam).view(1, beam)
    return ((b + j * (b + 1) + 1) % cur).to(DEV)  # another pattern per image


@pytest.mark.parametrize("pattern", ["first", "last", "per_image"])
@pytest.mark.parametrize("B,cur,beam,t_old,d", KV_CASES)
def test_kv_append_takes_each_row_from_its_source_beam(B, cur, beam, t_old, d, pattern):
    """b * cur + src[r] (not b * beam + src[r]) with cur > beam and cur < beam; exact, and nothing else is written or modified."""
    old_k, old_v, new_k, new_v = _kv_codes(B, cur, beam, t_old, d)
    keep_k, keep_v = old_k.clone(), old_v.clone()
    src = _kv_src(pattern, B, cur, beam)
    lib, stream = _lib()
    kbuf, out_k = _out((B * beam, t_old + 1, d), BF16)
    vbuf, out_v = _out((B * beam, t_old + 1, d), BF16)
    st = lib.grit_kv_append(_ptr(old_k), _ptr(old_v), _ptr(src), B, cur, beam, t_old, d * 2, _ptr(new_k), _ptr(new_v), d * 2, _ptr(out_k),
                            _ptr(out_v), stream)
    assert st == OK
    assert torch.equal(_bits(out_k), _bits(dm.kv_append(old_k, src, new_k, B, cur, beam)))
    assert torch.equal(_bits(out_v), _bits(dm.kv_append(old_v, src, new_v, B, cur, beam)))
    assert torch.equal(_bits(old_k), _bits(keep_k)) and torch.equal(_bits(old_v), _bits(keep_v))
    _canary_intact(kbuf, vbuf)


@pytest.mark.parametrize("layout", ["one_projection", "two_widths", "permuted_old"])
def test_kv_append_operand_layouts(layout):
    from grit_amd.ops import kv_cache
    B, cur, beam, t_old, d = 3, 5, 2, 6, 8
    old_k, old_v, new_k, new_v = _kv_codes(B, cur, beam, t_old, d)
    src = _kv_src("per_image", B, cur, beam)
    want_k, want_v = dm.kv_append(old_k, src, new_k, B, cur, beam), dm.kv_append(old_v, src, new_v, B, cur, beam)
    if layout == "one_projection":  # strided rows: slices of one [rows, 1, 3 d] projection
        qkv = torch.zeros(B * beam, 1, 3 * d, dtype=BF16, device=DEV)
        qkv[..., d:2 * d], qkv[..., 2 * d:] = new_k, new_v
        new_k, new_v = qkv[..., d:2 * d], qkv[..., 2 * d:]
        assert not new_k.is_contiguous()
    elif layout == "two_widths":  # row strides differ: the wrapper's contiguous() path
        wide_k = torch.zeros(B * beam, 1, 2 * d, dtype=BF16, device=DEV)
        wide_v = torch.zeros(B * beam, 1, 3 * d, dtype=BF16, device=DEV)
        wide_k[..., :d], wide_v[..., d:2 * d] = new_k, new_v
        new_k, new_v = wide_k[..., :d], wide_v[..., d:2 * d]
        assert new_k.stride(0) != new_v.stride(0)
    else:
        old_k = old_k.permute(1, 0, 2).contiguous().permute(1, 0, 2)
        assert not old_k.is_contiguous()
    got_k, got_v = kv_cache.append(old_k, old_v, src, new_k, new_v, beam=beam)
    assert torch.equal(_bits(got_k), _bits(want_k)) and torch.equal(_bits(got_v), _bits(want_v))


def test_kv_append_refuses_rows_that_are_no_whole_vectors():
    """bf16, d = 4: an 8-byte cache row."""
    from grit_amd.ops import kv_cache
    B, cur, beam, t_old, d = 2, 2, 2, 3, 4
    old_k, old_v, new_k, new_v = _kv_codes(B, cur, beam, t_old, d)
    src = _kv_src("per_image", B, cur, beam)
    with pytest.raises(binding.GritHipError):
        kv_cache.append(old_k, old_v, src, new_k, new_v, beam=beam)
    lib, stream = _lib()
    out_k = torch.full((B * beam * (t_old + 1) * d + PAD,), SENTINEL, dtype=BF16, device=DEV)
    out_v = out_k.clone()
    st = lib.grit_kv_append(_ptr(old_k), _ptr(old_v), _ptr(src), B, cur, beam, t_old, d * 2, _ptr(new_k), _ptr(new_v), d * 2, _ptr(out_k),
                            _ptr(out_v), stream)
    assert st == UNSUPPORTED
    torch.cuda.synchronize()
    _untouched(out_k, out_v)


# --------------------------------------------------------------------------------------------------------- decode_step_inputs

VOCAB, N_POS, PAD_IDX = 30, 140, 1


@functools.lru_cache(maxsize=None)
def _tables(d, dtype):
    word, pos = dm.tie_tables(VOCAB, N_POS, d, dtype, torch.Generator().manual_seed(d))
    return word, pos, word.to(DEV), pos.to(DEV)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("R", [1, 40])
@pytest.mark.parametrize("d", [8, 72, 200, 512])
def test_decode_step_inputs_edges(d, R, dtype):
    """Mask copy over 0, 1 and several passes of the 64-lane loop, embedding loop below / over one pass, per-row step counters, the
    position table's last row, tokens 0 / <pad> / vocab - 1, bf16 rounding ties: bit-equal to the written-out composition."""
    from grit_amd.ops import decode_inputs
    word, pos, word_d, pos_d = _tables(d, dtype)
    g = torch.Generator().manual_seed(d + R)
    special = [0, PAD_IDX, VOCAB - 1]
    for n, t_old in enumerate([0, 1, 63, 64, 65, 130]):
        tokens = torch.randint(0, VOCAB, (R, 1), generator=g)
        seq = torch.randint(0, N_POS - 2, (R, 1), generator=g)
        if R == 1:
            tokens[0, 0] = special[n % 3]
            if n >= 3:
                seq[0, 0] = N_POS - 2
        else:
            tokens[:6, 0] = torch.tensor(special + special)
            seq[3:6, 0] = N_POS - 2  # each special token also at the table's last row
        old_mask = torch.rand(R, 1, 1, t_old, generator=g) < 0.4
        want_x, want_mask, want_pad, want_seq = dm.step_inputs(tokens, PAD_IDX, word, pos, seq.view(-1), old_mask)
        tok_d, seq_d, mask_d = tokens.to(DEV), seq.to(DEV), old_mask.to(DEV)
        with torch.no_grad():
            assert decode_inputs.supported(tok_d, word_d, pos_d, seq_d, mask_d)
            x, new_mask, mask_pad = decode_inputs.step_inputs(tok_d, PAD_IDX, word_d, pos_d, seq_d, mask_d)
        assert x.shape == (R, 1, d) and x.dtype == dtype and torch.equal(_bits(x).cpu(), _bits(want_x)), t_old
        assert new_mask.dtype == torch.bool and new_mask.shape == (R, 1, 1, t_old + 1) and torch.equal(new_mask.cpu(), want_mask), t_old
        assert mask_pad.shape == (R, 1, 1) and torch.equal(_bits(mask_pad).cpu(), _bits(want_pad)), t_old
        assert torch.equal(seq_d.cpu().view(-1), want_seq) and torch.equal(want_seq, seq.view(-1) + 1)
        assert torch.equal(mask_d.cpu(), old_mask) and torch.equal(tok_d.cpu(), tokens)
    if dtype == BF16:  # the ties are really there: row 0 / vocab - 1 of the word table plus any position row
        assert (word[0] + pos[N_POS - 1])[:3].tolist() == [256.0, 260.0, -256.0]


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_decode_step_counter_stops_at_the_position_table(dtype):
    """max_len = 6: step 6 reads position 6, the table's last row; step 7 raises IndexError and changes no state."""
    import grit_amd.models.caption.cap_generator as CG
    torch.manual_seed(2)
    R, d = 3, 8
    gen = CG.CaptionGenerator(vocab_size=20, max_len=6, n_layers=1, pad_idx=PAD_IDX, d_model=d, n_heads=1, d_ff=16).to(DEV, dtype).eval()
    w, p = gen.word_emb.weight, gen.pos_emb.weight
    assert p.shape[0] == 7
    with torch.no_grad(), gen.statefulness(R):
        for step in range(1, 7):
            tokens = torch.tensor([[0], [PAD_IDX], [19]], device=DEV)
            fused = gen._step_inputs(tokens)
            assert fused is not None
            x, mask_x, mask_pad = fused
            assert torch.equal(_bits(x), _bits((w[tokens.view(-1)] + p[step]).unsqueeze(1)))
            assert mask_x.shape == (R, 1, 1, step) and bool((gen.running_seq == step).all())
            for layer in gen.layers:
                layer.self_att.timestep += 1
        seq, mask = gen.running_seq.clone(), gen.running_mask_x.clone()
        with pytest.raises(IndexError):
            gen._step_inputs(tokens)
        torch.cuda.synchronize()
        assert torch.equal(gen.running_seq, seq) and torch.equal(gen.running_mask_x, mask)


# ------------------------------------------------------------------------------------------------------------- MSDA geometry

LEVEL_SHAPES = [[40, 30], [20, 15], [10, 8], [5, 4]]  # (H, W), W != H: swapping them shows
GEO_LP = [(1, 1), (1, 17), (3, 11), (4, 9), (4, 16), (2, 8)]  # L*P = 1, 17, 33, 36, 64, 16 -> G = 16, 32, 64, 64, 64, 16


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("L,P", GEO_LP)
def test_sampling_geometry_edges(L, P, M, ref_dim, dtype):
    """Every lane-group width, M = 1 and an M that leaves the last block partly empty (N * Lq * M = 15 or 5 groups), logit rows that
    are random / all equal / one-hot / on a large common offset, zero-size boxes, bf16 reference points, operands that are column
    slices of a wider tensor; three losses (loc only, aw only, both) against the float64 model at the bounds of the kernels' first test."""
    from grit_amd.ops.glue import sampling_geometry
    N, Lq, LP = 1, 5, L * P
    g = torch.Generator().manual_seed(L * 1000 + P * 10 + M)
    shapes = torch.tensor(LEVEL_SHAPES[:L])
    shapes_d = shapes.to(DEV)
    ref = torch.rand(N, Lq, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[0, 0, :, 2:] = 0  # a box of zero width and height
        ref[0, 1, :, 2] = 0
    c_loc = torch.randn(N, Lq, M, L, P, 2, generator=g)
    c_aw = torch.randn(N, Lq, M, L, P, generator=g)
    gtol = dict(rtol=1e-5, atol=1e-6) if dtype == F32 else dict(rtol=1e-2, atol=1e-3)
    for kind, sliced, ref_in in [("random", False, ref), ("equal", False, ref), ("onehot", False, ref), ("offset", False, ref),
                                 ("random", True, ref), ("onehot", True, ref.bfloat16())]:
        off = torch.randn(N, Lq, M * LP * 2, generator=g).to(dtype)
        log = dm.logit_rows(kind, (N, Lq, M), LP, dtype, g).view(N, Lq, M * LP)
        if sliced:  # both operands as column slices of one wider tensor
            wide = torch.cat([torch.zeros(N, Lq, 3, dtype=dtype), off, log, torch.zeros(N, Lq, 5, dtype=dtype)], -1).to(DEV).requires_grad_(True)
            off_d, log_d = wide[..., 3:3 + M * LP * 2], wide[..., 3 + M * LP * 2:3 + M * LP * 3]
            assert not off_d.is_contiguous()
        else:
            off_d, log_d = off.to(DEV).requires_grad_(True), log.to(DEV).requires_grad_(True)
        ref64 = ref_in.float()
        want_loc, want_aw = dm.geometry(off, log, ref64, shapes, M, L, P)
        for loss in ("loc", "aw", "both"):
            out = sampling_geometry(off_d, log_d, ref_in.to(DEV), shapes_d, M, L, P)
            assert out is not None
            loc, aw = out
            assert loc.dtype == aw.dtype == F32 and loc.shape == (N, Lq, M, L, P, 2) and aw.shape == (N, Lq, M, L, P)
            g_loc = c_loc if loss != "aw" else torch.zeros_like(c_loc)
            g_aw = c_aw if loss != "loc" else torch.zeros_like(c_aw)
            total = (loc * c_loc.to(DEV)).sum() if loss == "loc" else (aw * c_aw.to(DEV)).sum() if loss == "aw" else \
                (loc * c_loc.to(DEV)).sum() + (aw * c_aw.to(DEV)).sum()
            leaves = (wide,) if sliced else (off_d, log_d)
            grads = torch.autograd.grad(total, leaves)
            if sliced:
                d_off, d_log = grads[0][..., 3:3 + M * LP * 2], grads[0][..., 3 + M * LP * 2:3 + M * LP * 3]
                assert bool((grads[0][..., :3] == 0).all()) and bool((grads[0][..., 3 + M * LP * 3:] == 0).all())
            else:
                d_off, d_log = grads
            what = "%s %s sliced=%s" % (kind, loss, sliced)
            loc_c, aw_c = loc.detach().cpu().double(), aw.detach().cpu().double()
            torch.testing.assert_close(loc_c, want_loc, rtol=1e-6, atol=1e-6, msg=lambda m: what + " loc: " + m)
            torch.testing.assert_close(aw_c, want_aw, rtol=1e-5, atol=1e-6, msg=lambda m: what + " aw: " + m)
            # the reference backward starts from the float64 weights; the kernel's starts from its own float32 ones, which the
            # assertion above holds to 1e-5 / 1e-6 of them: a difference far inside the gradient bounds
            want_off, want_log = dm.geometry_grad(g_loc, g_aw, want_aw, ref64, shapes, M, L, P)
            assert d_off.dtype == d_log.dtype == dtype
            torch.testing.assert_close(d_off.cpu().double(), want_off, msg=lambda m: what + " d_off: " + m, **gtol)
            torch.testing.assert_close(d_log.cpu().double(), want_log, msg=lambda m: what + " d_log: " + m, **gtol)
            # rows of weights sum to 1, rows of logit gradients to 0
            assert float((aw_c.view(N, Lq, M, LP).sum(-1) - 1).abs().max()) <= LP * 1e-6, what
            ga_max = g_aw.double().view(N, Lq, M, LP).abs().amax(-1)
            row = d_log.cpu().double().view(N, Lq, M, LP).sum(-1).abs()
            # bf16 outputs: each term is rounded (half an ulp: up to 2^-8 relative) and sum |a (ga - dot)| <= 2 max |ga|
            slack = LP * 1e-6 * ga_max + (2.0 ** -7 * ga_max if dtype == BF16 else 0)
            assert bool((row <= slack).all()), (what, float((row - slack).max()))


# ---------------------------------------------------------------------------------------------------------------- box_refine

def _box_delta(rows, dtype, gen, shift=0):
    delta = 3 * torch.randn(rows, 4, generator=gen)
    hard = torch.tensor([100.0, -100.0, float("inf"), float("-inf")])
    flat = delta.view(-1)
    n = min(flat.numel(), 8 if rows > 1 else 4)
    flat[:n] = torch.cat([hard.roll(shift), hard.roll(shift + 1)])[:n]
    if rows > 1:  # the same four against every reference value: a column of each
        for c in range(4):
            delta[8 + c:8 + c + 28:4, c] = hard.repeat(7)[:len(delta[8 + c:8 + c + 28:4, c])]
    return delta.to(dtype)


def _box_check(delta, ref, ref_dev=None):
    """`ref_dev`: the reference as the wrapper is to see it (a device view); default a dense device copy of `ref`."""
    from grit_amd.ops.glue import box_refine
    got = box_refine(delta.to(DEV), ref.to(DEV) if ref_dev is None else ref_dev)
    assert got is not None and got.dtype == F32 and got.shape == delta.shape
    got = got.cpu()
    want = dm.box_refine(delta, ref)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6, equal_nan=True)
    # saturation is exact: 1 + exp(-v) is 1 for v >= 17 and infinite for v <= -89 in float
    v = delta.double().clone()
    v[..., :ref.shape[-1]] += dm.inverse_sigmoid64(ref)
    assert bool((got[v >= 88] == 1).all()) and bool((got[v <= -89] == 0).all())
    assert bool((got[delta.float() == float("inf")] == 1).all()) and bool((got[delta.float() == float("-inf")] == 0).all())
    return got, want


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("rows", [1, 65])
def test_box_refine_clamps_and_saturation(rows, ref_dim, dtype):
    """References from {-0.3, 0, 1e-5, 0.5, 1 - 1e-5, 1, 1.7} (both clamps, both eps branches and their edges), deltas with +-100
    and +-inf, the 2-d reference as a slice of a 4-d tensor; float64 model at the bounds of the kernel's first test."""
    g = torch.Generator().manual_seed(rows + ref_dim)
    for shift in range(7 if rows == 1 else 1):
        ref4 = dm.box_references(rows, 4, g).roll(shift, -1)
        if rows == 1:
            ref4 = torch.tensor(dm.BOX_REF_VALUES, dtype=F32).roll(shift)[:4].view(1, 4)
        ref4_dev = ref4.to(DEV)
        if ref_dim == 2:  # sliced ON the device: a copy across devices would hand the wrapper a dense tensor
            ref, ref_dev = ref4[..., :2], ref4_dev[..., :2]
            assert ref_dev.stride(0) == 4 and (rows == 1 or not ref_dev.is_contiguous())
            ref4_dev[..., 2:] = 0.5  # what a kernel reading the slice as dense rows would pick up instead of the next row's centre
        else:
            ref, ref_dev = ref4, ref4_dev
        got, want = _box_check(_box_delta(rows, dtype, g, shift), ref, ref_dev)
        assert not bool(got.isnan().any())


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_box_refine_clamped_references_are_bit_equal(ref_dim):
    """Bit level: every reference below the lower clamp gives the bits of reference 0 (-0 and a value under eps included, which
    both end in eps / 1), every reference above the upper clamp the bits of reference 1, for the same deltas."""
    from grit_amd.ops.glue import box_refine
    g = torch.Generator().manual_seed(9)
    rows = 33
    delta = (3 * torch.randn(rows, 4, generator=g)).to(DEV)
    outs = {v: box_refine(delta, torch.full((rows, ref_dim), v, device=DEV)) for v in
            (0.0, -0.0, -0.3, -1e30, float("-inf"), 1e-30, 1.0, 1.7, 1e30, float("inf"), 0.5)}
    for v in (-0.0, -0.3, -1e30, float("-inf"), 1e-30):
        assert torch.equal(_bits(outs[v]), _bits(outs[0.0])), v
    for v in (1.7, 1e30, float("inf")):
        assert torch.equal(_bits(outs[v]), _bits(outs[1.0])), v
    assert not torch.equal(_bits(outs[0.0]), _bits(outs[1.0])) and not bool(outs[0.0].isnan().any() | outs[1.0].isnan().any())
    # reference 0.5: inverse_sigmoid is log(1) = 0 exactly, the refined columns are those of the unrefined delta
    assert torch.equal(_bits(outs[0.5][:, :2]), _bits(box_refine(torch.cat([delta[:, 2:], delta[:, :2]], 1),
                                                                  torch.full((rows, 2), 0.5, device=DEV))[:, 2:]))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_box_refine_passes_nan_on(ref_dim, dtype):
    """A NaN reference point or delta gives NaN in exactly the outputs where the composed form (torch.clamp passes NaN on) gives it:
    a diverged run must not look healthy on the device path only."""
    from grit_amd.utils.misc import inverse_sigmoid
    rows = 65
    g = torch.Generator().manual_seed(ref_dim)
    ref = dm.box_references(rows, ref_dim, g)
    delta = _box_delta(rows, dtype, g)
    for c in range(ref_dim):
        ref[3 + c, c] = float("nan")
    ref[40] = float("nan")
    delta[50, 3] = delta[51, 0] = float("nan")
    got, want = _box_check(delta, ref)
    d, r = delta.to(DEV).float(), ref.to(DEV)
    composed = (d + inverse_sigmoid(r)).sigmoid() if ref_dim == 4 else torch.cat([d[..., :2] + inverse_sigmoid(r), d[..., 2:]], -1).sigmoid()
    print("box_refine NaN outputs: kernel %d, composed form %d, float64 model %d" %
          (int(got.isnan().sum()), int(composed.isnan().sum()), int(want.isnan().sum())))
    assert torch.equal(got.isnan(), composed.isnan().cpu()) and torch.equal(got.isnan(), want.isnan())
    assert int(got.isnan().sum()) == 2 * ref_dim + 2


# -------------------------------------------------------------------------------------------------------------- relu_dropout

SEEDS = (0, 1, 2 ** 63 + 5, 2 ** 64 - 1)
BF16_TINY = 2.0 ** -133  # the smallest positive bf16 subnormal


@functools.lru_cache(maxsize=None)
def _dropout_inputs(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).bfloat16()  # bf16 values: the same inputs serve both dtypes
    x[0] = BF16_TINY
    dy = torch.randn(n, generator=g).bfloat16()
    dy = torch.where(dy == 0, torch.ones_like(dy), dy)
    return x, dy


@pytest.mark.parametrize("p", [0.1, 0.5, 0.999])
@pytest.mark.parametrize("n", [1, 255, 257, 1048576 + 257])
def test_relu_dropout_mask_is_the_counter_hash(n, p):
    """Which positive inputs come out as zero is decided by keep_scale's hash alone -- the one gemm.hip's epilogues reproduce -- so the
    test holds the kernel to the NumPy model of it element for element: forward and backward, fp32 and bf16, four seeds given as
    two's-complement int64, the grid-stride loop wrapped at the largest n.  Kept values are x * (1 / (1 - p)) rounded once.
    NaN inputs are left out on purpose: `x > 0 ? x * k : 0` (a NaN becomes 0) is shared with the ReLU epilogues of gemm.hip and has
    to stay bit-equal to them; changing both belongs to a pull request of its own."""
    lib, stream = _lib()
    x, dy = _dropout_inputs(n)
    inv_keep = torch.tensor(np.float32(1) / (np.float32(1) - np.float32(p)))
    pos = x > 0
    for seed in SEEDS:
        keep = torch.from_numpy(dm.keep_mask(seed, n, p))
        seed_dev = torch.tensor([dm.seed_as_int64(seed)], dtype=torch.int64, device=DEV)
        live = pos & keep
        masks = []
        for dtype in (F32, BF16):
            bf = int(dtype == BF16)
            xd, dyd = x.to(DEV, dtype), dy.to(DEV, dtype)
            ybuf, y = _out((n,), dtype)
            assert lib.grit_relu_dropout_fwd(_ptr(xd), n, p, _ptr(seed_dev), bf, _ptr(y), stream) == OK
            dbuf, dx = _out((n,), dtype)
            assert lib.grit_relu_dropout_bwd(_ptr(xd), _ptr(dyd), n, p, _ptr(seed_dev), bf, _ptr(dx), stream) == OK
            d2buf, dx2 = _out((n,), dtype)  # from the forward's OUTPUT in place of x (ops/glue.py relu_dropout_backward)
            assert lib.grit_relu_dropout_bwd(_ptr(y), _ptr(dyd), n, p, _ptr(seed_dev), bf, _ptr(dx2), stream) == OK
            _canary_intact(ybuf, dbuf, d2buf)
            y_c, dx_c = y.cpu(), dx.cpu()
            assert torch.equal(y_c != 0, live), (seed, dtype)  # no tolerance, no rate
            assert torch.equal(dx_c != 0, live), (seed, dtype)
            # x > 0 ? v * k : 0 with k = 0 for a dropped element: a dropped negative gradient is -0, as in torch's dropout backward
            zero, k = torch.zeros((), dtype=dtype), torch.where(keep, inv_keep, torch.zeros(()))
            want_y = torch.where(pos, (x.float() * k).to(dtype), zero)
            want_dx = torch.where(pos, (dy.float() * k).to(dtype), zero)
            assert torch.equal(_bits(y_c), _bits(want_y)) and torch.equal(_bits(dx_c), _bits(want_dx)), (seed, dtype)
            # the same gradient; only the zero of a dropped negative dy differs in sign (from y it is the `: 0` branch, +0)
            assert torch.equal(dx2, dx) and torch.equal(_bits(dx2)[live.to(DEV)], _bits(dx)[live.to(DEV)]), (seed, dtype)
            assert not bool((_bits(dx2)[~live.to(DEV)] != 0).any()), (seed, dtype)
            masks.append(y_c != 0)
        assert torch.equal(masks[0], masks[1])
    assert bool(pos[0])  # the subnormal is a positive input: kept or dropped by the hash like any other


@pytest.mark.parametrize("seed", SEEDS)
def test_relu_dropout_keeps_the_element_whose_draw_equals_p(seed):
    """keep iff u >= p: with p set to the draw of one element (a multiple of 2^-24, exact as a float), that element is kept.  At the
    three rates above u == p is a one-in-2^24 event, which a million elements need not contain."""
    lib, stream = _lib()
    n = 257
    u = dm.dropout_uniform(seed, n)
    x = torch.ones(n, device=DEV)
    for i in [int(j) for j in np.argsort(np.abs(u - 0.5))[:3]]:  # the three draws nearest one half
        p = float(u[i])
        assert 0 < p < 1
        keep = torch.from_numpy(dm.keep_mask(seed, n, p))
        assert bool(keep[i])
        seed_dev = torch.tensor([dm.seed_as_int64(seed)], dtype=torch.int64, device=DEV)
        ybuf, y = _out((n,), F32)
        assert lib.grit_relu_dropout_fwd(_ptr(x), n, p, _ptr(seed_dev), 0, _ptr(y), stream) == OK
        _canary_intact(ybuf)
        assert torch.equal(y.cpu() != 0, keep), (seed, i, p)


# -------------------------------------------------------------------------------------------------------- gate_bwd_a / gate_bwd_b

BWD_SHAPES = [(1, 1), (5, 7), (2051, 520)]  # d no multiple of 8 (the scalar kernels take any d); 1 066 520 elements: the loop wraps


def _bwd_case(rows, d, dtype):
    g = torch.Generator().manual_seed(rows * 3 + d)
    c = {k: v.to(DEV) for k, v in dm.gate_case(rows, d, dtype, g).items()}
    c["d_out"] = torch.randn(rows, d, generator=g).to(dtype).to(DEV)
    dX = torch.randn(2 * rows, 2 * d, generator=g).to(DEV).double()
    # in a third of the elements dX is -(t * s) rounded to the dtype: t * s + dX cancels to rounding
    t = c["d_out"].double() * c["mask"].double().view(-1, 1) * dm.C_F32
    ts = torch.cat([t * dm.sigmoid64(c["G"][:rows]), t * dm.sigmoid64(c["G"][rows:])], 0)
    cancel = torch.rand(2 * rows, d, generator=g).to(DEV) < 1 / 3
    dX[:, d:] = torch.where(cancel, -ts, dX[:, d:])
    c["dX"] = dX.to(dtype)
    c["ts"] = ts
    return c


def _bwd_run(c, rows, d, dtype):
    lib, stream = _lib()
    bf = int(dtype == BF16)
    gbuf, dG = _out((2 * rows, d), dtype)
    st = lib.grit_gate_bwd_a(_ptr(c["d_out"]), _ptr(c["enc1"]), _ptr(c["enc2"]), _ptr(c["G"]), _ptr(c["mask"]), rows, d, DIV, bf, _ptr(dG),
                             stream)
    assert st == OK
    bufs, outs = zip(*[_out((rows, d), dtype) for _ in range(3)])
    st = lib.grit_gate_bwd_b(_ptr(c["d_out"]), _ptr(c["G"]), _ptr(c["mask"]), _ptr(c["dX"]), rows, d, DIV, bf, _ptr(outs[0]), _ptr(outs[1]),
                             _ptr(outs[2]), stream)
    assert st == OK
    _canary_intact(gbuf, *bufs)
    return (dG,) + outs


def _bwd_composed(c, rows, d):
    """torch's composed form of the two stages in the tensors' own dtype."""
    m = c["mask"].view(-1, 1)
    t = c["d_out"] * m * dm.C_F32
    s1, s2 = torch.sigmoid(c["G"][:rows]), torch.sigmoid(c["G"][rows:])
    dG = torch.cat([t * (c["enc1"] * m) * s1 * (1 - s1), t * (c["enc2"] * m) * s2 * (1 - s2)], 0)
    x = c["dX"]
    return dG, x[:rows, :d] + x[rows:, :d], (t * s1 + x[:rows, d:]) * m, (t * s2 + x[rows:, d:]) * m


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("rows,d", BWD_SHAPES)
def test_gate_backward_stages(rows, d, dtype, device_cases):
    """Direct calls on synthetic G and dX against the float64 model.
    bf16: |err| <= 2^-8 |ref| + 2^-20 u + UNDERFLOW with u = |t s| + |dX| for d_enc_i and u = |t e s| for dG (module docstring).
    fp32: |err| <= max(4 k, K_MIN) 2^-24 (|ref| + u) + UNDERFLOW, k = torch's own fp32 composed form on the same inputs, k < 32.
    d_self is one addition: bit-equal to torch's.  Rows with mask 0 give exact zeros in dG, d_enc1 and d_enc2.
    Measured on gfx950, k of torch / of the kernel for dG, d_enc1, d_enc2: (1, 1) 0.000 / 0.000, 0.054 / 0.054, 0.018 / 0.018;
    (5, 7) 0.295 / 0.295, 0.406 / 0.406, 0.496 / 0.496; (2051, 520) 1.528 / 1.528, 1.520 / 1.204, 1.473 / 1.126."""
    c = device_cases(_bwd_case, rows, d, dtype)
    got = _bwd_run(c, rows, d, dtype)
    want = (dm.gate_bwd_a(c["d_out"], c["enc1"], c["enc2"], c["G"], c["mask"], c=dm.C_F32),) + \
        dm.gate_bwd_b(c["d_out"], c["G"], c["mask"], c["dX"], c=dm.C_F32)
    m = c["mask"].double().view(-1, 1)
    tes = torch.cat([c["ts"][:rows] * (c["enc1"].double() * m), c["ts"][rows:] * (c["enc2"].double() * m)], 0).abs()
    x = c["dX"].double()
    units = (tes, None, (c["ts"][:rows].abs() + x[:rows, d:].abs()) * m, (c["ts"][rows:].abs() + x[rows:, d:].abs()) * m)
    composed = _bwd_composed(c, rows, d)
    assert torch.equal(_bits(got[1]), _bits(composed[1]))  # d_self: the plain sum of the two halves, mask or no mask
    torch.testing.assert_close(got[1].double(), want[1], rtol=2.0 ** -8 if dtype == BF16 else 2.0 ** -23, atol=UNDERFLOW)
    for name, y, w, u, comp in [(n, got[i], want[i], units[i], composed[i]) for i, n in ((0, "dG"), (2, "d_enc1"), (3, "d_enc2"))]:
        assert not bool(y.isnan().any()), name
        if dtype == BF16:
            bound = 2.0 ** -8 * w.abs() + 2.0 ** -20 * u + UNDERFLOW
            excess = (y.double() - w).abs() - bound
            assert bool((excess <= 0).all()), (name, float(excess.max()))
        else:
            unit = 2.0 ** -24 * (w.abs() + u)
            k_torch, k_kernel = _ratio(comp, w, unit), _ratio(y, w, unit)
            print("gate_bwd fp32 (%d, %d) %s: k torch %.3f  kernel %.3f" % (rows, d, name, k_torch, k_kernel))
            assert k_torch < K_MAX, name
            assert k_kernel <= max(4 * k_torch, K_MIN), name
    dead = c["mask"] == 0
    assert bool((got[0][torch.cat([dead, dead])] == 0).all()) and bool((got[2][dead] == 0).all()) and bool((got[3][dead] == 0).all())


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_gated_merge_training_node_against_float64_autograd(dtype):
    """B * T = 3, d = 8 through gated_merge_train: the output and all five gradients against float64 autograd of the composed form on
    the same (dtype-rounded) inputs.  The yardstick is the composed form in the SAME dtype: its own largest error against float64,
    measured here per tensor; the fused node may have at most twice that.
    Measured on gfx950 in bf16, composed form / fused node: out 4.90e-3 / 4.90e-3, d_self 1.77e-3 / 7.49e-4, d_enc1 1.54e-3 /
    9.22e-4, d_enc2 3.02e-3 / 1.11e-3, dW 6.17e-3 / 3.93e-3, db 2.35e-3 / 1.29e-3.  In fp32 (an addition of this test, with a floor
    of its own, below) out 7.95e-8 / 7.52e-8, d_self 1.96e-8 / 2.16e-8, d_enc1 4.43e-8 / 4.43e-8, d_enc2 3.47e-8 / 5.94e-8, dW
    9.41e-8 / 2.77e-7: one mm over K = 6 where autograd adds two of K = 3."""
    from grit_amd.ops.glue import gated_merge_train
    from grit_amd.ops.linear import Linear
    g = torch.Generator().manual_seed(21)
    B, T, d = 3, 1, 8
    fc = Linear(2 * d, d).to(DEV, dtype)
    mk = lambda: torch.randn(B, T, d, generator=g).to(DEV, dtype).requires_grad_(True)
    s, e1, e2 = mk(), mk(), mk()
    mask = torch.tensor([1.0, 0.0, 1.0], device=DEV).to(dtype).view(B, T, 1)
    cot = torch.randn(B, T, d, generator=g).to(DEV, dtype)

    def composed(s_, e1_, e2_, mask_, w_, b_, cot_):
        a, b = e1_ * mask_, e2_ * mask_
        lin = lambda z: torch.nn.functional.linear(z, w_, b_)
        g1, g2 = torch.sigmoid(lin(torch.cat([s_, a], -1))), torch.sigmoid(lin(torch.cat([s_, b], -1)))
        out = ((a * g1 + b * g2) / np.sqrt(2)) * mask_
        return [out.detach()] + list(torch.autograd.grad(out, (s_, e1_, e2_, w_, b_), cot_))

    leaves = (s, e1, e2, fc.weight, fc.bias)
    want = composed(*[t.detach().double().requires_grad_(True) for t in (s, e1, e2)], mask.double(),
                    fc.weight.detach().double().requires_grad_(True), fc.bias.detach().double().requires_grad_(True), cot.double())
    same = composed(s, e1, e2, mask, fc.weight, fc.bias, cot)
    out = gated_merge_train(s, e1, e2, mask, fc)
    assert out is not None
    got = [out.detach()] + list(torch.autograd.grad(out, leaves, cot))
    for name, y, c, w in zip(("out", "d_self", "d_enc1", "d_enc2", "dW", "db"), got, same, want):
        err_same = float((c.double() - w).abs().max())
        err = float((y.double() - w).abs().max())
        print("gated_merge_train %s %s: composed form %.3e  fused node %.3e" % (str(dtype)[6:], name, err_same, err))
        # fp32 (not asked of the composed form's luck on 24 numbers, which can be a fraction of an ulp): at least 8 units in the last
        # place of the tensor's largest element -- six roundings of the chain and the K = 6 dot products of dW / dX
        floor = 8 * 2.0 ** -24 * float(w.abs().max()) if dtype == F32 else 0.0
        assert err <= max(2 * err_same, floor), (name, err, err_same)
    assert bool((got[0][1] == 0).all()) and bool((got[2][1] == 0).all()) and bool((got[3][1] == 0).all())
