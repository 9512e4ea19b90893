"""The lattice inputs of tests/msda_lattice.py, checked on the CPU: on every configuration tests/test_msda_exact_gpu.py uses,
the C oracle gives the SAME BITS in float32 and in float64 -- forward and all three gradients.  That is the proof that `==`
against the float64 oracle is the right expectation for a float32 kernel, whatever its summation order: a float32 sum that
is exact in one order and not in another would need a partial sum beyond 24 bits, and the magnitudes here stay far below
(the oracle walks rows, points and channels in the reference's order; the kernels walk them in theirs)."""
import numpy as np
import pytest

from oracle import msda as omsda
from tests import msda_lattice as ml


@pytest.mark.parametrize("name", sorted(ml.CONFIGS))
def test_oracle_f32_equals_f64_bit_for_bit(name):
    c = ml.case(name)
    out32 = omsda.msda_forward(*c.inputs(np.float32))
    assert out32.dtype == np.float32 and np.array_equal(out32.astype(np.float64), c.ref_forward())
    got = omsda.msda_backward(*c.inputs(np.float32), c.cot.astype(np.float32))
    for g32, g64 in zip(got, c.ref_backward()):
        assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g64)
    assert np.abs(c.ref_forward()).max() > 0 and all(np.abs(g).max() > 0 for g in c.ref_backward())


@pytest.mark.parametrize("name", sorted(ml.CONFIGS))
def test_every_special_coordinate_occurs_per_level_and_axis(name):
    c = ml.case(name)
    for l, (H, W) in enumerate(c.shapes.tolist()):
        x, y = ml.pixel_coords(c, l)
        step = 2 if c.coarse else 4
        assert np.array_equal(np.round(x * step), x * step) and np.array_equal(np.round(y * step), y * step)  # on the lattice
        for s in ml.specials(W, c.coarse):
            assert (x == s).any(), (name, l, "x", s)
        for s in ml.specials(H, c.coarse):
            assert (y == s).any(), (name, l, "y", s)
    if c.nrows > 1:  # the one-row case has 16 points for 18 coordinates: there the two axes share points
        assert min(ml.special_counts(c).values()) >= 1  # ... with the other axis live: the coordinate alone decides
    # inputs are what the header says: integers and halves, exact in bf16
    assert np.array_equal(c.value, np.round(c.value)) and np.abs(c.value).max() <= 4
    assert np.array_equal(c.cot, np.round(c.cot)) and np.abs(c.cot).max() <= (1 if c.coarse else 2)
    assert np.array_equal(2 * c.aw, np.round(2 * c.aw)) and np.abs(c.aw).max() <= (1 if c.coarse else 2)


@pytest.mark.parametrize("name", sorted(n for n, cfg in ml.CONFIGS.items() if cfg.get("coarse")))
def test_packed_configurations_stay_inside_bf16(name):
    """Packed-bf16 atomics round after every add: exact iff every partial sum fits 8 significant bits.  All terms are multiples
    of 1/4; a sum of magnitudes of at most 32 keeps every partial sum, in any order, a multiple of 1/4 below 64."""
    c = ml.case(name)
    absmap = omsda.msda_backward(c.value, c.shapes, c.lsi, c.loc, np.abs(c.aw), np.abs(c.cot))[0]
    assert absmap.max() == c.abs_sum_max <= 32.0
    assert np.array_equal(absmap * 4, np.round(absmap * 4))
    gv = c.ref_backward()[0]
    assert np.array_equal(ml.to_bf16(gv).double().numpy(), gv)  # the expected map itself is a bf16 map


def test_branches_and_hot_cells_the_gpu_cases_rely_on():
    for name in ("d64_cluster", "pk_cluster"):
        merged, pairs = ml.merge_branches(ml.case(name))
        assert merged >= 8 and pairs >= 8, (name, merged, pairs)
    assert ml.merge_branches(ml.case("d64_lp8_p2")) == (0, 0) and ml.merge_branches(ml.case("pk_lp8_p2")) == (0, 0)
    assert ml.max_records_per_cell(ml.case("val_hot")) > 64      # runs cross the 32-record steps of msda_bwd_value twice
    assert ml.max_records_per_cell(ml.case("pk_lp16")) >= 24     # a few dozen packed adds into one cell
    rows = sorted({ml.case(n).nrows for n in ml.CONFIGS})
    assert set(rows) >= {1, 5, 15, 16, 17, 63, 65, 100}


def test_weight_split_case_is_exact_and_needs_every_term():
    c, want = ml.build_weight_split()
    for dtype in (np.float32, np.float64):
        gv = omsda.msda_backward(*c.inputs(dtype), c.cot.astype(dtype))[0]
        assert np.array_equal(gv.astype(np.float64), want)
    assert np.array_equal(ml.to_bf16(want).double().numpy(), want)  # +-2^k: the final rounding to bf16 changes nothing
    assert ml.max_records_per_cell(c) <= 8 and int(ml.corner_geometry(c)[1][0, :, 0].sum()) > 32  # one tile, > 32 records
    need_mid = need_lo = 0
    for a, d in ml.split_pairs():
        hi, mid, lo = ml.bf16_split3(a + d)
        assert hi + mid + lo == a + d
        hi0, mid0, lo0 = ml.bf16_split3(a)
        # what the pair leaves in the cell when a term is dropped: all three are needed somewhere
        need_mid += (hi - hi0) + (lo - lo0) != d
        need_lo += (hi - hi0) + (mid - mid0) != d
    assert need_mid >= 10 and need_lo >= 4
