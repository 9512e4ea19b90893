"""grit_beam_step with beam groups on the device: every check is bit-equality of all five outputs against the host statement of
the grouped step (grit_amd/ops/beam.py: beam_step_groups_host, itself checked against a loop-per-candidate reference in
tests/test_beam_groups_cpu.py) on the same device tensors -- at both list lengths of stage 1, at the 128-candidate ceiling, on the
scalar and the 16-byte load path, with slices that are empty at the first step, under constraints and for the ensemble mean; one
group against the plain and the constrained step; the limits; then the grouped decode of the fixture-G15 model from a captured
graph against the eager loop on the host form."""
import copy

import pytest
import torch

from tests.helpers import BEAM_STEP_OUTPUTS, beam_step_raw, load, t
from tests.test_sample_cpu import EOS, FEATS, decode, g15_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("sel_beam", "sel_word", "seq_logprob", "seq_mask", "picked")
LAMBDAS = (0.0, 0.5, 1e4)


def assert_same(got, want, tag=""):
    for n, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape, (tag, n)
        assert torch.equal(a, b), (tag, n)
        if a.dtype == torch.float32:  # signed zeros included (picked of a finished beam is logp * 0 = -0.0)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, n)


def state(B, beam, G, V, later, quantised, seed, n_maps=1, ld=None):
    """word log-probabilities (multiples of 2^-3 in a narrow range, so that penalised scores tie exactly; or log_softmax(3 randn)),
    running scores, and at a later step a mask and previous words with finished rows: group 0 of image 0 whole, and all of the last
    image when there is more than one.  ld: the maps are views with that row stride."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    cur = beam if later else 1
    maps = []
    for _ in range(n_maps):
        if quantised:
            m = -torch.randint(0, 16, (B, cur, V), device=DEV, generator=gen).float() / 8
        else:
            m = torch.log_softmax(3 * torch.randn(B, cur, V, device=DEV, generator=gen), -1)
        if ld is not None:
            wide = torch.zeros(B, cur, ld, device=DEV)
            wide[:, :, :V] = m
            m = wide[:, :, :V]
        maps.append(m)
    if quantised:
        seq_lp = -torch.randint(0, 8, (B, cur, 1), device=DEV, generator=gen).float() / 8
    else:
        seq_lp = -torch.rand(B, cur, 1, device=DEV, generator=gen) * 2
    if not later:
        return maps, seq_lp, None, None
    seq_mask = (torch.rand(B, cur, 1, device=DEV, generator=gen) > 0.25).float()
    prev = torch.where(torch.rand(B * cur, 1, device=DEV, generator=gen) > 0.25, 9, EOS)
    prev[:beam // G] = EOS
    if B > 1:
        seq_mask[B - 1] = 0.0
    return maps, seq_lp, seq_mask, prev


def check(maps, seq_lp, seq_mask, prev, beam, G, lam, hist=None, step=0, con=None, tag=""):
    from grit_amd.ops.beam import beam_step_div, beam_step_groups_host
    got = beam_step_div(maps, seq_lp, seq_mask, prev, EOS, beam, G, lam, hist, step, con)
    assert got is not None, tag
    mean = maps[0] if len(maps) == 1 else torch.mean(torch.stack(maps), 0)
    want = beam_step_groups_host(mean, seq_lp, seq_mask, prev, EOS, beam, G, lam, hist, step, con)
    assert_same(got, want, tag)
    return got


# ---------------------------------------------------------------------------------------------------------------- the step
# (B, beam, G, V): both list lengths of stage 1 (beam <= 5 and above), the 128-candidate ceiling (beam 8), V that is and is not a
# multiple of 4, slices that are empty at the first step (V 9 and 40 over eight parts), the real vocabulary
SHAPES = [(3, 6, 3, 1003), (2, 6, 2, 1003), (2, 6, 6, 64), (2, 5, 5, 10201), (2, 8, 8, 257), (2, 8, 4, 257), (1, 8, 2, 40), (2, 2, 2, 9)]


@pytest.mark.parametrize("B,beam,G,V", SHAPES)
def test_step_equals_the_host_form(B, beam, G, V):
    ties = 0
    for later in (False, True):
        for quantised in (True, False):
            args = state(B, beam, G, V, later, quantised, 1000 * beam + V + later)
            for lam in LAMBDAS:
                tag = (later, quantised, lam)
                sel_beam, sel_word, new_lp, new_mask, _ = check(*args, beam, G, lam, tag=tag)
                assert ((sel_word >= 0) & (sel_word < V)).all() and ((sel_beam >= 0) & (sel_beam < (beam if later else 1))).all()
                if later:
                    g = beam // G
                    assert (sel_beam // g == torch.arange(beam, device=DEV) // g).all(), tag  # beams never change group
                    assert (new_mask[0, :g] == 0).all() and (B == 1 or (new_mask[B - 1] == 0).all())
                elif lam == 1e4 and V >= beam * 2:
                    assert all(len(set(row)) == beam for row in sel_word.tolist()), tag  # every group found a fresh word
                if quantised and lam == 0.5:
                    ties += int((new_lp[:, 1:] == new_lp[:, :-1]).sum())
    print("equal neighbouring scores under the penalty 0.5: %d" % ties)


def test_unaligned_rows_take_the_scalar_path():
    """rows V + 1 floats apart: three rows of four start off a 16-byte boundary and are read word by word"""
    B, beam, G, V = 2, 6, 3, 1003
    for later in (False, True):
        for quantised in (True, False):
            maps, *rest = state(B, beam, G, V, later, quantised, 5 + later, ld=V + 1)
            assert maps[0].stride(-2) == V + 1 and not maps[0].is_contiguous()
            got = check(maps, *rest, beam, G, 0.5, tag=(later, quantised))
            assert_same(got, check([maps[0].contiguous()], *rest, beam, G, 0.5))


def test_under_constraints():
    """min_len, no_repeat_ngram 2, no_repeat_word and two suppress ids at t = 3, on histories over few words so that every live
    beam has bigrams to ban; the hot words are banned for some beams and penalised for others"""
    from grit_amd.ops.beam import constraints
    B, beam, G, V, step = 3, 6, 3, 1003, 3
    con = constraints(V, min_len=5, no_repeat_ngram=2, no_repeat_word=True, suppress=(0, 501))
    gen = torch.Generator(device=DEV).manual_seed(3)
    for quantised in (True, False):
        maps, seq_lp, seq_mask, _ = state(B, beam, G, V, True, quantised, 31 + quantised)
        hist = torch.randint(4, 8, (B, beam, step), device=DEV, generator=gen)
        hist[:, 0, -1] = EOS  # row 0 of every image has finished
        prev = hist[:, :, -1].reshape(-1, 1).contiguous()
        maps[0][:, :, 4:8] += 6.0  # the words of the histories are the best candidates
        for lam in LAMBDAS:
            _, sel_word, new_lp, new_mask, _ = check(maps, seq_lp, seq_mask, prev, beam, G, lam, hist, step, con, tag=(quantised, lam))
            live = new_mask.squeeze(-1) != 0
            assert not set(sel_word[live].tolist()) & {0, 501, EOS} and torch.isfinite(new_lp).all()
    first = state(B, beam, G, V, False, True, 33)
    check(*first, beam, G, 0.5, None, 0, con, tag="first")


def test_mean_of_two_maps():
    for B, beam, G, V in ((2, 6, 3, 1003), (2, 5, 5, 10201)):
        for later in (False, True):
            for quantised in (True, False):
                args = state(B, beam, G, V, later, quantised, 41 + later, n_maps=2)
                for lam in LAMBDAS:
                    check(*args, beam, G, lam, tag=(V, later, quantised, lam))


def test_two_calls_give_the_same_bits():
    from grit_amd.ops.beam import beam_step_div
    args = state(3, 6, 3, 1003, True, True, 51)
    a = beam_step_div(*args, EOS, 6, 3, 0.5)
    b = beam_step_div(*args, EOS, 6, 3, 0.5)
    assert_same(a, b)


@pytest.mark.parametrize("B,beam,V", [(3, 5, 10201), (2, 8, 257), (2, 6, 64), (2, 2, 9)])
def test_one_group_is_the_plain_step(B, beam, V):
    from grit_amd.ops.beam import beam_step, beam_step_con, beam_step_div, beam_step_mean, constraints
    con = constraints(V, min_len=5, no_repeat_ngram=2, no_repeat_word=True, suppress=(0, 5))
    gen = torch.Generator(device=DEV).manual_seed(V)
    for later in (False, True):
        for quantised in (True, False):
            maps, seq_lp, seq_mask, prev = state(B, beam, beam, V, later, quantised, 61 + later, n_maps=2)
            hist = torch.randint(4, 8, (B, beam, 3), device=DEV, generator=gen) if later else None
            step = 3 if later else 0
            rest = (seq_lp, seq_mask, prev, EOS, beam)
            for lam in (0.0, 0.5):
                assert_same(beam_step_div(maps[:1], *rest, 1, lam), beam_step(maps[0], *rest), (later, quantised, lam))
                assert_same(beam_step_div(maps, *rest, 1, lam), beam_step_mean(maps, *rest), (later, quantised, lam, "mean"))
                assert_same(beam_step_div(maps[:1], *rest, 1, lam, hist, step, con),
                            beam_step_con(maps[:1], *rest, hist, step, con), (later, quantised, lam, "bans"))


def test_outside_the_limits_nothing_is_launched(monkeypatch):
    """a beam of 9, fewer words than beams, and a constrained step past t = 64: None, for the caller to take the host form"""
    from grit_amd import lib
    from grit_amd.ops import beam as beam_ops
    con = beam_ops.constraints(1003, no_repeat_ngram=2)
    wide = state(2, 9, 3, 1003, True, True, 71)
    small = state(2, 6, 3, 5, True, True, 72)
    late = state(2, 6, 3, 1003, True, True, 73)
    hist = torch.randint(4, 8, (2, 6, 65), device=DEV)
    L = lib.load()
    # the library itself refuses them without touching the outputs ...
    out = [torch.full((2, 9), -7, dtype=torch.int64, device=DEV), torch.full((2, 9), -7, dtype=torch.int64, device=DEV)] + \
        [torch.full((2, 9, 1), -7.0, device=DEV) for _ in range(3)]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    for (maps, seq_lp, seq_mask, prev), beam, V, step, ngram in ((wide, 9, 1003, 0, 0), (small, 6, 5, 0, 0), (late, 6, 1003, 65, 2)):
        st = beam_step_raw(maps=maps[:1], ld=V, seq_logprob=seq_lp, seq_mask=seq_mask, prev_words=prev, eos=EOS, first_step=0, B=2,
                           cur_beam=beam, V=V, k=beam, groups=3, diversity=0.5, history=hist, history_ld=65, t=step,
                           no_repeat_ngram=ngram, suppress=[0], n_suppress=0, workspace=ws, workspace_bytes=ws.numel(),
                           **dict(zip(BEAM_STEP_OUTPUTS, out)))
        assert st == lib.ERR_UNSUPPORTED and all((o == -7).all() for o in out), (beam, V, step)
    # ... and the wrapper does not even call it
    monkeypatch.setattr(lib, "load", lambda: pytest.fail("the library was called"))
    assert beam_ops.beam_step_div(*wide, EOS, 9, 3, 0.5) is None
    assert beam_ops.beam_step_div(*small, EOS, 6, 3, 0.5) is None
    assert beam_ops.beam_step_div(*late, EOS, 6, 3, 0.5, hist, 65, con) is None
    with torch.no_grad():
        assert not beam_ops.supported_div(wide[0], 9, 9, 3) and not beam_ops.supported_div(small[0], 6, 6, 3)
        assert beam_ops.supported_div(late[0], 6, 6, 3) and not beam_ops.supported_div(late[0], 6, 6, 4)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def g15_device():
    model, _ = g15_model(DEV)
    g = load("beam_g15.npz")
    return model, {k: t(g[k], device=DEV) for k in FEATS}


def run(model, vis, **kw):
    if hasattr(model, "models"):  # an Ensemble reads a dict as features
        with torch.no_grad():
            return model(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)
    return decode(model, vis, **kw)


SEARCHES = (dict(beam_size=6, out_size=6, num_groups=3, diversity=0.5),
            dict(beam_size=5, out_size=5, num_groups=5, diversity=1.0, no_repeat_ngram=2, length_penalty=1.0))


def check_decode(model, vis, monkeypatch):
    """graph (captured, then replayed) == eager loop on the host form, bit for bit; one graph per search; one group is the plain
    graphed search"""
    import grit_amd.models.caption.transformer as T
    model._decode_graphs.clear()
    graphed = []
    for n, kw in enumerate(SEARCHES):
        captured = run(model, vis, **kw)
        replayed = run(model, vis, **kw)
        assert len(model._decode_graphs) == n + 1
        assert torch.equal(captured[0], replayed[0]) and torch.equal(captured[1], replayed[1])
        graphed.append(captured)
    plain = run(model, vis, beam_size=6, out_size=6)
    one = run(model, vis, beam_size=6, out_size=6, num_groups=1, diversity=0.5)
    assert len(model._decode_graphs) == 3  # one group is the plain search's graph
    assert torch.equal(one[0], plain[0]) and torch.equal(one[1], plain[1])
    assert not torch.equal(graphed[0][0], plain[0])
    monkeypatch.setattr(T, "_GRAPH_DECODE", False)
    monkeypatch.setattr(T, "_FUSED_BEAM_STEP", False)
    for kw, got in zip(SEARCHES, graphed):
        host = run(model, vis, **kw)
        assert torch.equal(got[0], host[0]) and torch.equal(got[1], host[1]), kw
        assert torch.isfinite(got[1]).all()
    assert len(model._decode_graphs) == 3
    model._decode_graphs.clear()


def test_grouped_decode_of_the_model(g15_device, monkeypatch):
    model, vis = g15_device
    check_decode(model, vis, monkeypatch)


def test_grouped_decode_of_an_ensemble(g15_device, monkeypatch):
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis = g15_device
    twin = copy.deepcopy(model)
    with torch.no_grad():
        twin.cap_generator.fc.weight.mul_(0.8)
    check_decode(Ensemble([model, twin], config=model.config).eval(), vis, monkeypatch)
    assert not model._decode_graphs and not twin._decode_graphs
