"""grit_beam_step with forced words on the device: every check is bit-equality of all six outputs against the host statement of
the step (grit_amd/ops/beam.py: beam_step_forced_host, itself checked against a loop-per-candidate reference in
tests/test_beam_forced_cpu.py) on the same device tensors -- at both list lengths of stage 1, at the 320-candidate ceiling, with
duplicates, words in two sets, banned forced words, finished rows and empty sets, for a strided map and the ensemble mean; empty
sets against the constrained step; the limits; then the decode of the fixture-G15 model with forced words from a captured graph
against the eager loop on the host form."""

import pytest
import torch

from tests.helpers import BEAM_STEP_OUTPUTS, beam_step_raw, load, t
from tests.test_beam_forced_cpu import sets_for
from tests.test_sample_cpu import EOS, FEATS, decode, g15_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("sel_beam", "sel_word", "seq_logprob", "seq_mask", "picked", "met")


def assert_same(got, want, tag="", names=NAMES):
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, n)
        assert torch.equal(a, b), (tag, n)
        if a.dtype == torch.float32:  # signed zeros included (picked of a finished beam is logp * 0 = -0.0)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, n)


def state(B, beam, V, C, W, later, quantised, seed, n_maps=1, ld=None):
    """word log-probabilities (multiples of 2^-3 in a narrow range, so that scores tie exactly; or log_softmax(3 randn)), running
    scores, sets of words in [4, V) with padding (the last set of image 0 empty), and at a later step a mask, previous words and
    masks of met sets: row 1 of image 0 finished with every set met, row 0 of image 0 live with every set met, and all of the last
    image finished.  ld: the maps are views with that row stride."""
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
    fw = torch.randint(4, V, (B, C, W), device=DEV, generator=gen)
    fw[torch.rand(B, C, W, device=DEV, generator=gen) < 0.3] = -1
    fw[0, C - 1] = -1
    if not later:
        return maps, seq_lp, None, None, fw, None
    seq_mask = (torch.rand(B, cur, 1, device=DEV, generator=gen) > 0.25).float()
    prev = torch.where(torch.rand(B * cur, 1, device=DEV, generator=gen) > 0.25, 9, EOS)
    met = torch.randint(0, 1 << C, (B, cur), device=DEV, generator=gen).int()
    seq_mask[0, 0], prev[0], met[0, 0] = 1.0, 9, (1 << C) - 1
    prev[1], met[0, 1] = EOS, (1 << C) - 1
    seq_mask[B - 1] = 0.0
    return maps, seq_lp, seq_mask, prev, fw, met


def check(maps, seq_lp, seq_mask, prev, fw, met, beam, hist=None, step=0, con=None, tag=""):
    from grit_amd.ops.beam import beam_step_forced, beam_step_forced_host
    got = beam_step_forced(maps, seq_lp, seq_mask, prev, EOS, beam, fw, met, hist, step, con)
    assert got is not None, tag
    mean = maps[0] if len(maps) == 1 else torch.mean(torch.stack(maps), 0)
    want = beam_step_forced_host(mean, seq_lp, seq_mask, prev, EOS, beam, fw, met, hist, step, con)
    assert_same(got, want, tag)
    return got


# ---------------------------------------------------------------------------------------------------------------- the step
# (B, beam, V): both list lengths of stage 1 (beam <= 5 and above), the widest beam, V that is and is not a multiple of 4, slices that
# are empty at the first step (V 9 and 40 over eight parts), the real vocabulary
SHAPES = [(3, 5, 1003), (2, 6, 257), (2, 8, 40), (2, 2, 9), (2, 5, 10201)]


@pytest.mark.parametrize("B,beam,V", SHAPES)
def test_step_equals_the_host_form(B, beam, V):
    ties = 0
    for C in (1, 3, 8):
        for W in (1, 4):
            for later in (False, True):
                for quantised in (True, False):
                    tag = (C, W, later, quantised)
                    args = state(B, beam, V, C, W, later, quantised, 1000 * beam + V + 10 * C + W + later)
                    sel_beam, sel_word, new_lp, new_mask, _, new_met = check(*args, beam, tag=tag)
                    assert ((sel_word >= 0) & (sel_word < V)).all() and ((sel_beam >= 0) & (sel_beam < (beam if later else 1))).all()
                    live, full = new_mask.squeeze(-1) != 0, new_met == (1 << C) - 1
                    assert not ((sel_word == EOS) & live & ~full).any(), tag  # <eos> only from rows that owe nothing
                    if later:
                        assert (new_mask[B - 1] == 0).all()  # the image whose rows are all finished
                    if quantised:
                        ties += int((new_lp[:, 1:] == new_lp[:, :-1]).sum())
    print("equal neighbouring scores among the chosen: %d" % ties)


def test_strided_rows():
    """rows V + 1 floats apart: three rows of four start off a 16-byte boundary and are read word by word, in both stages"""
    B, beam, V = 2, 6, 1003
    for later in (False, True):
        for quantised in (True, False):
            maps, *rest = state(B, beam, V, 3, 4, later, quantised, 5 + later, ld=V + 1)
            assert maps[0].stride(-2) == V + 1 and not maps[0].is_contiguous()
            got = check(maps, *rest, beam, tag=(later, quantised))
            assert_same(got, check([maps[0].contiguous()], *rest, beam))


def test_mean_of_three_maps():
    for B, beam, V in ((2, 6, 1003), (2, 5, 10201)):
        for later in (False, True):
            for quantised in (True, False):
                args = state(B, beam, V, 3, 4, later, quantised, 41 + later, n_maps=3)
                check(*args, beam, tag=(V, later, quantised))


def test_forced_words_among_the_best_are_kept_once():
    """the forced words are every row's best candidates: A and F hold the same (row, word) and the step keeps one of them"""
    for beam, V in ((5, 1003), (8, 40)):
        for later in (False, True):
            maps, seq_lp, seq_mask, prev, fw, met = state(2, beam, V, 3, 4, later, True, 7 + later)
            for w in fw[fw >= 0].unique().tolist():
                maps[0][:, :, w] += 6.0
            sel_beam, sel_word, *_ = check(maps, seq_lp, seq_mask, prev, fw, met, beam, tag=(beam, later))
            pairs = (sel_beam * V + sel_word).tolist()
            assert all(len(set(row)) == beam for row in pairs[:1])  # (the last image of a later step is all finished rows)


def test_one_word_in_two_sets():
    """word 5 is in sets 0 and 2: choosing it jumps two banks"""
    B, beam, V = 2, 5, 257
    for later in (False, True):
        maps, seq_lp, seq_mask, prev, fw, met = state(B, beam, V, 3, 4, later, True, 11 + later)
        fw[:] = torch.tensor([[5, 10, -1, -1], [6, 7, -1, -1], [11, 5, -1, -1]], device=DEV)
        if later:
            met[:] = 0
        _, sel_word, _, new_mask, _, new_met = check(maps, seq_lp, seq_mask, prev, fw, met, beam, tag=later)
        assert sel_word[0, 0] == 5 and new_met[0, 0] == 5 and new_mask[0, 0] == 1  # the top bank's best takes the first slot


def test_under_constraints():
    """min_len, no_repeat_ngram, no_repeat_word and suppress at t = 3 on histories over few words: a forced word that is suppressed,
    one that the n-gram rule bans for the rows whose history has it, and the words of the histories as the best candidates"""
    from grit_amd.ops.beam import constraints
    B, beam, V, step = 3, 6, 1003, 3
    gen = torch.Generator(device=DEV).manual_seed(3)
    for ngram in (1, 2, 3):
        con = constraints(V, min_len=5, no_repeat_ngram=ngram, no_repeat_word=True, suppress=(0, 501))
        for quantised in (True, False):
            maps, seq_lp, seq_mask, _, fw, met = state(B, beam, V, 3, 4, True, quantised, 31 + quantised)
            hist = torch.randint(4, 8, (B, beam, step), device=DEV, generator=gen)
            hist[:, 1, -1] = EOS  # row 1 of every image has finished
            prev = hist[:, :, -1].reshape(-1, 1).contiguous()
            fw[:, 0, 0], fw[:, 1, 0], fw[:, 2, 1] = 501, 5, hist[:, 0, 1]
            met[:, 2:] = 0
            maps[0][:, :, 4:8] += 6.0
            _, sel_word, new_lp, new_mask, _, _ = check(maps, seq_lp, seq_mask, prev, fw, met, beam, hist, step, con, tag=(ngram, quantised))
            live = new_mask.squeeze(-1) != 0
            assert not set(sel_word[live].tolist()) & {0, 501, EOS} and torch.isfinite(new_lp).all()
        first = state(B, beam, V, 3, 4, False, True, 33)
        check(*first, beam, None, 0, con, tag="first")


def test_the_candidate_ceiling():
    """beam 8, 8 sets of 4 disjoint words, nothing met: 8 x (8 + 32) = 320 candidates of an image, every one of them valid"""
    B, beam, V = 2, 8, 257
    for quantised in (True, False):
        maps, seq_lp, seq_mask, prev, fw, met = state(B, beam, V, 8, 4, True, quantised, 91)
        fw[:] = (torch.arange(32, device=DEV) * 7 + 20).view(8, 4)
        seq_mask[:], prev[:], met[:] = 1.0, 9, 0
        maps[0][:, :, :20] += 4.0  # the rows' best are no forced words
        _, sel_word, _, _, _, new_met = check(maps, seq_lp, seq_mask, prev, fw, met, beam, tag=quantised)
        assert (new_met[:, 0] != 0).all() and (new_met[:, 1] == 0).all()  # bank 1's best, then bank 0's
        first = state(B, beam, V, 8, 4, False, quantised, 92)
        check(*first, beam, tag=("first", quantised))


def test_forced_words_nearly_exhaust_the_vocabulary():
    """V 9, beam 2: the sets hold every word from 4 on, <eos> is banned, and -inf candidates take slots through bank -1"""
    from grit_amd.ops.beam import constraints
    B, beam, V = 2, 2, 9
    con = constraints(V, suppress=(0, 1, 2, 4, 5))
    for later in (False, True):
        maps, seq_lp, seq_mask, prev, fw, met = state(B, beam, V, 3, 4, later, True, 17 + later)
        fw[:] = torch.tensor([[4, 5, 6, -1], [7, 8, -1, -1], [-1, 6, 4, 8]], device=DEV)
        hist = torch.full((B, beam, 2), 9, device=DEV) if later else None
        check(maps, seq_lp, seq_mask, prev, fw, met, beam, hist, 2 if later else 0, con, tag=later)
        check(maps, seq_lp, seq_mask, prev, fw, met, beam, tag=(later, "free"))


def test_two_calls_give_the_same_bits():
    from grit_amd.ops.beam import beam_step_forced
    args = state(3, 6, 1003, 3, 4, True, True, 51)
    assert_same(beam_step_forced(*args[:4], EOS, 6, *args[4:]), beam_step_forced(*args[:4], EOS, 6, *args[4:]))


@pytest.mark.parametrize("B,beam,V", [(3, 5, 10201), (2, 8, 257), (2, 6, 64)])
def test_empty_sets_are_the_constrained_step(B, beam, V):
    """every set empty, and one live row per image so that the constrained step has no -999 candidate to select: the first five
    outputs are those of the constrained step and of the plain step"""
    from grit_amd.ops.beam import beam_step, beam_step_con, beam_step_forced, constraints
    con = constraints(V, min_len=5, no_repeat_ngram=2, no_repeat_word=True, suppress=(0, 5))
    gen = torch.Generator(device=DEV).manual_seed(V)
    for later in (False, True):
        for quantised in (True, False):
            maps, seq_lp, seq_mask, prev, fw, met = state(B, beam, V, 3, 4, later, quantised, 61 + later, n_maps=2)
            fw[:] = -1
            hist = None
            if later:
                hist = torch.randint(6, 10, (B, beam, 3), device=DEV, generator=gen)
                seq_mask[:, 0], prev[0::beam], met[:] = 1.0, 9, 7
            step = 3 if later else 0
            rest = (seq_lp, seq_mask, prev, EOS, beam)
            got = beam_step_forced(maps[:1], *rest, fw, met)
            assert_same(got[:5], beam_step(maps[0], *rest), (later, quantised), NAMES[:5])
            assert (got[5] == 7).all()
            for m in (maps[:1], maps):
                got = beam_step_forced(m, *rest, fw, met, hist, step, con)
                assert_same(got[:5], beam_step_con(m, *rest, hist, step, con), (later, quantised, len(m)), NAMES[:5])


def test_outside_the_limits_nothing_is_launched(monkeypatch):
    """a beam of 9, fewer words than beams, 9 sets, 5 words a set and a constrained step past t = 64: None, for the caller to take
    the host form"""
    from grit_amd import lib
    from grit_amd.ops import beam as beam_ops
    con = beam_ops.constraints(1003, no_repeat_ngram=2)
    wide = state(2, 9, 1003, 3, 4, True, True, 71)
    small = state(2, 6, 5, 3, 4, True, True, 72)
    late = state(2, 6, 1003, 3, 4, True, True, 73)
    sets = state(2, 6, 1003, 9, 4, True, True, 74)
    words = state(2, 6, 1003, 3, 5, True, True, 75)
    hist = torch.randint(4, 8, (2, 6, 65), device=DEV)
    L = lib.load()
    # the library itself refuses them without touching the outputs ...
    out = [torch.full((2, 9), -7, dtype=torch.int64, device=DEV), torch.full((2, 9), -7, dtype=torch.int64, device=DEV)] + \
        [torch.full((2, 9, 1), -7.0, device=DEV) for _ in range(3)] + [torch.full((2, 9), -7, dtype=torch.int32, device=DEV)]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    for (maps, seq_lp, seq_mask, prev, fw, met), beam, V, step, ngram in ((wide, 9, 1003, 0, 0), (small, 6, 5, 0, 0), (late, 6, 1003, 65, 2),
                                                                         (sets, 6, 1003, 0, 0), (words, 6, 1003, 0, 0)):
        st = beam_step_raw(maps=maps[:1], ld=V, seq_logprob=seq_lp, seq_mask=seq_mask, prev_words=prev, eos=EOS, first_step=0, B=2,
                           cur_beam=beam, V=V, k=beam, force_words=fw, n_sets=fw.shape[1], n_words=fw.shape[2], met_in=met,
                           history=hist, history_ld=65, t=step, no_repeat_ngram=ngram, suppress=[0], n_suppress=0, workspace=ws,
                           workspace_bytes=ws.numel(), **dict(zip(BEAM_STEP_OUTPUTS, out)))
        assert st == lib.ERR_UNSUPPORTED and all((o == -7).all() for o in out), (beam, V, step, tuple(fw.shape))
    # ... and the wrapper does not even call it
    monkeypatch.setattr(lib, "load", lambda: pytest.fail("the library was called"))
    assert beam_ops.beam_step_forced(*wide[:4], EOS, 9, *wide[4:]) is None
    assert beam_ops.beam_step_forced(*small[:4], EOS, 6, *small[4:]) is None
    assert beam_ops.beam_step_forced(*late[:4], EOS, 6, *late[4:], hist, 65, con) is None
    assert beam_ops.beam_step_forced(*sets[:4], EOS, 6, *sets[4:]) is None
    assert beam_ops.beam_step_forced(*words[:4], EOS, 6, *words[4:]) is None
    with torch.no_grad():
        assert not beam_ops.supported_forced(wide[0], 9, 9) and not beam_ops.supported_forced(small[0], 6, 6)
        assert beam_ops.supported_forced(late[0], 6, 6)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def g15_device():
    model, _ = g15_model(DEV)
    g = load("beam_g15.npz")
    vis = {k: t(g[k], device=DEV) for k in FEATS}
    base, _ = decode(model, vis, beam_size=5, out_size=5)
    model._decode_graphs.clear()
    return model, vis, base


def run(model, vis, **kw):
    if hasattr(model, "models"):  # an Ensemble reads a dict as features
        with torch.no_grad():
            return model(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)
    return decode(model, vis, **kw)


def holds_every_set(tokens, fw):
    for b in range(tokens.shape[0]):
        caption = tokens[b].tolist()
        words = set(caption[:caption.index(EOS)] if EOS in caption else caption)
        if not all(words & set(w for w in fw[b, c].tolist() if w >= 0) for c in range(fw.shape[1])):
            return False
    return True


def check_decode(model, vis, base, monkeypatch):
    """graph (captured, then replayed) == eager loop on the host form, bit for bit; other words of the same shape replay the same
    graph and give their own result; where the kernel does not apply (17 suppress ids) the eager loop takes the host form"""
    import grit_amd.models.caption.transformer as T
    from grit_amd.ops import beam as beam_ops
    model._decode_graphs.clear()
    fw = sets_for(model.models[0] if hasattr(model, "models") else model, base.cpu(), 3).to(DEV)
    other = fw.flip(0).contiguous()
    searches = (dict(beam_size=5, out_size=5, force_words=fw), dict(beam_size=5, out_size=5, force_words=other),
                dict(beam_size=6, out_size=6, force_words=fw[:, :1], no_repeat_ngram=2, length_penalty=1.0))
    graphed = []
    for kw, graphs in zip(searches, (1, 1, 2)):
        captured = run(model, vis, **kw)
        replayed = run(model, vis, **kw)
        assert len(model._decode_graphs) == graphs
        assert torch.equal(captured[0], replayed[0]) and torch.equal(captured[1], replayed[1])
        graphed.append(captured)
    again = run(model, vis, **searches[0])  # back to the first words on the graph that last ran the others
    assert len(model._decode_graphs) == 2 and torch.equal(again[0], graphed[0][0]) and torch.equal(again[1], graphed[0][1])
    assert not torch.equal(graphed[0][0], graphed[1][0])
    assert holds_every_set(graphed[0][0][:, 0], fw) and holds_every_set(graphed[1][0][:, 0], other)
    monkeypatch.setattr(T, "_GRAPH_DECODE", False)
    refused, step = [], beam_ops.beam_step_forced
    monkeypatch.setattr(beam_ops, "beam_step_forced", lambda *a, **kw: refused.append(step(*a, **kw)) or refused[-1])
    free = sorted(set(range(4, 400)) - set(fw.flatten().tolist()))[:17]
    beyond = dict(beam_size=5, out_size=1, force_words=fw, suppress=tuple(free))
    fallback = run(model, vis, **beyond)
    assert len(refused) == 20 and all(r is None for r in refused)
    monkeypatch.setattr(T, "_FUSED_BEAM_STEP", False)
    for kw, got in zip(searches, graphed):
        host = run(model, vis, **kw)
        assert torch.equal(got[0], host[0]) and torch.equal(got[1], host[1]), kw
        assert torch.isfinite(got[1]).all()
    host = run(model, vis, **beyond)
    assert len(refused) == 20 and torch.equal(fallback[0], host[0]) and torch.equal(fallback[1], host[1])
    assert holds_every_set(fallback[0], fw)
    model._decode_graphs.clear()


def test_forced_decode_of_the_model(g15_device, monkeypatch):
    model, vis, base = g15_device
    check_decode(model, vis, base, monkeypatch)


def test_forced_decode_of_an_ensemble(g15_device, monkeypatch):
    import copy
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis, base = g15_device
    twin = copy.deepcopy(model)
    with torch.no_grad():
        twin.cap_generator.fc.weight.mul_(0.8)
    check_decode(Ensemble([model, twin], config=model.config).eval(), vis, base, monkeypatch)
    assert not model._decode_graphs and not twin._decode_graphs
