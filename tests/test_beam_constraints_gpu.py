"""grit_beam_step with its bans on the device: every check is bit-equality of all five outputs against the composed torch form on the
same device (the reference's step arithmetic, grit_amd/ops/beam.py: banned_words_host as one masked_fill(-inf), a stable descending
sort), at the slice boundaries, on the scalar load path, for the ensemble mean and at the limits; then the constrained decode of
the fixture-G15 model: fused step against composed step, graph replay against the eager loop, one graph per constraint tuple."""
import copy

import pytest
import torch

from tests.helpers import BEAM_STEP_OUTPUTS, beam_step_raw, load, t
from tests.test_beam_constraints_cpu import ALPHA, CASES, violations
from tests.test_sample_cpu import EOS, FEATS, decode, g15_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("sel_beam", "sel_word", "seq_logprob", "seq_mask", "picked")


def con(min_len=0, no_repeat_ngram=0, no_repeat_word=False, suppress=()):
    from grit_amd.ops.beam import Constraints
    return Constraints(min_len, no_repeat_ngram, no_repeat_word, tuple(suppress))  # also with every rule off


def composed(maps, seq_lp, seq_mask, prev, eos, beam, hist, step, c):
    """The reference's arithmetic op by op (models/caption/transformer.py:208-240, ensemble.py:128-162) with the bans."""
    from grit_amd.ops.beam import banned_words_host
    word_logprob = maps[0] if len(maps) == 1 else torch.mean(torch.stack(maps), 0)
    B, cur, V = word_logprob.shape
    first = prev is None
    candidates = seq_lp + word_logprob
    if not first:
        alive = (prev.view(B, cur) != eos).float().unsqueeze(-1)
        seq_mask = seq_mask * alive
        word_logprob = word_logprob * seq_mask
        frozen = seq_lp.expand_as(candidates).contiguous()
        frozen[:, :, 1:] = -999
        candidates = seq_mask * candidates + frozen * (1 - seq_mask)
    history = hist if hist is not None else torch.zeros((B, cur, 0), dtype=torch.long, device=DEV)
    banned = banned_words_host(history, None if first else seq_mask, step, eos, V, **c._asdict())
    candidates = candidates.masked_fill(banned, float("-inf"))
    sv, si = torch.sort(candidates.view(B, -1), dim=-1, descending=True, stable=True)
    sel_lp, sel_idx = sv[:, :beam], si[:, :beam]
    sel_beam = torch.div(sel_idx, V, rounding_mode="floor")
    sel_word = sel_idx - sel_beam * V
    col = sel_beam.unsqueeze(-1)
    new_mask = torch.ones(B, beam, 1, device=DEV) if first else torch.gather(seq_mask, 1, col)
    picked = torch.gather(torch.gather(word_logprob, 1, col.expand(B, beam, V)), 2, sel_word.unsqueeze(-1))
    return sel_beam, sel_word, sel_lp.unsqueeze(-1), new_mask, picked


def launch(maps, seq_lp, seq_mask, prev, eos, beam, hist, step, c, hist_ld=None):
    """grit_beam_step with the bans as the C ABI states it: maps [B, cur, V] with any row stride (rows evenly spaced, words adjacent).
    Returns the status and the five outputs."""
    from grit_amd import lib
    L = lib.load()
    B, cur, V = maps[0].shape
    for m in maps:
        assert m.stride(2) == 1 and m.stride(0) == cur * m.stride(1) and m.stride(1) == maps[0].stride(1)
    nbytes = L.grit_beam_step_workspace(B, cur, beam)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=DEV)
    out = [torch.full((B, beam), -7, dtype=torch.int64, device=DEV), torch.full((B, beam), -7, dtype=torch.int64, device=DEV),
           torch.full((B, beam, 1), -7.0, device=DEV), torch.full((B, beam, 1), -7.0, device=DEV),
           torch.full((B, beam, 1), -7.0, device=DEV)]
    first = prev is None
    slp = seq_lp.reshape(-1).contiguous()
    sm = None if first else seq_mask.reshape(-1).contiguous()
    pw = None if first else prev.reshape(-1).contiguous()
    if hist is not None:
        assert hist.dtype == torch.int64 and hist.stride(-1) == 1
        hist_ld = hist_ld or hist.stride(-2)
    st = beam_step_raw(maps=maps, ld=maps[0].stride(1), seq_logprob=slp, seq_mask=sm, prev_words=pw, eos=eos, first_step=int(first),
                       B=B, cur_beam=cur, V=V, k=beam, history=hist, history_ld=hist_ld or 0, t=step,
                       no_repeat_ngram=c.no_repeat_ngram, no_repeat_word=int(c.no_repeat_word), ban_eos=int(step < c.min_len),
                       suppress=c.suppress, workspace=ws, workspace_bytes=nbytes, **dict(zip(BEAM_STEP_OUTPUTS, out)))
    return st, tuple(out)


def assert_same(got, want, tag=""):
    for n, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape, (tag, n)
        assert torch.equal(a, b), (tag, n)
        if a.dtype == torch.float32:  # signed zeros included (picked of a finished beam is logp * 0 = -0.0)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, n)


def check(maps, seq_lp, seq_mask, prev, eos, beam, hist, step, c, tag=""):
    st, got = launch(maps, seq_lp, seq_mask, prev, eos, beam, hist, step, c)
    assert st == 0, (tag, st)
    want = composed(maps, seq_lp, seq_mask, prev, eos, beam, hist, step, c)
    assert_same(got, want, tag)
    return got


def state(B, cur, V, seed, hot=(), n_maps=1):
    """word log-probabilities with the words `hot` far above the rest, the first the most probable (so that banning them changes
    the selection), scores, a mask with every beam alive and previous words that are not <eos>"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    maps = []
    for _ in range(n_maps):
        logits = torch.randn(B, cur, V, device=DEV, generator=g) * 3
        for rank, w in enumerate(hot):
            logits[:, :, w] = 40 - rank
        maps.append(torch.log_softmax(logits, -1))
    seq_lp = -torch.rand(B, cur, 1, device=DEV, generator=g) * 2
    seq_mask = torch.ones(B, cur, 1, device=DEV)
    prev = torch.full((B * cur, 1), 9, dtype=torch.int64, device=DEV)
    return maps, seq_lp, seq_mask, prev


# ---------------------------------------------------------------------------------------------------------------- the step
V = 10201
EDGE = (0, 5103, 5104, 10200)  # two parts per beam row, seg = 5104: the last word of the first slice, the first of the second


@pytest.mark.parametrize("n", [2, 3])
def test_bans_on_both_sides_of_the_slice_boundary(n):
    B, cur, beam, step = 3, 5, 5, 12
    maps, seq_lp, seq_mask, prev = state(B, cur, V, 100 + n, hot=EDGE)
    if n == 2:  # 7 was followed by all four edge words
        rows = [[7, 0, 7, 5103, 7, 5104, 7, 10200, 9, 9, 8, 7],
                [7, 10200, 7, 5104, 4, 5, 6, 8, 9, 10, 11, 7]]
    else:       # (6, 7) was followed by three of them, or by the two at the boundary
        rows = [[6, 7, 0, 6, 7, 5103, 6, 7, 10200, 5, 6, 7],
                [6, 7, 5104, 6, 7, 5103, 11, 12, 13, 14, 6, 7]]
    hist = torch.tensor([rows[0], rows[1], rows[0], rows[1], rows[0]], device=DEV).expand(B, cur, step).contiguous()
    prev = hist[:, :, -1].reshape(-1, 1).contiguous()
    prev[4::cur] = EOS       # beam 4 of every image has finished (its history bans nothing) ...
    seq_lp[:, 4] = 0.5       # ... and scores above every live candidate: it survives through word 0
    c = con(no_repeat_ngram=n, suppress=(0, 1, 2))
    sel_beam, sel_word, _, new_mask, _ = check(maps, seq_lp, seq_mask, prev, EOS, beam, hist, step, c, "n=%d" % n)
    assert (sel_beam[:, 0] == 4).all() and (sel_word[:, 0] == 0).all() and (new_mask[:, 0] == 0).all()
    live = sel_beam != 4
    assert (sel_word[live] > 2).all()  # word 0 is banned for the live beams
    for b in range(B):
        for j, w in zip(sel_beam[b].tolist(), sel_word[b].tolist()):
            assert j == 4 or not violations(hist[b, j].tolist() + [w], no_repeat_ngram=n), (b, j, w)
    # the bans decide: the same step without them picks the edge words, word 0 of the best live beam first
    _, plain = launch(maps, seq_lp, seq_mask, prev, EOS, beam, hist, step, con())
    assert (plain[1][:, 1] == 0).all() and set(plain[1].flatten().tolist()) <= set(EDGE)


def test_first_step_eight_parts():
    """cur_beam 1: eight parts of seg = 1276 words; <eos> banned by the minimum length, suppress ids on both sides of a boundary"""
    B, beam = 3, 5
    hot = (EOS, 1275, 1276, 1277, 5000, 7000, 9000, 10200)
    maps, seq_lp, _, _ = state(B, 1, V, 7, hot=hot)
    seq_lp.zero_()
    c = con(min_len=4, suppress=(1275, 1276))
    _, sel_word, _, _, _ = check(maps, seq_lp, None, None, EOS, beam, None, 0, c)
    assert sel_word.tolist() == [[1277, 5000, 7000, 9000, 10200]] * B
    _, plain = launch(maps, seq_lp, None, None, EOS, beam, None, 0, con())
    assert plain[1].tolist() == [[EOS, 1275, 1276, 1277, 5000]] * B


def test_small_vocabulary_selects_banned_candidates():
    """V 13, k 8 at the first step: seg = 4, the slices of parts 4 - 7 are empty; six suppressed words leave seven finite
    candidates, so the eighth is a banned one (-inf, by index).  Word 0 is among the suppressed ones: the composed form's
    `mask * candidates + frozen * (1 - mask)` turns a running score of -inf into NaN at word 0 (-inf * 0), which the ban covers.
    Then the next step, cur_beam 8, from that state."""
    B, Vs, beam = 2, 13, 8
    sup = (0, 2, 5, 6, 11, 12)
    maps, seq_lp, _, _ = state(B, 1, Vs, 13)
    seq_lp.zero_()
    c = con(suppress=sup)
    sel_beam, sel_word, new_lp, new_mask, _ = check(maps, seq_lp, None, None, EOS, beam, None, 0, c, "first")
    assert ((sel_word >= 0) & (sel_word < Vs)).all() and (sel_beam == 0).all()
    assert (sel_word[:, 7] == 0).all() and (new_lp[:, 7] == float("-inf")).all() and torch.isfinite(new_lp[:, :7]).all()
    nxt, _, _, _ = state(B, beam, Vs, 14)
    c = con(suppress=sup, no_repeat_word=True)
    hist = sel_word.view(B, beam, 1).contiguous()
    got = check(nxt, new_lp, new_mask, sel_word.view(-1, 1), EOS, beam, hist, 1, c, "second")
    assert ((got[1] >= 0) & (got[1] < Vs)).all() and ((got[0] >= 0) & (got[0] < beam)).all()


def test_unaligned_rows_take_the_scalar_path():
    """rows 10203 floats apart, the first 12 bytes past a 16-byte boundary: most rows are read word by word, every fourth in fours"""
    B, cur, beam, step, ld = 2, 5, 5, 4, 10203
    maps, seq_lp, seq_mask, prev = state(B, cur, V, 21, hot=EDGE)
    flat = torch.zeros(B * cur * ld + 3, device=DEV)
    rows = flat[3:].view(B, cur, ld)[:, :, :V]
    rows.copy_(maps[0])
    assert rows.data_ptr() % 16 == 12 and rows.stride(1) == ld
    hist = torch.tensor([8, 5103, 8, 10200], device=DEV).expand(B, cur, step).contiguous()
    hist[:, 1] = torch.tensor([8, 0, 8, 5104], device=DEV)
    c = con(no_repeat_ngram=1, suppress=(1,))
    got = check([rows], seq_lp, seq_mask, prev, EOS, beam, hist, step, c)
    _, same = launch(maps, seq_lp, seq_mask, prev, EOS, beam, hist, step, c)
    assert_same(got, same)


def test_mean_of_three_maps():
    B, cur, beam, step = 3, 5, 5, 7
    maps, seq_lp, seq_mask, prev = state(B, cur, V, 31, hot=EDGE, n_maps=3)
    hist = torch.tensor([7, 0, 7, 5103, 7, 5104, 7], device=DEV).expand(B, cur, step).contiguous()
    prev[2::cur] = EOS
    c = con(no_repeat_ngram=2, no_repeat_word=True, min_len=9, suppress=(10200,))
    _, sel_word, _, _, _ = check(maps, seq_lp, seq_mask, prev, EOS, beam, hist, step, c)
    assert not set(sel_word.flatten().tolist()) & {5103, 5104, 10200}
    first_maps, first_lp, _, _ = state(B, 1, V, 32, hot=EDGE, n_maps=3)
    check(first_maps, first_lp.zero_(), None, None, EOS, beam, None, 0, c, "first")


def test_history_lengths_at_the_limits():
    from grit_amd import lib
    from grit_amd.ops import beam as beam_ops
    B, cur, beam = 2, 5, 5
    maps, seq_lp, seq_mask, prev = state(B, cur, V, 41, hot=(40, 41, 42, 43))
    g = torch.Generator(device=DEV).manual_seed(41)
    long = torch.randint(40, 44, (B, cur, 65), device=DEV, generator=g)
    # t = 1 with n = 2: a single word has no bigram yet
    one = long[:, :, :1].contiguous()
    got = check(maps, seq_lp, seq_mask, prev, EOS, beam, one, 1, con(no_repeat_ngram=2), "t=1")
    assert_same(got, launch(maps, seq_lp, seq_mask, prev, EOS, beam, one, 1, con())[1])
    # t = 64, the longest history, as rows of a longer tensor (row stride 65)
    for n in (1, 2, 3, 64, 65):
        check(maps, seq_lp, seq_mask, prev, EOS, beam, long[:, :, :64], 64, con(no_repeat_ngram=n, no_repeat_word=True), "t=64 n=%d" % n)
    # t = 65: outside the kernel, nothing is written; the wrapper says so and the search takes the composed form
    st, out = launch(maps, seq_lp, seq_mask, prev, EOS, beam, long, 65, con(no_repeat_ngram=2))
    assert st == lib.ERR_UNSUPPORTED and all((o == -7).all() for o in out)
    assert beam_ops.beam_step_con(maps, seq_lp, seq_mask, prev, EOS, beam, long, 65, con(no_repeat_ngram=2)) is None
    st, out = launch(maps, seq_lp, seq_mask, prev, EOS, beam, one, 1, con(suppress=range(17)))
    assert st == lib.ERR_UNSUPPORTED and all((o == -7).all() for o in out)
    assert beam_ops.beam_step_con(maps, seq_lp, seq_mask, prev, EOS, beam, one, 1, con(suppress=range(17))) is None
    # and the wrapper inside the limits is the raw call
    c = con(no_repeat_ngram=2, suppress=range(16), min_len=70)
    assert_same(beam_ops.beam_step_con(maps, seq_lp, seq_mask, prev, EOS, beam, long[:, :, :64], 64, c),
                composed(maps, seq_lp, seq_mask, prev, EOS, beam, long[:, :, :64], 64, c))


def test_bad_arguments_write_nothing():
    from grit_amd import lib
    maps, seq_lp, seq_mask, prev = state(2, 5, 100, 51)
    hist = torch.zeros((2, 5, 3), dtype=torch.int64, device=DEV)
    for c, kw in ((con(suppress=(100,)), {}), (con(suppress=(-1,)), {}), (con(no_repeat_ngram=-1), {}),
                  (con(no_repeat_word=True), dict(hist_ld=2))):  # a live rule: with none, t and history are not read
        st, out = launch(maps, seq_lp, seq_mask, prev, EOS, 5, hist, 3, c, **kw)
        assert st == lib.ERR_BAD_ARG and all((o == -7).all() for o in out), c
    st, out = launch(maps, seq_lp, seq_mask, prev, EOS, 5, None, 3, con(no_repeat_ngram=2))
    assert st == lib.ERR_BAD_ARG and all((o == -7).all() for o in out)
    st, out = launch(maps, seq_lp, seq_mask, prev, 100, 5, hist, 3, con(min_len=9))  # <eos> outside the vocabulary cannot be banned
    assert st == lib.ERR_BAD_ARG and all((o == -7).all() for o in out)


def test_history_words_outside_the_vocabulary():
    B, cur, beam, step = 2, 5, 5, 6
    maps, seq_lp, seq_mask, prev = state(B, cur, V, 61, hot=EDGE)
    hist = torch.tensor([-1, 5103, V, 5104, -1, V], device=DEV).expand(B, cur, step).contiguous()
    hist[:, 1] = torch.tensor([V, 0, -1, 10200, 7, -1], device=DEV)    # (-1) was followed by 10200: banned; -1 itself bans nothing
    hist[:, 2] = torch.tensor([1 << 40, 0, 5, 5, -(1 << 40), 1 << 40], device=DEV)  # 64-bit words are compared as such
    for c in (con(no_repeat_ngram=1, no_repeat_word=True), con(no_repeat_ngram=2, no_repeat_word=True), con(no_repeat_ngram=3)):
        got = check(maps, seq_lp, seq_mask, prev, EOS, beam, hist, step, c, str(c))
        assert ((got[1] >= 0) & (got[1] < V)).all()


@pytest.mark.parametrize("B,cur,Vs,beam", [(64, 5, 10201, 5), (3, 1, 10201, 5), (5, 8, 1031, 8), (4, 2, 6, 4)])
def test_everything_off_equals_the_plain_step(B, cur, Vs, beam):
    from grit_amd.ops.beam import beam_step, beam_step_mean
    first = cur == 1
    for n_maps in (1, 3):
        maps, seq_lp, seq_mask, prev = state(B, cur, Vs, B + cur + n_maps, n_maps=n_maps)
        g = torch.Generator(device=DEV).manual_seed(B)
        seq_mask = (torch.rand(B, cur, 1, device=DEV, generator=g) > 0.3).float()
        prev = torch.randint(0, 6, (B * cur, 1), device=DEV, generator=g)
        hist = torch.randint(0, Vs, (B, cur, 3), device=DEV, generator=g)
        args = (seq_lp, None if first else seq_mask, None if first else prev, EOS, beam)
        st, got = launch(maps, *args, None if first else hist, 0 if first else 3, con())
        assert st == 0
        want = beam_step(maps[0], *args) if n_maps == 1 else beam_step_mean(maps, *args)
        assert_same(got, want, "%d maps" % n_maps)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def g15_device():
    model, _ = g15_model(DEV)
    g = load("beam_g15.npz")
    return model, {k: t(g[k], device=DEV) for k in FEATS}


def run(model, vis, **kw):
    if hasattr(model, "models"):  # an Ensemble reads a dict as features
        with torch.no_grad():
            return model(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=5, out_size=5, **kw)
    return decode(model, vis, beam_size=5, out_size=5, **kw)


def check_decode(model, vis, monkeypatch):
    """graph (captured, then replayed) == eager loop with the fused step == eager loop with the composed step, bit for bit; a
    second constraint tuple and a tuple beyond the kernel's limits get graphs of their own"""
    import grit_amd.models.caption.transformer as T
    model._decode_graphs.clear()
    kw = dict(CASES["all"], length_penalty=ALPHA)
    captured = run(model, vis, **kw)
    replayed = run(model, vis, **kw)
    assert len(model._decode_graphs) == 1
    monkeypatch.setattr(T, "_GRAPH_DECODE", False)
    fused = run(model, vis, **kw)
    plain = run(model, vis)
    monkeypatch.setattr(T, "_FUSED_BEAM_STEP", False)
    host = run(model, vis, **kw)
    for other in (replayed, fused, host):
        assert torch.equal(captured[0], other[0]) and torch.equal(captured[1], other[1])
    assert len(model._decode_graphs) == 1 and not torch.equal(captured[0], plain[0])
    assert torch.isfinite(captured[1]).all()
    for row in captured[0].reshape(-1, 20).tolist():
        assert not violations(row, **CASES["all"])
    # more suppress ids than the kernel takes: the composed step, still from a graph
    many = dict(suppress=tuple(range(17)), no_repeat_ngram=3)
    host_many = run(model, vis, **many)
    monkeypatch.setattr(T, "_FUSED_BEAM_STEP", True)
    monkeypatch.setattr(T, "_GRAPH_DECODE", True)
    other = run(model, vis, no_repeat_ngram=3)
    assert len(model._decode_graphs) == 2
    assert torch.equal(run(model, vis, **kw)[0], captured[0]) and len(model._decode_graphs) == 2
    graphed_many = run(model, vis, **many)
    assert len(model._decode_graphs) == 3
    assert torch.equal(graphed_many[0], host_many[0]) and torch.equal(graphed_many[1], host_many[1])
    assert not torch.equal(other[0], captured[0])
    model._decode_graphs.clear()


def test_constrained_decode_of_the_model(g15_device, monkeypatch):
    model, vis = g15_device
    check_decode(model, vis, monkeypatch)


def test_constrained_decode_of_an_ensemble(g15_device, monkeypatch):
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis = g15_device
    twin = copy.deepcopy(model)
    with torch.no_grad():
        twin.cap_generator.fc.weight.mul_(0.8)
    check_decode(Ensemble([model, twin], config=model.config).eval(), vis, monkeypatch)
    assert not model._decode_graphs and not twin._decode_graphs
