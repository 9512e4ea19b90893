"""Diverse (group) beam search without a GPU: the host statement of the grouped step (grit_amd/ops/beam.py: beam_step_groups_host)
against a loop-per-candidate reference that shares no code with it, one group against the plain composed step of `_beam_advance`,
Transformer.forward / Ensemble.forward with num_groups and diversity on fixture G15 under the oracle ops, what is refused, and the
configuration keys.  Every comparison is bit-equality: the rule defines its own arithmetic."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import default_config, load, oracle_ops, t
from tests.test_sample_cpu import EOS, FEATS, decode, g15_model

NAMES = ("sel_beam", "sel_word", "seq_logprob", "seq_mask", "picked")
F = np.float32


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_symbol():
    import ctypes
    from grit_amd import abi, lib
    a = abi.read()
    fields = dict(a.structs["grit_beam_step_args"])  # the argument struct of the one step
    assert (fields["groups"], fields["diversity"]) == (ctypes.c_int, ctypes.c_float)
    assert "grit_beam_step_div_f32" not in a.functions and hasattr(ctypes.CDLL(lib.LIB_PATH), "grit_beam_step")
    assert lib.load().grit_abi_version() == a.version >= 61


# ---------------------------------------------------------------------------------------------------------------- the rule
def brute_force(lp, slp, mask, prev, beam, G, lam, banned=()):
    """The rule of the issue, candidate by candidate, in numpy float32 scalars: lp [B, cur, V], slp [B, cur], mask / prev [B, cur]
    or None at the first step; `banned` words score -inf on live rows.  Returns the five outputs as nested lists and the number of
    exact ties between a penalised candidate and another one at the selection boundary or inside the selection."""
    B, cur, V = lp.shape
    g = beam // G
    out = [[[None] * beam for _ in range(B)] for _ in NAMES]
    ties = 0
    for b in range(B):
        counts = [0] * V
        for i in range(G):
            rows = [0] if cur == 1 else list(range(i * g, (i + 1) * g))
            cands = []
            for j in rows:
                alive = F(1) if prev is None else F(mask[b, j]) * F(prev[b, j] != EOS)
                for w in range(V):
                    if alive != 0:
                        value = F(slp[b, j]) + (F(lp[b, j, w]) - F(lam) * F(counts[w]))
                        if w in banned:
                            value = F(-np.inf)
                    else:
                        value = F(slp[b, j]) if w == 0 else F(-999)
                    cands.append((value, j * V + w, j, w, alive, alive != 0 and counts[w] > 0))
            cands.sort(key=lambda c: (-float(c[0]), c[1]))
            for x, y in zip(cands[:g], cands[1:g + 1]):
                ties += bool(x[0] == y[0] and (x[5] or y[5]) and lam > 0 and np.isfinite(x[0]))
            new_counts = list(counts)
            for r, (value, _, j, w, alive, _) in enumerate(cands[:g]):
                at = i * g + r
                out[0][b][at], out[1][b][at], out[2][b][at], out[3][b][at] = j, w, value, alive
                out[4][b][at] = F(lp[b, j, w]) * alive
                if alive != 0:
                    new_counts[w] += 1
            counts = new_counts
    return out, ties


def quantised_state(rng, B, cur, V, later):
    """log-probs and scores that are multiples of 2^-3 (every operation of the rule is exact, and penalised ties abound); at a
    later step finished rows, with group 0 of image 0 and all of image 1 finished"""
    lp = -rng.integers(0, 16, (B, cur, V)).astype(np.float32) / 8
    slp = -rng.integers(0, 8, (B, cur)).astype(np.float32) / 8
    if not later:
        return lp, slp, None, None
    mask = (rng.random((B, cur)) > 0.25).astype(np.float32)
    prev = np.where(rng.random((B, cur)) > 0.25, 9, EOS).astype(np.int64)
    return lp, slp, mask, prev


def host(lp, slp, mask, prev, beam, G, lam, con=None, hist=None, step=0):
    from grit_amd.ops.beam import beam_step_groups_host
    B, cur, _ = lp.shape
    return beam_step_groups_host(t(lp), t(slp).view(B, cur, 1), None if mask is None else t(mask).view(B, cur, 1),
                                 None if prev is None else t(prev).view(B * cur, 1), EOS, beam, G, lam, hist, step, con)


def assert_equal_to_lists(got, want, tag):
    for name, a, w in zip(NAMES, got, want):
        w = np.asarray(w)
        a = a.numpy().reshape(w.shape)
        if a.dtype == np.float32:  # bits, signed zeros included (picked of a finished beam is logp * 0 = -0.0)
            assert np.array_equal(a.view(np.int32), w.astype(np.float32).view(np.int32)), (tag, name)
        else:
            assert np.array_equal(a, w), (tag, name)


def test_host_form_equals_brute_force():
    rng = np.random.default_rng(2016)
    B, ties, cases = 3, 0, 0
    for beam, G in [(beam, d) for beam in (2, 4, 5, 6, 8) for d in range(1, beam + 1) if beam % d == 0]:
        g = beam // G
        for V in (9, 40):
            for later in (False, True):
                for lam in (0.0, 0.5, 1e4):
                    lp, slp, mask, prev = quantised_state(rng, B, beam if later else 1, V, later)
                    if later:
                        prev[0, :g] = EOS   # a whole group finished ...
                        mask[1, :] = 0.0    # ... and a whole image
                    want, n = brute_force(lp, slp, mask, prev, beam, G, lam)
                    got = host(lp, slp, mask, prev, beam, G, lam)
                    assert_equal_to_lists(got, want, (beam, G, V, later, lam))
                    assert got[0].shape == got[1].shape == (B, beam) and got[2].shape == got[3].shape == got[4].shape == (B, beam, 1)
                    if later:
                        assert (got[3][1] == 0).all() and (got[3][0, :g] == 0).all()
                        assert (got[0] // g == torch.arange(beam) // g).all()  # beams never change group
                    ties += n
                    cases += 1
    print("%d cases, %d penalised ties at or inside the selection" % (cases, ties))
    assert ties > 0  # the index rule decided among penalised candidates


def test_host_form_with_bans_equals_brute_force():
    """banned words stay -inf under the penalty, and are selected by index once nothing else is left"""
    from grit_amd.ops.beam import Constraints
    rng = np.random.default_rng(77)
    for beam, G, V, lam in ((6, 3, 9, 0.5), (4, 2, 9, 1e4), (8, 4, 40, 0.5)):
        con = Constraints(5, 0, False, tuple(range(V - 1)) if V == 9 else (0, 7))  # V 9: one finite word per live row
        for later in (False, True):
            lp, slp, mask, prev = quantised_state(rng, 3, beam if later else 1, V, later)
            hist = torch.full((3, beam if later else 1, 2 if later else 0), 9, dtype=torch.long)
            banned = set(con.suppress) | {EOS}
            want, _ = brute_force(lp, slp, mask, prev, beam, G, lam, banned)
            got = host(lp, slp, mask, prev, beam, G, lam, con, hist, 2 if later else 0)
            assert_equal_to_lists(got, want, (beam, G, V, later))


class Search(object):
    """the running search that `_beam_advance` reads and writes, and its own single member"""

    def __init__(self, slp, mask, prev):
        self.seq_logprob, self.seq_mask, self.selected_words, self.log_probs = slp, mask, prev, []

    def _follow_beams(self, selected_beam, *rest):
        self.selected_beam = selected_beam


@pytest.mark.parametrize("beam,V", [(5, 40), (8, 9), (2, 9), (6, 1003)])
def test_one_group_is_the_plain_composed_step(beam, V):
    from grit_amd.models.caption.transformer import BeamSearchSteps

    class Plain(Search, BeamSearchSteps):
        pass

    g = torch.Generator().manual_seed(beam * V)
    B = 3
    for later in (False, True):
        cur = beam if later else 1
        lp = torch.log_softmax(3 * torch.randn(B, cur, V, generator=g), -1)
        slp = -torch.rand(B, cur, 1, generator=g) * 2 if later else torch.zeros(B, 1, 1)
        mask = prev = None
        if later:
            mask = (torch.rand(B, cur, 1, generator=g) > 0.3).float()
            prev = torch.where(torch.rand(B * cur, 1, generator=g) > 0.3, 9, EOS)
            mask[:, 0], prev[0::cur] = 1.0, 9  # one live row per image: the plain step's torch.topk never has to order -999 ties
        for lam in (0.0, 0.5, 1e4):
            got = host(lp.numpy(), slp.numpy().reshape(B, cur), None if mask is None else mask.numpy().reshape(B, cur),
                       None if prev is None else prev.numpy().reshape(B, cur), beam, 1, lam)
            s = Plain(slp, torch.ones(B, beam, 1) if mask is None else mask.clone(), prev)
            outputs = s._beam_advance((s,), 1 if later else 0, lp, None, [], False, B, beam, EOS)
            want = (s.selected_beam, outputs[-1].squeeze(-1), s.seq_logprob, s.seq_mask, s.log_probs[-1])
            for name, a, w in zip(NAMES, got, want):
                assert a.shape == w.shape and torch.equal(a, w), (later, lam, name)
                if a.dtype == torch.float32:
                    assert torch.equal(a.view(torch.int32), w.view(torch.int32)), (later, lam, name)


def test_group_tuple():
    from grit_amd.ops.beam import Groups, groups
    assert groups(5) is None and groups(6, 1, 3.5) is None
    assert groups(6, 3, 0.5) == Groups(3, 0.5) and groups(5, 5) == Groups(5, 0.0) and hash(groups(8, 4, 1)) is not None
    for bad in ((5, 0), (5, -1), (5, 2), (6, 4), (6, 7), (6, 3, -0.5), (6, 3, math.inf), (6, 3, math.nan), (6, 1, -1.0), (6, 1.5)):
        with pytest.raises(ValueError):
            groups(*bad)


# ---------------------------------------------------------------------------------------------------------------- fixture G15
@pytest.fixture(scope="module")
def g15():
    model, _ = g15_model()
    g = load("beam_g15.npz")
    vis = {k: t(g[k]) for k in FEATS}
    with oracle_ops():
        base = decode(model, vis, beam_size=5, out_size=5)
    return model, vis, base


def test_one_group_is_the_plain_search(g15):
    model, vis, (base, base_lps) = g15
    with oracle_ops():
        for lam in (0.0, 2.5):
            tokens, lps = decode(model, vis, beam_size=5, out_size=5, num_groups=1, diversity=lam)
            assert torch.equal(tokens, base) and torch.equal(lps, base_lps)


def live_steps(tokens):
    """[..., T] bool: the beam is live when it chooses word t (no <eos> before t)"""
    ended = (tokens == EOS).long().cumsum(-1)
    return torch.cat([torch.zeros_like(ended[..., :1]), ended[..., :-1]], -1) == 0


@pytest.fixture(scope="module")
def diverse(g15):
    model, vis, _ = g15
    with oracle_ops():
        return decode(model, vis, beam_size=5, out_size=5, num_groups=5, diversity=1e4)


def test_five_groups_choose_distinct_words(g15, diverse):
    """groups of one beam never change row, so a final hypothesis is one group's path: under a penalty above every log-prob gap the
    words that the live beams of an image choose at a step are pairwise distinct"""
    _, _, (base, _) = g15
    tokens, lps = diverse
    assert tokens.shape == lps.shape == (8, 5, 20) and torch.isfinite(lps).all()
    live = live_steps(tokens)
    compared = 0
    for b in range(8):
        for step in range(20):
            words = tokens[b, live[b, :, step], step].tolist()
            assert len(set(words)) == len(words), (b, step, words)
            compared += len(words) > 1
    assert compared > 20
    assert (tokens[~live] == 0).all()  # a finished beam lives on through word 0
    changed = int((tokens != base).any(-1).any(-1).sum())
    print("5 groups, diversity 1e4: %d of 8 images decode differently" % changed)
    assert changed == 8  # the plain search's beams share their first words; an ignored keyword would give `base`


def test_ensemble_of_one_is_the_model(g15, diverse):
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis, _ = g15
    ens = Ensemble([model], config=model.config).eval()
    with oracle_ops(), torch.no_grad():
        got = ens(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=5, out_size=5, num_groups=5, diversity=1e4)
        want = decode(model, vis, beam_size=6, out_size=6, num_groups=3, diversity=0.5, no_repeat_ngram=2, length_penalty=1.0)
        both = ens(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=6, out_size=6, num_groups=3, diversity=0.5,
                   no_repeat_ngram=2, length_penalty=1.0)
    assert torch.equal(got[0], diverse[0]) and torch.equal(got[1], diverse[1])
    assert torch.equal(both[0], want[0]) and torch.equal(both[1], want[1])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_validation_and_refusals(g15):
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis, _ = g15
    ens = Ensemble([model], config=model.config).eval()

    def run_ens(**kw):
        return ens(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)

    with oracle_ops():
        for run in (lambda **kw: decode(model, vis, **kw), run_ens):
            for bad in (dict(num_groups=0), dict(num_groups=-2), dict(beam_size=5, num_groups=2), dict(beam_size=6, num_groups=4),
                        dict(num_groups=5, diversity=-0.5), dict(num_groups=5, diversity=math.inf),
                        dict(num_groups=5, diversity=math.nan), dict(num_groups=1, diversity=-1.0)):
                with pytest.raises(ValueError):
                    run(**bad)
            with pytest.raises(NotImplementedError):
                run(decode='sample', beam_size=4, num_groups=2, diversity=0.5)
        with pytest.raises(ValueError):  # validated before the refusal
            decode(model, vis, decode='sample', beam_size=4, num_groups=3)


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_keys_default_to_off_and_older_configs_load():
    from grit_amd.config import beam_constraints, beam_groups
    cfg = default_config()
    assert cfg.model.beam_groups == 1 and cfg.model.beam_diversity == 0.0
    assert beam_groups(cfg) == dict(num_groups=1, diversity=0.0)
    constraints = dict(min_len=0, no_repeat_ngram=0, no_repeat_word=False, suppress=(), length_penalty=0.0)
    assert beam_constraints(cfg) == constraints
    delattr(cfg.model, "beam_groups")
    delattr(cfg.model, "beam_diversity")
    assert beam_groups(cfg) == dict(num_groups=1, diversity=0.0)
    cfg = default_config(**{'model.beam_groups': 3, 'model.beam_diversity': 0.5, 'model.beam_min_len': 4})
    assert beam_groups(cfg) == dict(num_groups=3, diversity=0.5)
    assert beam_constraints(cfg) == dict(constraints, min_len=4)


def test_evaluate_metrics_honours_the_config(g15, diverse):
    from grit_amd.engine.caption_engine import evaluate_metrics
    model, vis, (base, _) = g15
    cfg = default_config(**{'model.beam_groups': 5, 'model.beam_diversity': 1e4, 'model.beam_length_penalty': 1.0})
    model.cached_features = True
    try:
        with oracle_ops():
            tokens, _ = evaluate_metrics(model, None, [{'samples': vis}], None, config=cfg, log_and_save=False)
            want, _ = model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=5, out_size=5, num_groups=5,
                            diversity=1e4, length_penalty=1.0)
    finally:
        model.cached_features = False
    assert torch.equal(tokens[0], want[:, 0])
    # the five final hypotheses are the five groups' paths, whatever their order
    assert sorted(map(tuple, want[0].tolist())) == sorted(map(tuple, diverse[0][0].tolist()))
    assert not torch.equal(want, base)


def test_inference_arguments_parse():
    import inference_caption
    a = inference_caption.build_parser().parse_args(["--img", "x.npy", "--beam", "6", "--groups", "3", "--diversity", "0.5", "--n-best", "4"])
    assert (a.beam, a.groups, a.diversity, a.n_best) == (6, 3, 0.5, 4)
    a = inference_caption.build_parser().parse_args(["--img", "x.npy"])
    assert (a.groups, a.diversity, a.n_best) == (1, 0.0, 1)
