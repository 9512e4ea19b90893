"""Beam-search constraints without a GPU: the C ABI of the bans of grit_beam_step, the host statement of the banned set
(grit_amd/ops/beam.py: banned_words_host) against a brute-force enumerator, Transformer.forward / Ensemble.forward with
min_len, no_repeat_ngram, no_repeat_word, suppress and length_penalty on fixture G15 under the oracle ops, and what is refused."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import default_config, load, oracle_ops, t
from tests.test_sample_cpu import EOS, FEATS, decode, g15_model

V_SMALL = 11  # an alphabet in which repeats abound


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_symbol_and_constants():
    from grit_amd import abi, lib
    a = abi.read()
    assert "grit_beam_step" in a.functions and "grit_beam_step_con_f32" not in a.functions
    names = [name for name, _ in a.structs["grit_beam_step_args"]]  # the eight fields of the bans, in the struct of the one step
    at = names.index("history")
    assert names[at:at + 8] == ["history", "history_ld", "t", "no_repeat_ngram", "no_repeat_word", "ban_eos", "suppress", "n_suppress"]
    assert "grit_beam_step" in lib.SIGNATURES
    assert a.constants["GRIT_BEAM_MAX_HISTORY"] == lib.BEAM_MAX_HISTORY == 64
    assert a.constants["GRIT_BEAM_MAX_SUPPRESS"] == lib.BEAM_MAX_SUPPRESS == 16
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "grit_beam_step")
    assert lib.load().grit_abi_version() == a.version >= 61


# ---------------------------------------------------------------------------------------------------------------- host form
def enumerate_bans(h, live, t, eos, V, min_len, suppress, no_repeat_word, n):
    """The definition, word by word: a plain loop over all pairs of n-grams of one beam's history h[0:t]."""
    banned = set()
    if not live:
        return banned
    if t < min_len:
        banned.add(eos)
    banned.update(suppress)
    if no_repeat_word and t >= 1:
        banned.add(h[t - 1])
    if n >= 1:
        for i in range(0, t - n + 1):
            if all(h[i + q] == h[t - n + 1 + q] for q in range(n - 1)):
                banned.add(h[i + n - 1])
    return {w for w in banned if 0 <= w < V}


def host(history, alive, t, V=V_SMALL, **kw):
    from grit_amd.ops.beam import banned_words_host
    return banned_words_host(history, alive, t, EOS, V, **kw)


def bans_of(row, V=V_SMALL, **kw):
    """the banned words of a single live beam with the history `row`"""
    h = torch.tensor(row, dtype=torch.long).view(1, 1, -1)
    return sorted(torch.nonzero(host(h, None, len(row), V, **kw)[0, 0]).flatten().tolist())


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_host_form_equals_the_enumerator(n):
    rng = np.random.default_rng(40 + n)
    B, cur = 3, 5
    checked = hits = 0
    for tt in range(0, 21):
        hist = rng.integers(0, V_SMALL, (B, cur, tt))
        if tt >= 2:
            hist[0, 1, rng.integers(0, tt)] = -1        # words outside the vocabulary: they ban nothing ...
            hist[1, 2, rng.integers(0, tt)] = V_SMALL   # ... and still take part in the comparisons
            hist[2, 0, :] = V_SMALL + 3
        alive = rng.random((B, cur)) > 0.3              # finished rows have no bans
        for min_len, suppress, nrw in ((0, (), False), (6, (0, 1, 2), True), (0, (10,), True)):
            got = host(torch.from_numpy(hist), torch.from_numpy(alive.astype(np.float32)).view(B, cur, 1), tt, min_len=min_len,
                       suppress=suppress, no_repeat_word=nrw, no_repeat_ngram=n)
            assert got.shape == (B, cur, V_SMALL) and got.dtype == torch.bool
            for b in range(B):
                for j in range(cur):
                    want = enumerate_bans(hist[b, j].tolist(), alive[b, j], tt, EOS, V_SMALL, min_len, suppress, nrw, n)
                    assert set(torch.nonzero(got[b, j]).flatten().tolist()) == want, (tt, b, j, min_len, suppress, nrw)
                    checked += 1
                    hits += bool(want - set(suppress) - {EOS})
    assert checked == 21 * 3 * B * cur and (hits > 100 or n == 0)  # the rules that read the history are exercised


def test_hand_written_histories():
    assert bans_of([5, 6], no_repeat_ngram=3) == []                   # t = n - 1: nothing
    assert bans_of([5, 6, 5], no_repeat_ngram=3) == []                # t = n: one window, (5, 6) against (6, 5)
    assert bans_of([5, 5, 5], no_repeat_ngram=3) == [5]               # t = n: (5, 5) repeats and was followed by 5
    assert bans_of([7], no_repeat_ngram=2) == []                      # t = 1 with n = 2
    assert bans_of([7, 7], no_repeat_ngram=2) == [7]
    assert bans_of([4, 8, 9, 4, 8, 6, 4, 8], no_repeat_ngram=3) == [6, 9]  # the prefix matches twice: both continuations
    assert bans_of([4, 8, 9, 4, 8, 6, 4, 8], no_repeat_ngram=2) == [6, 9]  # 8 was followed by 9 and by 6
    assert bans_of([4, 8, 9, 4], no_repeat_ngram=1) == [4, 8, 9]
    assert bans_of([4, 8, 9, 4], no_repeat_word=True) == [4]
    assert bans_of([], min_len=1, no_repeat_word=True, no_repeat_ngram=1) == [EOS]
    assert bans_of([4] * 5, min_len=5) == [] and bans_of([4] * 4, min_len=5) == [EOS]
    assert bans_of([4, -1, 4, -1], no_repeat_ngram=2) == [4]          # -1 compares equal to -1; the word after it is banned
    assert bans_of([-1, 4, -1], no_repeat_ngram=2, no_repeat_word=True) == [4]
    assert bans_of([V_SMALL, 4], no_repeat_ngram=1, no_repeat_word=True, suppress=(0, 10)) == [0, 4, 10]
    h = torch.tensor([[[4, 8, 4], [4, 8, 4]]])
    got = host(h, torch.tensor([[1.0, 0.0]]), 3, no_repeat_ngram=2, suppress=(0,), min_len=9)
    assert torch.nonzero(got[0, 0]).flatten().tolist() == [0, EOS, 8] and not got[0, 1].any()  # the finished beam keeps word 0


def test_constraint_tuple():
    from grit_amd.ops.beam import Constraints, constraints
    assert constraints(100) is None and constraints(100, 0, 0, False, ()) is None
    assert constraints(100, 2, 3, 1, [5, 6]) == Constraints(2, 3, True, (5, 6))
    assert hash(constraints(100, suppress=range(20))) is not None and len(constraints(100, suppress=range(20)).suppress) == 20
    for bad in (dict(min_len=-1), dict(no_repeat_ngram=-2), dict(suppress=(100,)), dict(suppress=(-1,))):
        with pytest.raises(ValueError):
            constraints(100, **bad)


# ---------------------------------------------------------------------------------------------------------------- fixture G15
CASES = {
    "word": dict(no_repeat_word=True),
    "bigram": dict(no_repeat_ngram=2),
    "trigram": dict(no_repeat_ngram=3),
    "min_len": dict(min_len=6),
    "all": dict(no_repeat_word=True, no_repeat_ngram=2, min_len=6, suppress=(0, 1, 2)),
}
# images of the 8 whose five beams change under the constraint, from a CPU prototype of the definition (oracle ops)
CHANGED = {"word": 7, "bigram": 8, "trigram": 6, "min_len": 5, "all": 8}


def live_words(row):
    """a hypothesis up to and including its first <eos>"""
    row = list(row)
    return row[:row.index(EOS) + 1] if EOS in row else row


def violations(row, min_len=0, no_repeat_ngram=0, no_repeat_word=False, suppress=()):
    w = live_words(row)
    out = []
    if EOS in w and len(w) - 1 < min_len:
        out.append("ends after %d words" % (len(w) - 1))
    if no_repeat_word and any(a == b for a, b in zip(w, w[1:])):
        out.append("adjacent repeat")
    n = no_repeat_ngram
    if n:
        grams = [tuple(w[i:i + n]) for i in range(len(w) - n + 1)]
        if len(grams) != len(set(grams)):
            out.append("repeated %d-gram" % n)
    if set(w) & set(suppress):
        out.append("suppressed word")
    return out


def check_constrained(tokens, lps, base, kw, name):
    assert tokens.shape == lps.shape == (8, 5, 20)
    assert torch.isfinite(lps).all()
    for b in range(8):
        for j in range(5):
            assert not violations(tokens[b, j].tolist(), **kw), (name, b, j, tokens[b, j].tolist())
    changed = int((tokens != base).any(-1).any(-1).sum())
    print("%s: %d of 8 images decode differently" % (name, changed))
    assert changed >= 1
    return changed


@pytest.fixture(scope="module")
def g15():
    model, _ = g15_model()
    g = load("beam_g15.npz")
    vis = {k: t(g[k]) for k in FEATS}
    with oracle_ops():
        base = decode(model, vis, beam_size=5, out_size=5)
    return model, vis, base


def test_the_fixture_needs_constraints(g15):
    """what the unconstrained decode gives: best beams that end after a word or two, or repeat themselves"""
    best = g15[2][0][:, 0]
    short = sum(len(live_words(r)) - 1 <= 2 for r in best.tolist())
    repeats = sum(bool(violations(r, no_repeat_word=True)) for r in best.tolist())
    assert short == 5 and repeats >= 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_constrained_decode_on_the_fixture(g15, name):
    model, vis, (base, _) = g15
    with oracle_ops():
        tokens, lps = decode(model, vis, beam_size=5, out_size=5, **CASES[name])
    assert check_constrained(tokens, lps, base, CASES[name], name) == CHANGED[name]


def test_everything_off_is_the_plain_decode(g15):
    model, vis, (base, base_lps) = g15
    with oracle_ops():
        tokens, lps = decode(model, vis, beam_size=5, out_size=5, min_len=0, no_repeat_ngram=0, no_repeat_word=False, suppress=(),
                             length_penalty=0.0)
    assert torch.equal(tokens, base) and torch.equal(lps, base_lps)


def test_more_suppress_ids_than_the_kernel_takes(g15):
    model, vis, (base, _) = g15
    used = sorted(set(base[:, 0].flatten().tolist()) - {0, EOS})[:20]
    assert len(used) > 16
    with oracle_ops():
        tokens, lps = decode(model, vis, beam_size=5, out_size=5, suppress=used)
    check_constrained(tokens, lps, base, dict(suppress=used), "20 suppressed ids")


# ---------------------------------------------------------------------------------------------------------------- length penalty
ALPHA = 1.0  # the fixture's short `... <eos>` beams lose against the 10 - 20 word ones


def test_length_penalty_reorders_the_final_beams(g15):
    model, vis, (base, base_lps) = g15
    with oracle_ops():
        tokens, lps = decode(model, vis, beam_size=5, out_size=5, length_penalty=ALPHA)
        zero, zero_lps = decode(model, vis, beam_size=5, out_size=5, length_penalty=0.0)
        best, _ = decode(model, vis, beam_size=5, out_size=1, length_penalty=ALPHA)
    assert torch.equal(zero, base) and torch.equal(zero_lps, base_lps)
    moved = 0
    for b in range(8):
        rows = list(zip(base[b].tolist(), base_lps[b].tolist()))
        scored = []
        for j, (words, word_lps) in enumerate(rows):
            length = len(live_words(words))
            score = float(np.float32(np.sum(np.float32(word_lps), dtype=np.float64)))  # the search's own running score, nearly
            scored.append((score / length ** ALPHA, j))
        order = [j for _, j in sorted(scored, key=lambda s: -s[0])]
        gaps = sorted(s for s, _ in scored)
        assert min(b2 - a for a, b2 in zip(gaps, gaps[1:])) > 1e-4, "the fixture's normalised scores are not tied"
        assert tokens[b].tolist() == [rows[j][0] for j in order], b
        assert lps[b].tolist() == [rows[j][1] for j in order], b
        moved += order[0] != 0
    print("length penalty %g: the best hypothesis changes for %d of 8 images" % (ALPHA, moved))
    assert moved >= 1
    assert torch.equal(best, tokens[:, 0])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_validation_and_refusals(g15):
    model, vis, _ = g15
    with oracle_ops():
        for bad in (dict(min_len=-1), dict(no_repeat_ngram=-1), dict(suppress=(10201,)), dict(suppress=(-1,)),
                    dict(length_penalty=-0.5)):
            with pytest.raises(ValueError):
                decode(model, vis, **bad)
        for con in (dict(min_len=2), dict(no_repeat_ngram=2), dict(no_repeat_word=True), dict(suppress=(0,)),
                    dict(length_penalty=1.0)):
            with pytest.raises(NotImplementedError):
                decode(model, vis, decode='sample', **con)


def test_ensemble_takes_the_constraints(g15):
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis, _ = g15
    ens = Ensemble([model], config=model.config).eval()
    kw = CASES["all"]
    with oracle_ops():
        want = decode(model, vis, beam_size=5, out_size=5, length_penalty=ALPHA, **kw)
        got = ens(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=5, out_size=5, length_penalty=ALPHA, **kw)
        with pytest.raises(ValueError):
            ens(vis, None, use_beam_search=True, suppress=(10201,))
        with pytest.raises(NotImplementedError, match="sample"):
            ens(vis, None, use_beam_search=True, decode='sample', min_len=3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_config_keys_default_to_off_and_older_configs_load():
    from grit_amd.config import beam_constraints
    cfg = default_config()
    off = dict(min_len=0, no_repeat_ngram=0, no_repeat_word=False, suppress=(), length_penalty=0.0)
    assert beam_constraints(cfg) == off
    for key in ("beam_min_len", "beam_no_repeat_ngram", "beam_no_repeat_word", "beam_suppress", "beam_length_penalty"):
        assert hasattr(cfg.model, key)
        delattr(cfg.model, key)
    assert beam_constraints(cfg) == off
    cfg = default_config(**{'model.beam_min_len': 5, 'model.beam_no_repeat_ngram': 2, 'model.beam_suppress': [0, 1]})
    assert beam_constraints(cfg) == dict(off, min_len=5, no_repeat_ngram=2, suppress=(0, 1))


def test_evaluate_metrics_honours_the_config(g15):
    from grit_amd.engine.caption_engine import evaluate_metrics
    model, vis, (base, _) = g15
    cfg = default_config(**{'model.beam_min_len': 6, 'model.beam_no_repeat_ngram': 2})
    model.cached_features = True
    try:
        with oracle_ops():
            tokens, _ = evaluate_metrics(model, None, [{'samples': vis}], None, config=cfg, log_and_save=False)
            want, _ = model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=5, out_size=1, min_len=6,
                            no_repeat_ngram=2)
    finally:
        model.cached_features = False
    assert torch.equal(tokens[0], want) and not torch.equal(want, base[:, 0])
    assert not any(violations(r, min_len=6, no_repeat_ngram=2) for r in want.tolist())
