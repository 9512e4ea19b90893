"""Beam search with forced words without a GPU: the host statement of the step (grit_amd/ops/beam.py: beam_step_forced_host) against
a loop-per-candidate reference that shares no code with it, the guarantee of the search on fixture G15 under the oracle ops (the
first caption of every image holds a word of every set), empty sets against the free search, Ensemble([model]) against the model,
what is refused, and the word mapping of the configuration and the command line.  Every comparison is bit-equality."""
import numpy as np
import pytest
import torch

from tests.helpers import default_config, load, oracle_ops, t
from tests.test_sample_cpu import EOS, FEATS, decode, g15_model

NAMES = ("sel_beam", "sel_word", "seq_logprob", "seq_mask", "picked", "met")
F = np.float32
BOS, PAD = 2, 1


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_symbol_and_constants():
    import ctypes
    from grit_amd import abi, lib
    a = abi.read()
    assert a.constants["GRIT_BEAM_MAX_FORCED_SETS"] == lib.BEAM_MAX_FORCED_SETS == 8
    assert a.constants["GRIT_BEAM_MAX_FORCED_WORDS"] == lib.BEAM_MAX_FORCED_WORDS == 4
    # the sets (pointer, C, W) and met_in in the argument struct of the one step, new_met behind the other outputs
    fields = a.structs["grit_beam_step_args"]
    at = [name for name, _ in fields].index("force_words")
    assert fields[at:at + 4] == [("force_words", ctypes.c_void_p), ("n_sets", ctypes.c_int), ("n_words", ctypes.c_int),
                                 ("met_in", ctypes.c_void_p)]
    assert fields[-1] == ("new_met", ctypes.c_void_p)
    assert "grit_beam_step_forced_f32" not in a.functions and hasattr(ctypes.CDLL(lib.LIB_PATH), "grit_beam_step")
    assert lib.load().grit_abi_version() == a.version >= 61


# ---------------------------------------------------------------------------------------------------------------- the rule
def rule_bans(hist, step, min_len, ngram, repeat_word, suppress):
    """the banned words of one live row under the constrained step's rules, from its history (a list of `step` words)"""
    bans = set(suppress)
    if step < min_len:
        bans.add(EOS)
    if repeat_word and step >= 1:
        bans.add(hist[step - 1])
    if ngram >= 1:
        tail = hist[step - ngram + 1:step] if ngram > 1 else []
        for i in range(0, step - ngram + 1):
            if hist[i:i + ngram - 1] == tail:
                bans.add(hist[i + ngram - 1])
    return bans


def brute_force(lp, slp, mask, prev, beam, fw, met, hist=None, step=0, rules=None):
    """The step of the issue, candidate by candidate, in numpy float32 scalars: lp [B, cur, V], slp / mask / prev / met [B, cur]
    (mask, prev and met None at the first step), fw [B, C, W].  Returns the six outputs as nested lists and the number of exact
    score ties between neighbours inside a bank among the chosen."""
    B, cur, V = lp.shape
    C = fw.shape[1]
    full = (1 << C) - 1
    out = [[[None] * beam for _ in range(B)] for _ in NAMES]
    ties = 0
    for b in range(B):
        sets = [set(int(w) for w in fw[b, c] if w >= 0) for c in range(C)]
        start = sum(1 << c for c in range(C) if not sets[c])
        cands = {}  # (j, w) -> (score, met', alive)
        for j in range(cur):
            alive = F(1) if prev is None else F(mask[b, j]) * F(prev[b, j] != EOS)
            have = start if met is None else int(met[b, j])
            if alive == 0:
                cands[(j, 0)] = (F(slp[b, j]), have, alive)
                continue
            bans = rule_bans([int(x) for x in hist[b, j]], step, *rules) if rules is not None else set()
            if have != full:
                bans = bans | {EOS}

            def scored(w):
                return F(-np.inf) if w in bans else F(slp[b, j]) + F(lp[b, j, w])

            def hit(w):
                return have | sum(1 << c for c in range(C) if w in sets[c])

            best = sorted(range(V), key=lambda w: (-float(scored(w)), w))[:beam]
            for w in best:
                cands[(j, w)] = (scored(w), hit(w), alive)
            for c in range(C):
                if not (have >> c) & 1:
                    for w in sets[c]:
                        if w not in bans:
                            cands[(j, w)] = (scored(w), hit(w), alive)
        banks = {}
        for (j, w), (score, m, alive) in cands.items():
            bank = -1 if score == F(-np.inf) else bin(m).count("1")
            banks.setdefault(bank, []).append((score, j * V + w, j, w, m, alive))
        for members in banks.values():
            members.sort(key=lambda c: (-float(c[0]), c[1]))
        chosen, r = [], 0
        while len(chosen) < beam:
            assert any(len(members) > r for members in banks.values())
            for bank in range(C, -2, -1):
                members = banks.get(bank, [])
                if len(members) > r and len(chosen) < beam:
                    chosen.append(members[r])
                    ties += bool(r > 0 and members[r][0] == members[r - 1][0])
            r += 1
        for at, (score, _, j, w, m, alive) in enumerate(chosen):
            out[0][b][at], out[1][b][at], out[2][b][at], out[3][b][at] = j, w, score, alive
            out[4][b][at], out[5][b][at] = F(lp[b, j, w]) * alive, m
    return out, ties


def quantised_state(rng, B, cur, V, C, W, later):
    """log-probs and scores that are multiples of 2^-3 (exact adds, ties abound); sets of words in [4, V) with padding, one set of
    image 0 empty; at a later step finished rows and random masks of met sets, with all of image 1 finished and row 0 of image 2
    having met everything"""
    lp = -rng.integers(0, 16, (B, cur, V)).astype(np.float32) / 8
    slp = -rng.integers(0, 8, (B, cur)).astype(np.float32) / 8
    fw = rng.integers(4, V, (B, C, W)).astype(np.int64)
    fw[rng.random((B, C, W)) < 0.3] = -1
    fw[0, C - 1] = -1
    if not later:
        return lp, slp, None, None, fw, None
    mask = (rng.random((B, cur)) > 0.25).astype(np.float32)
    prev = np.where(rng.random((B, cur)) > 0.25, 9, EOS).astype(np.int64)
    met = rng.integers(0, 1 << C, (B, cur)).astype(np.int32)
    mask[1, :] = 0.0
    mask[2, 0], prev[2, 0], met[2, 0] = 1.0, 9, (1 << C) - 1
    return lp, slp, mask, prev, fw, met


def host(lp, slp, mask, prev, beam, fw, met, hist=None, step=0, con=None):
    from grit_amd.ops.beam import beam_step_forced_host
    B, cur, _ = lp.shape
    return beam_step_forced_host(t(lp), t(slp).view(B, cur, 1), None if mask is None else t(mask).view(B, cur, 1),
                                 None if prev is None else t(prev).view(B * cur, 1), EOS, beam, t(fw), None if met is None else t(met),
                                 None if hist is None else t(hist), step, con)


def assert_equal_to_lists(got, want, tag):
    for name, a, w in zip(NAMES, got, want):
        w = np.asarray(w)
        a = a.numpy().reshape(w.shape)
        if a.dtype == np.float32:  # bits, signed zeros included (picked of a finished beam is logp * 0 = -0.0)
            assert np.array_equal(a.view(np.int32), w.astype(np.float32).view(np.int32)), (tag, name)
        else:
            assert np.array_equal(a, w), (tag, name)


def test_host_form_equals_brute_force():
    rng = np.random.default_rng(2018)
    B, ties, cases = 3, 0, 0
    for beam in (2, 5, 6, 8):
        for V in (9, 40):
            for C, W in ((1, 1), (3, 4), (8, 1), (8, 4), (3, 1)):
                for later in (False, True):
                    lp, slp, mask, prev, fw, met = quantised_state(rng, B, beam if later else 1, V, C, W, later)
                    want, n = brute_force(lp, slp, mask, prev, beam, fw, met)
                    got = host(lp, slp, mask, prev, beam, fw, met)
                    assert_equal_to_lists(got, want, (beam, V, C, W, later))
                    assert got[0].shape == got[1].shape == got[5].shape == (B, beam) and got[5].dtype == torch.int32
                    assert got[2].shape == got[3].shape == got[4].shape == (B, beam, 1)
                    if later:
                        assert (got[3][1] == 0).all()  # an image whose rows are all finished
                    live = got[3].squeeze(-1) != 0
                    full = got[5] == (1 << C) - 1
                    assert not ((got[1] == EOS) & live & ~full).any()  # <eos> only from rows that owe nothing
                    ties += n
                    cases += 1
    print("%d cases, %d exact ties inside a bank among the chosen" % (cases, ties))
    assert ties > 0


def test_host_form_under_constraints_equals_brute_force():
    """the rules of the constrained step ban forced words per row: suppressed ids, the repeated word, n-gram continuations"""
    from grit_amd.ops.beam import Constraints
    rng = np.random.default_rng(77)
    B, step = 3, 3
    for beam, V, C, W in ((5, 40, 3, 4), (6, 9, 3, 1), (8, 40, 8, 4), (2, 9, 1, 4)):
        for ngram in (1, 2, 3):
            con = Constraints(5, ngram, True, (0, 7))
            rules = (5, ngram, True, (0, 7))
            lp, slp, mask, prev, fw, met = quantised_state(rng, B, beam, V, C, W, True)
            hist = rng.integers(4, 8, (B, beam, step)).astype(np.int64)  # few words: every row has n-grams to ban
            fw[:, 0, 0] = 7                                              # a forced word that is suppressed
            fw[:, C - 1, W - 1] = hist[:, 0, 1]                          # and one that row 0's history may ban, for that row only
            prev = hist[:, :, -1].copy()
            prev[:, 1] = EOS
            hist[:, 1, -1] = EOS
            want, _ = brute_force(lp, slp, mask, prev, beam, fw, met, hist, step, rules)
            got = host(lp, slp, mask, prev, beam, fw, met, hist, step, con)
            assert_equal_to_lists(got, want, (beam, V, C, W, ngram))
            live = (got[3].squeeze(-1) != 0) & torch.isfinite(got[2].squeeze(-1))  # (bank -1 gives its -inf candidates a slot)
            assert not set(got[1][live].tolist()) & {0, 7, EOS}  # min_len 5 at step 3
        lp, slp, _, _, fw, _ = quantised_state(rng, B, 1, V, C, W, False)
        want, _ = brute_force(lp, slp, None, None, beam, fw, None, np.zeros((B, 1, 0), np.int64), 0, rules)
        assert_equal_to_lists(host(lp, slp, None, None, beam, fw, None, None, 0, con), want, (beam, V, C, W, "first"))


def test_one_word_in_two_sets_jumps_two_banks():
    """word 5 is in both sets: the one candidate that chooses it lands in bank 2 and takes the first slot, whatever its score"""
    lp = np.full((1, 1, 9), -1.0, np.float32)
    lp[0, 0, 5] = -8.0
    fw = np.array([[[5, 6], [5, -1]]], np.int64)
    got = host(lp, np.zeros((1, 1), np.float32), None, None, 3, fw, None)
    assert got[1][0].tolist() == [5, 6, 0] and got[5][0].tolist() == [3, 1, 0]
    assert got[2][0, :, 0].tolist() == [-8.0, -1.0, -1.0]


def test_validation_of_the_sets():
    from grit_amd.ops.beam import forced, initial_met
    assert forced(40, None, EOS, BOS, PAD) is None
    assert forced(40, torch.zeros((2, 0, 3), dtype=torch.long), EOS) is None and forced(40, torch.zeros((2, 3, 0), dtype=torch.long), EOS) is None
    fw = forced(40, [[[4, 5], [6, -1]], [[-1, -1], [39, 4]]], EOS, BOS, PAD)
    assert fw.dtype == torch.int64 and fw.shape == (2, 2, 2) and fw.is_contiguous()
    assert initial_met(fw).tolist() == [0, 1] and initial_met(fw).dtype == torch.int32
    for bad in ([[[40]]], [[[4, EOS]]], [[[BOS]]], [[[PAD, 5]]], torch.full((1, 9, 1), 5), torch.full((1, 1, 5), 5),
                torch.full((1, 1), 5), torch.full((1, 1, 1), 5.0)):
        with pytest.raises(ValueError):
            forced(40, bad, EOS, BOS, PAD)
    with pytest.raises(ValueError, match="39"):
        forced(39, [[[39]]], EOS, BOS, PAD)


# ---------------------------------------------------------------------------------------------------------------- fixture G15
@pytest.fixture(scope="module")
def g15():
    model, _ = g15_model()
    g = load("beam_g15.npz")
    vis = {k: t(g[k]) for k in FEATS}
    with oracle_ops():
        base = decode(model, vis, beam_size=5, out_size=5)
    return model, vis, base


def unused_words(model, base, n):
    """n ids that no beam of the free search produced for any image (and no special id)"""
    V = model.cap_generator.fc.weight.shape[0]
    free = sorted(set(range(4, V)) - set(base.unique().tolist()))
    assert len(free) >= n
    step = len(free) // n
    return [free[i * step] for i in range(n)]


def sets_for(model, base, C):
    """[8, C, 2] : C sets per image, of one or two words that the free search never produced; the images differ in their sets"""
    B = base.shape[0]
    words = unused_words(model, base, 2 * C + B)
    fw = torch.full((B, C, 2), -1, dtype=torch.long)
    for b in range(B):
        for c in range(C):
            fw[b, c, 0] = words[(2 * c + b) % len(words)]
            if (b + c) % 2:
                fw[b, c, 1] = words[(2 * c + 1 + b) % len(words)]
    return fw


@pytest.mark.parametrize("C", [1, 3])
def test_the_first_caption_holds_a_word_of_every_set(g15, C):
    model, vis, (base, _) = g15
    fw = sets_for(model, base, C)
    with oracle_ops():
        tokens, lps = decode(model, vis, beam_size=5, out_size=1, force_words=fw)
    assert tokens.shape == lps.shape == (8, 20)
    for b in range(8):
        caption = tokens[b].tolist()
        words = set(caption[:caption.index(EOS)] if EOS in caption else caption)
        assert not set(base[b].unique().tolist()) & set(fw[b].flatten().tolist())  # the free search had none of them
        for c in range(C):
            assert words & set(w for w in fw[b, c].tolist() if w >= 0), (b, c, caption)
    assert not torch.equal(tokens, base[:, 0])


def test_empty_sets_are_the_free_search(g15):
    model, vis, (base, base_lps) = g15
    with oracle_ops():
        tokens, lps = decode(model, vis, beam_size=5, out_size=5, force_words=torch.full((8, 2, 3), -1, dtype=torch.long))
    assert torch.equal(tokens, base) and torch.equal(lps, base_lps)
    assert torch.equal(lps.view(torch.int32), base_lps.view(torch.int32))


def test_ensemble_of_one_and_the_other_paths(g15):
    """Ensemble([model]) is the model; return_probs and the search with gradient run the host form and give the same captions;
    constraints and a length penalty go with forced words"""
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis, (base, _) = g15
    fw = sets_for(model, base, 3)
    ens = Ensemble([model], config=model.config).eval()
    kw = dict(beam_size=5, out_size=5, force_words=fw, no_repeat_ngram=2, length_penalty=0.5)
    with oracle_ops():
        want = decode(model, vis, **kw)
        with torch.no_grad():
            got = ens(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)
        probs = decode(model, vis, return_probs=True, **kw)
        model.cached_features = True
        try:
            grad = model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)
        finally:
            model.cached_features = False
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert len(probs) == 3 and torch.equal(probs[0], want[0]) and probs[2].shape[:3] == (8, 5, 20)
    assert torch.equal(grad[0], want[0]) and grad[1].requires_grad
    for b in range(8):  # the ranking: hypotheses that met more sets first
        met = [sum(bool(set(row) & set(w for w in fw[b, c].tolist() if w >= 0)) for c in range(3)) for row in want[0][b].tolist()]
        assert met == sorted(met, reverse=True) and met[0] == 3, (b, met)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_validation_and_refusals(g15):
    from grit_amd.models.caption.ensemble import Ensemble
    model, vis, (base, _) = g15
    V = model.cap_generator.fc.weight.shape[0]
    ens = Ensemble([model], config=model.config).eval()
    fw = sets_for(model, base, 1)

    def run_ens(**kw):
        return ens(vis, None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)

    with oracle_ops():
        for run in (lambda **kw: decode(model, vis, **kw), run_ens):
            for bad in (torch.full((8, 1, 1), V), torch.full((8, 1, 1), EOS), torch.full((8, 1, 1), model.bos_idx),
                        torch.full((8, 1, 1), model.config.model.pad_idx), torch.full((8, 9, 1), 5), torch.full((8, 1, 5), 5),
                        torch.full((3, 1, 1), 5)):
                with pytest.raises(ValueError):
                    run(beam_size=5, force_words=bad)
            with pytest.raises(NotImplementedError):
                run(beam_size=4, num_groups=2, diversity=0.5, force_words=fw)
            with pytest.raises(NotImplementedError):
                run(beam_size=4, decode='sample', force_words=fw)


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_words_map_through_the_vocabulary():
    from grit_amd.config import force_words_ids
    cfg = default_config()
    assert tuple(cfg.model.beam_force_words) == ()
    itos = ["<unk>", "<pad>", "<bos>", "<eos>", "a", "dog", "dogs", "frisbee"]
    assert force_words_ids((), itos) is None and force_words_ids(cfg.model.beam_force_words, itos) is None
    fw = force_words_ids(["dog|dogs", "frisbee"], itos)
    assert fw.dtype == torch.int64 and fw.tolist() == [[[5, 6], [7, -1]]]
    assert force_words_ids(["frisbee"], {w: i for i, w in enumerate(itos)}, batch_size=3).tolist() == [[[7]]] * 3
    with pytest.raises(ValueError, match="'cat'"):
        force_words_ids(["dog|cat"], itos)
    with pytest.raises(ValueError):
        force_words_ids(["|"], itos)
    cfg = default_config(**{'model.beam_force_words': ["dog|dogs"]})
    assert force_words_ids(cfg.model.beam_force_words, itos).tolist() == [[[5, 6]]]


def test_inference_arguments_parse():
    import inference_caption
    a = inference_caption.parse_args(["--img", "x.npy", "--force", "dog|dogs", "frisbee", "--beam", "6"])
    assert a.force == ["dog|dogs", "frisbee"] and a.beam == 6
    assert inference_caption.parse_args(["--img", "x.npy"]).force == []
    for bad in (["--sample", "3"], ["--groups", "2"]):
        with pytest.raises(SystemExit):
            inference_caption.parse_args(["--img", "x.npy", "--force", "dog"] + bad)


def test_evaluation_passes_the_batch_entry_through(g15):
    from grit_amd.engine.caption_engine import decode_consensus, evaluate_metrics
    model, vis, (base, _) = g15
    fw = sets_for(model, base, 1)
    cfg = default_config(**{'model.consensus_candidates': 3})
    model.cached_features = True
    try:
        with oracle_ops():
            tokens, _ = evaluate_metrics(model, None, [{'samples': vis, 'force_words': fw}], None, config=default_config(), log_and_save=False)
            free, _ = evaluate_metrics(model, None, [{'samples': vis}], None, config=default_config(), log_and_save=False)
            want, _ = model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=5, out_size=3, force_words=fw)
            seen = []
            decode_consensus(model, vis, cfg, lambda tok, lps: seen.append(tok) or type("Chosen", (), dict(tokens=tok[:, :1], log_probs=lps[:, :1])),
                             force_words=fw)
    finally:
        model.cached_features = False
    assert torch.equal(tokens[0], want[:, 0]) and torch.equal(free[0], base[:, 0])
    assert torch.equal(seen[0], want)
