"""Consensus reranking under CIDEr-D without a GPU: the ABI, the host form (grit_amd/ops/consensus.py: consensus_host) against
Cider.compute_score, its edge cases, the configuration keys, what evaluate_metrics refuses -- and the input recipe of the device
tests (tests/test_consensus_gpu.py) with the tie condition that makes an argmax comparable."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, default_config

EOS = 3


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_symbols():
    import ctypes
    from grit_amd import abi, lib
    a = abi.read()
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert a.functions["grit_cider_consensus"] == (I, [P, I, I, I, I, P, P, P, P, P, P, P, P])
    assert a.functions["grit_cider_consensus_workspace"] == (L, [I, I, I])
    assert a.constants["GRIT_CONSENSUS_MAX_CANDIDATES"] == lib.CONSENSUS_MAX_CANDIDATES == 32
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, "grit_cider_consensus") and hasattr(so, "grit_cider_consensus_workspace")
    assert lib.load().grit_abi_version() == a.version >= 57
    ws = lib.load().grit_cider_consensus_workspace
    assert ws(2, 5, 20) == 10 * ws(1, 1, 20) and 9 * 1024 < ws(1, 1, 20) <= 10 * 1024  # at most 8 KB + 1 KB per row, and a little
    assert ws(1, 33, 20) == 0 and ws(0, 5, 20) == 0


# ---------------------------------------------------------------------------------------------------------------- host form
@functools.lru_cache(maxsize=None)
def g14():
    """The `train` corpus of fixture G14 as a Cider, and a vocabulary of its words."""
    from grit_amd.datasets.caption.metrics import Cider
    g = json.load(open(os.path.join(GOLDEN, "cider_g14.json")))
    train = {int(k): v for k, v in g["train"].items()}
    words = sorted({w for caps in train.values() for c in caps for w in c.split()})
    itos = ['<unk>', '<pad>', '<bos>', '<eos>'] + words + ['zebra']
    return Cider(train), itos, {w: i for i, w in enumerate(itos)}


def rows(stoi, captions, T):
    """captions (strings) -> [n, T] ids: <eos> behind the words, then words that must be ignored"""
    out = []
    for c in captions:
        ids = [stoi[w] for w in c.split()] + [EOS]
        out.append((ids + [stoi['man'], stoi['dog']] * T)[:T])
    return out


def test_three_candidates_by_hand():
    from grit_amd.ops.consensus import candidate_captions, consensus_host
    cider, itos, stoi = g14()
    caps = ['a man holding a a a umbrella', 'a man holding food', 'dog riding a bike next to a man holding a umbrella']
    tokens = np.asarray([rows(stoi, caps, 14)], np.int64)
    assert candidate_captions(itos, tokens, collapse=False) == [caps]
    sim, score, best = consensus_host(cider, itos, tokens, collapse=False)
    assert sim.shape == (1, 3, 3) and score.shape == (1, 3) and best.shape == (1,) and sim.dtype == score.dtype == np.float64
    for i in range(3):
        others = [caps[j] for j in range(3) if j != i]
        want = cider.compute_score({0: others}, {0: [caps[i]]})[1][0]
        assert score[0, i] == want and want > 0, (i, score[0, i], want)  # exactly
        vi = cider.cook([caps[i]])[0]
        for j in range(3):
            assert sim[0, i, j] == (0.0 if i == j else cider._similarity(vi, cider.cook([caps[j]])[0]))
    # 'a' three times in candidate 0 against once or twice elsewhere: min(w_h, w_r) * w_r is not min(w_r, w_h) * w_h
    assert sim[0, 0, 1] != sim[0, 1, 0] and sim[0, 0, 2] != sim[0, 2, 0]
    assert best[0] == int(np.argmax(score[0])) and score[0, best[0]] > np.delete(score[0], best[0]).max()
    # the same through a tensor
    again = consensus_host(cider, itos, torch.from_numpy(tokens), collapse=False)
    assert all(np.array_equal(a, b) for a, b in zip(again, (sim, score, best)))


def test_one_candidate_identical_candidates_and_an_empty_one():
    from grit_amd.ops.consensus import consensus_host
    cider, itos, stoi = g14()
    one = np.asarray([rows(stoi, ['a man holding food'], 8)], np.int64)
    sim, score, best = consensus_host(cider, itos, one)
    assert sim.tolist() == [[[0.0]]] and score.tolist() == [[0.0]] and best.tolist() == [0]
    same = np.asarray([rows(stoi, ['a man holding food'] * 4, 8)], np.int64)
    sim, score, best = consensus_host(cider, itos, same)
    assert len(set(score[0].tolist())) == 1 and score[0, 0] > 0 and best.tolist() == [0]
    # an empty candidate: similarity 0 in both directions, and it still counts in the others' denominators
    caps = ['a man holding food', '', 'a man holding a umbrella']
    sim, score, best = consensus_host(cider, itos, np.asarray([rows(stoi, caps, 8)], np.int64))
    assert score[0, 1] == 0.0 and (sim[0, 1] == 0).all() and (sim[0, :, 1] == 0).all()
    pair = consensus_host(cider, itos, np.asarray([rows(stoi, [caps[0], caps[2]], 8)], np.int64))
    assert score[0, 0] == pair[0][0, 0, 1] / 2 * 10.0 and pair[1][0, 0] == pair[0][0, 0, 1] / 1 * 10.0
    assert best[0] in (0, 2)
    empty = consensus_host(cider, itos, np.asarray([rows(stoi, ['', '', ''], 8)], np.int64))
    assert (empty[1] == 0).all() and empty[2].tolist() == [0]


def test_collapse_and_out_of_vocabulary():
    from grit_amd.datasets.caption.metrics import Cider
    from grit_amd.ops.consensus import candidate_captions, consensus_host
    cider, itos, stoi = g14()
    caps = ['a man man holding food', 'a man holding food', 'a dog holding food food']
    tokens = np.asarray([rows(stoi, caps, 8)], np.int64)
    assert candidate_captions(itos, tokens, collapse=True) == [['a man holding food', 'a man holding food', 'a dog holding food']]
    on, off = consensus_host(cider, itos, tokens, collapse=True), consensus_host(cider, itos, tokens, collapse=False)
    assert on[0][0, 0, 1] == on[0][0, 1, 0] and off[0][0, 0, 1] != off[0][0, 1, 0]  # collapsed: candidates 0 and 1 are one caption
    assert not np.array_equal(on[1], off[1])
    for bad in (len(itos), -1):
        broken = tokens.copy()
        broken[0, 1, 2] = bad
        with pytest.raises(ValueError):
            consensus_host(cider, itos, broken)
        broken = tokens.copy()
        broken[0, 1, 6] = bad  # behind <eos>: ignored
        assert np.array_equal(consensus_host(cider, itos, broken)[1], on[1])
    with pytest.raises(ValueError):
        consensus_host(Cider(), itos, tokens)  # no corpus statistics


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_keys_default_to_off_and_older_configs_load():
    from grit_amd.config import consensus_options
    cfg = default_config()
    sample = dict(temperature=1.0, top_k=0, top_p=1.0, seed=None)
    assert cfg.model.consensus_candidates == 0 and cfg.model.consensus_decode == 'beam'
    assert consensus_options(cfg) == dict(candidates=0, decode='beam', sample=sample)
    for key in ('consensus_candidates', 'consensus_decode', 'consensus_temperature', 'consensus_top_k', 'consensus_top_p', 'consensus_seed'):
        delattr(cfg.model, key)
    assert consensus_options(cfg) == dict(candidates=0, decode='beam', sample=sample)
    assert consensus_options(default_config(**{'model.consensus_candidates': 1}))['candidates'] == 0
    cfg = default_config(**{'model.consensus_candidates': 8, 'model.consensus_decode': 'sample', 'model.consensus_top_k': 50,
                            'model.consensus_seed': 7})
    assert consensus_options(cfg) == dict(candidates=8, decode='sample', sample=dict(sample, top_k=50, seed=7))
    for bad in ({'model.consensus_decode': 'greedy'}, {'model.consensus_candidates': -1}):
        with pytest.raises(ValueError):
            consensus_options(default_config(**bad))


class Refuses(torch.nn.Module):
    def forward(self, *a, **kw):
        raise AssertionError("the model must not be called")


def test_evaluate_metrics_refuses_a_cider_without_statistics_before_decoding():
    from grit_amd.datasets.caption.metrics import Cider
    from grit_amd.engine.caption_engine import decode_consensus, evaluate_metrics
    cfg = default_config(**{'model.consensus_candidates': 4})
    with pytest.raises(ValueError, match="corpus statistics"):
        evaluate_metrics(Refuses(), None, [{'samples': None}], None, config=cfg, log_and_save=False, consensus=Cider())
    with pytest.raises(ValueError, match="text_field"):
        evaluate_metrics(Refuses(), None, [{'samples': None}], None, config=cfg, log_and_save=False, consensus=g14()[0])
    with pytest.raises(ValueError, match="beam_size"):  # more candidates than beams
        decode_consensus(Refuses(), None, default_config(**{'model.consensus_candidates': 6}), lambda *a: None)
    with pytest.raises(ValueError):
        decode_consensus(Refuses(), None, default_config(), lambda *a: None)


def test_inference_arguments():
    import inference_caption
    a = inference_caption.parse_args(["--img", "x.npy", "--sample", "8", "--consensus", "--consensus-corpus", "c.json"])
    assert a.consensus and a.consensus_corpus == "c.json"
    a = inference_caption.parse_args(["--img", "x.npy"])
    assert not a.consensus and a.consensus_corpus is None
    for bad in (["--consensus", "--n-best", "4"], ["--consensus", "--consensus-corpus", "c.json"]):
        with pytest.raises(SystemExit):
            inference_caption.parse_args(["--img", "x.npy"] + bad)


def test_consensus_corpus_file(tmp_path):
    import inference_caption
    path = tmp_path / "corpus.json"
    path.write_text(json.dumps([["A man holding food.", "a dog"], ["a man riding a bike"]]))
    cider = inference_caption.consensus_cider(str(path))
    assert cider.doc_frequency[('a',)] == 2.0 and cider.doc_frequency[('man', 'holding')] == 1.0 and cider.ref_len == np.log(2.0)
    path.write_text(json.dumps({"0": ["a"]}))
    with pytest.raises(ValueError):
        inference_caption.consensus_cider(str(path))


# ---------------------------------------------------------------------------------------------------------------- the input recipe
@functools.lru_cache(maxsize=None)
def setup():
    """The real vocabulary, a pool of 40 frequent plain words, a synthetic corpus over the pool as a Cider, and the words whose
    tokenisation expands or differs at the end of a sentence (device tables packed on the CPU: nothing is launched)."""
    from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
    from grit_amd.ops.cider import DeviceCider
    itos = json.load(open(os.path.join(GOLDEN, "vocab_g10.json")))["itos"]
    rng = np.random.RandomState(2015)
    pool = [i for i in range(4, 80) if itos[i].isalpha() and itos[i].islower() and
            PTBTokenizer.tokenize([itos[i] + ' zz'])[0] == [itos[i] + ' zz']][:40]
    assert len(pool) == 40
    corpus = {i: [' '.join(itos[int(x)] for x in rng.choice(pool, int(rng.randint(5, 14)))) for _ in range(int(rng.randint(1, 6)))]
              for i in range(300)}
    cider = Cider(PTBTokenizer.tokenize(corpus))
    tables = DeviceCider(cider, itos, device='cpu')
    meta = tables._meta_host
    final = [i for i, w in enumerate(itos) if w in set(tables.final_words) and i != EOS]
    expanding = [i for i in range(len(itos)) if (meta[i] & 15) > 1]
    assert final and expanding
    return itos, cider, pool, final, expanding


def recipe(B, n, T, seed):
    """tokens [B, n, T] int64 (numpy): per image a base caption over the pool and candidates derived from it by a few seeded
    substitutions, deletions, insertions, word doublings and truncations, so that candidates overlap as real ones do (random ids
    over 10 201 words share no n-gram and all tie at 0).  Words that expand or differ sentence-finally are inserted, what follows
    <eos> is garbage, and every fifth candidate is an exact copy of the one in front of it.

    Two candidates with one caption have one vector, hence the same terms in their score sums -- but in another order unless they
    are neighbours, and then the last bit decides between them, on the host as on the device.  So equal captions (with and
    without the collapse of repeated words) occur as neighbours only; a derived candidate that repeats an earlier caption is
    drawn again."""
    itos, _, pool, final, expanding = setup()
    rng = np.random.RandomState(seed)
    collapsed = lambda ids: [w for k, w in enumerate(ids) if k == 0 or w != ids[k - 1]]
    out = np.zeros((B, n, T), np.int64)
    for b in range(B):
        base = [int(x) for x in rng.choice(pool, int(rng.randint(min(5, T - 2), min(12, T - 1) + 1)))]
        cands, seen = [], set()
        while len(cands) < n:
            c = len(cands)
            if c == 0:
                ids = list(base)
            elif c % 5 == 4:
                ids = list(cands[-1])  # an exact duplicate, next to its twin
            else:
                ids = list(base)
                for _ in range(int(rng.randint(1, 4))):
                    op, at = int(rng.randint(0, 6)), int(rng.randint(0, max(1, len(ids))))
                    if op == 0 and ids:
                        ids[at] = int(rng.choice(pool))
                    elif op == 1 and len(ids) > 2:
                        del ids[at]
                    elif op == 2:
                        ids.insert(at, int(rng.choice(pool if rng.rand() < 0.6 else expanding)))
                    elif op == 3 and ids:
                        ids.insert(at, ids[at])  # a doubled word
                    elif op == 4 and len(ids) > 3:
                        ids = ids[:len(ids) - int(rng.randint(1, 3))]
                    elif op == 5:
                        ids.append(int(rng.choice(final)))  # tokenised differently as the last word
                ids = ids[:T - 1]
                if tuple(ids) in seen or tuple(collapsed(ids)) in seen:
                    continue
            cands.append(ids)
            seen.update((tuple(ids), tuple(collapsed(ids))))
        for c, ids in enumerate(cands):
            out[b, c] = (ids + [EOS] + [int(x) for x in rng.randint(0, len(itos), T)])[:T]
    return out


# (B, n, T, seed) of the device tests; the seeds are fixed here, under the tie condition below
CASES = ((3, 1, 8, 11), (3, 2, 8, 12), (4, 5, 20, 13), (2, 16, 20, 14), (2, 32, 20, 15), (40, 5, 12, 16))


def near_ties(captions, score, best):
    """[B] bool: the image's best score does NOT exceed, by more than 1e-9 relative, the best score among the candidates whose
    caption differs from the winner's.  Where it is False, an argmax computed to 1e-11 must agree with the host's."""
    out = np.zeros(len(captions), bool)
    for b, caps in enumerate(captions):
        top = score[b, best[b]]
        others = [score[b, i] for i, c in enumerate(caps) if c != caps[best[b]]]
        out[b] = bool(others) and not (top - max(others) > 1e-9 * abs(top))
    return out


@functools.lru_cache(maxsize=None)
def host_case(B, n, T, seed, collapse):
    """(tokens, (sim, score, best), captions, near-tie mask) of one case: computed once, shared by the tests, never modified"""
    from grit_amd.ops.consensus import candidate_captions, consensus_host
    itos, cider = setup()[:2]
    tokens = recipe(B, n, T, seed)
    ref = consensus_host(cider, itos, tokens, collapse=collapse)
    captions = candidate_captions(itos, tokens, collapse=collapse)
    for a in (tokens,) + ref:
        a.setflags(write=False)
    return tokens, ref, captions, near_ties(captions, ref[1], ref[2])


def test_recipe_meets_the_tie_condition():
    """A condition on the INPUTS, asserted on the host form alone: in at least 95 % of the images the winner is clear."""
    itos, _, _, final, expanding = setup()
    images = ties = clipped = 0
    for collapse in (True, False):
        for B, n, T, seed in CASES:
            tokens, (sim, score, best), captions, tie = host_case(B, n, T, seed, collapse)
            assert tokens.shape == (B, n, T) and (tokens == EOS).any(-1).all()
            if n > 1:
                images, ties = images + B, ties + int(tie.sum())
                assert (score.max(-1) > 0).all()  # candidates overlap
            if n >= 5:
                assert any(caps[3] == caps[4] for caps in captions)  # exact duplicates
                front = [tokens[b, i, :list(tokens[b, i]).index(EOS)] for b in range(B) for i in range(n)]
                assert any(np.isin(f, final).any() for f in front) and any(np.isin(f, expanding).any() for f in front)
                assert any((f[1:] == f[:-1]).any() for f in front)  # doubled words
                clipped += int((np.abs(sim - sim.transpose(0, 2, 1)) > 1e-6).sum())
    print("%d images with n > 1, %d near ties, %d pairs where the clipping bites" % (images, ties, clipped))
    assert ties <= 0.05 * images and clipped > 20
