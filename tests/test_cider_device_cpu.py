"""The host side of the device CIDEr-D reward (grit_amd/ops/cider.py), without a GPU: the per-word expansion tables against the
tokenizer on the joined string, the packed idf / reference arrays against the reference-generated scores of fixture G14, and
the public switches (cider_reward_fn(reward=...), config.optimizer.sc_reward)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN

EOS = 3


def _vocab():
    return json.load(open(os.path.join(GOLDEN, "vocab_g10.json")))["itos"]


def _g14():
    g = json.load(open(os.path.join(GOLDEN, "cider_g14.json")))
    fix = lambda d: {int(k): v for k, v in d.items()}
    return g, fix(g["train"]), fix(g["gts"]), fix(g["res"])


def _tiny_cider():
    from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
    return Cider(PTBTokenizer.tokenize({0: ["a dog sits.", "A dog runs"], 1: ["a cat sits", "a cat runs!"]}))


def _decode(itos, row):
    """TextField.decode of the reference (datasets/caption/field.py:258-283) for one row."""
    words = []
    for t in row:
        if itos[t] == '<eos>':
            break
        words.append(itos[t])
    return ' '.join(words)


def test_expansion_tables_equal_the_tokenizer_on_the_joined_string():
    from grit_amd.datasets.caption.metrics import PTBTokenizer
    from grit_amd.datasets.caption.metrics.tokenizer import PUNCTUATIONS, ptb_tokens
    from grit_amd.ops.cider import DeviceCider
    itos = _vocab()
    assert itos[EOS] == '<eos>'
    dc = DeviceCider(_tiny_cider(), itos, device='cpu')  # the verification of every word passes

    drop = set(PUNCTUATIONS)
    tok = lambda s: [t for t in ptb_tokens(s) if t not in drop]
    differs = [w for w in itos if tok('zz ' + w)[1:] != tok('zz ' + w + ' zz')[1:-1]]
    assert sorted(dc.final_words) == sorted(differs) and len(differs) >= 1
    multi = [i for i, w in enumerate(itos) if len(tok('zz ' + w + ' zz')) != 3 or w in differs]
    assert EOS in multi and len(multi) >= 10

    rng = np.random.RandomState(20240)
    strings = dc.token_strings()
    n_rows, mismatches, with_eos0, without_eos = 20000, [], 0, 0
    for r in range(n_rows + 2):
        n = int(rng.randint(0, 21))
        row = [int(rng.choice(multi)) if rng.rand() < 0.25 else int(rng.randint(0, len(itos))) for _ in range(n)]
        if r == 0:
            row = [EOS] + row[1:] if row else [EOS]
        elif r == 1:
            row = [t for t in row if t != EOS]
        elif n and rng.rand() < 0.6:  # an <eos> somewhere (position 0 included); what follows it stays in the row
            row[int(rng.randint(0, n))] = EOS
        with_eos0 += bool(row) and row[0] == EOS
        without_eos += EOS not in row
        want = PTBTokenizer.tokenize([_decode(itos, row)])[0][0].split()
        got = [strings[t] for t in dc.expand(row)]
        if got != want:
            mismatches.append((row, got, want))
    assert with_eos0 > 100 and without_eos > 100
    assert not mismatches, "%d rows differ, e.g. %r" % (len(mismatches), mismatches[0])


@pytest.mark.parametrize("word", ['""\'a', 'a,b,c,d,e,f,g,h,i'])
def test_constructor_names_the_words_it_cannot_tabulate(word):
    from grit_amd.ops.cider import DeviceCider
    with pytest.raises(ValueError) as err:
        DeviceCider(_tiny_cider(), ['<unk>', '<pad>', '<bos>', '<eos>', 'a', 'dog', word], device='cpu')
    assert repr(word) in str(err.value)


def _find(keys, lo, hi, key):
    while lo < hi:
        mid = (lo + hi) // 2
        if keys[mid] == key:
            return mid
        if keys[mid] < key:
            lo = mid + 1
        else:
            hi = mid
    return -1


def _walk(arrays, tokens, slot):
    """The kernel's algorithm over the packed arrays in plain Python (float64): one hypothesis (token ids) against a slot."""
    L = len(tokens)
    weights, norms = [], []
    for k in range(4):
        w, sq = {}, 0.0
        for i in range(L - k):
            ngram = tuple(tokens[i:i + k + 1])
            if ngram in w:
                continue
            tf = sum(1 for j in range(L - k) if tuple(tokens[j:j + k + 1]) == ngram)
            node, idf = 0, None
            for j in range(k + 1):
                at = _find(arrays['idf_key'], arrays['idf_start'][j], arrays['idf_start'][j + 1], (node << 32) | ngram[j])
                if at < 0:
                    idf = arrays['log_corpus']
                    break
                node, idf = at - arrays['idf_start'][j], float(arrays['idf_val'][at])
            w[ngram] = tf * idf
            sq += w[ngram] * w[ngram]
        weights.append(w)
        norms.append(math.sqrt(sq))
    r0, r1 = arrays['slot_ref_start'][slot], arrays['slot_ref_start'][slot + 1]
    total = 0.0
    for r in range(r0, r1):
        delta = float(max(L - 1, 0) - arrays['ref_len'][r])
        penalty = math.exp(-(delta * delta) / (2.0 * arrays['sigma'] ** 2))
        sim = 0.0
        for k in range(4):
            e0, e1 = arrays['ref_ent_start'][4 * r + k], arrays['ref_ent_start'][4 * r + k + 1]
            ref = {tuple(int(x) for x in arrays['ent_tok'][e][:k + 1]): float(arrays['ent_w'][e]) for e in range(e0, e1)}
            assert all((arrays['ent_tok'][e][k + 1:] == -1).all() for e in range(e0, e1))
            val = sum(min(wh, ref[g]) * ref[g] for g, wh in weights[k].items() if g in ref)
            nr = float(arrays['ref_norm'][r][k])
            if norms[k] != 0 and nr != 0:
                val /= norms[k] * nr
            sim += val * penalty
        total += sim / 4
    return total / (r1 - r0) * 10.0


def test_packed_arrays_reproduce_the_reference_generated_scores():
    """Fixture G14 (scores written by the reference's own cider_scorer.py): vocabulary = G14's words + specials, one slot per image,
    then a walk over the packed idf trie and reference entries -- no Cider call on the hypothesis side."""
    from grit_amd.datasets.caption.metrics import Cider
    from grit_amd.ops.cider import DeviceCider
    g, train, gts, res = _g14()
    words = sorted({w for caps in list(train.values()) + list(gts.values()) + list(res.values()) for c in caps for w in c.split()})
    itos = ['<unk>', '<pad>', '<bos>', '<eos>'] + words
    stoi = {w: i for i, w in enumerate(itos)}
    dc = DeviceCider(Cider(train), itos, device='cpu')
    keys = sorted(gts)
    slots = dc.reference_slots([gts[k] for k in keys])
    seen = {}  # one slot per distinct caption list, kept when the image comes again
    assert all(seen.setdefault(tuple(gts[k]), s) == s for k, s in zip(keys, slots)) and len(seen) == dc.n_slots == max(slots) + 1
    assert dc.reference_slots([gts[keys[-1]], gts[keys[0]]]) == [slots[-1], slots[0]]
    arrays = dc.host_arrays()
    for a, b in zip(arrays['idf_start'][:-1], arrays['idf_start'][1:]):
        assert (np.diff(arrays['idf_key'][a:b]) > 0).all()  # sorted and exact: no two n-grams share a key
    scores = []
    for k, slot in zip(keys, slots):
        ids = [stoi[w] for w in res[k][0].split()] + [EOS, 5, 6]
        scores.append(_walk(arrays, dc.expand(ids), slot))
    np.testing.assert_allclose(scores, g["scores"], rtol=1e-12, atol=0)


def test_interface_switches():
    from grit_amd.config import default_config
    from grit_amd.datasets.caption.metrics import Cider
    from grit_amd.engine.caption_engine import cider_reward_fn
    from grit_amd.ops.cider import DeviceCider

    class Field(object):  # the slice of TextField the reward needs (tests/test_metrics.py)
        itos = ['<unk>', '<pad>', '<bos>', '<eos>', 'a', 'dog', 'cat', 'sits', 'runs']

        def decode(self, rows):
            return [_decode(self.itos, r) for r in rows.tolist()]

    cider = _tiny_cider()
    tokens = torch.tensor([[[4, 5, 7, 3], [4, 6, 7, 3]], [[4, 6, 8, 3], [4, 5, 3, 3]]])
    batch = {'captions': [["A dog sits.", "a dog runs"], ["a cat runs", "A cat sits"]]}
    default = cider_reward_fn(cider, Field())(tokens, batch)
    host = cider_reward_fn(cider, Field(), reward='host')(tokens, batch)
    assert default.dtype == torch.float32 and default.shape == (2, 2) and torch.equal(default, host)

    assert default_config().optimizer.sc_reward == 'host'

    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        cider_reward_fn(cider, Field(), reward='device')(tokens, batch)
    with pytest.raises(ValueError):
        cider_reward_fn(cider, Field(), tokenize=lambda c: c, reward='device')
    with pytest.raises(ValueError):
        cider_reward_fn(cider, Field(), reward='somewhere')
    with pytest.raises(ValueError):
        DeviceCider(Cider(), Field.itos, device='cpu')
    with pytest.raises(ValueError):
        cider_reward_fn(Cider(), Field(), reward='device')
