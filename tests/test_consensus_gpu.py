"""Consensus reranking on the device (grit_cider_consensus, grit_amd/csrc/consensus.hip) against the host form
(grit_amd/ops/consensus.py: consensus_host) on the overlapping candidates of tests/test_consensus_cpu.py: recipe, its limits and
edge rows, tables without references, determinism and freedom from synchronisation, the kernels it shares a header with, and the
model-level paths (decode_consensus, evaluate_metrics(consensus=...)).

Bounds.  sim and the float64 score: rtol 1e-11, atol 0 -- the bound tests/test_cider_device_gpu.py derives for this arithmetic: a
similarity is a sum of non-negative terms (idf >= 0), fewer than 200 roundings of 1.1e-16 plus exp / sqrt / division at <= 1 ulp
each give about 3e-14; a score adds at most 31 such non-negative similarities (31 more roundings, no cancellation), one division
and one product: still below 1e-13.  1e-11 leaves two orders for a different libm.  float32 score: at most one float32 ulp from
float32(reference) (double rounding).  best: equal to the host's wherever the host's winner is clear by more than 1e-9 relative
(near_ties of the CPU file: two orders above the bound, so a device argmax cannot differ there); in a near tie the chosen
candidate's host score is within 1e-9 relative of the host maximum."""
import numpy as np
import pytest
import torch

from tests.helpers import build_model, load, t
from tests.test_consensus_cpu import CASES, EOS, host_case, recipe, setup

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def tables():
    from grit_amd.ops.cider import DeviceCider
    itos, cider = setup()[:2]
    return DeviceCider(cider, itos, device=DEV)


def assert_against_host(what, got, ref, tie, tokens, log_probs):
    sim, score, best = ref
    d_sim, d_score, d_best = got.sim.cpu().numpy(), got.score64.cpu().numpy(), got.best.cpu().numpy()
    d32 = got.score.cpu().numpy()
    ref32 = score.astype(np.float32)
    ulps = np.abs(d32.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30))).astype(np.float64)
    nz = sim != 0
    rel = (np.abs(d_sim - sim)[nz] / sim[nz]).max() if nz.any() else 0.0
    print("%s: %d similarities non-zero of %d, max rel err %.3g, float32 max ulp %.3g, %d near ties, best differs in %d images"
          % (what, int(nz.sum()), sim.size, rel, ulps.max(), int(tie.sum()), int((d_best != best).sum())))
    assert got.sim.dtype == got.score64.dtype == torch.float64 and got.score.dtype == torch.float32 and got.best.dtype == torch.int64
    assert np.isfinite(d_sim).all() and (got.bad.cpu().numpy() == 0).all()
    np.testing.assert_allclose(d_sim, sim, rtol=1e-11, atol=0)
    np.testing.assert_allclose(d_score, score, rtol=1e-11, atol=0)
    assert (ulps <= 1.0).all(), (what, ulps.max())
    assert np.array_equal(d_best[~tie], best[~tie])
    for b in np.nonzero(tie)[0]:
        assert abs(score[b, d_best[b]] - score[b, best[b]]) <= 1e-9 * abs(score[b, best[b]])
    B, n, T = tokens.shape
    rows = torch.arange(B, device=DEV)
    assert got.tokens.shape == (B, 1, T) and torch.equal(got.tokens[:, 0], tokens[rows, got.best])
    assert torch.equal(got.log_probs[:, 0].view(torch.int32), log_probs[rows, got.best].view(torch.int32))  # bit for bit


@pytest.mark.parametrize("collapse", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-n%d-T%d" % c[:3])
def test_kernel_against_the_host_form(tables, case, collapse):
    tokens, ref, _, tie = host_case(*case, collapse)
    tok = t(tokens.copy(), device=DEV)
    log_probs = -torch.rand(tok.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(case[3]))
    got = tables.consensus(tok, log_probs, collapse=collapse, return_matrix=True)
    assert_against_host("%r collapse %s" % (case, collapse), got, ref, tie, tok, log_probs)
    plain = tables.consensus(tok, collapse=collapse)
    assert plain.log_probs is None and plain.sim is None and plain.score64 is None
    assert torch.equal(plain.best, got.best) and torch.equal(plain.score, got.score) and torch.equal(plain.tokens, got.tokens)


def test_near_ties_are_rare(tables):
    images = ties = 0
    for collapse in (True, False):
        for case in CASES:
            if case[1] > 1:
                tie = host_case(*case, collapse)[3]
                images, ties = images + len(tie), ties + int(tie.sum())
    assert ties <= 0.05 * images


def test_limits(tables):
    """A row that expands to exactly GRIT_CIDER_MAX_TOKENS tokens, one that would exceed it, and 33 candidates."""
    from grit_amd import lib
    from grit_amd.ops.cider import DeviceCider
    from grit_amd.ops.consensus import consensus_host
    from tests.test_consensus_cpu import g14
    cider, itos, _ = g14()
    itos = itos + ['$1$2$3$4']  # eight tokens: $ 1 $ 2 $ 3 $ 4
    E, MAX = lib.CIDER_MAX_EXPANSION, lib.CIDER_MAX_TOKENS
    tables = DeviceCider(cider, itos, device=DEV)
    widest = len(itos) - 1
    assert int(tables._meta_host[widest] & 15) == E and MAX % E == 0
    T = MAX // E                                            # T words at the widest expansion fill the row exactly
    rng = np.random.RandomState(5)
    pool = np.arange(4, len(itos) - 1)
    tokens = np.full((2, 3, T), widest, np.int64)           # no <eos>: T words, T * E tokens
    tokens[0, 1, T // 2:] = rng.choice(pool, T - T // 2)
    tokens[0, 2, ::2] = rng.choice(pool, (T + 1) // 2)
    tokens[1] = rng.choice(pool, (3, T))
    tokens[1, :, 10] = EOS
    assert len(tables.expand(tokens[0, 0].tolist())) == MAX
    for collapse in (False, True):
        ref = consensus_host(cider, itos, tokens, collapse=collapse)
        got = tables.consensus(t(tokens, device=DEV), collapse=collapse, return_matrix=True)
        np.testing.assert_allclose(got.sim.cpu().numpy(), ref[0], rtol=1e-11, atol=0)
        np.testing.assert_allclose(got.score64.cpu().numpy(), ref[1], rtol=1e-11, atol=0)
        assert (ref[1][0] > 0).all() and np.array_equal(got.best.cpu().numpy(), ref[2])
    assert lib.load().grit_cider_consensus_workspace(2, 3, T + 1) > 0  # the size function does not know the tables' width
    for shape in ((2, 3, T + 1), (1, 33, 8)):
        with pytest.raises(lib.GritHipError, match="grit_cider_consensus failed"):
            tables.consensus(torch.full(shape, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(lib.GritHipError):
        tables.consensus(torch.full((1, 2, 8), 4, dtype=torch.int64))  # on the CPU


def test_edge_rows(tables):
    itos, cider = setup()[:2]
    from grit_amd.ops.consensus import consensus_host
    V, n, T = len(itos), 5, 12
    base = recipe(6, n, T, 21)
    tokens = base.copy()
    tokens[0, 2, 0] = EOS                       # image 0: one empty candidate
    tokens[1, :, 0] = EOS                       # image 1: all empty
    tokens[2] = tokens[2, 0]                    # image 2: all identical
    cut = [list(tokens[3, i]).index(EOS) for i in range(n)]
    tokens[3, 1, cut[1] - 1] = V                # image 3: an id >= V in front of <eos>
    tokens[4, 3, 0] = -1                        # image 4: an id < 0 in front of <eos>
    cut5 = list(tokens[5, 0]).index(EOS)
    tokens[5, 0, cut5 + 1:] = [V, -1, V + 5, -7][:T - cut5 - 1] + [V] * max(0, T - cut5 - 5)   # image 5: the same ids behind <eos>
    got = tables.consensus(t(tokens, device=DEV), return_matrix=True)
    sim, score, best, bad = (x.cpu().numpy() for x in (got.sim, got.score64, got.best, got.bad))
    good = [0, 1, 2, 5]
    ref = consensus_host(cider, itos, tokens[good])
    np.testing.assert_allclose(sim[good], ref[0], rtol=1e-11, atol=0)
    np.testing.assert_allclose(score[good], ref[1], rtol=1e-11, atol=0)
    assert bad.tolist() == [0, 0, 0, 1, 1, 0]
    assert (sim[0, 2] == 0).all() and (sim[0, :, 2] == 0).all() and score[0, 2] == 0 and score[0].max() > 0
    assert (score[1] == 0).all() and best[1] == 0
    assert len(set(score[2].tolist())) == 1 and score[2, 0] > 0 and best[2] == 0
    for b in (3, 4):
        assert np.isnan(score[b]).all() and np.isnan(sim[b]).all() and best[b] == 0
        assert torch.isnan(got.score[b]).all() and torch.equal(got.tokens[b, 0].cpu(), torch.from_numpy(tokens[b, 0]))
    unhurt = consensus_host(cider, itos, base[[5]])
    assert np.array_equal(ref[1][3], unhurt[1][0]) and best[5] == unhurt[2][0] and best[0] == ref[2][0]
    for bad_image in (3, 4):
        with pytest.raises(ValueError):
            consensus_host(cider, itos, tokens[[bad_image]])


def test_tables_without_references_and_the_kernels_that_share_the_header():
    """A DeviceCider that has cooked nothing runs consensus; reward() and the evaluation's scores on one fixed input give the same
    bits before and after consensus calls in the process, and the object's rewards equal a fresh object's."""
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    from grit_amd.ops.cider import DeviceCider
    itos, cider = setup()[:2]
    tokens, ref, _, tie = host_case(*CASES[2], True)
    tok = t(tokens.copy(), device=DEV)
    captions = [[' '.join(itos[i] for i in row[:6]) for row in image[:2]] for image in tokens.tolist()]
    fresh = DeviceCider(cider, itos, device=DEV)
    before32, before64 = fresh.reward(tok, captions, return_float64=True)
    scorer = DeviceCaptionScorer(captions, itos, device=DEV)
    scores_before = scorer.launch(tok[:, 0])
    used = DeviceCider(cider, itos, device=DEV)
    assert used.n_slots == 0
    got = used.consensus(tok, return_matrix=True)
    np.testing.assert_allclose(got.score64.cpu().numpy(), ref[1], rtol=1e-11, atol=0)
    assert np.array_equal(got.best.cpu().numpy()[~tie], ref[2][~tie]) and used.n_slots == 0
    after32, after64 = used.reward(tok, captions, return_float64=True)
    again = used.consensus(tok, return_matrix=True)
    assert torch.equal(again.score64, got.score64) and torch.equal(again.sim, got.sim)
    assert torch.equal(after32, before32) and torch.equal(after64, before64) and (before64 > 0).any()
    same32, same64 = fresh.reward(tok, captions, return_float64=True)
    assert torch.equal(same32, before32) and torch.equal(same64, before64)
    for a, b in zip(scorer.launch(tok[:, 0]), scores_before):
        assert torch.equal(a, b)


def test_determinism_and_no_synchronisation(tables):
    tokens = t(host_case(*CASES[3], True)[0].copy(), device=DEV)
    log_probs = -torch.rand(tokens.shape, device=DEV)
    first = tables.consensus(tokens, log_probs, return_matrix=True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        second = tables.consensus(tokens, log_probs, return_matrix=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    third = tables.consensus(tokens, log_probs, return_matrix=True)
    for other in (second, third):
        for a, b in zip(first, other):
            assert torch.equal(a, b)
        assert torch.equal(first.sim.view(torch.int64), other.sim.view(torch.int64))
        assert torch.equal(first.score64.view(torch.int64), other.score64.view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------- model level
class Field(object):
    eos_token = '<eos>'

    def __init__(self, itos):
        self.itos = list(itos)


class Loader(object):
    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


@pytest.fixture(scope="module")
def captioner():
    from grit_amd.utils.misc import NestedTensor
    g = load("sc_g9.npz")
    model, cfg = build_model(3, **{'model.dropout': 0.0, 'model.detector.dropout': 0.0})
    model.to(DEV).eval()
    cfg.model.beam_size, cfg.model.beam_len = 5, 20
    images = t(g["images"], device=DEV)
    B = images.shape[0]
    sample = lambda lo, hi: NestedTensor(images[lo:hi], torch.zeros(hi - lo, *images.shape[-2:], dtype=torch.bool, device=DEV))
    cut = max(1, B // 2)
    return model, cfg, [sample(0, cut), sample(cut, B)] if B > 1 else [sample(0, B)]


def host_choice(tokens):
    from grit_amd.ops.consensus import candidate_captions, consensus_host
    from tests.test_consensus_cpu import near_ties
    itos, cider = setup()[:2]
    _, score, best = consensus_host(cider, itos, tokens.cpu())
    return score, best, near_ties(candidate_captions(itos, tokens.cpu()), score, best)


@pytest.mark.parametrize("decode,n", [("sample", 8), ("beam", 5)])
def test_decode_consensus_returns_the_hosts_row(captioner, tables, decode, n):
    from grit_amd.config import beam_constraints, beam_groups
    from grit_amd.engine.caption_engine import decode_consensus
    model, cfg, batches = captioner
    cfg.model.consensus_candidates, cfg.model.consensus_decode, cfg.model.consensus_seed = n, decode, 1234
    try:
        for samples in batches:
            common = dict(seq=None, use_beam_search=True, max_len=20, eos_idx=EOS)
            with torch.no_grad():
                if decode == 'sample':
                    cands, lps = model(samples, beam_size=n, out_size=n, decode='sample', temperature=1.0, top_k=0, top_p=1.0, seed=1234,
                                       **common)
                else:
                    cands, lps = model(samples, beam_size=5, out_size=n, return_probs=False, **beam_constraints(cfg),
                                       **beam_groups(cfg), **common)
            tokens, log_probs = decode_consensus(model, samples, cfg, tables.consensus)
            B = cands.shape[0]
            assert cands.shape[:2] == (B, n) and tokens.shape == (B, 1, cands.shape[-1]) == log_probs.shape
            score, best, tie = host_choice(cands)
            print(decode, "host scores", np.round(score, 3).tolist(), "best", best.tolist(), "near ties", tie.tolist())
            for b in range(B):
                if not tie[b]:
                    assert torch.equal(tokens[b, 0], cands[b, best[b]]) and torch.equal(log_probs[b, 0], lps[b, best[b]])
                else:
                    row = next(i for i in range(n) if torch.equal(tokens[b, 0], cands[b, i]))
                    assert abs(score[b, row] - score[b, best[b]]) <= 1e-9 * abs(score[b, best[b]])
    finally:
        cfg.model.consensus_candidates, cfg.model.consensus_decode, cfg.model.consensus_seed = 0, 'beam', None


def test_evaluate_metrics_scores_the_chosen_rows(captioner):
    from grit_amd.engine.caption_engine import decode_consensus, evaluate_metrics
    from grit_amd.ops.cider import DeviceCider
    itos, cider = setup()[:2]
    model, cfg, samples = captioner
    field = Field(itos)
    captions = [['a man sitting on a table', 'two people standing next to a street'], ['a woman holding a white plate']]
    batches = [{'samples': s, 'captions': [captions[(i + b) % 2] for b in range(s.tensors.shape[0])]} for i, s in enumerate(samples)]
    plain, _ = evaluate_metrics(model, None, batches, None, config=cfg)
    off, _ = evaluate_metrics(model, None, batches, field, config=cfg, consensus=cider)  # the keys are off
    assert all(torch.equal(a, b) for a, b in zip(plain, off))
    cfg.model.consensus_candidates = 5
    try:
        chosen, _ = evaluate_metrics(model, None, batches, field, config=cfg, consensus=cider)
        tables = next(iter(cider._device_scorers.values()))
        assert isinstance(tables, DeviceCider)  # kept on the Cider, as the device reward keeps its tables
        manual = [decode_consensus(model, b['samples'], cfg, tables.consensus)[0][:, 0] for b in batches]
        assert all(torch.equal(a, b) and a.shape == p.shape for a, b, p in zip(chosen, manual, plain))
        loader = Loader(batches)
        got = evaluate_metrics(model, None, loader, field, config=cfg, scorer='device', consensus=cider)
        ready = evaluate_metrics(model, None, Loader(batches), field, config=cfg, scorer='device', consensus=tables)  # a ready reranker
        scorer = loader._grit_caption_scorers[next(iter(loader._grit_caption_scorers))]
        want = scorer.aggregate(*scorer.launch(torch.cat(manual)))
        assert got == want == ready and set(got) == {'BLEU', 'ROUGE', 'CIDEr'}
        assert len(cider._device_scorers) == 1
    finally:
        cfg.model.consensus_candidates = 0
