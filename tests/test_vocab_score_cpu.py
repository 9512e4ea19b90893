"""Caption likelihood scoring without a GPU: the composed form of the head (ops/vocab_score.py vocab_score_host), the split of
CaptionGenerator.forward into `hidden` + projection, Transformer.score / Ensemble.score, engine.caption_engine.score_captions and
evaluate_loss(head='fused'), and the --score plumbing of inference_caption.  The oracle of every value is float64 torch or the
existing model(samples, captions) path."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import build_model, load, oracle_ops, t
from tests.test_ensemble_cpu import g16_features, g16_member

PAD, BOS, EOS = 1, 2, 3


# ------------------------------------------------------------------------------------------------------------------- the head
def test_host_head_hand_computed():
    from grit_amd.ops.vocab_score import vocab_score_host
    # x = rows of the identity (padded to D = 4): logits of row r are column r of w
    x = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 2, 0]])
    w = torch.tensor([[0., 1, 0, 9], [math.log(2), 1, 0, 9], [math.log(3), 1, 0, 9], [0., 1, 0.5, 9], [0., 1, 0, 9]])  # [V = 5, D = 4]
    target = torch.tensor([2, 0, 3])
    logp, lse = vocab_score_host(x, w, target, pad_idx=99)
    # row 0: logits (0, ln2, ln3, 0, 0): sum of exp = 1 + 2 + 3 + 1 + 1 = 8; row 1: five ones; row 2: (0, 0, 0, 1, 0)
    want_lse = [math.log(8), 1 + math.log(5), math.log(4 + math.e)]
    want_lp = [math.log(3) - want_lse[0], 1 - want_lse[1], 1 - want_lse[2]]
    assert logp.dtype == lse.dtype == torch.float32 and logp.shape == lse.shape == (3,)
    np.testing.assert_allclose(lse.double().numpy(), want_lse, rtol=0, atol=4 * 2.0 ** -23)
    np.testing.assert_allclose(logp.double().numpy(), want_lp, rtol=0, atol=4 * 2.0 ** -23)


def test_host_head_pad_out_of_range_and_float64_lse():
    from grit_amd.ops.vocab_score import vocab_score_host
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(6, 64, generator=g), torch.randn(37, 64, generator=g) * 0.3
    target = torch.tensor([5, PAD, 37, -1, 36, 0])
    logp, lse = vocab_score_host(x, w, target, PAD)
    logits = x.double() @ w.double().t()
    want_lse = torch.logsumexp(logits, -1)
    want = logits.gather(1, target.clamp(0, 36)[:, None])[:, 0] - want_lse
    assert logp[1].item() == 0.0 and not np.signbit(logp[1].item())
    assert torch.isnan(logp[2]) and torch.isnan(logp[3])
    for r in (0, 4, 5):
        assert abs(logp[r].item() - want[r].item()) < 1e-5
    np.testing.assert_allclose(lse.double().numpy(), want_lse.numpy(), rtol=0, atol=37 * 2.0 ** -23 + 8 * 2.0 ** -22)
    # a pad index outside the vocabulary is still pad, not out of range
    assert vocab_score_host(x, w, torch.full((6,), -7), -7)[0].eq(0).all()
    # bf16 operands on the CPU take the float32 projection of the same operands
    lp16, _ = vocab_score_host(x.bfloat16(), w.bfloat16(), target, PAD)
    ref16 = F.log_softmax(F.linear(x.bfloat16().float(), w.bfloat16().float()), -1)
    assert torch.equal(lp16[0], ref16[0, 5])


def test_supported_is_false_without_a_device():
    from grit_amd.ops import vocab_score as vs
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(9, 64, dtype=torch.bfloat16)
    assert not vs.supported(x, w)
    from grit_amd import lib
    with pytest.raises(lib.GritHipError):
        vs.vocab_score(x, w, torch.zeros(4, dtype=torch.int64), PAD)


# ------------------------------------------------------------------------------------------------------------------ the model
def test_hidden_plus_projection_is_forward_bit_for_bit():
    model, _ = build_model(2)
    model.eval()
    g = load("model_g7.npz")
    vis = {k: t(g[k]) for k in ("gri_feat", "gri_mask", "reg_feat", "reg_mask")}
    model.cached_features = True
    with oracle_ops(), torch.no_grad():
        vis = model._visual_inputs(vis)
        gen = model.cap_generator
        want = gen(t(g["seq"]), vis)
        hidden = gen.hidden(t(g["seq"]), vis)
        got = F.log_softmax(F.linear(hidden.float(), gen.fc.weight.float()), dim=-1)
    assert hidden.shape == (1, 20, 512)
    assert torch.equal(got, want)


@pytest.fixture(scope="module")
def scorer():
    model, cfg = g16_member(0)
    model.cached_features = True
    feats = g16_features(load("ensemble_g16.npz"))
    return model, cfg, feats


def _captions():
    # image 0: N = 3 captions: full length, pad at the end, a pad INSIDE (a hole the loss ignores)
    a = [BOS, 11, 12, 13, 14, 15, EOS]
    b = [BOS, 21, 22, EOS, PAD, PAD, PAD]
    c = [BOS, 31, PAD, 33, EOS, PAD, PAD]
    return torch.tensor([[a, b, c], [b, c, a], [c, a, b]])  # [B = 3, N = 3, T = 7]


def test_transformer_score_against_the_teacher_forcing_path(scorer):
    model, _, feats = scorer
    caps = _captions()
    with oracle_ops(), torch.no_grad():
        got = model.score(feats, caps)
        assert type(got).__name__ == "CaptionScores" and got._fields == ("log_probs", "total", "length")
        assert got.log_probs.shape == (3, 3, 6) and got.log_probs.dtype == torch.float32
        assert got.total.shape == (3, 3) and got.length.shape == (3, 3) and got.length.dtype == torch.int64
        np.testing.assert_array_equal(got.length.numpy(), [[6, 3, 3], [3, 3, 6], [3, 6, 3]])
        for n in range(3):  # the target shift: position t is scored against token t + 1 of the existing path's log-softmax
            full = model(feats, caps[:, n])  # [B, T, V]
            target = caps[:, n, 1:]
            want = full[:, :-1].gather(-1, target.unsqueeze(-1)).squeeze(-1) * (target != PAD)
            # N captions in one call against separate calls: float32 round-off of the decoder (batch 9 against batch 3)
            np.testing.assert_allclose(got.log_probs[:, n].numpy(), want.numpy(), rtol=0, atol=2e-4)
            alone = model.score(feats, caps[:, n])
            np.testing.assert_allclose(got.log_probs[:, n].numpy(), alone.log_probs[:, 0].numpy(), rtol=0, atol=2e-4)
            assert torch.equal(alone.log_probs[:, 0], want)  # same batch, same decoder run: the same floats
        assert (got.log_probs[caps[..., 1:] == PAD] == 0).all()
        assert torch.equal(got.total, got.log_probs.sum(-1))
        mean = model.score(feats, caps, normalize='mean')
        assert torch.equal(mean.total, got.total / got.length) and torch.equal(mean.log_probs, got.log_probs)
        two, three = model.score(feats, caps[:, 0]), model.score(feats, caps[:, :1])
        assert two.log_probs.shape == (3, 1, 6)
        for x, y in zip(two, three):
            assert torch.equal(x, y)


def test_transformer_score_refusals(scorer):
    model, cfg, feats = scorer
    caps = _captions()
    with oracle_ops():
        with pytest.raises(RuntimeError, match="no_grad"):
            model.score(feats, caps)  # autograd on
        model.train()
        try:
            with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
                model.score(feats, caps)
        finally:
            model.eval()
        with torch.no_grad():
            too_long = torch.full((3, cfg.model.max_len + 1), 7)
            with pytest.raises(ValueError, match="position table"):
                model.score(feats, too_long)
            model.score(feats, too_long[:, :-1])  # max_len tokens fit
            with pytest.raises(ValueError, match="normalize"):
                model.score(feats, caps, normalize='sum')
            with pytest.raises(ValueError, match="int64"):
                model.score(feats, caps.int())
            with pytest.raises(ValueError, match="images"):
                model.score(feats, caps[:2])


def test_ensemble_score_is_the_stacked_mean(scorer):
    from grit_amd.models.caption.ensemble import Ensemble
    a, _, feats = scorer
    b, _ = g16_member(1)
    caps = _captions()
    ens = Ensemble([a, b]).eval()
    with oracle_ops(), torch.no_grad():
        got = ens.score(feats, caps, normalize='mean')
        b.cached_features = True
        want = torch.stack([a.score(feats, caps).log_probs, b.score(feats, caps).log_probs]).mean(0)
        b.cached_features = False
        assert torch.equal(got.log_probs, want)
        assert torch.equal(got.total, want.sum(-1) / got.length)
        per_member = ens.score([feats, feats], caps)
        assert torch.equal(per_member.log_probs, want)
        with pytest.raises(NotImplementedError, match="teacher-forcing"):
            ens(feats, caps[:, 0])
    assert b.cached_features is False


# ----------------------------------------------------------------------------------------------------------------- the engine
def test_evaluate_loss_fused_head_and_score_captions(scorer):
    from torch.nn import NLLLoss
    from grit_amd.config import default_config
    from grit_amd.engine import caption_engine as ce
    model, _, feats = scorer
    caps = _captions()
    batches = [{'samples': feats, 'captions': caps[:, 0]}, {'samples': feats, 'captions': caps[:, 2]}]
    loss_fn = NLLLoss(ignore_index=PAD)
    with oracle_ops():
        want = ce.evaluate_loss(model, batches, loss_fn, None, 0, None, head='torch')
        got = ce.evaluate_loss(model, batches, loss_fn, None, 0, None, head='fused')
        assert want == ce.evaluate_loss(model, batches, loss_fn, None, 0, None)  # the default is the reference's loop
        # a mean of <= 12 float32 log-probs per batch in two orders
        assert abs(got - want) <= 16 * 2.0 ** -23 * abs(want)
        with pytest.raises(ValueError, match="head"):
            ce.evaluate_loss(model, batches, loss_fn, None, 0, None, head='cuda')
        with pytest.raises(ValueError, match="pad"):
            ce.evaluate_loss(model, batches, NLLLoss(ignore_index=0), None, 0, None, head='fused')
        model.train()
        scores = ce.score_captions(model, feats, caps, normalize='mean')  # switches to eval / no_grad and back
        assert model.training
        model.eval()
        with torch.no_grad():
            assert torch.equal(scores.total, model.score(feats, caps, normalize='mean').total)
    assert default_config().exp.eval_loss_head == 'torch'
    assert ce._eval_loss_head(default_config(**{'exp.eval_loss_head': 'fused'})) == 'fused'


# -------------------------------------------------------------------------------------------------------------------- the CLI
def test_caption_ids_and_parser():
    import inference_caption as ic
    itos = ['<unk>', '<pad>', '<bos>', '<eos>', 'a', 'dog', 'catches', 'frisbee']
    ids = ic.caption_ids(["A dog  catches a Frisbee", "a dog"], itos, BOS, EOS, PAD)
    assert ids.dtype == torch.int64
    assert ids.tolist() == [[BOS, 4, 5, 6, 4, 7, EOS], [BOS, 4, 5, EOS, PAD, PAD, PAD]]
    assert ic.caption_ids("a dog", {w: i for i, w in enumerate(itos)}, BOS, EOS, PAD).tolist() == [[BOS, 4, 5, EOS]]
    with pytest.raises(ValueError, match="'zebra'"):
        ic.caption_ids(["a zebra"], itos, BOS, EOS, PAD)
    with pytest.raises(ValueError, match="no word"):
        ic.caption_ids(["  "], itos, BOS, EOS, PAD)
    a = ic.parse_args(['--img', 'x.npy', '--score', 'a dog', 'a frisbee', '--checkpoint', 'p.pth', 'q.pth'])
    assert a.score == ['a dog', 'a frisbee'] and a.checkpoint == ['p.pth', 'q.pth']
    assert ic.parse_args(['--img', 'x.npy']).score == []
    for extra in (['--sample', '3'], ['--force', 'dog'], ['--consensus', '--n-best', '3', '--consensus-corpus', 'c.json']):
        with pytest.raises(SystemExit):
            ic.parse_args(['--img', 'x.npy', '--score', 'a dog'] + extra)

