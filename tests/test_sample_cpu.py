"""Sampled caption decoding without a GPU: the C ABI of grit_sample_step_f32, the host statement of its nine steps
(grit_amd/ops/sample.py: sample_step_host) on hand-written integer cases and as a distribution, Transformer.forward(decode='sample')
on fixture G15 under the oracle ops, and the self-critical step with optimizer.sc_decode = 'sample'."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import build_model, default_config, load, oracle_ops, t

FEATS = ("gri_feat", "gri_mask", "reg_feat", "reg_mask")
NOISE = 5e-5  # tests/test_beam_eos.py: fp32 round-off of a score through the 3-layer decoder
EOS = 3
ONE = 1 << 32  # top_p = 1
X_MAX = (1 << 64) - 1


def u64(*values):
    return np.array(values, np.uint64)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_symbol_and_constant():
    from grit_amd import abi, lib
    a = abi.read()
    assert "grit_sample_step_f32" in a.functions and len(a.functions["grit_sample_step_f32"][1]) == 18
    assert "grit_sample_step_f32" in lib.SIGNATURES
    assert a.constants["GRIT_SAMPLE_MAX_V"] == lib.SAMPLE_MAX_V >= 16384
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "grit_sample_step_f32")
    assert lib.load().grit_abi_version() == a.version >= 53


# ---------------------------------------------------------------------------------------------------------------- integer cases
ROW = np.array([-1.0, -2.0, -2.0, -2.0, -3.0], np.float32)  # one group of three equal log-probs
W = u64(8, 4, 4, 4, 2)                                      # explicit weights, S = 22


def kept(top_k, q32, row=ROW, w=W):
    from grit_amd.ops.sample import kept_host
    return np.nonzero(kept_host(row, w, top_k, q32))[0].tolist()


def test_prefix_selection_on_explicit_weights():
    assert kept(0, ONE) == [0, 1, 2, 3, 4]
    assert kept(3, ONE) == [0, 1, 2]                       # the top-k boundary inside the tie group: by index
    assert kept(2, ONE) == [0, 1]
    assert kept(5, ONE) == kept(15, ONE) == [0, 1, 2, 3, 4]  # top_k >= V
    q = int(round(0.6 * ONE))
    assert kept(0, q) == [0, 1, 2]                         # need = floor(0.6 * 22) = 13: sums 8, 12, 16 -> the boundary is in the group
    assert kept(3, q) == [0, 1]                            # S_K = 16, need = 9: sums 8, 12
    assert kept(0, int(round(8 / 22 * ONE)) + 1) == [0]    # need = 8 is reached by the first word alone
    assert kept(0, 1) == [0]                               # (1 * 22) >> 32 = 0: need is clamped to 1, one word stays
    assert kept(1, ONE, np.array([-1.0, -0.5, -0.5], np.float32), u64(5, 9, 9)) == [1]  # top_k = 1: the lowest-index argmax
    assert kept(0, ONE // 2, np.array([-0.0, 0.0, -1.0], np.float32), u64(4, 4, 1)) == [0]  # -0.0 == +0.0: by index


def test_pick_on_explicit_weights():
    from grit_amd.ops.sample import pick_host
    everything = np.ones(5, bool)
    assert pick_host(W, everything, 0) == 0                      # target = 0
    assert pick_host(W, everything, X_MAX) == 4                  # target = S - 1
    assert pick_host(W, everything, (8 << 64) // 22 + 1) == 1    # target = 8: the first word's weights are 0 .. 7
    assert pick_host(W, everything, (8 << 64) // 22 - 1) == 0    # target = 7
    some = np.array([False, True, False, True, False])
    assert pick_host(W, some, 0) == 1 and pick_host(W, some, X_MAX) == 3 and pick_host(W, some, 1 << 63) == 3  # target 4 of 8
    assert pick_host(u64(0, 0, 6, 0), np.ones(4, bool), 0) == 2  # zero weights are never picked


def test_finished_rows_and_greedy_rows():
    from grit_amd.ops.sample import sample_step_host
    rng = np.random.default_rng(5)
    logp = torch.log_softmax(torch.from_numpy(rng.normal(0, 3, (6, 50)).astype(np.float32)), -1).numpy()
    logp[4, 7] = logp[4, 31] = logp[4].max() + 0.5  # a tied maximum
    prev = np.array([5, EOS, 9, 0, 8, EOS], np.int64)
    alive_in = np.array([1, 1, 0, 1, 1, 0], np.float32)
    words, picked, alive = sample_step_host(logp, 6, 1, prev, alive_in, EOS, 0, 1.0, 1, ONE, 99, 4)
    np.testing.assert_array_equal(alive, [1, 0, 0, 1, 1, 0])
    for r in (1, 2, 5):
        assert words[r] == 0 and picked[r] == 0 and not np.signbit(picked[r])
    for r in (0, 3):
        assert words[r] == logp[r].argmax() and picked[r] == logp[r].max()
    assert words[4] == 7
    fill = sample_step_host(logp, 6, 1, prev, alive_in, EOS, 17, 1.0, 0, ONE, 99, 4)[0]
    assert fill[1] == fill[2] == fill[5] == 17
    first = sample_step_host(logp[:2], 6, 3, None, None, EOS, 0, 1.0, 0, ONE, 99, 0)
    assert first[2].tolist() == [1] * 6 and all(first[1][r] == logp[r // 3, first[0][r]] for r in range(6))
    with pytest.raises(ValueError):
        sample_step_host(logp, 6, 1, prev, None, EOS, 0, 1.0, 0, ONE, 99, 4)
    with pytest.raises(ValueError):
        sample_step_host(logp, 6, 1, None, None, EOS, 0, 1.0, 0, ONE, 99, 4096)


# ---------------------------------------------------------------------------------------------------------------- distribution
@pytest.mark.parametrize("inv_t", [0.5, 1.0, 2.0])
def test_weights_follow_the_tempered_softmax(inv_t):
    from grit_amd.ops.sample import weights_host
    logits = np.random.default_rng(int(inv_t * 10)).normal(0, 3, 10201)
    logp = torch.log_softmax(torch.from_numpy(logits.astype(np.float32)), 0).numpy()
    w = weights_host(logp, inv_t)
    assert int(w.max()) == 1 << 40
    p = w.astype(np.float64) / float(w.sum())
    x = logp.astype(np.float64) * inv_t
    q = np.exp(x - x.max())
    q /= q.sum()
    tv = 0.5 * np.abs(p - q).sum()
    print("total variation at inv_T %g: %.3g" % (inv_t, tv))
    assert tv <= 1e-6


def test_draws_follow_the_weights():
    from grit_amd.ops.sample import sample_step_host
    p = np.array([0.30, 0.20, 0.15, 0.10, 0.10, 0.08, 0.05, 0.02])
    logp = np.log(p).astype(np.float32)[None]
    n = 200000
    words = sample_step_host(logp, n, n, None, None, EOS, 0, 1.0, 0, ONE, 12345, 0)[0]
    expected = np.exp(logp[0].astype(np.float64))
    expected *= n / expected.sum()
    chi2 = float(((np.bincount(words, minlength=8) - expected) ** 2 / expected).sum())
    print("chi-square of %d draws over 8 words: %.3f" % (n, chi2))
    assert chi2 < 24.32  # the 99.9 % point at 7 degrees of freedom


# ---------------------------------------------------------------------------------------------------------------- fixture G15
def g15_model(device="cpu"):
    model, cfg = build_model(3)
    with torch.no_grad():
        model.cap_generator.fc.weight[EOS] *= 6.0
    return model.eval().to(device), cfg


def decode(model, vis, **kw):
    model.cached_features = True
    try:
        with torch.no_grad():
            return model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, **kw)
    finally:
        model.cached_features = False


def teacher_forced(model, vis, tokens):
    """log-probs [rows, T, V] of the decoder fed <bos> + tokens[:-1] ([rows, T]); vis has one entry per row"""
    bos = torch.full((tokens.shape[0], 1), model.bos_idx, dtype=torch.long, device=tokens.device)
    model.cached_features = True
    try:
        return model(vis, torch.cat([bos, tokens[:, :-1]], 1))
    finally:
        model.cached_features = False


def live_steps(tokens):
    """1 up to and including the first <eos> of every row of tokens [rows, T]"""
    ended = (tokens == EOS).long().cumsum(-1) - (tokens == EOS).long()
    return ended == 0


def check_greedy(model, vis):
    """decode='sample' with top_k = 1 against the model's beam-1 decode; returns how many images were compared"""
    tokens, lps = decode(model, vis, beam_size=3, out_size=3, decode='sample', top_k=1, seed=7)
    assert tokens.shape == lps.shape == (8, 3, 20)
    assert (tokens == tokens[:, :1]).all()  # three identical rows per image
    # their log-probs come from three rows of one decoder batch: equal up to the round-off of the fixture's own comparison
    print("largest log-prob difference between the samples of an image: %.3g" % (lps - lps[:, :1]).abs().max().item())
    np.testing.assert_allclose(lps.cpu().numpy(), lps[:, :1].expand_as(lps).cpu().numpy(), rtol=1e-4, atol=1e-4)
    beam1, beam1_lps = decode(model, vis, beam_size=1, out_size=1)
    with torch.no_grad():
        full = teacher_forced(model, vis, beam1)
    top2 = full.topk(2, -1).values
    live = live_steps(beam1)
    gaps = torch.where(live, top2[..., 0] - top2[..., 1], torch.full_like(top2[..., 0], float("inf"))).min(-1).values
    print("smallest top-two gaps over the live steps:", ["%.3g" % x for x in gaps.tolist()])
    pinned = gaps > 2 * NOISE
    assert int(pinned.sum()) >= 7
    assert torch.equal(tokens[pinned][:, 0], beam1[pinned])
    np.testing.assert_allclose(lps[pinned][:, 0].cpu().numpy(), beam1_lps[pinned].cpu().numpy(), rtol=1e-4, atol=1e-4)
    return tokens[:, 0], lps[:, 0], pinned


def check_eos_fill(tokens, lps, pinned):
    has = (tokens == EOS).any(-1)
    first = torch.where(has, (tokens == EOS).long().argmax(-1), torch.full_like(has, -1, dtype=torch.long))
    expected = torch.tensor([2, 2, 15, 7, -1, 9, 7, 9], device=tokens.device)
    assert torch.equal(first[pinned], expected[pinned])
    behind = ~live_steps(tokens)
    assert behind.any() and (tokens[behind] == 0).all() and (lps[behind] == 0).all()


def check_teacher_forced(model, vis, tokens, lps):
    B, n, T = tokens.shape
    rows = {k: v.repeat_interleave(n, 0) for k, v in vis.items()}
    flat = tokens.reshape(B * n, T)
    with torch.no_grad():
        full = teacher_forced(model, rows, flat)
    want = full.gather(-1, flat.unsqueeze(-1)).squeeze(-1) * live_steps(flat)
    np.testing.assert_allclose(lps.reshape(B * n, T).cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def g15():
    model, _ = g15_model()
    g = load("beam_g15.npz")
    return model, {k: t(g[k]) for k in FEATS}


def test_greedy_sampling_is_the_beam_of_one(g15):
    model, vis = g15
    with oracle_ops():
        tokens, lps, pinned = check_greedy(model, vis)
        check_eos_fill(tokens, lps, pinned)
    assert pinned.all()  # on the CPU path all eight images are above the line


def test_sampling_at_temperature_one(g15):
    model, vis = g15
    with oracle_ops():
        a, a_lps = decode(model, vis, beam_size=5, out_size=5, decode='sample', seed=11)
        b, _ = decode(model, vis, beam_size=5, out_size=5, decode='sample', seed=11)
        c, _ = decode(model, vis, beam_size=5, out_size=5, decode='sample', seed=12)
        two, _ = decode(model, vis, beam_size=5, out_size=2, decode='sample', seed=11)
        check_teacher_forced(model, vis, a, a_lps)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(two, a[:, :2])  # the first out_size of the n samples
    assert all(not (a[i] == a[i, :1]).all() for i in range(8))  # an image's five samples are not all equal
    behind = ~live_steps(a.reshape(40, 20))
    assert behind.any() and (a.reshape(40, 20)[behind] == 0).all() and (a_lps.reshape(40, 20)[behind] == 0).all()


def test_arguments_that_are_refused(g15):
    model, vis = g15
    with oracle_ops():
        with pytest.raises(ValueError, match="decode"):
            decode(model, vis, decode='greedy')
        with pytest.raises(NotImplementedError):
            decode(model, vis, decode='sample', return_probs=True)
        with pytest.raises(ValueError, match="top_p"):
            decode(model, vis, decode='sample', top_p=0.0)
        with pytest.raises(ValueError, match="temperature"):
            decode(model, vis, decode='sample', temperature=0.0)


# ---------------------------------------------------------------------------------------------------------------- training
def count_reward(tokens, batch):
    """a reward that counts tokens: the share of a caption's words with an even index"""
    return ((tokens % 2 == 0) & (tokens > EOS)).float().mean(-1)


# Largest relative deviations of train_sc_step(sc_decode='sample') from the recomputation through teacher forcing, measured on the
# CPU path (oracle ops): loss 6.4e-8, gradient of cap_generator.fc.weight 8.2e-7 of its largest entry.  The test asserts four times
# the larger of the two, which is far below the cap of 1e-3.
SC_MEASURED = 8.2e-7


def test_self_critical_step_with_sampled_captions():
    from grit_amd.engine.caption_engine import build_optimizers, sc_loss, train_sc_step
    model, cfg = build_model(3, **{'model.dropout': 0.0, 'model.detector.dropout': 0.0})
    model.train()
    g = load("beam_g15.npz")
    vis = {k: t(g[k][:3]) for k in FEATS}
    cfg.model.beam_len = 8
    cfg.optimizer.sc_decode, cfg.optimizer.sc_samples = 'sample', 4
    opts = build_optimizers(model, cfg, mode='sc')
    seen = {}

    def reward_fn(tokens, batch):
        seen['tokens'] = tokens.clone()
        return count_reward(tokens, batch)

    model.cached_features = True
    try:
        with oracle_ops():
            # the tokens of the step, ahead of it: the CPU seed comes from torch's generator
            torch.manual_seed(21)
            with torch.no_grad():
                tokens, _ = model(vis, seq=None, use_beam_search=True, max_len=8, eos_idx=EOS, beam_size=4, out_size=4, decode='sample')
            assert tokens.shape == (3, 4, 8)
            flat = tokens.reshape(12, 8)
            full = teacher_forced(model, {k: v.repeat_interleave(4, 0) for k, v in vis.items()}, flat)
            model.cached_features = True
            lps = (full.gather(-1, flat.unsqueeze(-1)).squeeze(-1) * live_steps(flat)).view(3, 4, 8)
            want_loss, _ = sc_loss(lps, count_reward(tokens, None))
            want_grad, = torch.autograd.grad(want_loss, model.cap_generator.fc.weight)
            torch.manual_seed(21)
            loss, reward, baseline = train_sc_step(model, {'samples': vis}, opts, reward_fn, cfg)
    finally:
        model.cached_features = False
    assert torch.equal(seen['tokens'], tokens)
    assert torch.isfinite(loss) and abs(reward.item() - baseline.item()) < 1e-6
    got_grad = model.cap_generator.fc.weight.grad
    assert got_grad.abs().max() > 0
    d_loss = abs(loss.item() - want_loss.item()) / abs(want_loss.item())
    d_grad = ((got_grad - want_grad).abs().max() / want_grad.abs().max()).item()
    print("sampled self-critical step: loss %.9g (recomputed %.9g, relative %.3g), fc gradient relative %.3g"
          % (loss.item(), want_loss.item(), d_loss, d_grad))
    bound = min(4 * SC_MEASURED, 1e-3)
    assert d_loss <= bound and d_grad <= bound


def test_defaults_and_ensemble_refusal():
    from grit_amd.models.caption.ensemble import Ensemble
    opt = default_config().optimizer
    assert opt.sc_decode == 'beam' and opt.sc_samples is None and opt.sc_temperature == 1.0
    from grit_amd.models.caption import Transformer
    cfg = default_config(**{'model.cap_generator.n_layers': 1})
    ens = Ensemble([Transformer(None, cfg).eval()], config=cfg)
    g = load("beam_g15.npz")
    with pytest.raises(NotImplementedError, match="sample"):
        ens({k: t(g[k][:1]) for k in FEATS}, None, use_beam_search=True, decode='sample', beam_size=3)
