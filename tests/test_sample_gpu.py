"""grit_sample_step_f32 on the device against its host statement (grit_amd/ops/sample.py: sample_step_host), exactly; its refusals;
and Transformer.forward(decode='sample') on the device: greedy = beam of one, the fill behind <eos>, eager = graph replay, teacher-
forced log-probs, and the self-critical step with optimizer.sc_decode = 'sample' in fp32 and under Bf16Compute."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import build_model, disable_drop_path, load, t
from tests.test_sample_cpu import EOS, FEATS, check_eos_fill, check_greedy, check_teacher_forced, count_reward, decode, g15_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64  # sentinel elements on each side of every output buffer
ONE = 1 << 32


def max_v():
    from grit_amd import lib
    return lib.SAMPLE_MAX_V


def make_rows(kind, n, V, rng):
    if kind == "softmax":
        x = rng.normal(0, 3, (n, V))
    elif kind == "ties":  # eight levels: the top-k and the nucleus boundary fall inside groups of equal log-probs
        x = np.floor(rng.normal(0, 3, (n, V)).clip(-6, 5.99) / 1.5) * 1.5
    elif kind == "inf":  # -inf entries, down to a single finite one in every fourth row
        x = rng.normal(0, 3, (n, V))
        x[rng.random((n, V)) < 0.5] = -np.inf
        x[::4] = -np.inf
        x[np.arange(n), rng.integers(0, V, n)] = 1.0
    elif kind == "dominant":
        x = np.full((n, V), -200.0)
        x[np.arange(n), rng.integers(0, V, n)] = 0.0
        return x.astype(np.float32)
    return torch.log_softmax(torch.from_numpy(x.astype(np.float32)), -1).numpy()


def padded(n, dtype, sentinel):
    return torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device=DEV)


def launch(logp, ld_pad, rows, fan, prev, alive_in, fill, inv_t, top_k, q32, seed, step):
    """the kernel on logp [rows / fan, V] (numpy) stored with row stride V + ld_pad -> (words, picked, alive) as numpy, after
    asserting that the sentinels around the three outputs are untouched"""
    from grit_amd import lib
    n, V = logp.shape
    stored = np.zeros((n, V + ld_pad), np.float32)  # 0.0 in the gap: above every log-prob, so a read past V would show
    stored[:, :V] = logp
    d_logp = torch.from_numpy(stored).to(DEV)
    d_seed = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=DEV)
    d_prev = None if prev is None else torch.from_numpy(prev).to(DEV)
    d_alive = None if alive_in is None else torch.from_numpy(alive_in).to(DEV)
    words, picked, alive = padded(rows, torch.int64, -7), padded(rows, torch.float32, -7.0), padded(rows, torch.float32, -7.0)
    at = lambda x, size: ctypes.c_void_p(x.data_ptr() + PAD * size)
    st = lib.load().grit_sample_step_f32(lib.ptr(d_logp), V + ld_pad, rows, fan, V, lib.ptr(d_prev), lib.ptr(d_alive), EOS, fill,
                                         inv_t, top_k, q32, lib.ptr(d_seed), step, at(words, 8), at(picked, 4), at(alive, 4),
                                         lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert st == 0, st
    out = []
    for x in (words, picked, alive):
        x = x.cpu().numpy()
        assert (x[:PAD] == -7).all() and (x[-PAD:] == -7).all()
        out.append(x[PAD:-PAD])
    return out


def compare(V, ld_pad, rows, fan, step, inv_t, top_k, top_p, kind, seed):
    from grit_amd.ops.sample import sample_step_host, top_p_q32
    rng = np.random.default_rng(seed)
    logp = make_rows(kind, rows // fan, V, rng)
    prev = alive_in = None
    if step > 0:  # finished and live rows mixed
        prev = rng.integers(0, 8, rows).astype(np.int64)
        alive_in = (rng.random(rows) < 0.8).astype(np.float32)
    q32 = top_p_q32(top_p)
    inv_t = float(np.float32(inv_t))
    device_seed = int(rng.integers(0, 1 << 63)) * 2 + 1
    got = launch(logp, ld_pad, rows, fan, prev, alive_in, 0, inv_t, top_k, q32, device_seed, step)
    want = sample_step_host(logp, rows, fan, prev, alive_in, EOS, 0, inv_t, top_k, q32, device_seed, step)
    what = "V %d ld+%d rows %d fan %d step %d inv_T %g k %d p %g %s" % (V, ld_pad, rows, fan, step, inv_t, top_k, top_p, kind)
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(got[2], want[2], err_msg=what)
    return got


VS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 10201, "max"]
# (inv_T, top_k, top_p); top_k "V" and "V+10" are resolved per vocabulary
SETTINGS = [(1.0, 0, 1.0), (1 / 0.7, 0, 1.0), (1.0, 1, 1.0), (1.0, 5, 1.0), (1.0, "V", 1.0), (1.0, "V+10", 1.0), (1.0, 0, 0.9),
            (1.0, 0, 1e-6), (1.0, 50, 0.8), (100.0, 0, 1.0), (0.01, 0, 1.0)]
ROWS_FAN = [(1, 1), (5, 5), (320, 5), (320, 1)]
KINDS = ["softmax", "ties", "inf", "dominant"]
STEPS = [0, 1, 19]


@pytest.mark.parametrize("vi", range(len(VS)), ids=[str(v) for v in VS])
def test_kernel_equals_the_host_form(vi):
    """Every vocabulary size with every setting; leading dimension, (rows, fan), step and the kind of row rotate with the pair, so
    that over the eleven vocabularies each setting meets every one of them (the pruned product)."""
    V = max_v() if VS[vi] == "max" else VS[vi]
    for si, (inv_t, k, p) in enumerate(SETTINGS):
        k = {"V": V, "V+10": V + 10}.get(k, k)
        rows, fan = ROWS_FAN[(si + vi) % 4]
        compare(V, 3 * ((si // 2 + vi) % 2), rows, fan, STEPS[(si + vi // 2) % 3], inv_t, k, p, KINDS[(si + 2 * vi + vi // 4) % 4],
                1000 * vi + si)


@pytest.mark.parametrize("kind", KINDS)
def test_truncation_boundaries_on_every_kind_of_row(kind):
    """top-k alone, nucleus alone and both, at the flagship vocabulary and at one that is no multiple of anything"""
    for V, rows, fan in ((10201, 10, 1), (1000, 40, 5)):
        for si, (k, p) in enumerate(((5, 1.0), (50, 1.0), (0, 0.9), (0, 0.5), (50, 0.8), (3, 0.3))):
            compare(V, 3 * (si % 2), rows, fan, si % 2, 1.0, k, p, kind, 77 + si)


def test_many_rows_in_one_launch():
    words, _, alive = compare(300, 0, 4096, 1, 1, 1.0, 20, 0.95, "softmax", 5)
    assert 0 < alive.sum() < 4096 and len(set(words.tolist())) > 20


def test_fan_out_rows_share_a_source_row_and_differ_in_the_draw():
    words, picked, _ = compare(10201, 0, 320, 5, 0, 1.0, 0, 1.0, "softmax", 9)
    assert any(len(set(words[i:i + 5].tolist())) > 1 for i in range(0, 320, 5))


def test_bad_arguments_return_their_status_and_write_nothing():
    from grit_amd import lib
    L = lib.load()
    V, rows = 100, 6
    logp = torch.from_numpy(make_rows("softmax", rows, V, np.random.default_rng(0))).to(DEV)
    big = torch.zeros((1, max_v() + 1), device=DEV)
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)
    prev = torch.zeros(rows, dtype=torch.int64, device=DEV)
    alive_in = torch.ones(rows, device=DEV)
    words, picked, alive = padded(rows, torch.int64, -7), padded(rows, torch.float32, -7.0), padded(rows, torch.float32, -7.0)
    good = dict(logp=logp, ld=V, rows=rows, fan=1, V=V, prev=prev, alive_in=alive_in, inv_t=1.0, top_k=0, q32=ONE, seed=seed, step=1,
                words=words, picked=picked, alive=alive)

    def call(**over):
        a = dict(good, **over)
        at = lambda x, size: ctypes.c_void_p(x.data_ptr() + PAD * size) if x is not None else None
        return L.grit_sample_step_f32(lib.ptr(a['logp']), a['ld'], a['rows'], a['fan'], a['V'], lib.ptr(a['prev']),
                                      lib.ptr(a['alive_in']), EOS, 0, a['inv_t'], a['top_k'], a['q32'], lib.ptr(a['seed']), a['step'],
                                      at(a['words'], 8), at(a['picked'], 4), at(a['alive'], 4), lib.current_stream_ptr())

    bad = [dict(logp=None), dict(seed=None), dict(words=None), dict(picked=None), dict(alive=None), dict(rows=0), dict(fan=0),
           dict(fan=4), dict(V=0), dict(ld=V - 1), dict(prev=None), dict(alive_in=None), dict(step=-1), dict(step=4096),
           dict(top_k=-1), dict(q32=0), dict(q32=ONE + 1), dict(inv_t=0.0), dict(inv_t=-1.0), dict(inv_t=float("inf")),
           dict(inv_t=float("nan"))]
    for over in bad:
        assert call(**over) == lib.ERR_BAD_ARG, over
    assert call(logp=big, rows=1, V=max_v() + 1, ld=max_v() + 1, prev=None, alive_in=None) == lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for x in (words, picked, alive):
        assert (x == -7).all()
    assert call() == lib.OK
    torch.cuda.synchronize()
    assert (words[PAD:-PAD] != -7).all() and (words[:PAD] == -7).all() and (words[-PAD:] == -7).all()


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from grit_amd import lib
    from grit_amd.ops import sample as sample_ops
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)
    for lp in (torch.zeros((2, 50), device=DEV, dtype=torch.bfloat16), torch.zeros((2, max_v() + 1), device=DEV),
               torch.zeros((2, 100), device=DEV)[:, ::2]):
        assert not sample_ops.supported(lp)
        with pytest.raises(lib.GritHipError):
            sample_ops.sample_step(lp, 1, None, None, EOS, 1.0, 0, 1.0, seed, 0)
    with pytest.raises(lib.GritHipError, match="seed"):
        sample_ops.sample_step(torch.zeros((2, 50), device=DEV), 1, None, None, EOS, 1.0, 0, 1.0, seed.cpu(), 0)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def g15_device():
    model, _ = g15_model(DEV)
    g = load("beam_g15.npz")
    return model, {k: t(g[k], device=DEV) for k in FEATS}


def test_greedy_sampling_is_the_beam_of_one_on_the_device(g15_device):
    model, vis = g15_device
    tokens, lps, pinned = check_greedy(model, vis)
    check_eos_fill(tokens, lps, pinned)


def test_graph_replay_equals_the_eager_loop(g15_device, monkeypatch):
    import grit_amd.models.caption.transformer as T
    model, vis = g15_device
    model._decode_graphs.clear()
    kw = dict(beam_size=5, out_size=5, decode='sample', temperature=0.9, top_k=40, top_p=0.95)
    a, a_lps = decode(model, vis, seed=31, **kw)
    assert len(model._decode_graphs) == 1
    b, b_lps = decode(model, vis, seed=32, **kw)  # the same graph, another seed
    again, again_lps = decode(model, vis, seed=31, **kw)
    assert len(model._decode_graphs) == 1
    assert torch.equal(a, again) and torch.equal(a_lps, again_lps) and not torch.equal(a, b)
    monkeypatch.setattr(T, "_GRAPH_DECODE", False)
    eager, eager_lps = decode(model, vis, seed=31, **kw)
    eager_b, _ = decode(model, vis, seed=32, **kw)
    assert len(model._decode_graphs) == 1
    assert torch.equal(a, eager) and torch.equal(a_lps, eager_lps) and torch.equal(b, eager_b)
    # the beam search of the same shapes keeps a graph of its own
    monkeypatch.setattr(T, "_GRAPH_DECODE", True)
    decode(model, vis, beam_size=5, out_size=5)
    assert len(model._decode_graphs) == 2


def test_log_probs_are_the_teacher_forced_ones_on_the_device(g15_device):
    model, vis = g15_device
    tokens, lps = decode(model, vis, beam_size=5, out_size=5, decode='sample', seed=11)
    assert all(not (tokens[i] == tokens[i, :1]).all() for i in range(8))
    check_teacher_forced(model, vis, tokens, lps)


def sc_setup(wrap):
    from grit_amd.engine.caption_engine import build_optimizers
    from grit_amd.utils.misc import NestedTensor
    g = load("sc_g9.npz")
    model, cfg = build_model(3, **{'model.dropout': 0.0, 'model.detector.dropout': 0.0})
    model.train().to(DEV)
    disable_drop_path(model)
    cfg.model.beam_len = 6
    cfg.optimizer.sc_decode, cfg.optimizer.sc_samples = 'sample', 3
    if wrap:
        from grit_amd.amp import Bf16Compute
        model = Bf16Compute(model)
    images = t(g["images"], device=DEV)
    batch = {'samples': NestedTensor(images, torch.zeros(images.shape[0], *images.shape[-2:], dtype=torch.bool, device=DEV))}
    return model, cfg, build_optimizers(model, cfg, mode='sc'), batch


def test_self_critical_step_with_sampled_captions_fp32():
    from grit_amd.engine.caption_engine import train_sc_step
    model, cfg, opts, batch = sc_setup(False)
    seen = {}

    def reward_fn(tokens, b):
        seen['shape'] = tuple(tokens.shape)
        return count_reward(tokens, b)

    torch.manual_seed(2)
    loss, reward, baseline = train_sc_step(model, batch, opts, reward_fn, cfg)
    assert seen['shape'] == (batch['samples'].tensors.shape[0], 3, 6)
    assert torch.isfinite(loss) and torch.isfinite(reward) and abs(reward.item() - baseline.item()) < 1e-6
    for name in ('cap_generator.fc.weight', 'grid_net.fc.weight', 'detector.input_proj.1.0.weight'):
        grad = dict(model.named_parameters())[name].grad
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0, name


def test_self_critical_step_with_sampled_captions_bf16():
    from grit_amd.engine.caption_engine import train_sc_step
    wrapped, cfg, opts, batch = sc_setup(True)
    masters = dict(wrapped.named_master_parameters())
    picks = ('cap_generator.fc.weight', 'grid_net.fc.weight')
    before = {n: masters[n].detach().float().clone() for n in picks}
    torch.manual_seed(2)
    loss, reward, baseline = train_sc_step(wrapped, batch, opts, count_reward, cfg)
    assert torch.isfinite(loss) and torch.isfinite(reward) and loss.item() != 0
    after = dict(wrapped.named_master_parameters())
    for n in picks:
        assert torch.isfinite(after[n]).all() and not torch.equal(after[n].detach().float(), before[n]), n
