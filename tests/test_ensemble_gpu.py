"""Ensemble beam search on the device: grit_beam_step on the mean of several maps against the torch composition of the
reference's step, the graphed and eager ensemble decode against fixture G16 and against its members, and the entry points."""
import copy
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, build_model, deterministic_fill_, load
from tests.test_ensemble_cpu import g16_features, g16_member

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------------------- kernel
def _torch_step(maps, seq_lp, seq_mask, prev, eos, beam):
    """Reference ensemble.py:128-214 in torch on the device: stack().mean(0), then Transformer.iter's composed arithmetic;
    selection = stable descending sort (equal scores by ascending index, the kernel's documented order)."""
    wl = torch.stack(maps).mean(0)
    B, cur, V = wl.shape
    cand = seq_lp + wl
    if prev is not None:
        alive = (prev.view(B, cur) != eos).float().unsqueeze(-1)
        seq_mask = seq_mask * alive
        wl = wl * seq_mask
        frozen = seq_lp.expand_as(cand).contiguous()
        frozen[:, :, 1:] = -999
        cand = seq_mask * cand + frozen * (1 - seq_mask)
    else:
        seq_mask = torch.ones((B, cur, 1), device=wl.device)
    val, idx = torch.sort(cand.reshape(B, -1), dim=-1, descending=True, stable=True)
    val, idx = val[:, :beam], idx[:, :beam]
    sb = torch.div(idx, V, rounding_mode='floor')
    sw = idx - sb * V
    col = sb.unsqueeze(-1)
    picked = torch.gather(torch.gather(wl, 1, col.expand(B, beam, V)), 2, sw.unsqueeze(-1))
    return sb, sw, val.unsqueeze(-1), torch.gather(seq_mask, 1, col), picked


def _case(K, B, cur, V, beam, seed):
    g = torch.Generator().manual_seed(seed)
    maps = [torch.log_softmax(torch.randn(B, cur, V, generator=g) * 3, -1) for _ in range(K)]
    for m in maps:  # exact ties at the top: every row's best value also at words 7 and V - 1, in every map (so in the mean)
        top = m.max(-1).values
        m[..., 7 % V] = top
        m[..., V - 1] = top
    seq_lp = (torch.randn(B, cur, 1, generator=g) * 2).floor() - 6  # integral scores: ties across beams too
    first = cur == 1
    seq_mask = prev = None
    if not first:
        seq_mask = (torch.rand(B, cur, 1, generator=g) > 0.2).float()  # finished beams
        prev = torch.randint(0, 6, (B * cur, 1), generator=g)           # ... and beams that end now (eos = 3)
    to = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    return [m.to(DEV) for m in maps], seq_lp.to(DEV), to(seq_mask), to(prev)


@pytest.mark.parametrize("V", [10201, 37])
@pytest.mark.parametrize("cur", [1, 5])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_mean_step_kernel_bit_exact(K, B, cur, V):
    from grit_amd.ops import beam as beam_ops
    beam = 5
    maps, seq_lp, seq_mask, prev = _case(K, B, cur, V, beam, seed=1000 * K + 10 * B + cur + V)
    with torch.no_grad():
        got = beam_ops.beam_step_mean(maps, seq_lp, seq_mask, prev, 3, beam)
        want = _torch_step(maps, seq_lp, seq_mask, prev, 3, beam)
        torch.cuda.synchronize()
    for name, a, b in zip(("sel_beam", "sel_word", "seq_logprob", "seq_mask", "picked"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.equal(a, b), (name, a.flatten()[:10], b.flatten()[:10])
    if K == 1:
        single = beam_ops.beam_step(maps[0], seq_lp, seq_mask, prev, 3, beam)
        for a, b in zip(got, single):
            assert torch.equal(a, b)


def test_mean_matches_torch_stack_mean_order():
    """The kernel's average IS torch.stack(maps).mean(0): picked log-probs of a one-beam step over every word (k = V)."""
    from grit_amd.ops import beam as beam_ops
    g = torch.Generator().manual_seed(5)
    for K in range(1, 9):
        maps = [(torch.randn(1, 1, 8, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g))).to(DEV)
                for _ in range(K)]
        sb, sw, _, _, picked = beam_ops.beam_step_mean(maps, torch.zeros(1, 1, 1, device=DEV), None, None, 3, 8)
        mean = torch.stack(maps).mean(0).view(-1)
        assert torch.equal(picked.view(-1), mean[sw.view(-1)]), K


def test_mean_step_refusals():
    from grit_amd import lib
    from grit_amd.ops import beam as beam_ops
    maps = [torch.zeros(2, 1, 11, device=DEV) for _ in range(9)]
    with torch.no_grad():
        assert beam_ops.supported_mean(maps[:8], 1, 5) and not beam_ops.supported_mean(maps, 1, 5)
        with pytest.raises(lib.GritHipError, match="grit_beam_step failed"):
            beam_ops.beam_step_mean(maps, torch.zeros(2, 1, 1, device=DEV), None, None, 3, 5)


# ------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def g16_members():
    return [g16_member(i)[0].to(DEV) for i in range(3)]


def _dev_features(g):
    return {k: v.to(DEV) for k, v in g16_features(g).items()}


def _run(model, feats, beam, out_size, graphed, monkeypatch):
    from grit_amd.models.caption import transformer as tr
    monkeypatch.setattr(tr, "_GRAPH_DECODE", graphed)
    was = getattr(model, "cached_features", None)
    model.cached_features = True
    try:
        with torch.no_grad():
            out = model(feats, seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=beam, out_size=out_size)
    finally:
        model.cached_features = was
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("graphed", [True, False])
@pytest.mark.parametrize("K", [2, 3])
def test_ensemble_matches_reference_fixture(g16_members, K, graphed, monkeypatch):
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    ens = Ensemble(g16_members[:K]).eval()
    for beam, out_size in ((1, 1), (5, 1), (5, 5)):
        tag = 'k%d_b%d_o%d' % (K, beam, out_size)
        tokens, lps = _run(ens, _dev_features(g), beam, out_size, graphed, monkeypatch)
        np.testing.assert_array_equal(tokens.cpu().numpy(), g[tag + '_tokens'], err_msg=tag)
        np.testing.assert_allclose(lps.cpu().numpy(), g[tag + '_logprobs'], rtol=1e-3, atol=1e-3, err_msg=tag)
    assert bool(ens._decode_graphs) == graphed
    for m in g16_members[:K]:
        assert not m._is_stateful and not m._decode_graphs and m.cached_features is False


@pytest.mark.parametrize("graphed", [True, False])
def test_single_and_duplicated_member_equal_the_model(g16_members, graphed, monkeypatch):
    """Ensemble([m]) and Ensemble([m, copy of m]) decode exactly what m decodes: (x + x) * 0.5 == x and x * 1 == x."""
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    m = g16_members[0]
    twin = copy.deepcopy(m)
    for beam, out_size in ((1, 1), (5, 1), (5, 5)):
        want = _run(m, _dev_features(g), beam, out_size, graphed, monkeypatch)
        for ens in (Ensemble([m]), Ensemble([m, twin])):
            got = _run(ens.eval(), _dev_features(g), beam, out_size, graphed, monkeypatch)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (len(ens.models), beam, out_size)
    m._decode_graphs.clear()


def test_ensemble_batched_equals_per_image(g16_members, monkeypatch):
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    ens = Ensemble(g16_members[:2]).eval()
    feats = _dev_features(g)
    tb, lb = _run(ens, feats, 5, 1, True, monkeypatch)
    for i in range(3):
        one = {k: v[i:i + 1] for k, v in feats.items()}
        ti, li = _run(ens, one, 5, 1, True, monkeypatch)
        assert torch.equal(tb[i:i + 1], ti), i
    assert not torch.equal(tb[0], tb[2])


def test_shared_then_per_member_features_replay_correctly(g16_members, monkeypatch):
    """One ensemble, same shapes: first every member reads one dict (the same tensors), then each member its own dict.  The
    second call must decode each member from its own features -- as the eager loop does -- not from what the first call's
    capture shared."""
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    ens = Ensemble(g16_members[:2]).eval()
    shared = _dev_features(g)
    flipped = {k: (v.flip(0) if k.endswith('feat') else v) for k, v in _dev_features(g).items()}
    flipped['gri_feat'] = -flipped['gri_feat']
    calls = [shared, [_dev_features(g), flipped], shared, [flipped, _dev_features(g)]]
    results = [_run(ens, c, 5, 1, True, monkeypatch) for c in calls]
    assert len(ens._decode_graphs) == 1
    for c, got in zip(calls, results):
        want = _run(ens, c, 5, 1, False, monkeypatch)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(results[0][0], results[1][0]) and not torch.equal(results[1][0], results[3][0])


@pytest.fixture(scope="module")
def image_members():
    out = []
    for i in range(2):
        model, cfg = build_model(2, fill=False)
        deterministic_fill_(model, 'e%d.' % i)
        out.append(model.eval().to(DEV))
    return out, cfg


def test_from_images_equals_member_features_and_replays(image_members, monkeypatch):
    """NestedTensor input: every member runs its own detector; the result equals the decode from each member's detector output
    (eager), for a first and a second batch of the same shape (the second replays the captured graph)."""
    from grit_amd.models.caption.ensemble import Ensemble
    from grit_amd.utils.misc import NestedTensor
    members, _ = image_members
    ens = Ensemble(members).eval()
    gen = torch.Generator().manual_seed(21)
    mask = torch.zeros(2, 224, 224, dtype=torch.bool)
    mask[1, :, 192:] = True
    for batch in range(2):
        images = torch.randn(2, 3, 224, 224, generator=gen)
        images[1, :, :, 192:] = 0
        samples = NestedTensor(images.to(DEV), mask.to(DEV))
        graphed = _run(ens, samples, 5, 1, True, monkeypatch)
        with torch.no_grad():
            feats = [dict(m.detector(samples)) for m in members]
        eager = _run(ens, feats, 5, 1, False, monkeypatch)
        assert torch.equal(graphed[0], eager[0]) and torch.equal(graphed[1], eager[1]), batch
    assert len(ens._decode_graphs) == 1


def test_caption_stream_takes_an_ensemble(image_members):
    from grit_amd.models.caption.ensemble import Ensemble
    from grit_amd.utils.misc import NestedTensor
    from inference_caption import caption_stream
    members, cfg = image_members
    ens = Ensemble(members).eval()
    gen = torch.Generator().manual_seed(22)
    batches = [NestedTensor(torch.randn(2, 3, 224, 224, generator=gen).to(DEV), torch.zeros(2, 224, 224, dtype=torch.bool,
                                                                                            device=DEV)) for _ in range(2)]
    import torch.cuda.tunable as tunable
    was = tunable.is_enabled()
    tunable.enable(False)  # what caption_stream runs with
    try:
        # sequential first, as in test_caption_stream_pipelined_equals_sequential: the graphs captured outside inference mode
        # stay alive while caption_stream (inference mode) captures its own
        with torch.no_grad():
            want = [ens(b, None, use_beam_search=True, max_len=cfg.model.beam_len, eos_idx=cfg.model.eos_idx, beam_size=5)
                    for b in batches]
        streamed = list(caption_stream(ens, batches, cfg, 5))
        torch.cuda.synchronize()
    finally:
        tunable.enable(was)
    assert len(streamed) == 2
    for (tokens, lps), (wt, wl) in zip(streamed, want):
        assert torch.equal(tokens, wt) and torch.equal(lps, wl)
    assert ens.cached_features is False and ens.training is False


def test_bf16_config5_graphed_equals_eager_and_members_unchanged(monkeypatch):
    """B 64, beam 5, bf16 weights, 2 members: the replayed graph gives the eager tokens; each member's own beam search gives the
    same tokens before and after the ensemble ran (no state, no graph cache of the members touched)."""
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.ensemble import Ensemble
    members = []
    for i in range(2):
        cfg = default_config()
        members.append(deterministic_fill_(Transformer(None, cfg), 'c5_%d.' % i).eval().to(DEV).to(torch.bfloat16))
    gen = torch.Generator().manual_seed(5)
    B, Ng = 64, 100  # config 5 shapes as in test_configs_gpu (the bf16 attention takes up to 160 keys)
    feats = {'gri_feat': torch.randn(B, Ng, 1024, generator=gen).to(DEV, torch.bfloat16),
             'gri_mask': torch.zeros(B, 1, 1, Ng, dtype=torch.bool, device=DEV),
             'reg_feat': torch.randn(B, 150, 512, generator=gen).to(DEV, torch.bfloat16),
             'reg_mask': torch.zeros(B, 1, 1, 150, dtype=torch.bool, device=DEV)}
    before = [_run(m, feats, 5, 1, True, monkeypatch)[0] for m in members]
    ens = Ensemble(members).eval()
    graphed = _run(ens, feats, 5, 1, True, monkeypatch)
    again = _run(ens, feats, 5, 1, True, monkeypatch)
    eager = _run(ens, feats, 5, 1, False, monkeypatch)
    assert graphed[0].shape == (B, 20)
    assert torch.equal(graphed[0], eager[0]) and torch.equal(graphed[1], eager[1])
    assert torch.equal(again[0], graphed[0])
    assert not all(torch.equal(graphed[0], b) for b in before)
    for m, b in zip(members, before):
        assert len(m._decode_graphs) == 1 and not m._is_stateful
        assert torch.equal(_run(m, feats, 5, 1, True, monkeypatch)[0], b)
        assert torch.equal(_run(m, feats, 5, 1, False, monkeypatch)[0], b)


_CLI = r'''
import contextlib, io, json, sys, torch
sys.path.insert(0, %(root)r)
import inference_caption as ic
from grit_amd.config import default_config
ckpts, img = %(ckpts)r, %(img)r
res = {}
for n in (1, 2):
    torch.manual_seed(0)
    sys.argv = ['inference_caption.py', '--img', img, '--vocab', '/nonexistent/vocab.json', '--checkpoint'] + ckpts[:n]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ic.run_main()
    res['cli%%d' %% n] = json.loads(buf.getvalue().strip().splitlines()[-1])
    torch.manual_seed(0)
    cfg = default_config()
    models = [ic.build_model(cfg, torch.device('cuda:0'), c) for c in ckpts[:n]]
    from models.caption.ensemble import Ensemble
    model = models[0] if n == 1 else Ensemble(models, config=cfg).eval()
    import numpy as np
    image = torch.from_numpy(np.load(img)).float()
    res['want%%d' %% n] = ic.caption_tokens(model, image, cfg)[0].tolist()
print(json.dumps(res))
'''


def test_inference_caption_checkpoints(tmp_path):
    """--checkpoint a b captions with the ensemble of the two checkpoints; --checkpoint a is today's single model.  The
    checkpoints hold the caption side only (strict=False loading), the detectors come from the same seed."""
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    ckpts = []
    for i in range(2):
        model = deterministic_fill_(Transformer(None, default_config()), 'cli%d.' % i)
        path = str(tmp_path / ('ckpt%d.pth' % i))
        torch.save({'state_dict': model.state_dict()}, path)
        ckpts.append(path)
    img = str(tmp_path / 'image.npy')
    np.save(img, torch.randn(3, 224, 224, generator=torch.Generator().manual_seed(3)).numpy())
    r = subprocess.run([sys.executable, '-c', _CLI % {'root': ROOT, 'ckpts': ckpts, 'img': img}], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['cli1'] == res['want1'] and res['cli2'] == res['want2']
    assert res['cli1'] != res['cli2']
