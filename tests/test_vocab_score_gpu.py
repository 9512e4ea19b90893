"""grit_vocab_score_bf16 on the device, through the op (ops/vocab_score.py) and the C ABI, and the model surface above it.

1. Lattice: x rows are c * e_k (one nonzero, a power of two), column k of w is 0 on "hot" vocabulary rows and `cold` elsewhere, the
   rest of w is random, so logit[v] = c * w[v, k] exactly and lse = log(n_hot + n_cold exp(c cold)) in closed form (float64).  Hot
   rows: 0, V - 1, both sides of every slice boundary, both sides of every 16-column MFMA tile boundary of the first and the last
   slice (rows with k = 7 instead see ONE hot row, V - 1, so that their maximum lies in the last slice while their target is
   column 0).  Tolerance per row, derived: V 2^-23 (float32 summation of V terms relative to the sum, through the log) +
   8 ulp32(max(|lse|, |logit_target|, 1)) (exp, log, two subtractions).  At V = 10 201 there are 136 hot rows: one dropped or
   doubled moves lse by log(136 / 135) = 7.4e-3 against a tolerance of 1.2e-3; at V = 1 300 with c = 2 a dropped cold tile of 16
   moves it by 1.0e-2 against 1.6e-4.
2. Random data against float64 on the same bf16 operands, with the composed form's own error as the yardstick.
3. Row subsets and permutations bit for bit.  4. Determinism, no synchronisation, graph capture, pad / out-of-range rows.
5. Status codes.  6. Transformer.score, Ensemble.score and evaluate_loss(head='fused') on the small bf16 decoder."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.helpers import load
from tests.test_ensemble_cpu import g16_features, g16_member

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 1
KSET = (0, 7, 8, 31, 32, 63, 64)


def _vs():
    from grit_amd.ops import vocab_score as vs
    return vs


def ulp32(a):
    return 2.0 ** (math.floor(math.log2(max(abs(a), 1.0))) - 23)


def hot_rows(V, slice_w):
    hot = {0, V - 1}
    for b in range(slice_w, V, slice_w):
        hot.update((b - 1, b))
    last = ((V - 1) // slice_w) * slice_w
    for lo, hi in ((0, min(V, slice_w)), (last, V)):
        for b in range(lo + 16, hi, 16):
            hot.update((b - 1, b))
    return sorted(hot)


def lattice(R, V, D, c, cold, ldx=None, ldw=None, seed=0):
    """-> x [R, D], w [V, D], target [R] on the device, and per row (lse, logit_target) in float64."""
    vs = _vs()
    slice_w = vs.slice_width(V, D)
    assert slice_w > 0 and slice_w % 128 == 0
    ks = [k for k in KSET if k < D] + [D - 1]
    g = torch.Generator(device=DEV).manual_seed(seed)
    wbuf = torch.randn(V, ldw or D, generator=g, device=DEV).to(torch.bfloat16)
    xbuf = torch.zeros(R, ldx or D, device=DEV, dtype=torch.bfloat16)
    if ldx:
        xbuf[:, D:] = float('nan')  # the padding of a row is never read
    if ldw:
        wbuf[:, D:] = float('nan')
    x, w = xbuf[:, :D], wbuf[:, :D]
    hot = hot_rows(V, slice_w)
    hot_of = {}
    for k in ks:
        hk = [V - 1] if (k == 7 and V > 1) else hot
        hot_of[k] = set(hk)
        w[:, k] = cold
        w[torch.tensor(hk, device=DEV), k] = 0.0
    cands = [0, V - 1, hot[len(hot) // 2], min(V - 1, 3), V // 2, min(V - 1, slice_w + 5)]
    target, want = [], []
    for r in range(R):
        k = ks[r % len(ks)]
        tg = cands[(r // len(ks) + r) % len(cands)]
        if k == 7:
            tg = 0  # the row's maximum is column V - 1 (last slice), its target the first column of the first slice
        target.append(tg)
        if R >= 3 and r == R - 1:  # a zero row: every logit 0
            want.append((math.log(V), 0.0))
            continue
        x[r, k] = c
        n_hot = len(hot_of[k])
        terms = [math.log(n_hot)] + ([math.log(V - n_hot) + c * cold] if V > n_hot else [])
        m = max(terms)
        want.append((m + math.log(sum(math.exp(t - m) for t in terms)), 0.0 if tg in hot_of[k] else c * cold))
    return x, w, torch.tensor(target, device=DEV), want


def check_lattice(R, V, D, c, cold, **kw):
    vs = _vs()
    x, w, target, want = lattice(R, V, D, c, cold, **kw)
    logp, lse = vs.vocab_score(x, w, target, pad_idx=-5)
    logp, lse = logp.double().cpu().tolist(), lse.double().cpu().tolist()
    worst = 0.0
    for r, (l, tl) in enumerate(want):
        tol = V * 2.0 ** -23 + 8 * ulp32(max(abs(l), abs(tl), 1.0))
        e1, e2 = abs(lse[r] - l), abs(logp[r] - (tl - l))
        worst = max(worst, e1 / tol, e2 / tol)
        assert e1 <= tol and e2 <= tol, (r, R, V, D, c, cold, lse[r], l, logp[r], tl - l, tol)
    print("lattice R %d V %d D %d c %g cold %g: worst error / tolerance %.3f" % (R, V, D, c, cold, worst))


# every V with an R and a D; every R at V = 641 (three slices, a partial last tile); every D at V = 10 201
SIZES = [(1, 1, 64), (15, 2, 192), (16, 15, 512), (17, 16, 64), (63, 17, 192), (64, 641, 512), (65, 1300, 64), (129, 10201, 512),
         (1, 641, 64), (15, 641, 192), (16, 641, 64), (17, 641, 512), (63, 641, 64), (65, 641, 192), (129, 641, 64),
         (17, 10201, 64), (65, 10201, 192), (129, 1300, 512)]


@pytest.mark.parametrize("R,V,D", SIZES)
def test_lattice_hot_columns(R, V, D):
    check_lattice(R, V, D, 32.0, -1.0)


@pytest.mark.parametrize("R,V,D", [(65, 641, 192), (129, 1300, 512), (17, 1300, 64)])
def test_lattice_cold_tiles_count(R, V, D):
    check_lattice(R, V, D, 2.0, -1.0)


@pytest.mark.parametrize("c", [64.0, -64.0])
@pytest.mark.parametrize("R,V,D", [(17, 641, 64), (65, 10201, 512)])
def test_lattice_needs_max_subtraction(R, V, D, c):
    """Logits 0 and -/+256: exp of the raw values underflows to nothing or overflows."""
    check_lattice(R, V, D, c, -4.0)


def test_lattice_leading_dimensions():
    check_lattice(65, 641, 192, 32.0, -1.0, ldx=192 + 8)
    check_lattice(65, 641, 192, 32.0, -1.0, ldw=192 + 24)


# ------------------------------------------------------------------------------------------------------------------- random data
@pytest.fixture(scope="module")
def random_case():
    g = torch.Generator(device=DEV).manual_seed(11)
    R, V, D = 129, 10201, 512
    x = torch.randn(R, D, generator=g, device=DEV).to(torch.bfloat16)
    w = (0.05 * torch.randn(V, D, generator=g, device=DEV)).to(torch.bfloat16)
    target = torch.randint(0, V, (R,), generator=g, device=DEV)
    logits = x.double() @ w.double().t()
    ref_lse = torch.logsumexp(logits, -1)
    ref_lp = logits.gather(1, target[:, None])[:, 0] - ref_lse
    absdot = (x.double().abs() @ w.double().abs().t()).max().item()
    return x, w, target, ref_lp, ref_lse, absdot


def test_random_against_float64(random_case):
    vs = _vs()
    x, w, target, ref_lp, ref_lse, absdot = random_case
    R, D = x.shape
    V = w.shape[0]
    assert ref_lp.abs().max().item() < 40 and (x.double() @ w.double().t()).abs().max().item() < 8
    lp, lse = vs.vocab_score(x, w, target, PAD)
    hp, hse = vs.vocab_score_host(x, w, target, PAD)
    keep = target != PAD
    err_k = max((lp.double() - ref_lp)[keep].abs().max().item(), (lse.double() - ref_lse).abs().max().item())
    err_h = max((hp.double() - ref_lp)[keep].abs().max().item(), (hse.double() - ref_lse).abs().max().item())
    cap = 2 * D * 2.0 ** -23 * absdot + V * 2.0 ** -23
    bound = 4 * err_h + 4 * ulp32(ref_lp.abs().max().item())
    print("random R %d V %d D %d: err_kernel %.3e err_host %.3e bound %.3e hard cap %.3e" % (R, V, D, err_k, err_h, bound, cap))
    assert err_k <= bound
    assert err_k <= cap


def test_row_invariance(random_case):
    vs = _vs()
    x, w, target, *_ = random_case
    lp, lse = vs.vocab_score(x, w, target, PAD)
    g = torch.Generator().manual_seed(3)
    for idx in (torch.tensor([77]), torch.randperm(129, generator=g)[:64], torch.randperm(129, generator=g)):
        idx = idx.to(DEV)
        lp2, lse2 = vs.vocab_score(x[idx], w, target[idx], PAD)
        assert torch.equal(lp2, lp[idx]) and torch.equal(lse2, lse[idx]), len(idx)


def test_determinism_no_sync_pad_and_out_of_range(random_case):
    vs = _vs()
    x, w, target, *_ = random_case
    V = w.shape[0]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a = vs.vocab_score(x, w, target, PAD)
        b = vs.vocab_score(x, w, target, PAD)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    t2 = target.clone()
    t2[5], t2[64], t2[100], t2[128] = PAD, V, -1, 2 ** 40
    lp, lse = vs.vocab_score(x, w, t2, PAD)
    assert lp[5].item() == 0.0 and not np.signbit(lp[5].item())
    assert torch.isnan(lp[[64, 100, 128]]).all()
    assert torch.equal(lse, a[1])  # lse is written for every row
    rest = torch.ones(129, dtype=torch.bool, device=DEV)
    rest[[5, 64, 100, 128]] = False
    assert torch.equal(lp[rest], a[0][rest])  # the neighbours are untouched
    # a pad index outside the vocabulary is pad, not out of range
    assert vs.vocab_score(x[:3], w, torch.full((3,), -1, device=DEV), -1)[0].eq(0).all()


def test_graph_capture_and_replay():
    vs = _vs()
    g = torch.Generator(device=DEV).manual_seed(2)
    R, V, D = 65, 641, 192
    def make():
        return (torch.randn(R, D, generator=g, device=DEV).to(torch.bfloat16),
                (0.1 * torch.randn(V, D, generator=g, device=DEV)).to(torch.bfloat16), torch.randint(0, V, (R,), generator=g, device=DEV))
    x, w, target = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vs.vocab_score(x, w, target, PAD)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = vs.vocab_score(x, w, target, PAD)
    for _ in range(2):
        nx, nw, nt = make()
        x.copy_(nx), w.copy_(nw), target.copy_(nt)
        graph.replay()
        want = vs.vocab_score(nx, nw, nt, PAD)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


# ------------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes():
    from grit_amd import lib
    L = lib.load()
    p = lib.ptr
    R, V = 4, 9
    x = torch.zeros(R, 640, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(V, 640, device=DEV, dtype=torch.bfloat16)
    target = torch.zeros(R, dtype=torch.int64, device=DEV)
    work = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    out = torch.full((2, R), 7.0, device=DEV)

    def call(xp=None, ldx=640, wp=None, ldw=640, tp=None, R_=R, V_=V, D=64, workp=None, lpp=None, lsep=None):
        return L.grit_vocab_score_bf16(p(x) if xp is None else xp, ldx, p(w) if wp is None else wp, ldw, p(target) if tp is None else tp,
                                       PAD, R_, V_, D, p(work) if workp is None else workp, p(out[0]) if lpp is None else lpp,
                                       p(out[1]) if lsep is None else lsep, lib.current_stream_ptr())

    null = ctypes.c_void_p(0)
    assert call(D=48) == lib.ERR_UNSUPPORTED and call(D=576) == lib.ERR_UNSUPPORTED
    assert call(ldx=636) == lib.ERR_UNSUPPORTED and call(ldw=60) == lib.ERR_UNSUPPORTED
    assert call(xp=ctypes.c_void_p(x.data_ptr() + 2)) == lib.ERR_UNSUPPORTED
    for kw in (dict(xp=null), dict(wp=null), dict(tp=null), dict(workp=null), dict(lpp=null), dict(lsep=null), dict(R_=0), dict(V_=0),
               dict(D=0), dict(R_=-3)):
        assert call(**kw) == lib.ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert out.eq(7.0).all()  # nothing was launched
    assert L.grit_vocab_score_slice(9, 48) == 0 and L.grit_vocab_score_workspace(4, 9, 576) == 0
    s = L.grit_vocab_score_slice(10201, 512)
    assert s > 0 and s % 128 == 0 and s == L.grit_vocab_score_slice(10201, 64)
    assert L.grit_vocab_score_workspace(R, V, 64) == (2 * ((V + s - 1) // s) + 1) * R * 4
    assert call() == lib.OK
    torch.cuda.synchronize()
    assert (out[1].double() - math.log(V)).abs().max().item() <= 2 * ulp32(math.log(V))  # all logits 0: the sum is exactly V
    vs = _vs()
    assert not vs.supported(x[:, :48], w[:, :48]) and not vs.supported(x.float(), w.float()) and vs.supported(x[:, :64], w[:, :64])


# ------------------------------------------------------------------------------------------------------------------- model level
def _captions():
    BOS, EOS = 2, 3
    a = [BOS, 11, 12, 13, 14, 15, EOS]
    b = [BOS, 21, 22, EOS, PAD, PAD, PAD]
    c = [BOS, 31, PAD, 33, EOS, PAD, PAD]
    return torch.tensor([[a, b, c], [b, c, a], [c, a, b]], device=DEV)


@pytest.fixture(scope="module")
def bf16_members():
    feats = {k: (v.to(DEV, torch.bfloat16) if v.is_floating_point() else v.to(DEV))
             for k, v in g16_features(load("ensemble_g16.npz")).items()}
    members = []
    for i in range(2):
        m, _ = g16_member(i)
        m = m.to(DEV).to(torch.bfloat16)
        m.cached_features = True
        members.append(m)
    return members, feats


def test_model_score_fused_against_composed(bf16_members, monkeypatch):
    vs = _vs()
    (model, _), feats = bf16_members
    caps = _captions()
    B, N, T = caps.shape
    with torch.no_grad():
        got = model.score(feats, caps)
        monkeypatch.setattr(vs, "VOCAB_HEAD", False)
        host = model.score(feats, caps)
        monkeypatch.setattr(vs, "VOCAB_HEAD", True)
        vis = model._visual_inputs(feats)
        vis = {k: v.repeat_interleave(N, 0) for k, v in vis.items()}
        hidden = model.cap_generator.hidden(caps.view(B * N, T), vis)
        assert hidden.dtype == torch.bfloat16 and vs.supported(hidden.view(-1, 512), model.cap_generator.fc.weight)
    w = model.cap_generator.fc.weight
    logits = hidden.double().view(-1, 512) @ w.double().t()
    ref = torch.log_softmax(logits, -1).view(B, N, T, -1)[:, :, :-1].gather(-1, caps[..., 1:, None])[..., 0] * (caps[..., 1:] != PAD)
    err_k, err_h = (got.log_probs.double() - ref).abs().max().item(), (host.log_probs.double() - ref).abs().max().item()
    absdot = (hidden.double().view(-1, 512).abs() @ w.double().abs().t()).max().item()
    cap = 2 * 512 * 2.0 ** -23 * absdot + w.shape[0] * 2.0 ** -23
    print("model: err_fused %.3e err_composed %.3e cap %.3e" % (err_k, err_h, cap))
    assert err_k <= 4 * err_h + 4 * ulp32(ref.abs().max().item()) and err_k <= cap
    assert got.log_probs.shape == (B, N, T - 1) and (got.log_probs[caps[..., 1:] == PAD] == 0).all()
    assert torch.equal(got.length, host.length) and got.length.tolist() == [[6, 3, 3], [3, 3, 6], [3, 6, 3]]
    assert torch.equal(got.total, got.log_probs.sum(-1))


def test_ensemble_score_is_the_stacked_mean_on_the_device(bf16_members):
    from grit_amd.models.caption.ensemble import Ensemble
    (a, b), feats = bf16_members
    caps = _captions()
    ens = Ensemble([a, b]).eval()
    with torch.no_grad():
        got = ens.score(feats, caps)
        want = torch.stack([a.score(feats, caps).log_probs, b.score(feats, caps).log_probs]).mean(0)
    assert torch.equal(got.log_probs, want)
    with pytest.raises(NotImplementedError):
        ens(feats, caps[:, 0])


def test_evaluate_loss_fused_on_the_device(bf16_members):
    from torch.nn import NLLLoss
    from grit_amd.engine import caption_engine as ce
    (model, _), feats = bf16_members
    caps = _captions()
    batches = [{'samples': feats, 'captions': caps[:, 0].contiguous()}, {'samples': feats, 'captions': caps[:, 2].contiguous()}]
    loss_fn = NLLLoss(ignore_index=PAD)
    want = ce.evaluate_loss(model, batches, loss_fn, None, 0, None, head='torch')
    got = ce.evaluate_loss(model, batches, loss_fn, None, 0, None, head='fused')
    # per token both heads are within the hard cap of rule 2 of the exact value, so the means of the <= 12 tokens of a batch are no
    # further apart than twice that (plus the float32 roundings of a mean of values below 16: 16 ulp32(16))
    w = model.cap_generator.fc.weight
    with torch.no_grad():
        absdot = max((model.cap_generator.hidden(b['captions'], model._visual_inputs(feats)).double().view(-1, 512).abs()
                      @ w.double().abs().t()).max().item() for b in batches)
    cap = 2 * (2 * 512 * 2.0 ** -23 * absdot + w.shape[0] * 2.0 ** -23) + 16 * ulp32(16.0)
    print("evaluate_loss: torch %.7f fused %.7f cap %.3e" % (want, got, cap))
    assert 0 < want < 16 and abs(got - want) <= cap


def test_fp32_model_takes_the_composed_form_exactly():
    vs = _vs()
    model, _ = g16_member(0)
    model = model.to(DEV)
    model.cached_features = True
    feats = {k: v.to(DEV) for k, v in g16_features(load("ensemble_g16.npz")).items()}
    caps = _captions()[:, 0]
    with torch.no_grad():
        hidden = model.cap_generator.hidden(caps, model._visual_inputs(feats))
        assert not vs.supported(hidden.view(-1, 512), model.cap_generator.fc.weight)
        got = model.score(feats, caps)
        full = model(feats, caps)
    want = full[:, :-1].gather(-1, caps[:, 1:, None])[..., 0] * (caps[:, 1:] != PAD)
    assert torch.equal(got.log_probs[:, 0], want)
