"""grit_mlp_s0_fwd_bf16 (grit_amd/csrc/mlp_s0.hip): norm2 -> fc1 + GELU -> fc2 -> residual add [-> next norm1] of a frozen C = 128 Swin
block as one launch, against the composition of the launches it replaces, called directly -- grit_layernorm_fwd,
grit_gemm_bf16_nt / GRIT_GEMM_BIAS_GELU, grit_gemm_bf16_nt_res (or GRIT_GEMM_BIAS + a bf16 add), grit_layernorm_fwd.  The contract is
bit-equality (torch.equal): no tolerance anywhere except in the one sanity comparison with float32 torch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, HID, TILE = 128, 512, 128  # (TILE: rows per workgroup of the kernel)
EPS = 1e-5
SENTINEL = -7.25  # exactly representable in bf16


def _params(scale=1.0, seed=0):
    """norm2, fc1, fc2 and next-norm parameters; weights at the model's initial scale (std 0.02) times `scale`."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return {"nw": (1 + 0.1 * r(C)).bfloat16(), "nb": (0.1 * r(C)).bfloat16(),
            "w1": (0.02 * scale * r(HID, C)).bfloat16(), "b1": (0.02 * scale * r(HID)).bfloat16(),
            "w2": (0.02 * scale * r(C, HID)).bfloat16(), "b2": (0.02 * scale * r(C)).bfloat16(),
            "nnw": (1 + 0.1 * r(C)).bfloat16(), "nnb": (0.1 * r(C)).bfloat16()}


def _composition(x, p, with_next, residual_epilogue):
    """The launches the kernel replaces, through their direct wrappers (no shape policy)."""
    from grit_amd.ops import gemm as G
    from grit_amd.ops.layer_norm import layer_norm
    n2 = layer_norm(x, p["nw"], p["nb"], EPS)
    act = G.gemm_nt(n2, p["w1"], G.BIAS_GELU, bias=p["b1"])
    if residual_epilogue:
        x_out = G.gemm_nt_residual(act, p["w2"], p["b2"], x)
    else:
        x_out = x + G.gemm_nt(act, p["w2"], G.BIAS, bias=p["b2"])
    return x_out, (layer_norm(x_out, p["nnw"], p["nnb"], EPS) if with_next else None)


def _fused(x, p, with_next, x_out=None, n_out=None):
    import ctypes
    from grit_amd import lib
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    rows = x.shape[0]
    x_out = torch.empty_like(x) if x_out is None else x_out
    n_out = (torch.empty_like(x) if n_out is None else n_out) if with_next else None
    st = lib.load().grit_mlp_s0_fwd_bf16(ptr(x), ptr(p["nw"]), ptr(p["nb"]), EPS, ptr(p["w1"]), ptr(p["b1"]), ptr(p["w2"]), ptr(p["b2"]),
                                         ptr(p["nnw"] if with_next else None), ptr(p["nnb"] if with_next else None), EPS, rows, C, HID,
                                         ptr(x_out), ptr(n_out), lib.current_stream_ptr())
    lib.check(st, "grit_mlp_s0_fwd_bf16")
    return x_out, n_out


def _check(x, p):
    for with_next in (False, True):
        got_x, got_n = _fused(x, p, with_next)
        for res_epi in (True, False):  # both forms the model runs: residual epilogue, and bias-only fc2 followed by torch's add
            ref_x, ref_n = _composition(x, p, with_next, res_epi)
            assert not torch.isnan(ref_x.float()).any()
            assert torch.equal(got_x, ref_x), (with_next, res_epi, (got_x.float() - ref_x.float()).abs().max().item())
            if with_next:
                assert torch.equal(got_n, ref_n), (res_epi, (got_n.float() - ref_n.float()).abs().max().item())


@pytest.mark.parametrize("rows", [1, 37, 128, 129, 256 + 8, 3 * TILE + 1, 1152])
def test_row_counts(rows):
    """Every tail shape: x is a row slice of a buffer whose other rows are NaN (a row read past the end poisons the result), the outputs
    are slices of buffers filled with a sentinel (a row written past the end shows)."""
    p = _params()
    g = torch.Generator(device="cuda").manual_seed(rows)
    pad = 160
    xb = torch.full((rows + 2 * pad, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    xb[pad:pad + rows] = torch.randn(rows, C, device="cuda", generator=g).bfloat16()
    x = xb[pad:pad + rows]
    _check(x, p)
    for with_next in (False, True):
        ob = torch.full((rows + 2 * pad, C), SENTINEL, device="cuda", dtype=torch.bfloat16)
        nb = torch.full((rows + 2 * pad, C), SENTINEL, device="cuda", dtype=torch.bfloat16)
        got_x, got_n = _fused(x, p, with_next, ob[pad:pad + rows], nb[pad:pad + rows])
        ref_x, ref_n = _composition(x, p, with_next, True)
        assert torch.equal(got_x, ref_x) and not torch.isnan(got_x.float()).any()
        for buf in (ob, nb):
            assert (buf[:pad] == SENTINEL).all() and (buf[pad + rows:] == SENTINEL).all()
        if with_next:
            assert torch.equal(got_n, ref_n) and not torch.isnan(got_n.float()).any()
        else:
            assert (nb == SENTINEL).all()


@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_hard_values(scale):
    """Zero variance (rstd = 1 / sqrt(eps)), a large mean against unit spread, pre-activations over [-12, 12] (the x^2 clamp of the
    GELU and its exp2 -> +inf branch), a row of zeros; weights at the initial scale and 8 x it."""
    rows = 256 + 8
    p = _params(scale, seed=3)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(rows, C, device="cuda", generator=g)
    x[0] = 3.0                                   # constant row
    x[1] = 0.0                                   # zeros
    x[2:40] += 100.0                             # mean 100, unit spread
    x = x.bfloat16()
    _check(x, p)
    # pre-activations over [-12, 12]: fc1 rows scaled so that the largest |pre-activation| of the normalised input is 12
    from grit_amd.ops.layer_norm import layer_norm
    n2 = layer_norm(x, p["nw"], p["nb"], EPS).float()
    pre = n2 @ p["w1"].float().t()
    q = dict(p)
    q["w1"] = (p["w1"].float() * (12.0 / pre.abs().max().item())).bfloat16()
    q["b1"] = torch.zeros_like(p["b1"])
    pre = n2 @ q["w1"].float().t()
    assert pre.max().item() > 7.5 and pre.min().item() < -7.5  # beyond the clamp at x^2 = 50 on both sides
    _check(x, q)


def test_against_float32():
    """One case against float32 torch with the exact GELU: a common-mode error of the two bf16 paths would pass every torch.equal."""
    from tests.test_gemm_gpu import _close
    rows = 256 + 8
    p = _params()
    x = torch.randn(rows, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).bfloat16()
    got_x, got_n = _fused(x, p, True)
    f = {k: v.float() for k, v in p.items()}
    xf = x.float()
    h = F.gelu(F.linear(F.layer_norm(xf, (C,), f["nw"], f["nb"], EPS), f["w1"], f["b1"]))
    ref_x = xf + F.linear(h, f["w2"], f["b2"])
    _close(got_x, ref_x)
    _close(got_n, F.layer_norm(ref_x, (C,), f["nnw"], f["nnb"], EPS))


def _workload_policies(monkeypatch):
    """The own-kernel policies of the long token maps, opened to the few rows of a test model (they are gated on the workload's size)."""
    from grit_amd.ops import gemm as G
    from grit_amd.ops import layer_norm as LN
    from grit_amd.ops import mlp as M
    monkeypatch.setattr(M, "MIN_ROWS", 1152)  # (the stage-0 map of the test models)
    monkeypatch.setattr(G, "prefers_own_narrow", lambda m, n, k: n in (128, 384) and k % 32 == 0 and k <= 512)
    monkeypatch.setattr(LN, "_residual_linear",
                        lambda inp, w, b, s2, scale, per: G.long_linear_residual(inp.reshape(-1, inp.shape[-1]), w, b, s2, scale, per))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_model_level(monkeypatch, mode):
    """A Swin backbone on 2 images of 96 x 96 (1 152 stage-0 rows; the 6 x 6 and 3 x 3 maps of the last stages are padded to the 12 x 12 window), bf16, no
    autograd: every output map equal with the knob on and off; with it on the new entry point runs for the two stage-0 blocks only."""
    from grit_amd import lib
    from grit_amd.models.common.swin_model import SwinTransformer
    from grit_amd.ops import mlp as M
    _workload_policies(monkeypatch)
    torch.manual_seed(0)
    model = SwinTransformer(embed_dim=128, depths=[2, 2, 2, 2], num_heads=[4, 8, 16, 32], window_size=12, frozen_stages=2,
                            pos_dim=256).to("cuda", torch.bfloat16)
    model.train() if mode == "train" else model.eval()
    img = torch.randn(2, 3, 96, 96, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).bfloat16()

    calls = []
    real = lib.load().grit_mlp_s0_fwd_bf16

    class _Counting(object):  # (lib.load() returns one cached library object: count on its attribute)
        def __call__(self, *a):
            calls.append(a[11])
            return real(*a)

    blocks = [blk for stage in model.layers for blk in stage.blocks]
    seen = []
    hooks = [blk.register_forward_hook(lambda m, i, o, k=k: seen.append((k, len(calls)))) for k, blk in enumerate(blocks)]

    def run(on):
        monkeypatch.setattr(M, "S0_MLP_FUSED", on)
        torch.manual_seed(7)  # (train mode: the trainable blocks draw drop-path factors)
        with torch.no_grad():
            return model(img)

    monkeypatch.setattr(lib.load(), "grit_mlp_s0_fwd_bf16", _Counting(), raising=False)
    on = run(True)
    for h in hooks:
        h.remove()
    assert calls == [1152, 1152]
    assert [n for _, n in seen] == [1, 2] + [2] * (len(blocks) - 2)  # one call inside each stage-0 block, none in any other
    n_on = len(calls)
    off = run(False)
    assert len(calls) == n_on
    assert len(on) == len(off) == 4
    for a, b in zip(on, off):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)


def _block(c, dtype):
    from grit_amd.models.common.swin_model import SwinTransformerBlock
    torch.manual_seed(2)
    blk = SwinTransformerBlock(c, c // 32, window_size=12).to("cuda", dtype).eval()
    blk.H = blk.W = 24
    return blk


@pytest.mark.parametrize("case", ["fp32", "requires_grad", "C256", "override"])
def test_fallback(monkeypatch, case):
    """Where the kernel does not apply the function says so (None), and the block computes what it computed without the knob."""
    from grit_amd.ops import mlp as M
    from tests.helpers import oracle_ops
    _workload_policies(monkeypatch)
    c = 256 if case == "C256" else C
    dtype = torch.float32 if case == "fp32" else torch.bfloat16
    blk = _block(c, dtype)
    for p_ in blk.parameters():
        p_.requires_grad_(False)
    x = torch.randn(2, 24 * 24, c, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)).to(dtype)
    if case == "requires_grad":
        x.requires_grad_(True)

    def run(on):
        monkeypatch.setattr(M, "S0_MLP_FUSED", on)
        if case == "override":
            with oracle_ops(), torch.no_grad():
                return M.mlp_norm_residual(x, blk.norm2, blk.mlp, None), blk(x)
        if case == "requires_grad":
            return M.mlp_norm_residual(x, blk.norm2, blk.mlp, None), blk(x)
        with torch.no_grad():
            return M.mlp_norm_residual(x, blk.norm2, blk.mlp, None), blk(x)

    fused_on, y_on = run(True)
    _, y_off = run(False)
    assert fused_on is None
    assert torch.equal(y_on, y_off) and torch.isfinite(y_on.float()).all()
    if case == "requires_grad":
        assert y_on.requires_grad
