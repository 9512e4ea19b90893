"""Time grit_mlp_s0_fwd_bf16 against the launches it replaces on the stage-0 map (819 200 x 128, bf16), check bit-equality there.

    python tools/micro/s0_mlp_time.py [rows] [iterations]
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from grit_amd import lib  # noqa: E402
from grit_amd.ops import gemm as G  # noqa: E402
from grit_amd.ops.layer_norm import layer_norm  # noqa: E402


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 819200
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x = r(rows, 128).bfloat16()
    nw, nb, nnw, nnb = (1 + 0.1 * r(128)).bfloat16(), (0.1 * r(128)).bfloat16(), (1 + 0.1 * r(128)).bfloat16(), (0.1 * r(128)).bfloat16()
    w1, b1 = (0.02 * r(512, 128)).bfloat16(), (0.02 * r(512)).bfloat16()
    w2, b2 = (0.02 * r(128, 512)).bfloat16(), (0.02 * r(128)).bfloat16()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    x_out, n_out = torch.empty_like(x), torch.empty_like(x)

    def fused(with_next):
        st = lib.load().grit_mlp_s0_fwd_bf16(ptr(x), ptr(nw), ptr(nb), 1e-5, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                             ptr(nnw if with_next else None), ptr(nnb if with_next else None), 1e-5, rows, 128, 512,
                                             ptr(x_out), ptr(n_out if with_next else None), lib.current_stream_ptr())
        lib.check(st, "grit_mlp_s0_fwd_bf16")

    def parts(with_next):
        n2 = layer_norm(x, nw, nb, 1e-5)
        act = G.gemm_nt(n2, w1, G.BIAS_GELU, bias=b1)
        xo = G.gemm_nt_residual(act, w2, b2, x)
        return xo, (layer_norm(xo, nnw, nnb, 1e-5) if with_next else None)

    def time_ms(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    for with_next in (False, True):
        ref_x, ref_n = parts(with_next)
        fused(with_next)
        eq = torch.equal(x_out, ref_x) and (not with_next or torch.equal(n_out, ref_n))
        print("rows %d next_norm %d: fused %.1f us, separate launches %.1f us, bit-equal %s"
              % (rows, with_next, 1e3 * time_ms(lambda: fused(with_next)), 1e3 * time_ms(lambda: parts(with_next)), eq), flush=True)


if __name__ == "__main__":
    main()
