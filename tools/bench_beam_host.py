"""Per-call cost of the five beam-step fronts of grit_amd/ops/beam.py on one GPU, as the host sees it: B 64, V 10 201, beam 5, a later
step, 2 000 back-to-back calls on the host clock with one synchronise after the loop.  One JSON line: per front `issue_us` (the
loop alone: marshalling, allocations and the two launches) and `with_sync_us` (the loop and the synchronise).  To compare two
commits, run it in a checkout of each, alternating, and compare medians against the spread of the repeats.

    python tools/bench_beam_host.py [--calls 2000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_host.py measures on a HIP device and there is none")
    from grit_amd.ops import beam as beam_ops
    dev = "cuda"
    B, V, K, EOS = 64, 10201, 5, 3
    gen = torch.Generator(device=dev).manual_seed(1)
    maps = [torch.log_softmax(3 * torch.randn(B, K, V, device=dev, generator=gen), -1) for _ in range(2)]
    seq_lp = -torch.rand(B, K, 1, device=dev, generator=gen) * 2
    seq_mask = torch.ones(B, K, 1, device=dev)
    prev = torch.full((B * K, 1), 9, dtype=torch.int64, device=dev)
    prev[2::K] = EOS  # one finished beam an image
    hist = torch.randint(4, 40, (B, K, 3), device=dev, generator=gen)
    con = beam_ops.constraints(V, min_len=5, no_repeat_ngram=2, no_repeat_word=True, suppress=(0, 5))
    fw = torch.randint(4, V, (B, 3, 4), device=dev, generator=gen)
    met = torch.zeros(B, K, dtype=torch.int32, device=dev)
    state = (seq_lp, seq_mask, prev, EOS, K)
    fronts = {
        "beam_step": lambda: beam_ops.beam_step(maps[0], *state),
        "beam_step_mean": lambda: beam_ops.beam_step_mean(maps, *state),
        "beam_step_con": lambda: beam_ops.beam_step_con(maps[:1], *state, hist, 3, con),
        "beam_step_div": lambda: beam_ops.beam_step_div(maps[:1], *state, 5, 0.5, hist, 3, con),
        "beam_step_forced": lambda: beam_ops.beam_step_forced(maps[:1], *state, fw, met, hist, 3, con),
    }
    out = {}
    with torch.no_grad():
        for name, call in fronts.items():
            for _ in range(200):
                result = call()
            assert result is not None, name
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out[name] = {"issue_us": round((t1 - t0) / a.calls * 1e6, 2), "with_sync_us": round((t2 - t0) / a.calls * 1e6, 2)}
    print(json.dumps({"B": B, "V": V, "beam": K, "calls": a.calls, "per_call": out}))


if __name__ == "__main__":
    main()
