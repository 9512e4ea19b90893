"""Beam search under constraints on one GPU: the constrained step (grit_beam_step with bans) against the plain step
(grit_beam_step), and the whole decode with and without constraints.

    python tools/bench_beam_constraints.py step    [--batch 64] [--vocab 10201] [--iters 200] [--legs 5] [--out FILE]
    python tools/bench_beam_constraints.py kernel  [--batch 64] [--vocab 10201] [--iters 50]   (run it under rocprofv3 --kernel-trace)
    python tools/bench_beam_constraints.py summary --trace KERNEL_TRACE.csv [--out FILE]
    python tools/bench_beam_constraints.py decode  [--batch 64] [--iters 5] [--legs 3] [--out FILE]

`step` times one step from device events in alternating legs at t = 1, 10 and 19: plain, and constrained with no_repeat_ngram 2,
no_repeat_word, min_len 6 and three suppress ids.  `kernel` captures those six steps (t = 1, 10, 19; plain then constrained) into
one HIP graph and replays it, for a kernel trace; `summary` reads the trace's dispatches in order and prints the stage-1 and stage-2
kernel times per position in the replay.  `decode` is tools/bench_decode.py's measurement (detector, then the 20-step decode, wall
clock around a device synchronise; BASELINE config 5) with and without constraints, alternating.  The spread of a leg (largest
minus smallest leg mean) is printed next to every mean: a difference inside it is no difference.  Every mode prints JSON lines; a
measurement path that finds no GPU fails."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = (1, 10, 19)
CONSTRAINTS = dict(min_len=6, no_repeat_ngram=2, no_repeat_word=True, suppress=(0, 1, 2))
BEAM, EOS = 5, 3


def summary(legs):
    return {"mean_ms": round(float(np.mean(legs)), 4), "spread_ms": round(max(legs) - min(legs), 4), "legs_ms": [round(x, 4) for x in legs]}


def event_ms(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def step_runs(a):
    """{name: callable} of the plain and the constrained step at every t of STEPS, on seeded inputs: histories over 40 words, so
    that every beam has repeated bigrams to ban"""
    import torch
    from grit_amd.ops import beam as beam_ops
    gen = torch.Generator(device="cuda").manual_seed(0)
    B, V = a.batch, a.vocab
    logp = torch.log_softmax(3.0 * torch.randn((B, BEAM, V), device="cuda", generator=gen), -1)
    seq_lp = -torch.rand((B, BEAM, 1), device="cuda", generator=gen)
    seq_mask = torch.ones((B, BEAM, 1), device="cuda")
    hist = torch.randint(4, 44, (B, BEAM, max(STEPS)), device="cuda", generator=gen)
    con = beam_ops.constraints(V, **CONSTRAINTS)
    runs = {}
    for t in STEPS:
        h = hist[:, :, :t].contiguous()
        prev = h[:, :, -1].reshape(-1, 1).contiguous()
        runs["plain_t%d" % t] = lambda prev=prev: beam_ops.beam_step(logp, seq_lp, seq_mask, prev, EOS, BEAM)
        runs["constrained_t%d" % t] = lambda prev=prev, h=h, t=t: beam_ops.beam_step_con([logp], seq_lp, seq_mask, prev, EOS, BEAM, h, t, con)
    return runs, logp


def mode_step(a, emit):
    runs, logp = step_runs(a)
    for fn in runs.values():
        assert fn() is not None
        event_ms(fn, 10)
    legs = {k: [] for k in runs}
    for _ in range(a.legs):
        for k, fn in runs.items():
            legs[k].append(event_ms(fn, a.iters))
    emit(item="step", batch=a.batch, beam=BEAM, vocab=a.vocab, constraints={k: list(v) if isinstance(v, tuple) else v for k, v in CONSTRAINTS.items()},
         iters_per_leg=a.iters, map_bytes=logp.numel() * 4, **{k: summary(v) for k, v in legs.items()})


def mode_kernel(a, emit):
    import torch
    runs, _ = step_runs(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in runs.values():
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for fn in runs.values()]
    for _ in range(a.iters):
        graph.replay()
    torch.cuda.synchronize()
    emit(item="kernel_runs", batch=a.batch, vocab=a.vocab, replays=a.iters, order=list(runs), outputs=len(keep))


def mode_summary(a, emit):
    """the beam kernels of a rocprofv3 kernel trace, in dispatch order: position p of a replay is dispatch p modulo 2 * len(order)"""
    order = [k for t in STEPS for k in ("plain_t%d" % t, "constrained_t%d" % t)]
    with open(a.trace) as f:
        rows = [r for r in csv.DictReader(f) if "beam_partial" in r["Kernel_Name"] or "beam_merge" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-(len(rows) // (2 * len(order)) - 1) * 2 * len(order):]  # the replays: the warm-up and the capture's eager pass come first
    out = {}
    for p, r in enumerate(rows):
        name = order[(p // 2) % len(order)]
        stage = "stage1" if "beam_partial" in r["Kernel_Name"] else "stage2"
        assert stage == ("stage1", "stage2")[p % 2] and ("Banned" in r["Kernel_Name"]) == (stage == "stage1" and name.startswith("constrained")), r
        out.setdefault(name, {}).setdefault(stage, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for name in order:
        emit(item="kernel_time", step=name, **{s: {"calls": len(v), "mean_us": round(float(np.mean(v)) / 1e3, 2), "min_us": round(min(v) / 1e3, 2),
                                                   "max_us": round(max(v) / 1e3, 2)} for s, v in out[name].items()})


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def mode_decode(a, emit):
    import torch
    from grit_amd.config import default_config
    from grit_amd.data import synthetic_batch
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.detector import build_detector
    from grit_amd.tuning import load_tuned_gemms
    cfg = default_config()
    load_tuned_gemms()
    torch.manual_seed(0)
    model = Transformer(build_detector(cfg), cfg).cuda().eval()
    batch = synthetic_batch(a.batch, 640, 640, device="cuda", seed=1)
    kinds = {"plain": {}, "constrained": CONSTRAINTS}
    graphs = len(model._decode_graphs)

    def once(kw):
        vis, t_det = wall(lambda: model.detector(batch['samples']))
        model.cached_features = True
        (tokens, _), t_dec = wall(lambda: model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, beam_size=BEAM, out_size=1, **kw))
        model.cached_features = False
        return t_det, t_dec, tokens

    with torch.no_grad():
        tokens = {k: once(kw)[2] for k, kw in kinds.items()}
        assert len(model._decode_graphs) == graphs + 2  # both decodes replay a captured graph
        for kw in list(kinds.values()) * 2:  # the detector's first batches are still warming up
            once(kw)
        legs = {k: {"detector": [], "decode": []} for k in kinds}
        for _ in range(a.legs):
            for k, kw in kinds.items():
                det, dec = zip(*[once(kw)[:2] for _ in range(a.iters)])
                legs[k]["detector"].append(float(np.mean(det)))
                legs[k]["decode"].append(float(np.mean(dec)))
    for k in kinds:
        total = np.mean(legs[k]["detector"]) + np.mean(legs[k]["decode"])
        emit(item="config5", kind=k, batch=a.batch, steps=20, beam=BEAM, iters_per_leg=a.iters, detector=summary(legs[k]["detector"]),
             decode_20_steps=summary(legs[k]["decode"]), captions_per_sec=round(a.batch / total * 1e3, 1),
             tokens_differ_from_plain=int((tokens[k] != tokens["plain"]).any(-1).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "kernel", "summary", "decode"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=10201)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--legs", type=int, default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode != "summary":
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_beam_constraints.py measures on a HIP device and there is none")
    defaults = {"step": (200, 5), "kernel": (50, 1), "summary": (0, 0), "decode": (5, 3)}[a.mode]
    a.iters, a.legs = (x if x is not None else d for x, d in zip((a.iters, a.legs), defaults))
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    {"step": mode_step, "kernel": mode_kernel, "summary": mode_summary, "decode": mode_decode}[a.mode](a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
