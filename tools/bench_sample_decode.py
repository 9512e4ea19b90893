"""Sampled decoding on one GPU: the step kernel (grit_sample_step_f32) against the torch composition it replaces, the whole decode
against beam search, and the self-critical step with sampled captions against the one with beams.

    python tools/bench_sample_decode.py step   [--rows 320] [--vocab 10201] [--iters 200] [--legs 5] [--out FILE]
    python tools/bench_sample_decode.py kernel [--rows 320] [--vocab 10201] [--iters 50]      (run it under rocprofv3 --kernel-trace --stats)
    python tools/bench_sample_decode.py decode [--batch 64] [--iters 5] [--legs 3] [--out FILE]
    python tools/bench_sample_decode.py sc     [--batch 16] [--iters 3] [--legs 3] [--out FILE]

`step` times one step from device events in alternating legs: the kernel, the torch composition (softmax(logp / T) -> multinomial; with
truncation sort -> cumsum -> mask -> multinomial) and, for orientation, grit_beam_step at the same rows.  The spread of a leg
(largest minus smallest leg mean) is printed next to every mean: a difference inside it is no difference.  Every mode prints JSON
lines; a measurement path that finds no GPU fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = [(1.0, 0, 1.0), (1.0, 50, 0.9)]  # (temperature, top_k, top_p)


def torch_step(logp, n, temperature, top_k, top_p):
    """what a user composes from torch ops: n words per row of logp [B, V], their log-probs"""
    probs = torch.softmax(logp / temperature, -1)
    if top_k > 0 or top_p < 1.0:
        sorted_p, order = torch.sort(probs, -1, descending=True)
        before = torch.cumsum(sorted_p, -1) - sorted_p
        drop = before >= top_p
        if top_k > 0:
            drop[:, top_k:] = True
        sorted_p = sorted_p.masked_fill(drop, 0.0)
        words = torch.gather(order, 1, torch.multinomial(sorted_p, n, replacement=True))
    else:
        words = torch.multinomial(probs, n, replacement=True)
    return words, torch.gather(logp, 1, words)


def event_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def summary(legs):
    return {"mean_ms": round(float(np.mean(legs)), 4), "spread_ms": round(max(legs) - min(legs), 4), "legs_ms": [round(x, 4) for x in legs]}


def step_inputs(a):
    from grit_amd.ops import sample as sample_ops
    gen = torch.Generator(device="cuda").manual_seed(0)
    src = torch.log_softmax(3.0 * torch.randn((a.rows // a.fan, a.vocab), device="cuda", generator=gen), -1)
    full = torch.log_softmax(3.0 * torch.randn((a.rows, a.vocab), device="cuda", generator=gen), -1)
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    prev = torch.full((a.rows,), 7, dtype=torch.int64, device="cuda")
    alive = torch.ones(a.rows, device="cuda")
    first = lambda s: sample_ops.sample_step(src, a.fan, None, None, 3, s[0], s[1], s[2], seed, 0)
    later = lambda s: sample_ops.sample_step(full, 1, prev, alive, 3, s[0], s[1], s[2], seed, 5)
    return src, full, first, later


def mode_kernel(a, emit):
    src, full, first, later = step_inputs(a)
    for s in SETTINGS:  # sample_step_kernel<false> for the first setting, <true> for the second: two rows of the kernel statistics
        for _ in range(a.iters):
            later(s)
    torch.cuda.synchronize()
    emit(item="kernel_runs", rows=a.rows, vocab=a.vocab, launches_per_setting=a.iters, settings=SETTINGS)


def mode_step(a, emit):
    from grit_amd.ops import beam as beam_ops
    src, full, first, later = step_inputs(a)
    B, beam = a.rows // a.fan, a.fan
    seq_lp = torch.zeros((B, beam, 1), device="cuda")
    seq_mask = torch.ones((B, beam, 1), device="cuda")
    prev = torch.full((a.rows, 1), 7, dtype=torch.int64, device="cuda")
    beam_later = lambda: beam_ops.beam_step(full.view(B, beam, -1), seq_lp, seq_mask, prev, 3, beam)
    for s in SETTINGS:
        runs = {"device_first": lambda: first(s), "device_later": lambda: later(s),
                "torch_first": lambda: torch_step(src, a.fan, *s), "torch_later": lambda: torch_step(full, 1, *s),
                "beam_step_later": beam_later}
        for fn in runs.values():  # warm-up
            event_ms(fn, 10)
        legs = {k: [] for k in runs}
        for _ in range(a.legs):
            for k, fn in runs.items():
                legs[k].append(event_ms(fn, a.iters))
        emit(item="step", rows=a.rows, vocab=a.vocab, fan=a.fan, temperature=s[0], top_k=s[1], top_p=s[2], iters_per_leg=a.iters,
             **{k: summary(v) for k, v in legs.items()})


def build():
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.detector import build_detector
    from grit_amd.tuning import load_tuned_gemms
    load_tuned_gemms()
    cfg = default_config()
    torch.manual_seed(cfg.exp.seed)
    return Transformer(build_detector(cfg), cfg).cuda(), cfg


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def mode_decode(a, emit):
    from grit_amd.data import synthetic_batch
    model, cfg = build()
    model.eval()
    batch = synthetic_batch(a.batch, 640, 640, device="cuda", seed=1)
    with torch.no_grad():
        vis = dict(model.detector(batch['samples']))
        model.cached_features = True
        runs = {"beam5": lambda: model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=5, out_size=1),
                "sample5": lambda: model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=5, out_size=5,
                                         decode='sample'),
                "sample5_k50_p09": lambda: model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=5, out_size=5,
                                                 decode='sample', top_k=50, top_p=0.9)}
        for fn in runs.values():
            wall_ms(fn, 2)
        legs = {k: [] for k in runs}
        for _ in range(a.legs):
            for k, fn in runs.items():
                legs[k].append(wall_ms(fn, a.iters))
    emit(item="decode_from_features", batch=a.batch, steps=20, n=5, iters_per_leg=a.iters,
         **{k: dict(summary(v), images_per_s=round(a.batch / np.mean(v) * 1e3, 1)) for k, v in legs.items()})


def mode_sc(a, emit):
    from grit_amd.amp import Bf16Compute
    from grit_amd.data import synthetic_batch
    from grit_amd.engine.caption_engine import build_optimizers, train_sc_step
    model, cfg = build()
    wrapped = Bf16Compute(model.train(), bucket_mb=64)
    opts = build_optimizers(wrapped, cfg, mode='sc')
    batches = [synthetic_batch(a.batch, 640, 640, cfg.model.beam_len, device="cuda", seed=i) for i in range(2)]
    reward = lambda tokens, batch: ((tokens % 2 == 0) & (tokens > 3)).float().mean(-1)  # the decode and the update are what is timed

    def run(kind):
        cfg.optimizer.sc_decode = kind
        for i in range(2):
            train_sc_step(wrapped, batches[i], opts, reward, cfg)

    for kind in ('beam', 'sample'):
        run(kind)
    legs = {'beam': [], 'sample': []}
    for _ in range(a.legs):
        for kind in legs:
            legs[kind].append(wall_ms(lambda: run(kind), a.iters) / 2)
    emit(item="sc_step", batch=a.batch, n=cfg.model.beam_size, steps=cfg.model.beam_len, compute="bf16", iters_per_leg=2 * a.iters,
         **{k: summary(v) for k, v in legs.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "kernel", "decode", "sc"])
    ap.add_argument("--rows", type=int, default=320)
    ap.add_argument("--fan", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=10201)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--legs", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_decode.py measures on a HIP device and there is none")
    defaults = {"step": (None, 200, 5), "kernel": (None, 50, 1), "decode": (64, 5, 3), "sc": (16, 3, 3)}[a.mode]
    a.batch, a.iters, a.legs = (x if x is not None else d for x, d in zip((a.batch, a.iters, a.legs), defaults))
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    {"step": mode_step, "kernel": mode_kernel, "decode": mode_decode, "sc": mode_sc}[a.mode](a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
