"""Beam search with forced words on one GPU: the step with forced words (grit_beam_step with force_words) against the plain step
(grit_beam_step), the constrained step (grit_beam_step with bans) and its own host form (grit_amd/ops/beam.py:
beam_step_forced_host), and the whole decode with and without forced words.

    python tools/bench_beam_forced.py step    [--batch 64] [--vocab 10201] [--iters 200] [--legs 5] [--out FILE]
    python tools/bench_beam_forced.py decode  [--batch 64] [--iters 5] [--legs 3] [--out FILE]

`step` times one later step (t = 10, every beam live, nothing met yet) from device events in alternating legs, for a beam of 5 and
of 6: the plain step, the constrained step (no_repeat_ngram 2), the step with C = 1 / 3 / 8 sets of two words, the step with three
sets under the same constraint, and the host form of every forced case at a tenth of the iterations.  `decode` is
tools/bench_decode.py's measurement (detector, then the 20-step decode, wall clock around a device synchronise) for the plain
search and the searches with forced words, alternating.  The spread of a leg (largest minus smallest leg mean) is printed next to
every mean: a difference inside it is no difference.  Both modes print JSON lines; without a GPU they fail."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEAMS, SETS, WORDS, EOS, STEP = (5, 6), (1, 3, 8), 2, 3, 10


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


def sets_of(B, C, V, gen):
    """[B, C, WORDS] distinct ids in [4, V) per image"""
    import torch
    rows = [torch.randperm(V - 4, device="cuda", generator=gen)[:C * WORDS] + 4 for _ in range(B)]
    return torch.stack(rows).view(B, C, WORDS)


def mode_step(a, emit):
    import torch
    from grit_amd.ops import beam as beam_ops
    gen = torch.Generator(device="cuda").manual_seed(0)
    B, V = a.batch, a.vocab
    con = beam_ops.constraints(V, no_repeat_ngram=2)
    runs, slow = {}, set()
    for beam in BEAMS:
        logp = torch.log_softmax(3.0 * torch.randn((B, beam, V), device="cuda", generator=gen), -1)
        seq_lp = -torch.rand((B, beam, 1), device="cuda", generator=gen)
        seq_mask = torch.ones((B, beam, 1), device="cuda")
        prev = torch.full((B * beam, 1), 9, dtype=torch.int64, device="cuda")
        hist = torch.randint(4, 44, (B, beam, STEP), device="cuda", generator=gen)
        met = torch.zeros((B, beam), dtype=torch.int32, device="cuda")
        state = (seq_lp, seq_mask, prev, EOS, beam)
        runs["beam%d_plain" % beam] = lambda logp=logp, state=state: beam_ops.beam_step(logp, *state)
        runs["beam%d_constrained" % beam] = lambda logp=logp, state=state, hist=hist: beam_ops.beam_step_con([logp], *state, hist, STEP, con)
        for C in SETS:
            fw = sets_of(B, C, V, gen)
            runs["beam%d_forced%d" % (beam, C)] = lambda logp=logp, state=state, fw=fw, met=met: \
                beam_ops.beam_step_forced([logp], *state, fw, met)
            host = "beam%d_forced%d_host" % (beam, C)
            runs[host] = lambda logp=logp, state=state, fw=fw, met=met: beam_ops.beam_step_forced_host(logp, *state, fw, met)
            slow.add(host)
            if C == 3:
                runs["beam%d_forced3_constrained" % beam] = lambda logp=logp, state=state, fw=fw, met=met, hist=hist: \
                    beam_ops.beam_step_forced([logp], *state, fw, met, hist, STEP, con)
    iters = {k: max(1, a.iters // 10) if k in slow else a.iters for k in runs}
    with torch.no_grad():
        for k, fn in runs.items():
            assert fn() is not None
            event_ms(fn, max(1, iters[k] // 20))
        legs = {k: [] for k in runs}
        for _ in range(a.legs):
            for k, fn in runs.items():
                legs[k].append(event_ms(fn, iters[k]))
    emit(item="step", batch=B, vocab=V, t=STEP, words_per_set=WORDS, iters_per_leg=a.iters, host_iters_per_leg=max(1, a.iters // 10),
         **{k: summary(v) for k, v in legs.items()})


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
    gen = torch.Generator(device="cuda").manual_seed(0)
    kinds = {}
    for beam, sets in ((5, SETS), (6, (3,))):
        kinds["beam%d_plain" % beam] = dict(beam_size=beam)
        for C in sets:
            kinds["beam%d_forced%d" % (beam, C)] = dict(beam_size=beam, force_words=sets_of(a.batch, C, cfg.model.vocab_size, gen))
    graphs = len(model._decode_graphs)

    def once(kw):
        vis, t_det = wall(lambda: model.detector(batch['samples']))
        model.cached_features = True
        (tokens, _), t_dec = wall(lambda: model(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=EOS, out_size=1, **kw))
        model.cached_features = False
        return t_det, t_dec, tokens

    def share_met(tokens, fw):
        """the share of (image, set) pairs of which the first caption holds a word"""
        hit = (tokens.view(tokens.shape[0], 1, 1, -1) == fw.unsqueeze(-1)).any(-1).any(-1)
        return round(float(hit.float().mean()), 4)

    with torch.no_grad():
        tokens = {k: once(kw)[2] for k, kw in kinds.items()}
        assert len(model._decode_graphs) == graphs + len(kinds)  # every decode replays a captured graph
        for kw in list(kinds.values()) * 2:  # the detector's first batches are still warming up
            once(kw)
        legs = {k: {"detector": [], "decode": []} for k in kinds}
        for _ in range(a.legs):
            for k, kw in kinds.items():
                det, dec = zip(*[once(kw)[:2] for _ in range(a.iters)])
                legs[k]["detector"].append(float(np.mean(det)))
                legs[k]["decode"].append(float(np.mean(dec)))
    for k, kw in kinds.items():
        total = np.mean(legs[k]["detector"]) + np.mean(legs[k]["decode"])
        fw = kw.get("force_words")
        emit(item="decode", kind=k, batch=a.batch, steps=20, iters_per_leg=a.iters, detector=summary(legs[k]["detector"]),
             decode_20_steps=summary(legs[k]["decode"]), captions_per_sec=round(a.batch / total * 1e3, 1), beam_size=kw["beam_size"],
             sets=0 if fw is None else fw.shape[1], sets_met_by_the_first_caption=None if fw is None else share_met(tokens[k], fw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "decode"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=10201)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--legs", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_forced.py measures on a HIP device and there is none")
    defaults = {"step": (200, 5), "decode": (5, 3)}[a.mode]
    a.iters, a.legs = (x if x is not None else d for x, d in zip((a.iters, a.legs), defaults))
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    {"step": mode_step, "decode": mode_decode}[a.mode](a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
