"""Ensemble beam search on one GPU: ms per batch of 64 images (beam 5, 20 steps, bf16 weights, decode from cached features)
for K = 1 ... 4 members next to the single model, and the fused ensemble step grit_beam_step with n_maps > 1 alone at BASELINE
config 5's size (B 64, beam 5, V 10 201) against its HBM bound.

    python tools/bench_ensemble.py [--batch 64] [--iters 10] [--max-models 4]

Each line is one JSON object.  The members are filled with different closed-form weights; the features are seeded
(the detector is not part of the measurement: `tools/bench_decode.py` reports it)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _decode_ms(model, feats, iters):
    def once():
        return model(feats, seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=5, out_size=1)

    with torch.no_grad():
        for _ in range(2):  # capture + first replay
            once()
        torch.cuda.synchronize()
        times = []
        for _ in range(iters):
            t0 = time.perf_counter()
            tokens, _ = once()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], tokens


def _kernel_us(B, beam, V, K, iters=200):
    from grit_amd.ops import beam as beam_ops
    g = torch.Generator().manual_seed(0)
    maps = [torch.log_softmax(torch.randn(B, beam, V, generator=g), -1).cuda() for _ in range(K)]
    seq_lp = torch.randn(B, beam, 1, generator=g).cuda()
    seq_mask = torch.ones(B, beam, 1, device="cuda")
    prev = torch.randint(4, V, (B * beam, 1), generator=g).cuda()
    with torch.no_grad():
        for _ in range(5):
            beam_ops.beam_step_mean(maps, seq_lp, seq_mask, prev, 3, beam)
        # the kernel pair alone, captured: no host-side work between the launches
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(20):
                beam_ops.beam_step_mean(maps, seq_lp, seq_mask, prev, 3, beam)
        graph.replay()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters // 20):
            graph.replay()
        end.record()
        torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / (iters // 20 * 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-models", type=int, default=4)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth for the bound (MI355X peak: 8 TB/s)")
    a = ap.parse_args()
    from fill import deterministic_fill_
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.ensemble import Ensemble
    from grit_amd.tuning import load_tuned_gemms
    load_tuned_gemms()
    cfg = default_config()
    models = [deterministic_fill_(Transformer(None, cfg), 'bench%d.' % i).eval().cuda().to(torch.bfloat16)
              for i in range(a.max_models)]
    gen = torch.Generator().manual_seed(1)
    B, Ng = a.batch, 100  # config-5 decode shapes of tests/test_configs_gpu.py
    feats = {'gri_feat': torch.randn(B, Ng, 1024, generator=gen).cuda().to(torch.bfloat16),
             'gri_mask': torch.zeros(B, 1, 1, Ng, dtype=torch.bool, device="cuda"),
             'reg_feat': torch.randn(B, 150, 512, generator=gen).cuda().to(torch.bfloat16),
             'reg_mask': torch.zeros(B, 1, 1, 150, dtype=torch.bool, device="cuda")}
    models[0].cached_features = True
    med, best, single = _decode_ms(models[0], feats, a.iters)
    print(json.dumps({"what": "single model", "batch": B, "decode_20_steps_ms": round(med, 3), "best_ms": round(best, 3)}))
    for K in range(1, a.max_models + 1):
        ens = Ensemble(models[:K]).eval()
        med_k, best_k, tokens = _decode_ms(ens, feats, a.iters)
        line = {"what": "ensemble", "models": K, "batch": B, "decode_20_steps_ms": round(med_k, 3), "best_ms": round(best_k, 3),
                "vs_single": round(med_k / med, 3)}
        if K == 1:
            line["tokens_equal_single"] = bool(torch.equal(tokens, single))
        print(json.dumps(line))
        del ens
    V = cfg.model.vocab_size
    for K in (1, 2, 4, 8):
        us = _kernel_us(B, 5, V, K)
        nbytes = K * B * 5 * V * 4  # every map read once (the candidates and the average stay in registers)
        bound = nbytes / (a.hbm_tbs * 1e12) * 1e6
        print(json.dumps({"what": "grit_beam_step with n_maps > 1 (two launches)", "models": K, "B": B, "beam": 5, "V": V,
                          "bytes_read": nbytes, "us": round(us, 2), "hbm_bound_us": round(bound, 2),
                          "fraction_of_bound": round(bound / us, 3)}))


if __name__ == "__main__":
    main()
