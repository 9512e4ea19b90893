"""Consensus reranking under CIDEr-D, device call against the host form, next to the sampled decode that produces the candidates:
one JSON line per item.

    python tools/bench_consensus.py [--batch 64] [--len 20] [--candidates 5 16 32] [--iters 20] [--image 224] [--out FILE]

Candidates: the overlapping-candidate recipe of tests/test_consensus_cpu.py (a base caption per image over a pool of frequent words,
candidates derived by a few edits), over the real vocabulary and a synthetic corpus.  Per number of candidates n:
  * device   DeviceCider.consensus on the tokens (grit_cider_consensus: two launches, plus the gather of the chosen rows), timed with
             HIP events after warm-up, three legs alternating with the decode (`spread` is max - min of a kind's legs)
  * decode   Transformer.forward(decode='sample') of n samples per image, a randomly initialised captioner on --image x --image
             inputs: the work whose output the reranker reads, so that its share can be seen
  * host     consensus_host on the same tokens after a copy to the host (wall clock, one run: it is seconds)
It prints the largest relative difference of the two score matrices as well; it asserts nothing about speed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--len', type=int, default=20)
    ap.add_argument('--candidates', type=int, nargs='+', default=[5, 16, 32])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--image', type=int, default=224)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consensus: needs a HIP device (a CPU timing says nothing about the kernels)")
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.detector import build_detector
    from grit_amd.ops.cider import DeviceCider
    from grit_amd.ops.consensus import consensus_host
    from grit_amd.utils.misc import NestedTensor
    from tests.test_consensus_cpu import recipe, setup
    dev = torch.device('cuda')
    itos, cider = setup()[:2]
    tables = DeviceCider(cider, itos, device=dev)
    B, T = args.batch, args.len
    torch.manual_seed(0)
    cfg = default_config(**{'model.dropout': 0.0, 'model.detector.dropout': 0.0})
    model = Transformer(build_detector(cfg), cfg).to(dev).eval()
    images = torch.randn(B, 3, args.image, args.image, device=dev)
    samples = NestedTensor(images, torch.zeros(B, args.image, args.image, dtype=torch.bool, device=dev))

    def timed(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters

    lines = []
    for n in args.candidates:
        tokens_host = recipe(B, n, T, 100 + n)
        tokens = torch.from_numpy(tokens_host).to(dev)

        def device_call():
            return tables.consensus(tokens)

        def decode():
            with torch.no_grad():
                return model(samples, seq=None, use_beam_search=True, max_len=T, eos_idx=cfg.model.eos_idx, beam_size=n, out_size=n,
                             decode='sample', seed=n)

        kinds = [('device', device_call, args.iters), ('decode', decode, max(2, args.iters // 10))]
        for _, fn, _ in kinds:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        legs = {name: [] for name, _, _ in kinds}
        for _ in range(3):
            for name, fn, iters in kinds:
                legs[name].append(timed(fn, iters))
        t0 = time.perf_counter()
        ref = consensus_host(cider, itos, tokens.cpu())
        host_ms = (time.perf_counter() - t0) * 1e3
        got = tables.consensus(tokens, return_matrix=True)
        nz = ref[1] != 0
        rel = float((np.abs(got.score64.cpu().numpy() - ref[1])[nz] / ref[1][nz]).max())
        shape = dict(batch=B, candidates=n, len=T, device=torch.cuda.get_device_name(0))
        for name, _, iters in kinds:
            ms = legs[name]
            lines.append(dict(item=name, ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms],
                              spread=round(max(ms) - min(ms), 4), iters=iters, **shape))
        lines.append(dict(item='host', ms=round(host_ms, 1), iters=1, **shape))
        lines.append(dict(item='parity', score_max_relative_difference=rel, best_equal=int((got.best.cpu().numpy() == ref[2]).sum()),
                          workspace_bytes=int(tables_workspace(B, n, T)), **shape))
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


def tables_workspace(B, n, T):
    from grit_amd import lib
    return lib.load().grit_cider_consensus_workspace(B, n, T)


if __name__ == '__main__':
    main()
