"""Caption likelihood head, fused (grit_vocab_score_bf16) against composed (bf16 mm with fp32 output + log_softmax + gather +
logsumexp: ops/vocab_score.py vocab_score_host), and Transformer.score with either head: one JSON line per item.

    python tools/bench_vocab_score.py [--rows 20 1280 6400] [--iters 50] [--out profiles/vocab_score/bench.jsonl]

  * head     V 10 201, D 512, bf16, per number of rows R: HIP events after warm-up, three legs per form alternating in one process
             (`spread` is max - min of a form's legs)
  * score    Transformer.score at B 64, N 5, T 20, bf16 decoder on cached features (the detector is not part of scoring N captions:
             its features are computed once per image), with GRIT_VOCAB_HEAD on and off
  * parity   the figures of tests/test_vocab_score_gpu.py::test_random_against_float64 (error of either form against float64 on the
             same bf16 operands, R 129), written to parity.txt next to --out
It asserts nothing about speed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def legs_of(kinds, warm=3):
    for _, fn, _ in kinds:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    legs = {name: [] for name, _, _ in kinds}
    for _ in range(3):
        for name, fn, iters in kinds:
            legs[name].append(timed(fn, iters))
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[20, 1280, 6400])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vocab_score: needs a HIP device (a CPU timing says nothing about the kernels)")
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    from grit_amd.ops import vocab_score as vs
    dev = torch.device('cuda')
    V, D, PAD = 10201, 512, 1
    name = torch.cuda.get_device_name(0)
    g = torch.Generator(device=dev).manual_seed(11)
    lines = []

    def record(item, legs, kinds, **shape):
        for kind, _, iters in kinds:
            ms = legs[kind]
            lines.append(dict(item=item, form=kind, ms=round(float(np.median(ms)), 4), legs=[round(x, 4) for x in ms],
                              spread=round(max(ms) - min(ms), 4), iters=iters, device=name, **shape))

    # ---- parity (the test's data: R 129) ----------------------------------------------------------------------------------------
    x = torch.randn(129, D, generator=g, device=dev).to(torch.bfloat16)
    w = (0.05 * torch.randn(V, D, generator=g, device=dev)).to(torch.bfloat16)
    target = torch.randint(0, V, (129,), generator=g, device=dev)
    logits = x.double() @ w.double().t()
    ref_lse = torch.logsumexp(logits, -1)
    ref_lp = logits.gather(1, target[:, None])[:, 0] - ref_lse
    keep = target != PAD
    with torch.no_grad():
        lp, lse = vs.vocab_score(x, w, target, PAD)
        hp, hse = vs.vocab_score_host(x, w, target, PAD)
    parity = dict(
        err_kernel_logp=(lp.double() - ref_lp)[keep].abs().max().item(), err_kernel_lse=(lse.double() - ref_lse).abs().max().item(),
        err_host_logp=(hp.double() - ref_lp)[keep].abs().max().item(), err_host_lse=(hse.double() - ref_lse).abs().max().item(),
        hard_cap=2 * D * 2.0 ** -23 * (x.double().abs() @ w.double().abs().t()).max().item() + V * 2.0 ** -23,
        max_abs_logit=logits.abs().max().item(), max_abs_logp=ref_lp.abs().max().item())
    lines.append(dict(item='parity', rows=129, vocab=V, d=D, device=name, **parity))

    # ---- the head alone ---------------------------------------------------------------------------------------------------------
    for R in args.rows:
        x = torch.randn(R, D, generator=g, device=dev).to(torch.bfloat16)
        target = torch.randint(0, V, (R,), generator=g, device=dev)
        with torch.no_grad():
            kinds = [('fused', lambda: vs.vocab_score(x, w, target, PAD), args.iters),
                     ('composed', lambda: vs.vocab_score_host(x, w, target, PAD), args.iters)]
            record('head', legs_of(kinds), kinds, rows=R, vocab=V, d=D, slice=vs.slice_width(V, D),
                   logit_map_bytes=R * V * 4)

    # ---- Transformer.score ------------------------------------------------------------------------------------------------------
    B, N, T, Ng = 64, 5, 20, 100
    torch.manual_seed(0)
    cfg = default_config(**{'model.dropout': 0.0})
    model = Transformer(None, cfg).eval().to(dev).to(torch.bfloat16)
    model.cached_features = True
    feats = {'gri_feat': torch.randn(B, Ng, 1024, generator=g, device=dev).to(torch.bfloat16),
             'gri_mask': torch.zeros(B, 1, 1, Ng, dtype=torch.bool, device=dev),
             'reg_feat': torch.randn(B, 150, 512, generator=g, device=dev).to(torch.bfloat16),
             'reg_mask': torch.zeros(B, 1, 1, 150, dtype=torch.bool, device=dev)}
    caps = torch.randint(4, V, (B, N, T), generator=g, device=dev)
    caps[..., 0] = cfg.model.bos_idx
    length = torch.randint(8, T, (B, N), generator=g, device=dev)
    pos = torch.arange(T, device=dev)
    caps = torch.where(pos == length[..., None], torch.full_like(caps, cfg.model.eos_idx), caps)
    caps = torch.where(pos > length[..., None], torch.full_like(caps, cfg.model.pad_idx), caps)

    def score_with(on):
        def run():
            vs.VOCAB_HEAD = on
            try:
                with torch.no_grad():
                    return model.score(feats, caps)
            finally:
                vs.VOCAB_HEAD = True
        return run

    kinds = [('fused', score_with(True), max(2, args.iters // 5)), ('composed', score_with(False), max(2, args.iters // 5))]
    record('score', legs_of(kinds, warm=2), kinds, batch=B, captions=N, len=T, vocab=V, layers=cfg.model.cap_generator.n_layers)
    a, b = score_with(True)(), score_with(False)()
    lines.append(dict(item='score_parity', max_abs_difference_per_token=(a.log_probs - b.log_probs).abs().max().item(),
                      max_abs_difference_total=(a.total - b.total).abs().max().item(), batch=B, captions=N, len=T, device=name))

    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        out_dir = os.path.dirname(os.path.abspath(args.out))
        os.makedirs(out_dir, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
        with open(os.path.join(out_dir, 'parity.txt'), 'w') as f:
            f.write("grit_vocab_score_bf16 against float64 on the same bf16 operands (R 129, V %d, D %d, x ~ N(0,1), w ~ 0.05 N(0,1); %s)\n"
                    % (V, D, name))
            for k, v in parity.items():
                f.write("%-18s %.6e\n" % (k, v))
            err_k = max(parity['err_kernel_logp'], parity['err_kernel_lse'])
            err_h = max(parity['err_host_logp'], parity['err_host_lse'])
            f.write("test bound          err_kernel %.3e <= 4 err_host + 4 ulp32(|logp|) = %.3e: %s\n"
                    % (err_k, 4 * err_h + 4 * 2.0 ** (int(np.floor(np.log2(max(parity['max_abs_logp'], 1.0)))) - 23),
                       err_k <= 4 * err_h + 4 * 2.0 ** (int(np.floor(np.log2(max(parity['max_abs_logp'], 1.0)))) - 23)))


if __name__ == '__main__':
    main()
