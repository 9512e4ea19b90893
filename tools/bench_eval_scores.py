"""The evaluation's caption scores, host against device (grit_amd/ops/caption_scores.py, grit_caption_scores): one JSON line per item.

    python tools/bench_eval_scores.py [--images 5000] [--calls 50] [--out FILE]

Seeded inputs: the real vocabulary (tests/golden/vocab_g10.json), a synthetic split of `--images` images with five captions each
drawn from a Zipf-like word pool (with punctuation and clitics, so the tokenizer has work to do), one hypothesis row per image
that looks like a beam (words of the image's captions, some repeated, <eos> after 8..14), T 20.
  * host          wall time of the reference's flow after beam search, by stage: copy + decode + collapse, tokenise (references
                  and hypotheses), BLEU, ROUGE, CIDEr
  * device_first  the first evaluation of a split: tokenise and cook the references, upload, one launch, aggregate
  * device_warm   every later evaluation: device time of `launch` (HIP events around `--calls` warmed launches) and the wall
                  time of launch + aggregate (the one copy back and the corpus formulas)
  * parity        the device scores against the host's for the same rows
  * packer        table sizes
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_sc_reward import EOS, T, corpus  # noqa: E402  (the same synthetic captions as the reward benchmark)


def split_tokens(itos, images, pool, p, seed=0):
    """One row per image: words of its captions from a random offset, one replaced, one doubled, <eos> after 8..14."""
    rng = np.random.RandomState(seed)
    stoi = {w: i for i, w in enumerate(itos)}
    rows = []
    for caps in images:
        words = [stoi[w] for w in ' '.join(caps).lower().replace(',', ' ').replace('.', ' ').split() if w in stoi]
        n = int(rng.randint(8, 15))
        at = int(rng.randint(0, max(1, len(words) - n)))
        ids = words[at:at + n]
        ids[int(rng.randint(0, len(ids)))] = int(rng.choice(pool, p=p))
        j = int(rng.randint(0, len(ids)))
        ids[j:j] = [ids[j]]  # a repeated word: the evaluation collapses it
        rows.append((ids + [EOS] + [int(x) for x in rng.randint(4, len(itos), T)])[:T])
    return torch.tensor(rows, dtype=torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the device scorer needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def emit(**item):
        line = json.dumps(item)
        print(line, flush=True)
        lines.append(line)

    from grit_amd.datasets.caption.metrics import Bleu, Cider, PTBTokenizer, Rouge
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    itos = json.load(open(os.path.join(ROOT, "tests", "golden", "vocab_g10.json")))["itos"]
    images, pool, p = corpus(itos, args.images)
    tokens = split_tokens(itos, images, pool, p)
    tok_dev = tokens.to(dev)
    torch.cuda.synchronize()

    # ---- host: the reference's flow after beam search ----------------------------------------------------------------------
    clock = time.perf_counter
    t0 = clock()
    gen, gts = {}, {}
    for i, row in enumerate(tok_dev.cpu().tolist()):
        words = [itos[w] for w in itertools.takewhile(lambda w: w != EOS, row)]
        gen[i] = [' '.join(k for k, _ in itertools.groupby(words))]
        gts[i] = images[i]
    t1 = clock()
    gts_t, gen_t = PTBTokenizer.tokenize(gts), PTBTokenizer.tokenize(gen)
    t2 = clock()
    bleu = Bleu().compute_score(gts_t, gen_t)[0]
    t3 = clock()
    rouge = Rouge().compute_score(gts_t, gen_t)[0]
    t4 = clock()
    cider = Cider().compute_score(gts_t, gen_t)[0]
    t5 = clock()
    host_s = t5 - t0
    emit(item="host", images=args.images, T=T, decode_s=round(t1 - t0, 3), tokenise_s=round(t2 - t1, 3), bleu_s=round(t3 - t2, 3),
         rouge_s=round(t4 - t3, 3), cider_s=round(t5 - t4, 3), total_s=round(host_s, 3))

    # ---- device: first evaluation of the split, then warm ------------------------------------------------------------------
    torch.cuda.synchronize()
    t0 = clock()
    scorer = DeviceCaptionScorer(images, itos, device=dev)
    t1 = clock()
    first = scorer.aggregate(*scorer.launch(tok_dev))
    t2 = clock()
    emit(item="device_first", images=args.images, build_s=round(t1 - t0, 3), launch_and_aggregate_s=round(t2 - t1, 4),
         total_s=round(t2 - t0, 3), note="tokenises and cooks the references once, uploads them, one launch, one copy back")
    for _ in range(5):
        scorer.aggregate(*scorer.launch(tok_dev))
    walls = []
    for _ in range(args.calls):
        torch.cuda.synchronize()
        t0 = clock()
        warm = scorer.aggregate(*scorer.launch(tok_dev))
        walls.append((clock() - t0) * 1e3)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(args.calls):
        scorer.launch(tok_dev)
    end.record()
    torch.cuda.synchronize()
    warm_ms = float(np.median(walls))
    emit(item="device_warm", images=args.images, calls=args.calls, launch_device_ms=round(start.elapsed_time(end) / args.calls, 4),
         launch_and_aggregate_wall_ms_median=round(warm_ms, 3), wall_ms_min=round(min(walls), 3), wall_ms_max=round(max(walls), 3),
         host_total_ms=round(host_s * 1e3, 1), host_over_device=round(host_s * 1e3 / warm_ms, 1))
    emit(item="parity", bleu_equal=warm['BLEU'] == bleu, rouge_equal=bool(warm['ROUGE'] == rouge),
         cider_rel_diff=abs(warm['CIDEr'] - cider) / cider, first_equals_warm=first == warm,
         BLEU=[round(b, 6) for b in bleu], ROUGE=round(float(rouge), 6), CIDEr=round(cider, 6))
    emit(item="packer", **scorer.stats)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
