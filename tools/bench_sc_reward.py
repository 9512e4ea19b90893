"""The self-critical reward, host against device (grit_amd/ops/cider.py, grit_cider_reward): one JSON line per item.

    python tools/bench_sc_reward.py [--images 3000] [--calls 200] [--step-iters 5] [--size 640] [--no-step] [--out FILE]

Seeded inputs: the real vocabulary (tests/golden/vocab_g10.json), a synthetic corpus of `--images` images with five captions
each drawn from a Zipf-like word pool (with punctuation and clitics, so the tokenizer has work to do), beam 5, T 20, B 16 and 32.
  * reward_host    wall time per call of cider_reward_fn(reward='host') on CPU tokens plus the copy the step pays (tokens on the device)
  * reward_device  device time per call (HIP events around `--calls` warmed calls) and the host time to enqueue one call
  * first_sight    the call that meets a batch of new images: tokenises and cooks their references, uploads them
  * sc_step        train_sc_step in ms on the model bench.py builds (bf16 compute), host and device reward alternating in one
                   process, three legs each; `spread` is max - min of a kind's three legs
  * packer         table sizes and build seconds
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

BEAM, T, EOS = 5, 20, 3


class Field(object):
    eos_token = '<eos>'

    def __init__(self, itos):
        self.itos = list(itos)

    def decode(self, rows):
        out = []
        for r in rows.tolist():
            words = []
            for i in r:
                if i == EOS:
                    break
                words.append(self.itos[i])
            out.append(' '.join(words))
        return out


def corpus(itos, n_images, seed=0):
    """n_images caption lists (five each) and the ids of the pool they are drawn from."""
    rng = np.random.RandomState(seed)
    pool = np.asarray([i for i, w in enumerate(itos) if w.isalpha() and w.islower()][:4000])
    p = 1.0 / np.arange(1, len(pool) + 1)
    p /= p.sum()
    images = []
    for _ in range(n_images):
        caps = []
        for r in range(5):
            words = [itos[i] for i in rng.choice(pool, int(rng.randint(8, 15)), p=p)]
            text = ' '.join(words)
            caps.append([text.capitalize() + '.', text + ', ' + words[0] + "'s " + words[-1], text][r % 3])
        images.append(caps)
    return images, pool, p


def batch_tokens(itos, images, pool, p, B, seed):
    """B images of the corpus and [B, BEAM, T] tokens that look like beams: words of the image's captions, <eos> after 8..14."""
    rng = np.random.RandomState(seed)
    stoi = {w: i for i, w in enumerate(itos)}
    picks = rng.choice(len(images), B, replace=False)
    rows = []
    for i in picks:
        words = [stoi[w] for w in ' '.join(images[i]).lower().replace(',', ' ').replace('.', ' ').split() if w in stoi]
        for _ in range(BEAM):
            n = int(rng.randint(8, 15))
            at = int(rng.randint(0, max(1, len(words) - n)))
            ids = words[at:at + n]
            ids[int(rng.randint(0, len(ids)))] = int(rng.choice(pool, p=p))
            rows.append((ids + [EOS] + [int(x) for x in rng.randint(4, len(itos), T)])[:T])
    return [images[i] for i in picks], torch.tensor(rows, dtype=torch.int64).view(B, BEAM, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the device reward needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def emit(**item):
        line = json.dumps(item)
        print(line, flush=True)
        lines.append(line)

    from grit_amd.datasets.caption.metrics import Cider, PTBTokenizer
    from grit_amd.engine.caption_engine import cider_reward_fn
    from grit_amd.ops.cider import DeviceCider
    itos = json.load(open(os.path.join(ROOT, "tests", "golden", "vocab_g10.json")))["itos"]
    field = Field(itos)
    images, pool, p = corpus(itos, args.images)
    t0 = time.perf_counter()
    cider = Cider(PTBTokenizer.tokenize({i: c for i, c in enumerate(images)}))
    t_corpus = time.perf_counter() - t0
    packer = DeviceCider(cider, itos, device=dev)
    emit(item="packer", images=args.images, corpus_statistics_s=round(t_corpus, 3), **packer.stats)
    del packer

    host_fn = cider_reward_fn(cider, field)
    dev_fn = cider_reward_fn(cider, field, reward='device')
    for B in (16, 32):
        caps, tok = batch_tokens(itos, images, pool, p, B, seed=B)
        batch = {'captions': caps}
        tok_dev = tok.to(dev)
        # host: as train_sc_step pays it -- tokens come from the device, the reward goes back
        times = []
        for _ in range(args.host_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r_host = host_fn(tok_dev.cpu(), batch).to(dev)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        emit(item="reward_host", B=B, beam=BEAM, T=T, calls=args.host_calls, ms_per_call_median=round(float(np.median(times)), 3),
             ms_per_call_min=round(min(times), 3), ms_per_call_max=round(max(times), 3))
        # device: first sight, then steady state
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r_dev = dev_fn(tok_dev, batch)
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        if B == 16:  # the very first call also builds the tables: report a second first-sight batch without that
            caps2, tok2 = batch_tokens(itos, images, pool, p, B, seed=1000 + B)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev_fn(tok2.to(dev), {'captions': caps2})
            torch.cuda.synchronize()
            emit(item="first_sight", B=B, includes_table_build=True, ms=round(first_ms, 3))
            first_ms = (time.perf_counter() - t0) * 1e3
        emit(item="first_sight", B=B, includes_table_build=False, ms=round(first_ms, 3),
             note="tokenises and cooks the references of B new images, uploads them, one launch")
        diff = (r_dev.double() - r_host.double()).abs().max().item()
        for _ in range(20):
            dev_fn(tok_dev, batch)
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        for _ in range(args.calls):
            dev_fn(tok_dev, batch)
        end.record()
        enqueue_ms = (time.perf_counter() - t0) * 1e3 / args.calls
        torch.cuda.synchronize()
        emit(item="reward_device", B=B, beam=BEAM, T=T, calls=args.calls, device_ms_per_call=round(start.elapsed_time(end) / args.calls, 4),
             host_enqueue_ms_per_call=round(enqueue_ms, 4), max_abs_diff_to_host=diff, mean_reward=round(float(r_host.mean()), 4))

    if not args.no_step:
        sc_step(args, dev, itos, field, cider, images, pool, p, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def sc_step(args, dev, itos, field, cider, images, pool, p, emit):
    from grit_amd.amp import Bf16Compute
    from grit_amd.config import default_config
    from grit_amd.data import synthetic_batch
    from grit_amd.engine.caption_engine import build_optimizers, cider_reward_fn, train_sc_step
    from grit_amd.models.caption import Transformer
    from grit_amd.models.caption.detector import build_detector
    config = default_config()
    torch.manual_seed(config.exp.seed)
    model = Transformer(build_detector(config), config).to(dev)  # bench.py's build()
    model.cached_features = False
    wrapped = Bf16Compute(model.train(), bucket_mb=64)
    optimizers = build_optimizers(wrapped, config, mode='sc')
    fns = {'host': cider_reward_fn(cider, field), 'device': cider_reward_fn(cider, field, reward='device')}
    for B in (16, 32):
        batches = []
        for i in range(2):
            b = synthetic_batch(B, args.size, args.size, T, device=dev, seed=i)
            b['captions'], _ = batch_tokens(itos, images, pool, p, B, seed=50 + 10 * B + i)
            batches.append(b)
        try:
            for kind in ('host', 'device'):  # warm-up: allocator, table build, first sight of the references
                for i in range(2):
                    train_sc_step(wrapped, batches[i], optimizers, fns[kind], config)
            legs = {'host': [], 'device': []}
            for leg in range(3):
                for kind in ('host', 'device'):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.step_iters):
                        train_sc_step(wrapped, batches[i % 2], optimizers, fns[kind], config)
                    torch.cuda.synchronize()
                    legs[kind].append((time.perf_counter() - t0) * 1e3 / args.step_iters)
            emit(item="sc_step", B=B, beam=config.model.beam_size, T=config.model.beam_len, size=args.size, iters_per_leg=args.step_iters,
                 host_ms=[round(x, 2) for x in legs['host']], device_ms=[round(x, 2) for x in legs['device']],
                 host_mean_ms=round(float(np.mean(legs['host'])), 2), device_mean_ms=round(float(np.mean(legs['device'])), 2),
                 host_spread_ms=round(max(legs['host']) - min(legs['host']), 2),
                 device_spread_ms=round(max(legs['device']) - min(legs['device']), 2))
        except Exception as e:  # say so in the output instead of losing the reward lines above
            emit(item="sc_step", B=B, error="%s: %s" % (type(e).__name__, str(e)[:400]))
            break


if __name__ == "__main__":
    main()
