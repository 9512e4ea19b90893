"""Cross-entropy training / evaluation loops of the captioner (reference engine/caption_engine.py).

Kept: build_optimizers :18-73 (two Adams split on 'detector' in the parameter name; the groups carry
`weight_decay_rate`, which torch.optim.Adam ignores -> effective weight decay 0), gather_result :76-80,
save_checkpoint :83-103 (same dict layout), evaluate_loss :287-309, train_xe :312-385 (same step order:
forward -> zero_grad x2 -> NLL on shifted log-probs -> backward -> Adam x2 -> scalar all-reduce -> scheduler, and the
extra scheduler.step() before each epoch's loop, Q8), evaluate_metrics :144-230 (the beam-search model call; scoring
is delegated to a caller-supplied scorer because the reference's PTB tokenizer / METEOR are Java programs).
train_sc :388-492 (next-row N2): beam search with gradient + reward supplied by the caller (the reference's CIDEr /
PTB tokenizer are host-side Java).  Out of scope: log_epoch, inference_coco_test.

MI355X specifics: with grit_amd.amp.Bf16Compute the two Adams are FlatAdam (one kernel per parameter run over the flat
bf16-gradient / fp32-master state), otherwise torch's fused multi-tensor Adam; the model may be wrapped either in
torch DDP or in grit_amd.ddp.BucketedDataParallel (gradient buckets all-reduced by RCCL on its side stream while
backward is still running); tqdm / TensorBoard are optional.
"""
import time

import torch
import torch.distributed as dist
from torch.nn import NLLLoss

from grit_amd.config import beam_constraints, beam_groups
from grit_amd.data import PAD
from grit_amd.utils.misc import get_rank, get_world_size, is_dist_avail_and_initialized


def _unwrap(model):
    return getattr(model, 'module', model)


def _consolidate(model):
    """End of a training epoch, EVERY rank: with a sharded optimizer (grit_amd.amp.Bf16Compute(shard_optimizer=True)) the fp32
    masters and Adam moments of the other ranks' slices are gathered, so that the checkpoints rank 0 (and the evaluation ranks,
    reference train_caption.py:149-204) write afterwards hold the whole model.  No-op for every other wrapper."""
    fn = getattr(model, 'consolidate', None)
    if fn is not None:
        fn()


def build_optimizers(model, config, mode='xe'):
    # grit_amd.amp.Bf16Compute exposes fp32 masters under the module's parameter names; otherwise the module's own
    masters = getattr(model, 'named_master_parameters', None)
    wrapper = model
    model = _unwrap(model)
    all_named = masters() if masters is not None else list(model.named_parameters())
    no_decay = ['bias', 'gamma', 'beta']

    def groups(in_detector):
        named = [(n, p) for n, p in all_named if p.requires_grad and (('detector' in n) == in_detector)]
        return [
            {'params': [p for n, p in named if any(nd in n for nd in no_decay)], 'weight_decay_rate': 0.0},
            {'params': [p for n, p in named if not any(nd in n for nd in no_decay)],
             'weight_decay_rate': config.optimizer.weight_decay},
        ]

    betas = (config.optimizer.beta_1, config.optimizer.beta_2)
    fused = all(p.is_cuda for _, p in all_named)

    flat = getattr(wrapper, 'flat_adam', None) if getattr(wrapper, 'flat_optimizer', False) else None

    def adam(param_groups, lr):
        param_groups = [g for g in param_groups if len(g['params'])] or param_groups
        if flat is not None:  # grit_amd.amp.FlatAdam: same arithmetic and state layout, one kernel per parameter run
            return flat(param_groups, lr, betas)
        return torch.optim.Adam(param_groups, lr=lr, betas=betas, **({'fused': True} if fused else {}))

    return {
        'model': adam(groups(False), getattr(config.optimizer, f'{mode}_lr', config.optimizer.sc_lr)),
        'backbone': adam(groups(True), getattr(config.optimizer, f'{mode}_backbone_lr', config.optimizer.sc_backbone_lr)),
        'mode': mode,
    }


def gather_result(value):
    """Average a tensor over the ranks (sum all-reduce, then 1/world)."""
    if isinstance(value, torch.Tensor) and is_dist_avail_and_initialized():
        dist.all_reduce(value, async_op=False)
        value.mul_(1.0 / get_world_size())
    return value


def _refuse_ensemble_checkpoint(model):
    """An Ensemble's state dict (keys `models.<i>.…`) is no checkpoint the single-model loaders read: refused, not written."""
    from grit_amd.models.caption.ensemble import Ensemble
    if isinstance(_unwrap(model), Ensemble):
        raise ValueError("an Ensemble has no single-model checkpoint: save each of its members instead (evaluate_metrics of "
                         "an Ensemble needs best_cider=None or log_and_save=False)")


def save_checkpoint(model, optimizers, epoch, scores, best_ciders, config=None, filename='checkpoint_last.pth',
                    scheduler=None):
    _refuse_ensemble_checkpoint(model)
    torch.save(
        {
            "state_dict": (model.master_state_dict() if hasattr(model, 'master_state_dict')
                           else _unwrap(model).state_dict()),
            "optim_model": optimizers['model'].state_dict(),
            "optim_backbone": optimizers['backbone'].state_dict(),
            "scores": scores,
            "best_ciders": best_ciders,
            "epoch": epoch,
            "exp_name": "" if config is None else config.exp.name,
            "scheduler": [] if scheduler is None else scheduler.state_dict(),
        }, filename)


def _progress(iterable, **kw):
    try:
        from tqdm import tqdm
        return tqdm(iterable, **kw)
    except Exception:  # pragma: no cover
        return iterable


def _pad_index(text_field):
    if text_field is None:
        return PAD
    return text_field.vocab.stoi['<pad>']


def xe_loss(model, batch, loss_fn):
    """NLL of token t+1 given tokens <= t (log-probs at positions 0..T-2 vs captions 1..T-1)."""
    out = model(batch['samples'], batch['captions'])
    target = batch['captions'][:, 1:].contiguous()
    out = out[:, :-1].contiguous()
    return loss_fn(out.view(-1, out.shape[-1]), target.view(-1))


def score_captions(model, samples, captions, normalize=None):
    """How likely `model` (a Transformer or an Ensemble, wrapped or not) finds `captions` [B, T] or [B, N, T] for `samples`:
    CaptionScores(log_probs, total, length) of models/caption/transformer.py.  Eval mode, no autograd."""
    net = _unwrap(model)
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            return net.score(samples, captions, normalize=normalize)
    finally:
        net.train(was_training)


def fused_xe_loss(model, batch, pad_idx):
    """xe_loss from the likelihood head: NLLLoss(ignore_index=pad, reduction='mean') = -sum of the non-pad targets' log-probs /
    their number, without the [rows, V] map.  The model's pad index must be the loss's."""
    net = _unwrap(model)
    if net.cap_generator.pad_idx != pad_idx:
        raise ValueError("head='fused' ignores the model's pad index %d, the loss ignores %d" % (net.cap_generator.pad_idx, pad_idx))
    scores = net.score(batch['samples'], batch['captions'])
    return -scores.log_probs.sum() / scores.length.sum()


def evaluate_loss(model, dataloader, loss_fn, text_field, epoch, writer, head='torch'):
    """head='torch': the reference's loop.  head='fused': the same loss per batch from model.score (ops/vocab_score.py)."""
    if head not in ('torch', 'fused'):
        raise ValueError("head must be 'torch' or 'fused', not %r" % (head,))
    model.eval()
    running = .0
    with torch.no_grad():
        for it, batch in enumerate(_progress(dataloader, desc='Epoch %d - validation' % epoch, unit='it')):
            if head == 'fused':
                loss = gather_result(fused_xe_loss(model, batch, loss_fn.ignore_index))
            else:
                loss = gather_result(xe_loss(model, batch, loss_fn))
            running += loss.item()
    val_loss = running / max(1, len(dataloader))
    if writer is not None and get_rank() == 0:
        writer.add_scalar('val_loss', val_loss, epoch)
    return val_loss


def _eval_loss_head(config):
    return getattr(getattr(config, 'exp', None), 'eval_loss_head', 'torch') or 'torch'


def train_xe_step(model, batch, optimizers, loss_fn, scheduler=None, autocast_dtype=None, gather=True):
    """One optimisation step in the reference's order; returns the (rank-averaged) loss tensor, no host sync.
    gather=False leaves the rank average of the loss to the caller (the segmented capture of the step issues it between replays)."""
    dev = batch['captions'].device.type
    with torch.autocast(dev, dtype=autocast_dtype, enabled=autocast_dtype is not None):
        out = model(batch['samples'], batch['captions'])
    optimizers['model'].zero_grad(set_to_none=False)
    optimizers['backbone'].zero_grad(set_to_none=False)
    target = batch['captions'][:, 1:].contiguous()
    out = out[:, :-1].contiguous()
    loss = loss_fn(out.view(-1, out.shape[-1]).float(), target.view(-1))
    loss.backward()
    finalize = getattr(model, 'finish_gradient_sync', None)
    if finalize is not None:
        finalize()
    optimizers['model'].step()
    optimizers['backbone'].step()
    post = getattr(model, 'after_optimizer_step', None)
    if post is not None:
        post()
    loss = gather_result(loss.detach()) if gather else loss.detach()
    if scheduler is not None:
        lr = scheduler.step()
        assert optimizers['model'].param_groups[0]['lr'] == lr, "LR scheduler doesn't work properly."
    return loss


class _XEStepper(object):
    """train_xe's step: the step graph (GRIT_TRAIN_STEP_GRAPH, default 1 since round 5: what bench.py times is what training runs), i.e. -- one rank, Bf16Compute + FlatAdam, no autocast -- the step
    captured ONCE as a HIP graph (grit_amd/engine/graph_step.py) after two eager steps on the first batch shape and replayed for
    every batch of that shape (collators that pad to a fixed size make that every batch but an epoch's last); other batches, and
    everything once the wrapper's live parameter set changed, run eagerly.  The captured graph is kept on the wrapper across epochs
    (one capture per wrapper and process)."""

    def __init__(self, model, optimizers, loss_fn, scheduler, autocast_dtype):
        import os
        self.args = (model, optimizers, loss_fn, scheduler, autocast_dtype)
        self.want = os.environ.get("GRIT_TRAIN_STEP_GRAPH", "1") != "0" and autocast_dtype is None
        self.eager_seen = 0

    def __call__(self, batch):
        model, optimizers, loss_fn, scheduler, autocast_dtype = self.args
        if self.want and batch['captions'].is_cuda:
            from grit_amd.engine import graph_step
            g = getattr(model, '_grit_step_graph', None)
            if g is not None and g.graph is not None:
                if g.loss_fn_ignore == loss_fn.ignore_index and g.matches(batch, optimizers):
                    g.scheduler = scheduler
                    return g(batch)
                if not g.matches(batch, optimizers) and g.matches_shapes(batch):
                    # same batch shape, yet the graph no longer fits: the optimizers were rebuilt (XE -> SC -> XE) or their runs
                    # re-derived (load_state_dict, a changed live set).  The recorded launches are stale for good: drop the graph
                    # (one capture per wrapper and process) and stay on eager launches
                    g.release()
                    model._grit_step_graph = None  # (the graph's private pool -- a full step of activations -- goes back to the allocator)
                    self.want = False
                    import sys
                    sys.stderr.write("train_xe: the captured step no longer fits this wrapper (optimizers rebuilt, load_state_dict or a changed "
                                     "live parameter set); dropped -- eager launches for the rest of the process\n")
            if g is None and graph_step.supported(model, optimizers) and not getattr(model, '_grit_step_graph_taken', False):
                # (with collectives the capture needs the bucket wrapper in steady state -- live set agreed, no late gradient in the
                # last step: until then the steps stay eager and the capture is simply tried again at the next batch)
                if self.eager_seen >= 2 and (not model.ddp.collective or model.ddp.capture_ready()):
                    try:
                        g = graph_step.GraphedXEStep(model, optimizers, loss_fn, batch, scheduler=scheduler, eager_steps=0)
                        g.loss_fn_ignore = loss_fn.ignore_index
                        model._grit_step_graph = g
                        return g(batch)  # (a capture records, it does not run: the first replay is this batch's step)
                    except Exception as e:  # stay on eager launches; say so once
                        import sys
                        sys.stderr.write("train_xe: step graph not captured (%s: %s); eager launches\n" % (type(e).__name__, str(e)[:200]))
                        self.want = False  # (GraphedXEStep cleaned up after itself: graph_step.abandon_capture)
                self.eager_seen += 1
        return train_xe_step(model, batch, optimizers, loss_fn, scheduler, autocast_dtype)


def train_xe(model, dataloaders, optimizers, text_field, epoch, rank=0, config=None, scheduler=None, writer=None,
             autocast_dtype=None, evaluate=True, checkpoint=True):
    model.train()
    loss_fn = NLLLoss(ignore_index=_pad_index(text_field))
    if scheduler is not None:
        scheduler.step()
    running = .0
    n = len(dataloaders['train'])
    stepper = _XEStepper(model, optimizers, loss_fn, scheduler, autocast_dtype)
    for it, batch in enumerate(_progress(dataloaders['train'], desc=f'Epoch {epoch} - train', unit='it')):
        loss = stepper(batch)
        running += loss.item()  # the reference syncs to the host every step as well (:343)
        if rank == 0 and writer is not None:
            writer.add_scalar('backbone_lr', optimizers['backbone'].param_groups[0]['lr'], epoch * n + it)
            writer.add_scalar('model_lr', optimizers['model'].param_groups[0]['lr'], epoch * n + it)
    _consolidate(model)
    val_loss = evaluate_loss(model, dataloaders['valid'], loss_fn, text_field, epoch, writer, head=_eval_loss_head(config)) \
        if evaluate and 'valid' in dataloaders else 0.0
    if rank == 0 and checkpoint:
        save_checkpoint(model=model, optimizers=optimizers, epoch=epoch, scores=[], best_ciders=(0, 0), config=config,
                        filename='checkpoint_last.pth', scheduler=scheduler)
    if is_dist_avail_and_initialized():
        dist.barrier()
    return {'loss': running / max(1, n), 'reward': 0, 'reward_baseline': 0, 'val_loss': val_loss}


def _host_scorer(gts, gen):
    """The reference's scoring (engine/caption_engine.py:205-207): PTB-tokenise both sides, metrics.compute_scores."""
    from grit_amd.datasets.caption import metrics
    return metrics.compute_scores(metrics.PTBTokenizer.tokenize(gts), metrics.PTBTokenizer.tokenize(gen))[0]


def _split_scorer(dataloader, caption_lists, text_field, device):
    """The DeviceCaptionScorer of a split: built at its first evaluation, kept on the dataloader object (or, where that takes no
    attribute, in a module table) and reused while the split's references are the same -- from the second epoch on a split costs
    one launch and no tokenisation."""
    from grit_amd.ops.caption_scores import DeviceCaptionScorer
    vocab = getattr(text_field, 'vocab', None)
    itos = vocab.itos if vocab is not None and hasattr(vocab, 'itos') else text_field.itos
    eos_token = getattr(text_field, 'eos_token', '<eos>')
    key = (tuple(tuple(c) for c in caption_lists), eos_token, hash(tuple(itos)), str(device))
    own = getattr(dataloader, '__dict__', None)  # (a plain list of batches takes no attribute)
    cache = own.setdefault('_grit_caption_scorers', {}) if own is not None else _SPLIT_SCORERS
    scorer = cache.get(key)
    if scorer is None:
        while len(cache) >= (1 if own is not None else 4):  # a loader keeps one, the module table the last few splits
            cache.pop(next(iter(cache)))
        scorer = cache[key] = DeviceCaptionScorer(caption_lists, itos, eos_token=eos_token, device=device)
    return scorer


_SPLIT_SCORERS = {}


def consensus_reranker(consensus, text_field):
    """What evaluate_metrics(consensus=...) takes, as `rerank(tokens [B, n, T], log_probs) -> Consensus`: a ready reranker (an
    object with a `consensus` method, such as a DeviceCider) is used as it is; a `Cider` with corpus statistics gets its device
    tables at the first call, on the device the tokens come from, and keeps them on the Cider object as the device reward does
    (one DeviceCider serves both).  A Cider without statistics is refused here, before anything is decoded."""
    if hasattr(consensus, 'consensus'):
        return consensus.consensus
    if getattr(consensus, 'doc_frequency', None) is None:
        raise ValueError("consensus reranking needs a Cider built with corpus statistics (Cider(gts)), or a ready reranker")
    if text_field is None:
        raise ValueError("consensus reranking with a Cider needs a text_field (its vocabulary)")
    vocab = getattr(text_field, 'vocab', None)
    itos = vocab.itos if vocab is not None and hasattr(vocab, 'itos') else text_field.itos
    eos_token = getattr(text_field, 'eos_token', '<eos>')
    holder = consensus.__dict__.setdefault('_device_scorers', {})
    vocab_key = (eos_token, hash(tuple(itos)))

    def rerank(tokens, log_probs=None, **kw):
        from grit_amd import lib
        from grit_amd.ops.cider import DeviceCider
        lib.require_device(tokens)
        tables = holder.get((tokens.device, vocab_key))
        if tables is None:
            tables = holder[(tokens.device, vocab_key)] = DeviceCider(consensus, itos, eos_token=eos_token, device=tokens.device)
        return tables.consensus(tokens, log_probs, **kw)

    return rerank


def decode_consensus(model, samples, config, reranker, force_words=None):
    """Decode model.consensus_candidates candidates per image as model.consensus_decode says ('beam': the N best final hypotheses
    of the configured search, constraints and groups honoured; 'sample': N samples) and keep the one that `reranker(tokens,
    log_probs)` chooses (DeviceCider.consensus, or consensus_reranker(...)).  Returns (tokens [B, 1, T], log_probs [B, 1, T]).
    An Ensemble decodes 'beam' only and raises for 'sample', as it does anywhere.  force_words: the batch's sets of forced words
    (Transformer.forward), for 'beam'; with 'sample' the model refuses them."""
    from grit_amd.config import consensus_options
    opt = consensus_options(config)
    n = opt['candidates']
    if n < 2:
        raise ValueError("decode_consensus needs model.consensus_candidates > 1")
    common = dict(seq=None, use_beam_search=True, max_len=config.model.beam_len, eos_idx=config.model.eos_idx)
    if force_words is not None:
        common['force_words'] = force_words
    with torch.no_grad():
        if opt['decode'] == 'sample':
            tokens, log_probs = model(samples, beam_size=n, out_size=n, decode='sample', **opt['sample'], **common)
        else:
            if n > config.model.beam_size:
                raise ValueError("model.consensus_candidates = %d exceeds model.beam_size = %d: a beam search has no more final "
                                 "hypotheses than beams" % (n, config.model.beam_size))
            tokens, log_probs = model(samples, beam_size=config.model.beam_size, out_size=n, return_probs=False,
                                      **beam_constraints(config), **beam_groups(config), **common)
        chosen = reranker(tokens, log_probs)
    return chosen.tokens, chosen.log_probs


def evaluate_metrics(model, optimizers, dataloader, text_field, epoch=0, split='test', config=None, train_res=None,
                     writer=None, best_cider=None, which='ft_xe', scheduler=None, log_and_save=True, scorer=None, scores_out=None,
                     consensus=None):
    """Beam-search every batch (reference :165-183) and score the captions (:194-207).
    scorer: None -- no scoring, returns (token tensors per batch, seconds per batch);
            a callable `scorer(gts, gen) -> dict` on the collapsed, joined, untokenised captions;
            'host' -- the reference's flow: decode, collapse repeated words, PTBTokenizer.tokenize, metrics.compute_scores;
            'device' -- the same scores with the tokens left where beam search wrote them: the references are collected during the
            loop, one launch of grit_caption_scores and one copy back at the end (grit_amd/ops/caption_scores.py).
    The scores dictionary has the keys 'BLEU' (a list of four), 'ROUGE' and 'CIDEr'; the reference's METEOR is not computed.
    With `best_cider` (and log_and_save) the best checkpoint is written when CIDEr >= best_cider and the CIDEr is returned;
    a dictionary passed as `scores_out` receives the scores in either case.
    `model` may be an Ensemble (models/caption/ensemble.py); it cannot save a best checkpoint, so with one best_cider must be
    None (or log_and_save False).
    consensus: a `Cider` with corpus statistics, or a ready reranker (DeviceCider).  With config.model.consensus_candidates = N > 1
    every batch is decoded into N candidates per image (`decode_consensus`) and the candidate that agrees most with the others
    under CIDEr-D is what both scorers see; with the keys off the argument changes nothing."""
    if isinstance(scorer, str) and scorer not in ('host', 'device'):
        raise ValueError("scorer must be None, a callable, 'host' or 'device', not %r" % (scorer,))
    if isinstance(scorer, str) and text_field is None:
        raise ValueError("scorer=%r needs a text_field" % (scorer,))
    if log_and_save and best_cider is not None:
        _refuse_ensemble_checkpoint(model)  # before the evaluation, not after it
    rerank = None
    if consensus is not None:
        from grit_amd.config import consensus_options
        rerank = consensus_reranker(consensus, text_field)  # (refuses a Cider without statistics before the loop)
        if consensus_options(config)['candidates'] < 2:
            rerank = None  # the keys are off: hypothesis 0, as without the argument
    model.eval()
    on_device = scorer == 'device'
    times, tokens, gen, gts, caption_lists = [], [], {}, {}, []
    for it, batch in enumerate(_progress(dataloader, desc=f'Epoch {epoch} - evaluation on {split}', unit='it')):
        t0 = time.time()
        if rerank is not None:
            out = decode_consensus(model, batch['samples'], config, rerank, batch.get('force_words'))[0][:, 0]
        else:
            forced = {} if batch.get('force_words') is None else dict(force_words=batch['force_words'])  # optional per batch
            with torch.no_grad():
                out, _ = model(batch['samples'], seq=None, use_beam_search=True, max_len=config.model.beam_len,
                               eos_idx=config.model.eos_idx, beam_size=config.model.beam_size, out_size=1,
                               return_probs=False, **beam_constraints(config), **beam_groups(config), **forced)
        if out.is_cuda:
            torch.cuda.synchronize()
        times.append(time.time() - t0)
        tokens.append(out)
        if on_device:
            caption_lists.extend(batch['captions'])
        elif text_field is not None and scorer is not None:
            import itertools
            for i, (gts_i, gen_i) in enumerate(zip(batch['captions'], text_field.decode(out, join_words=False))):
                gen[f'{it}_{i}'] = [' '.join(k for k, _ in itertools.groupby(gen_i))]
                gts[f'{it}_{i}'] = gts_i
    avg = sum(times) / max(1, len(times))
    if scorer is None:
        return tokens, avg
    if on_device:
        device_scorer = _split_scorer(dataloader, caption_lists, text_field, tokens[0].device)
        T = max(o.shape[-1] for o in tokens)
        if any(o.shape[-1] != T for o in tokens):  # a batch that ended early is padded with the id the scorer cuts at
            if device_scorer.eos_id is None:
                raise ValueError("batches of different lengths cannot be padded: %r is not in the vocabulary" % (device_scorer.tables.eos_token,))
            tokens_ = [torch.nn.functional.pad(o.reshape(-1, o.shape[-1]), (0, T - o.shape[-1]), value=device_scorer.eos_id) for o in tokens]
        else:
            tokens_ = [o.reshape(-1, T) for o in tokens]
        rows = torch.cat(tokens_)
        scores = device_scorer.aggregate(*device_scorer.launch(rows))
    else:
        scores = (_host_scorer if scorer == 'host' else scorer)(gts, gen)
    if scores_out is not None:
        scores_out.update(scores)
    if log_and_save and best_cider is not None and scores.get('CIDEr', 0) >= best_cider:
        best = (scores['CIDEr'], 0) if split == 'valid' else (0, scores['CIDEr'])
        save_checkpoint(model, optimizers=optimizers, epoch=epoch, scores=scores, best_ciders=best, config=config,
                        filename=f'checkpoint_best_{split}.pth', scheduler=scheduler)
        return scores['CIDEr']
    return scores


def sc_loss(log_probs, reward):
    """Self-critical loss (reference :440-443): -(mean token log-prob of each beam) x (reward - mean reward of the
    image's beams), averaged.  log_probs [B, beam, T] with grad, reward [B, beam]."""
    baseline = torch.mean(reward, -1, keepdim=True)
    return (-torch.mean(log_probs, -1) * (reward - baseline)).mean(), baseline


def train_sc_step(model, batch, optimizers, reward_fn, config):
    """One self-critical step in the reference's order (engine/caption_engine.py:421-449): zero_grad x2 -> beam search
    WITH gradient (out_size = beam_size) -> host reward -> loss -> backward -> barrier -> Adam x2.
    reward_fn(tokens [B, beam, T] int64, batch) -> float tensor [B, beam] on the model's device: in the reference it is
    CIDEr-D of the decoded, PTB-tokenised beams against the ground-truth captions (:433-438), a host-side (Java)
    component that the caller supplies.  Returns (loss, mean reward, mean baseline) as detached device tensors.
    config.optimizer.sc_decode = 'sample' replaces the beams by sc_samples independent samples per image at sc_temperature (no
    truncation; the seed comes from torch's device generator): the same shapes, reward and loss, the baseline being the mean
    reward of an image's samples."""
    beam_size, seq_len = config.model.beam_size, config.model.beam_len
    opt = getattr(config, 'optimizer', None)
    sc_decode = getattr(opt, 'sc_decode', 'beam')
    if sc_decode not in ('beam', 'sample'):
        raise ValueError("optimizer.sc_decode must be 'beam' or 'sample', not %r" % (sc_decode,))
    optimizers['model'].zero_grad()
    optimizers['backbone'].zero_grad()
    if sc_decode == 'sample':
        beam_size = getattr(opt, 'sc_samples', None) or beam_size
        outs, log_probs = model(batch['samples'], seq=None, use_beam_search=True, max_len=seq_len, eos_idx=config.model.eos_idx,
                                beam_size=beam_size, out_size=beam_size, decode='sample',
                                temperature=getattr(opt, 'sc_temperature', 1.0))
    else:
        outs, log_probs = model(batch['samples'], seq=None, use_beam_search=True, max_len=seq_len, eos_idx=config.model.eos_idx,
                                beam_size=beam_size, out_size=beam_size, return_probs=False)
    reward = reward_fn(outs.detach(), batch).to(log_probs.device, torch.float32).view(outs.shape[0], beam_size)
    loss, baseline = sc_loss(log_probs, reward)
    loss.backward()
    finalize = getattr(model, 'finish_gradient_sync', None)
    if finalize is not None:
        finalize()
    if is_dist_avail_and_initialized():
        dist.barrier()  # reference :443
    optimizers['model'].step()
    optimizers['backbone'].step()
    post = getattr(model, 'after_optimizer_step', None)
    if post is not None:
        post()
    return gather_result(loss.detach()), gather_result(reward.mean()), gather_result(baseline.mean())


def cider_reward_fn(cider, text_field, tokenizer_pool=None, tokenize=None, reward='host'):
    """The reference's reward (:433-438): text_field.decode -> PTB tokenisation of generated and ground-truth captions ->
    cider.compute_score(...)[1].  `tokenize` defaults to the native PTB-style tokenizer
    (grit_amd.datasets.caption.metrics.PTBTokenizer.tokenize; the reference's is a Java program); with a `tokenizer_pool` the
    two corpora are tokenised through pool.map as the reference does.
    reward='device': the same numbers from one kernel launch on the tokens where they are (grit_amd/ops/cider.py); the
    references of an image are tokenised and cooked when it is first seen, and the returned [B, beam] tensor stays on the device."""
    import itertools

    import numpy as np

    if reward == 'device':
        return _device_cider_reward_fn(cider, text_field, tokenize)
    if reward != 'host':
        raise ValueError("reward must be 'host' or 'device', not %r" % (reward,))

    if tokenize is None:
        from grit_amd.datasets.caption.metrics import PTBTokenizer
        tokenize = PTBTokenizer.tokenize

    def reward_fn(tokens, batch):
        B, beam, T = tokens.shape
        caps_gen = text_field.decode(tokens.view(-1, T))
        caps_gt = list(itertools.chain(*([c] * beam for c in batch['captions'])))
        caps_gen, caps_gt = (tokenizer_pool.map(tokenize, [caps_gen, caps_gt]) if tokenizer_pool is not None
                             else (tokenize(caps_gen), tokenize(caps_gt)))
        reward = cider.compute_score(caps_gt, caps_gen)[1].astype(np.float32)
        return torch.from_numpy(reward).view(B, beam)

    return reward_fn


def _device_cider_reward_fn(cider, text_field, tokenize):
    if tokenize is not None:
        raise ValueError("reward='device' scores with tables built from the native tokenizer: it takes no custom `tokenize`")
    if getattr(cider, 'doc_frequency', None) is None:
        raise ValueError("reward='device' needs a Cider built with corpus statistics (Cider(gts))")
    vocab = getattr(text_field, 'vocab', None)
    itos = vocab.itos if vocab is not None and hasattr(vocab, 'itos') else text_field.itos
    eos_token = getattr(text_field, 'eos_token', '<eos>')
    # the tables and the cooked references outlive this reward_fn (train_sc makes one per epoch): they are kept on the Cider
    holder = cider.__dict__.setdefault('_device_scorers', {})
    vocab_key = (eos_token, hash(tuple(itos)))

    def reward_fn(tokens, batch):
        from grit_amd import lib
        from grit_amd.ops.cider import DeviceCider
        lib.require_device(tokens)
        scorer = holder.get((tokens.device, vocab_key))
        if scorer is None:  # the tables live on the device the tokens come from; built at the first step
            scorer = holder[(tokens.device, vocab_key)] = DeviceCider(cider, itos, eos_token=eos_token, device=tokens.device)
        return scorer.reward(tokens, batch['captions'])

    return reward_fn


def train_sc(model, dataloaders, optimizers, cider, text_field, tokenizer_pool, device, epoch, config, rank=0, writer=None,
             tokenize=None, evaluate=True, checkpoint=True, reward=None):
    """Self-critical epoch (reference engine/caption_engine.py:388-492), same signature plus `tokenize` (the reference
    hard-wires metrics.PTBTokenizer.tokenize, a Java program that is not part of this build) and `reward` ('host' / 'device',
    default config.optimizer.sc_reward)."""
    model.train()
    if reward is None:
        reward = getattr(getattr(config, 'optimizer', None), 'sc_reward', 'host')
    reward_fn = cider_reward_fn(cider, text_field, tokenizer_pool, tokenize, reward=reward)
    running_loss = running_reward = running_baseline = 0.0
    n = len(dataloaders['train_dict'])
    for it, batch in enumerate(_progress(dataloaders['train_dict'], desc=f'Epoch {epoch} - train', unit='it')):
        loss, reward, baseline = train_sc_step(model, batch, optimizers, reward_fn, config)
        running_loss += loss.item()
        running_reward += reward.item()
        running_baseline += baseline.item()
        if rank == 0 and writer is not None:
            writer.add_scalar('backbone_lr', optimizers['backbone'].param_groups[0]['lr'], epoch * n + it)
            writer.add_scalar('model_lr', optimizers['model'].param_groups[0]['lr'], epoch * n + it)
    loss_fn = NLLLoss(ignore_index=_pad_index(text_field))
    _consolidate(model)
    val_loss = evaluate_loss(model, dataloaders['valid'], loss_fn, text_field, epoch, writer, head=_eval_loss_head(config)) \
        if evaluate and 'valid' in dataloaders else 0.0
    if rank == 0 and checkpoint:
        save_checkpoint(model=model, optimizers=optimizers, epoch=epoch, scores=[], best_ciders=(0, 0), config=config,
                        filename='checkpoint_last.pth', scheduler=None)
    if is_dist_avail_and_initialized():
        dist.barrier()
    n = max(n, 1)
    return {'loss': running_loss / n, 'reward': running_reward / n, 'reward_baseline': running_baseline / n,
            'val_loss': val_loss}
