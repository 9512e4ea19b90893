"""One optimisation step of detector pre-training (reference engine/det_solver.py:58-110, without its hook machinery), the
optimizers it is taken with (reference train_detector.py:24-89) and the validation epoch (engine/det_solver.py:192-263)."""
import torch
from torch.optim.lr_scheduler import MultiStepLR


def weighted_loss(loss_dict, weight_dict):
    """The sum the detector is trained on: every entry of loss_dict that weight_dict names, times its weight."""
    return sum(loss_dict[k] * weight_dict[k] for k in loss_dict if k in weight_dict)


def _is_wrapper(model):
    from grit_amd.amp import Bf16Compute
    return isinstance(model, Bf16Compute)


def build_optimizers_schedulers(model, config):
    """The reference's rule: AdamW over four groups -- head and backbone ('backbone' in the name), each with and without weight
    decay (1-D parameters, names ending in '.bias' and names whose last component is on the skip list are not decayed; the skip
    list is backbone.no_weight_decay() when the backbone has it, else ['query_embed']) -- with lr / lr_backbone / weight_decay of
    config.optimizer; a second AdamW at sp_lr for the parameters whose name contains one of config.optimizer.sp_names, when there
    are any; one MultiStepLR (lr_drop_epochs / sp_lr_drop_epochs, decay_rate) per optimizer.  Empty groups are dropped.

    For a grit_amd.amp.Bf16Compute wrapper the groups hold its fp32 masters and the optimizers are its flat AdamW
    (Bf16Compute.flat_adamw); for a plain module they are torch.optim.AdamW.  Returns (optimizers, lr_schedulers)."""
    wrapped = _is_wrapper(model)
    inner = model.module if wrapped else model
    backbone = getattr(inner, 'backbone', None)
    skip = backbone.no_weight_decay() if hasattr(backbone, 'no_weight_decay') else ['query_embed']
    named = model.named_master_parameters() if wrapped else [(n, p) for n, p in inner.named_parameters() if p.requires_grad]
    opt = config.optimizer
    sp_names = list(getattr(opt, 'sp_names', None) or [])
    head, det_no_decay, backbone_decay, backbone_no_decay, sp_params = [], [], [], [], []
    for name, param in named:
        if any(ns in name for ns in sp_names):
            sp_params.append(param)
            continue
        no_decay = len(param.shape) == 1 or name.endswith(".bias") or name.split('.')[-1] in skip
        if "backbone" in name:
            (backbone_no_decay if no_decay else backbone_decay).append(param)
        else:
            (det_no_decay if no_decay else head).append(param)
    groups = [{"params": head, "lr": opt.lr, "weight_decay": opt.weight_decay},
              {"params": det_no_decay, "lr": opt.lr, "weight_decay": 0.},
              {"params": backbone_no_decay, "lr": opt.lr_backbone, "weight_decay": 0.},
              {"params": backbone_decay, "lr": opt.lr_backbone, "weight_decay": opt.weight_decay}]
    groups = [g for g in groups if g["params"]]

    def adamw(params, lr):
        if wrapped:
            return model.flat_adamw(params, lr=lr, weight_decay=opt.weight_decay)
        return torch.optim.AdamW(params, lr=lr, weight_decay=opt.weight_decay)

    optimizers, drops = [], []
    if groups:
        optimizers.append(adamw(groups, opt.lr))
        drops.append(opt.lr_drop_epochs)
    if sp_params:
        optimizers.append(adamw(sp_params, opt.sp_lr))
        drops.append(opt.sp_lr_drop_epochs)
    schedulers = [MultiStepLR(o, list(d), gamma=opt.decay_rate) for o, d in zip(optimizers, drops)]
    return optimizers, schedulers


def train_step(model, criterion, optimizer, samples, targets, max_norm=0.1):
    """forward -> criterion -> weighted sum over criterion.weight_dict -> backward -> gradient clipping (max_norm > 0) -> step.
    `optimizer` is one optimizer or a list of them.  With a grit_amd.amp.Bf16Compute wrapper the gradients lie in its flat bf16
    buckets: backward -> finish_gradient_sync() -> clip_grad_norm_(max_norm) (norm and clip factor stay on the device) -> every
    optimizer's step() -> after_optimizer_step().
    Returns (total, loss_dict): device tensors, nothing is read back here."""
    optimizers = list(optimizer) if isinstance(optimizer, (list, tuple)) else [optimizer]
    model.train()
    criterion.train()
    loss_dict = criterion(model(samples), targets)
    total = weighted_loss(loss_dict, criterion.weight_dict)
    for o in optimizers:
        o.zero_grad(set_to_none=True)
    total.backward()
    if _is_wrapper(model):
        model.finish_gradient_sync()
        if max_norm and max_norm > 0:
            model.clip_grad_norm_(max_norm)
        for o in optimizers:
            o.step()
        model.after_optimizer_step()
    else:
        if max_norm and max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], max_norm)
        for o in optimizers:
            o.step()
    return total.detach(), {k: v.detach() for k, v in loss_dict.items()}


MAP_KEYS = ('map', 'map50', 'map75', 'map_small', 'map_medium', 'map_large')  # the first six COCO stats, the Valider's names


@torch.no_grad()
def evaluate(model, criterion, postprocessors, batches, evaluator, vg_evaluator=None):
    """The reference's validation epoch (engine/det_solver.py:192-263) on one rank.  batches: an iterable of (samples, targets) on
    the device, every target with 'image_id' and 'orig_size'; evaluator: datasets.detection.metrics.CocoEvaluator.  Per batch:
    model -> criterion -> postprocessors['bbox'] -> evaluator.update, with no host synchronisation inside the loop; the records
    come to the host once, in evaluator.accumulate().  Returns {'losses': the mean weighted sum, every weighted loss's mean,
    'bbox_map', 'bbox_map50', 'bbox_map75', 'bbox_map_small', 'bbox_map_medium', 'bbox_map_large', 'result_text'}.

    vg_evaluator: a datasets.detection.metrics.VGEvaluator, fed in the same loop with the same 'bbox' results as its kind 'obj'
    and, when it has the kind 'attr', with postprocessors['attr'](outputs, sizes) -- two more launches per batch, still no host
    synchronisation.  The result gains 'vg_obj_map', 'vg_obj_wmap', 'vg_text' and, with 'attr', 'vg_attr_map', 'vg_attr_wmap'."""
    model.eval()
    criterion.eval()
    if vg_evaluator is not None and 'attr' in vg_evaluator.kinds and 'attr' not in postprocessors:
        raise ValueError("evaluate: the VG evaluator has the kind 'attr' but the model gives no attribute detections "
                         "(postprocessors['attr'] comes with model.has_attr_head)")
    sums, steps = {}, 0
    for samples, targets in batches:
        outputs = model(samples)
        loss_dict = criterion(outputs, targets)
        weighted = {k: v * criterion.weight_dict[k] for k, v in loss_dict.items() if k in criterion.weight_dict}
        weighted['losses'] = sum(weighted.values())
        for k, v in weighted.items():
            sums[k] = sums[k] + v.detach() if k in sums else v.detach()
        sizes = torch.stack([t['orig_size'] for t in targets], dim=0)
        results = postprocessors['bbox'](outputs, sizes)
        evaluator.update(results, targets)
        if vg_evaluator is not None:
            vg_results = {'obj': results}
            if 'attr' in vg_evaluator.kinds:
                vg_results['attr'] = postprocessors['attr'](outputs, sizes)
            vg_evaluator.update(vg_results, targets)
        steps += 1
    evaluator.synchronize_between_processes()
    evaluator.accumulate()
    evaluator.summarize()
    box = evaluator.coco_eval['bbox']
    out = {k: float(v) / steps for k, v in sums.items()}
    out.update({'bbox_' + name: float(box.stats[i]) for i, name in enumerate(MAP_KEYS)})
    out['result_text'] = box.result_text
    if vg_evaluator is not None:
        vg_evaluator.synchronize_between_processes()
        vg_evaluator.accumulate()
        vg_evaluator.summarize()
        for kind in vg_evaluator.kinds:
            out['vg_%s_map' % kind] = float(vg_evaluator.stats[kind]['map'])
            out['vg_%s_wmap' % kind] = float(vg_evaluator.stats[kind]['wmap'])
        out['vg_text'] = vg_evaluator.result_text
    return out
