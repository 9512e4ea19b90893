"""Losses of detector pre-training: HungarianMatcher, SetCriterion, PostProcess (the surface of the reference's
models/detection/od_losses.py), with the hot part on the device (grit_amd/ops/det_loss.py).

The criterion of a step is two launches forward for ALL output layers together -- cost matrices + assignments, then the losses --
and one launch backward; the host is never waited for.  The reference does, per output layer, a dozen elementwise ops for the cost,
a copy to the host, one scipy solve per image, a one-hot target and some fifteen elementwise ops for the focal loss.

With an attribute head (`attr_logits` in the outputs) the reference's weighted_attr_loss of the last layer joins as 'loss_attr':
one more launch each way (grit_amd/ops/det_attr.py), fed by the last layer's slab of the same match -- no second match, and no
host-side index lists or `if target['has_attr']` on a device scalar as in the reference.

Out of scope, each refused: the `masks` loss, `enc_outputs`.
"""
import torch
from torch import nn
import torch.nn.functional as F

from grit_amd.ops import det_attr as _det_attr
from grit_amd.ops import det_eval as _det_eval
from grit_amd.ops import det_loss as _det


def sigmoid_focal_loss(inputs, targets, num_boxes, alpha=0.25, gamma=2):
    """Focal loss (Lin et al. 2017) of logits against 0 / 1 targets, averaged over dim 1, summed and divided by num_boxes; a
    negative alpha switches the class balancing off.  Plain torch, built from log-sigmoids the way the kernel's focal_terms is:
    a positive costs -log sigmoid(x) weighted by sigmoid(-x)^gamma, a negative -log sigmoid(-x) weighted by sigmoid(x)^gamma.
    The criterion below does not go through it (its kernel never builds `targets`)."""
    log_p, log_q = F.logsigmoid(inputs), F.logsigmoid(-inputs)
    on_positive = -log_p * torch.exp(gamma * log_q)
    on_negative = -log_q * torch.exp(gamma * log_p)
    if alpha >= 0:
        on_positive, on_negative = alpha * on_positive, (1 - alpha) * on_negative
    per_element = torch.where(targets > 0.5, on_positive, on_negative) if targets.dtype == torch.bool else \
        targets * on_positive + (1 - targets) * on_negative
    return per_element.mean(1).sum() / num_boxes


class HungarianMatcher(nn.Module):
    """Optimal one-to-one assignment of predictions to targets under
    cost_bbox * L1 + cost_class * (focal-style class cost) - cost_giou * GIoU, on the device."""

    def __init__(self, cost_class=1, cost_bbox=1, cost_giou=1):
        super().__init__()
        if cost_class == 0 and cost_bbox == 0 and cost_giou == 0:
            raise ValueError("HungarianMatcher: at least one of the three cost weights must be non-zero")
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou

    @torch.no_grad()
    def match_layers(self, logits, boxes, packed, return_cost=False):
        """All output layers at once: logits [L, B, Q, K], boxes [L, B, Q, 4] -> grit_amd.ops.det_loss.match(...)."""
        return _det.match(logits.float(), boxes.float(), packed, self.cost_class, self.cost_bbox, self.cost_giou, return_cost)

    @torch.no_grad()
    def forward(self, outputs, targets):
        """outputs: {'pred_logits': [B, Q, K], 'pred_boxes': [B, Q, 4]}; targets: per image {'labels': [T], 'boxes': [T, 4]}.
        Returns per image (index_i, index_j), int64 on the device: the matched predictions in increasing order and their targets,
        min(Q, T) of each -- the pairs and the order scipy.optimize.linear_sum_assignment gives on the same cost matrix."""
        packed = targets if isinstance(targets, _det.PackedTargets) else _det.pack_targets(targets)
        match_q, match_t = self.match_layers(outputs["pred_logits"][None], outputs["pred_boxes"][None], packed)
        Q = match_t.shape[-1]
        pairs = []
        for b, T in enumerate(packed.counts):
            if T <= Q:  # every target is matched: sort the pairs by prediction
                q = match_q[0, b, :T].to(torch.int64)
                order = torch.argsort(q)
                pairs.append((q[order], order))
            else:  # every prediction is matched
                pairs.append((torch.arange(Q, dtype=torch.int64, device=match_t.device), match_t[0, b].to(torch.int64)))
        return pairs


def build_matcher(args):
    """The matcher of a configuration's `det_module.matcher` group (keys set_cost_class, set_cost_bbox, set_cost_giou)."""
    weights = {name: getattr(args, 'set_cost_' + name) for name in ('class', 'bbox', 'giou')}
    return HungarianMatcher(weights['class'], weights['bbox'], weights['giou'])


class SetCriterion(nn.Module):
    """Matches predictions to targets, then supervises the matched pairs (class: sigmoid focal loss over every logit; box: L1 and
    GIoU) -- for the last output layer and every auxiliary one in the same launches.

    forward(outputs, targets) -> {'loss_ce', 'class_error', 'loss_bbox', 'loss_giou', 'cardinality_error'} and the same keys
    without class_error suffixed `_i` for outputs['aux_outputs'][i]; 0-d fp32 device tensors.  With outputs['attr_logits'] [B, Q, A]
    also 'loss_attr' (last layer only); the targets may then carry 'attributes' [T, A] and 'has_attr'.

    `losses` is kept for the reference's signature and only checked for 'masks': like the reference's forward, every call computes
    labels, boxes and cardinality whatever the list says.  When the outputs carry 'pred_logits_all' / 'pred_boxes_all' (the
    [levels, B, Q, *] stacks DetectionModule.detection_head adds in training, auxiliary levels first, the last level last) they are
    read as they are; otherwise the per-level tensors are stacked, which copies them."""

    def __init__(self, num_classes, matcher, weight_dict, losses, focal_alpha=0.25):
        super().__init__()
        if 'masks' in losses:
            raise NotImplementedError("SetCriterion: the masks loss is not implemented")
        self.num_classes, self.matcher, self.weight_dict, self.losses, self.focal_alpha = num_classes, matcher, weight_dict, losses, focal_alpha

    def forward(self, outputs, targets):
        if not isinstance(targets, list):
            raise TypeError("SetCriterion: targets must be a list with one dict per image, got %s" % type(targets).__name__)
        if 'enc_outputs' in outputs:
            raise NotImplementedError("SetCriterion: enc_outputs (two-stage proposals) are not implemented")
        if len(targets) == 0:
            return {}
        layers = list(outputs.get('aux_outputs', ())) + [outputs]
        if 'pred_logits_all' in outputs and 'pred_boxes_all' in outputs:
            logits, boxes = outputs['pred_logits_all'].float(), outputs['pred_boxes_all'].float()
            if logits.shape[0] != len(layers):
                raise ValueError("SetCriterion: %d stacked levels for %d outputs" % (logits.shape[0], len(layers)))
        else:
            logits = torch.stack([o['pred_logits'] for o in layers]).float()
            boxes = torch.stack([o['pred_boxes'] for o in layers]).float()
        attr_logits = outputs.get('attr_logits')
        packed = _det.pack_targets(targets, num_attr=None if attr_logits is None else attr_logits.shape[-1])
        _, match_t = self.matcher.match_layers(logits, boxes, packed)
        out = _det.set_criterion(logits, boxes, match_t, packed, self.focal_alpha)
        names = (('loss_ce', _det.LOSS_CE), ('loss_bbox', _det.LOSS_BBOX), ('loss_giou', _det.LOSS_GIOU),
                 ('cardinality_error', _det.CARDINALITY_ERROR))
        last = len(layers) - 1
        cell = out.reshape(-1).unbind(0)  # ONE autograd node hands the weighted sum's coefficients back to the criterion's backward
        at = lambda layer, col: cell[layer * _det.FIELDS + col]
        losses = {'loss_ce': at(last, _det.LOSS_CE), 'class_error': at(last, _det.CLASS_ERROR).detach()}
        for name, col in names[1:]:
            losses[name] = at(last, col)
        for i in range(last):
            for name, col in names:
                losses['%s_%d' % (name, i)] = at(i, col)
        if attr_logits is not None:  # the last layer only, as the reference; its slab of match_t is a contiguous view
            losses['loss_attr'] = _det_attr.attr_loss(attr_logits.float(), match_t[last], packed)
        for key in list(losses):
            if key.startswith('cardinality_error'):
                losses[key] = losses[key].detach()
        return losses


class PostProcess(nn.Module):
    """Model outputs -> per image the 100 best (score, label, box) with boxes in absolute corner form.  The selection and the boxes
    are grit_det_topk_f32 (grit_amd/ops/det_eval.py): it selects on the logits, the sigmoid is applied to the selected ones only."""

    @torch.no_grad()
    def forward(self, outputs, target_sizes):
        logits, boxes = outputs['pred_logits'], outputs['pred_boxes']
        if len(logits) != len(target_sizes) or target_sizes.shape[1] != 2:
            raise ValueError("PostProcess: target_sizes must be [batch, 2] (height, width)")
        K = logits.shape[2]
        top_logit, top_index, corners = _det_eval.det_topk(logits.float(), boxes.float(), target_sizes.float())
        scores, labels = top_logit.sigmoid(), top_index.to(torch.int64) % K
        return [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, corners)]


class PostProcessAttr(nn.Module):
    """Model outputs with 'attr_logits' [B, Q, A] -> per image the min(100, Q A) best (score, attribute, box): the attribute
    detections of the Visual Genome protocol (datasets/detection/metrics/vg_eval.py).  The reference has no counterpart; this is
    PostProcess on the attribute map -- grit_det_topk_f32 unchanged, score = the fp32 sigmoid of the selected logit, label = the
    attribute index, box = that query's box as absolute corners."""

    @torch.no_grad()
    def forward(self, outputs, target_sizes):
        if 'attr_logits' not in outputs:
            raise ValueError("PostProcessAttr: the outputs have no 'attr_logits' (model.has_attr_head is off)")
        logits, boxes = outputs['attr_logits'], outputs['pred_boxes']
        if len(logits) != len(target_sizes) or target_sizes.shape[1] != 2:
            raise ValueError("PostProcessAttr: target_sizes must be [batch, 2] (height, width)")
        A = logits.shape[2]
        top_logit, top_index, corners = _det_eval.det_topk(logits.float(), boxes.float(), target_sizes.float())
        scores, labels = top_logit.sigmoid(), top_index.to(torch.int64) % A
        return [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, corners)]
