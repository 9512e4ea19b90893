"""The detector's set criterion on the device (grit_det_match_f32, grit_lsa_f32, grit_det_loss_{fwd,bwd}_f32, include/grit_hip.h):
Hungarian matching of every (output layer, image) pair in one launch, the losses of all layers in one more, their gradient in one.
This module is the host side: it packs the targets, allocates the per-call workspaces and wraps the loss kernels in ONE autograd node.

Nothing here reads a device value back: the target counts are the shapes of the target tensors, known to the host; the offsets
and the box count travel through pinned memory with a non-blocking copy.
"""

import torch

from grit_amd import lib as _lib
from grit_amd.utils.misc import get_world_size, is_dist_avail_and_initialized

FIELDS = _lib.DET_LOSS_FIELDS
LOSS_CE, LOSS_BBOX, LOSS_GIOU, CARDINALITY_ERROR, CLASS_ERROR = range(5)  # columns of the criterion's [L, FIELDS] output

_p = _lib.ptr


class PackedTargets(object):
    """labels [sum T + 1] int64, boxes [sum T + 1, 4] fp32 (one padding row, so that an empty batch is no null pointer),
    offsets [B + 1] int32 and num_boxes [1] fp32 on the device; counts and t_max on the host.  For the attribute head
    (grit_amd/ops/det_attr.py) also attributes [sum T + 1, A] uint8, rows aligned with labels, and has_attr [B] bool on the
    device.  Both are None when no target carried 'attributes' or 'has_attr' and the caller named no number of attribute classes:
    a batch without attributes is packed with exactly the copies it always was."""

    def __init__(self, labels, boxes, offsets, num_boxes, counts, attributes=None, has_attr=None):
        self.labels, self.boxes, self.offsets, self.num_boxes = labels, boxes, offsets, num_boxes
        self.counts = list(counts)
        self.t_max = max(self.counts) if self.counts else 0
        self.attributes, self.has_attr = attributes, has_attr

    def add_attributes(self, num_attr):
        """Zero attribute rows and has_attr = False where the targets carried none."""
        if self.attributes is None:
            self.attributes = torch.zeros((self.labels.shape[0], int(num_attr)), dtype=torch.uint8, device=self.labels.device)
        if self.has_attr is None:
            self.has_attr = torch.zeros(len(self.counts), dtype=torch.bool, device=self.labels.device)

    def __len__(self):
        return len(self.counts)


def _pack_attributes(targets, counts, device, num_attr):
    """(attributes [sum T + 1, A] uint8 or None, has_attr [B] bool), both on the device.  An image without 'attributes' gets zero
    rows, one without 'has_attr' is False.  has_attr may be a Python bool, a CPU tensor or a device tensor: device values are
    stacked where they are, host values travel through pinned memory -- nothing is read back."""
    given = [t.get('attributes') for t in targets]
    for a, n in zip(given, counts):
        if a is None:
            continue
        if a.dim() != 2 or a.shape[0] != n:
            raise _lib.GritHipError("pack_targets: attributes %s for %d labels" % (tuple(a.shape), n))
        if num_attr is None:
            num_attr = int(a.shape[1])
        elif int(a.shape[1]) != int(num_attr):
            raise _lib.GritHipError("pack_targets: %d attribute classes in the targets, %d expected" % (a.shape[1], num_attr))
    attributes = None
    if num_attr is not None:
        rows = [(a != 0).to(torch.uint8) if a is not None else torch.zeros((n, num_attr), dtype=torch.uint8, device=device)
                for a, n in zip(given, counts)]
        attributes = torch.cat(rows + [torch.zeros((1, num_attr), dtype=torch.uint8, device=device)])
    flags = [t.get('has_attr', False) for t in targets]
    on_device = [isinstance(f, torch.Tensor) and f.is_cuda for f in flags]
    host = torch.tensor([False if dev else bool(f) for f, dev in zip(flags, on_device)], dtype=torch.bool)
    has_attr = host.pin_memory().to(device, non_blocking=True) if device.type == 'cuda' else host.to(device)
    if any(on_device):
        has_attr = torch.stack([f.reshape(()).to(device=device, dtype=torch.bool) if dev else has_attr[i]
                                for i, (f, dev) in enumerate(zip(flags, on_device))])
    return attributes, has_attr


def pack_targets(targets, device=None, num_attr=None):
    """targets: a list (one per image) of {'labels': [T_i] int, 'boxes': [T_i, 4] cxcywh normalised} device tensors, optionally
    with 'attributes' [T_i, A] (multi-hot, any dtype) and 'has_attr' (bool, CPU or device tensor).  num_attr: the number of
    attribute classes the caller expects; with it the attribute rows exist even when no target carries any."""
    if len(targets) == 0:
        raise _lib.GritHipError("pack_targets: an empty batch has nothing to pack")
    _lib.require_device(*[t[k] for t in targets for k in ('labels', 'boxes')] + [t.get('attributes') for t in targets])
    device = targets[0]['boxes'].device if device is None else torch.device(device)
    counts = [int(t['labels'].shape[0]) for t in targets]
    for t, n in zip(targets, counts):
        if tuple(t['boxes'].shape) != (n, 4):
            raise _lib.GritHipError("pack_targets: boxes %s for %d labels" % (tuple(t['boxes'].shape), n))
    labels = torch.cat([t['labels'].reshape(-1).to(torch.int64) for t in targets] + [torch.zeros(1, dtype=torch.int64, device=device)])
    boxes = torch.cat([t['boxes'].reshape(-1, 4).to(torch.float32) for t in targets] + [torch.zeros(1, 4, dtype=torch.float32, device=device)])
    offs = [0]
    for n in counts:
        offs.append(offs[-1] + n)
    offsets = torch.tensor(offs, dtype=torch.int32).pin_memory().to(device, non_blocking=True)
    # the number of boxes the losses are divided by: the mean over the ranks, at least 1 (reference od_losses.py:259-268, whose
    # .item() is not reproduced: the kernels read the scalar from device memory)
    if is_dist_avail_and_initialized():
        num_boxes = torch.tensor([float(offs[-1])], dtype=torch.float32).pin_memory().to(device, non_blocking=True)
        torch.distributed.all_reduce(num_boxes)
        num_boxes = torch.clamp(num_boxes / get_world_size(), min=1)
    else:
        num_boxes = torch.tensor([max(float(offs[-1]), 1.0)], dtype=torch.float32).pin_memory().to(device, non_blocking=True)
    attributes = has_attr = None
    if num_attr is not None or any('attributes' in t or 'has_attr' in t for t in targets):
        attributes, has_attr = _pack_attributes(targets, counts, device, num_attr)
    return PackedTargets(labels, boxes, offsets, num_boxes, counts, attributes, has_attr)


def _check_outputs(logits, boxes, packed, what):
    _lib.require_device(logits, boxes)
    if logits.dim() != 4 or boxes.dim() != 4 or boxes.shape != logits.shape[:3] + (4,):
        raise _lib.GritHipError("%s: logits [L, B, Q, K] and boxes [L, B, Q, 4], got %s and %s" % (what, tuple(logits.shape), tuple(boxes.shape)))
    if logits.dtype != torch.float32 or boxes.dtype != torch.float32:
        raise _lib.GritHipError("%s: fp32 only (cast the heads' outputs with .float()), got %s / %s" % (what, logits.dtype, boxes.dtype))
    if logits.shape[1] != len(packed):
        raise _lib.GritHipError("%s: %d images in the outputs, %d target entries" % (what, logits.shape[1], len(packed)))
    if packed.labels.device != logits.device:
        raise _lib.GritHipError("%s: outputs on %s, targets on %s" % (what, logits.device, packed.labels.device))


def match(logits, boxes, packed, cost_class=1.0, cost_bbox=1.0, cost_giou=1.0, return_cost=False):
    """logits [L, B, Q, K], boxes [L, B, Q, 4] fp32 -> match_q [L, B, max(Tmax, 1)] int32 (query of each target, -1 unmatched or
    padding) and match_t [L, B, Q] int32 (target of each query, or -1); with return_cost also the fp32 cost [L, B, Q, max(Tmax, 1)]
    the assignment is the optimum of.  One launch, no synchronisation.  Targets per image <= lib.DET_MAX_SIDE, and Q too."""
    _check_outputs(logits, boxes, packed, "det match")
    L, B, Q, K = logits.shape
    t_max = max(packed.t_max, 1)
    logits = logits.detach()
    boxes = boxes.detach()
    logits = logits if logits.is_contiguous() else logits.contiguous()
    boxes = boxes if boxes.is_contiguous() else boxes.contiguous()
    dev = logits.device
    cost = torch.empty((L, B, Q, t_max), dtype=torch.float32, device=dev)
    match_q = torch.empty((L, B, t_max), dtype=torch.int32, device=dev)
    match_t = torch.empty((L, B, Q), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with _lib.device_guard(dev):
        st = lib.grit_det_match_f32(_p(logits), _p(boxes), _p(packed.labels), _p(packed.boxes), _p(packed.offsets), L, B, Q, K, t_max,
                                    float(cost_class), float(cost_bbox), float(cost_giou), _p(cost), t_max, _p(match_q), _p(match_t),
                                    _lib.current_stream_ptr())
    _lib.check(st, "grit_det_match_f32")
    return (match_q, match_t, cost) if return_cost else (match_q, match_t)


def linear_sum_assignment(cost, counts, rows=None):
    """The solver alone.  cost [P, Q, ld] fp32 (problem p uses the columns [0, counts[p]) and, with `rows`, the rows [0, rows[p])),
    counts / rows [P] int32 on the device -> match_q [P, ld] int32 and match_t [P, Q] int32 as in `match`."""
    _lib.require_device(cost, counts, rows)
    if rows is not None and (rows.dtype != torch.int32 or rows.numel() != cost.shape[0] or not rows.is_contiguous()):
        raise _lib.GritHipError("lsa: rows must be [P] int32")
    if cost.dim() != 3 or cost.dtype != torch.float32 or not cost.is_contiguous():
        raise _lib.GritHipError("lsa: cost must be a contiguous [P, Q, ld] fp32 tensor")
    if counts.dtype != torch.int32 or counts.numel() != cost.shape[0] or not counts.is_contiguous():
        raise _lib.GritHipError("lsa: counts must be [P] int32")
    P, Q, ld = cost.shape
    match_q = torch.empty((P, ld), dtype=torch.int32, device=cost.device)
    match_t = torch.empty((P, Q), dtype=torch.int32, device=cost.device)
    lib = _lib.load()
    with _lib.device_guard(cost.device):
        st = lib.grit_lsa_f32(_p(cost), _p(counts), _p(rows), P, Q, ld, ld, _p(match_q), _p(match_t), _lib.current_stream_ptr())
    _lib.check(st, "grit_lsa_f32")
    return match_q, match_t


class _SetCriterionFn(torch.autograd.Function):
    """out [L, FIELDS] of grit_det_loss_fwd_f32; the backward is one launch that takes the upstream gradient of `out` as the
    per-layer loss weights."""

    @staticmethod
    def forward(ctx, logits, boxes, match_t, packed, alpha):
        L, B, Q, K = logits.shape
        dev = logits.device
        chunks = (Q + _lib.DET_LOSS_ROWS - 1) // _lib.DET_LOSS_ROWS
        partials = torch.empty((L * B * chunks, 8), dtype=torch.float64, device=dev)
        out = torch.empty((L, FIELDS), dtype=torch.float32, device=dev)
        # the finalising workgroup is found by a ticket counter: this call's own, zeroed by the entry point, so neither a second
        # stream nor a launch that did not finish can leave a later call with a stale count
        ticket = torch.empty(1, dtype=torch.int32, device=dev)
        lib = _lib.load()
        with _lib.device_guard(dev):
            st = lib.grit_det_loss_fwd_f32(_p(logits), _p(boxes), _p(packed.labels), _p(packed.boxes), _p(packed.offsets), _p(match_t),
                                           L, B, Q, K, float(alpha), _p(packed.num_boxes), _p(partials), _p(ticket), _p(out),
                                           _lib.current_stream_ptr())
        _lib.check(st, "grit_det_loss_fwd_f32")
        ctx.save_for_backward(logits, boxes, match_t)
        ctx.packed, ctx.alpha = packed, float(alpha)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        logits, boxes, match_t = ctx.saved_tensors
        packed = ctx.packed
        L, B, Q, K = logits.shape
        coef = grad_out.to(torch.float32)
        coef = coef if coef.is_contiguous() else coef.contiguous()
        dlogits = torch.empty_like(logits)
        dboxes = torch.empty_like(boxes)
        lib = _lib.load()
        with _lib.device_guard(logits.device):
            st = lib.grit_det_loss_bwd_f32(_p(logits), _p(boxes), _p(packed.labels), _p(packed.boxes), _p(packed.offsets), _p(match_t),
                                           L, B, Q, K, ctx.alpha, _p(packed.num_boxes), _p(coef), FIELDS, _p(dlogits), _p(dboxes),
                                           _lib.current_stream_ptr())
        _lib.check(st, "grit_det_loss_bwd_f32")
        return dlogits, dboxes, None, None, None


def set_criterion(logits, boxes, match_t, packed, focal_alpha=0.25):
    """logits [L, B, Q, K], boxes [L, B, Q, 4] fp32, match_t [L, B, Q] from `match` -> [L, FIELDS] fp32: per layer loss_ce,
    loss_bbox, loss_giou (differentiable), cardinality_error, class_error (columns LOSS_CE .. CLASS_ERROR)."""
    _check_outputs(logits, boxes, packed, "det criterion")
    if match_t.dtype != torch.int32 or tuple(match_t.shape) != tuple(logits.shape[:3]) or not match_t.is_contiguous():
        raise _lib.GritHipError("det criterion: match_t must be a contiguous [L, B, Q] int32 tensor")
    logits = logits if logits.is_contiguous() else logits.contiguous()
    boxes = boxes if boxes.is_contiguous() else boxes.contiguous()
    return _SetCriterionFn.apply(logits, boxes, match_t, packed, focal_alpha)
