"""Box helpers of the detector losses (the reference's utils.box_ops surface): plain torch, any device, no torchvision.
Boxes are either (cx, cy, w, h) or corner form (x0, y0, x1, y1) along the last dimension."""
import torch


def box_cxcywh_to_xyxy(x):
    centre, size = x[..., :2], x[..., 2:]
    return torch.cat([centre - 0.5 * size, centre + 0.5 * size], -1)


def box_xyxy_to_cxcywh(x):
    lo, hi = x[..., :2], x[..., 2:]
    return torch.cat([(lo + hi) / 2, hi - lo], -1)


def box_area(boxes):
    return (boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1])


def _pairwise_extent(boxes1, boxes2, inner):
    """[N, M] area of the intersection (inner) or of the smallest enclosing box of every pair."""
    if inner:
        lo = torch.max(boxes1[:, None, :2], boxes2[None, :, :2])
        hi = torch.min(boxes1[:, None, 2:], boxes2[None, :, 2:])
    else:
        lo = torch.min(boxes1[:, None, :2], boxes2[None, :, :2])
        hi = torch.max(boxes1[:, None, 2:], boxes2[None, :, 2:])
    side = (hi - lo).clamp(min=0)
    return side[..., 0] * side[..., 1]


def box_iou(boxes1, boxes2):
    """Pairwise IoU [N, M] of corner-form boxes, and the union areas it was divided by."""
    inter = _pairwise_extent(boxes1, boxes2, True)
    union = box_area(boxes1)[:, None] + box_area(boxes2)[None, :] - inter
    return inter / union, union


def generalized_box_iou(boxes1, boxes2):
    """Pairwise GIoU [N, M] of corner-form boxes (Rezatofighi et al. 2019): IoU - (hull - union) / hull.  Degenerate boxes
    (a corner pair in the wrong order) are refused, they would give inf / nan."""
    if not bool((boxes1[:, 2:] >= boxes1[:, :2]).all()) or not bool((boxes2[:, 2:] >= boxes2[:, :2]).all()):
        raise ValueError("generalized_box_iou: boxes must be (x0, y0, x1, y1) with x1 >= x0 and y1 >= y0")
    iou, union = box_iou(boxes1, boxes2)
    hull = _pairwise_extent(boxes1, boxes2, False)
    return iou - (hull - union) / hull
