"""Detector evaluation on the device (grit_det_topk_f32, grit_det_eval_img, include/grit_hip.h): the host side.

  * `det_topk(logits, boxes, sizes)`: the device half of PostProcess -- an image's 100 best (logit, flat index, absolute box).
  * `pack_ground_truth(dataset_like)`, once per split: the annotations as flat arrays, images in ascending id order (an image's
    slot is the rank of its id, the order in which the accumulation concatenates images before its stable sort), an image's
    annotations sorted by category and in annotation order within a category.
  * `DeviceGroundTruth`, `EvalRecords`, `eval_images(...)`: the per-image matching launch and the record buffers it fills, which
    span the split and stay on the device until the accumulation copies them once.
  * `pack_ground_truth_attr(dataset_like, num_attr)`, `VocRecords`, `voc_images(...)`: the same three steps for the Visual Genome
    protocol (grit_det_voc_img): PASCAL-VOC matching at one threshold, for objects over pack_ground_truth's arrays and for
    attributes over arrays in which an object stands once per attribute it carries.

Nothing here reads a device value back.  Accumulation and summary: grit_amd/datasets/detection/metrics/coco_eval.py and vg_eval.py.
"""
import collections
import ctypes

import numpy as np

from grit_amd import lib as _lib

TOPK = _lib.DET_TOPK
MAX_PER_IMAGE = _lib.DET_MAX_SIDE


class PackedGroundTruth(object):
    """Host arrays (numpy) of one split.  img_ids [I] int64 ascending; cat_ids: the evaluated category ids, ascending (a category
    id is a class index); n_cat = max id + 1; cat_valid [n_cat] uint8; img_off [I + 1] int32; per annotation box [G, 4] float64
    xywh, area [G] float64, cat [G] int32, crowd [G] uint8, ann_img [G] int32 (its image's slot), ann_id [G] int64."""

    def __init__(self, img_ids, cat_ids, img_off, box, area, cat, crowd, ann_img, ann_id):
        self.img_ids, self.cat_ids = np.asarray(img_ids, np.int64), np.asarray(cat_ids, np.int64)
        self.n_img, self.n_cat = len(self.img_ids), (int(self.cat_ids.max()) + 1 if len(self.cat_ids) else 0)
        self.cat_valid = np.zeros(self.n_cat, np.uint8)
        self.cat_valid[self.cat_ids] = 1
        self.img_off, self.box, self.area, self.cat, self.crowd, self.ann_img, self.ann_id = img_off, box, area, cat, crowd, ann_img, ann_id
        self.max_per_img = int(np.diff(img_off).max()) if self.n_img else 0


def pack_ground_truth(dataset_like):
    """dataset_like: the COCO API's surface -- getImgIds(), getCatIds(), getAnnIds(imgIds=[...]), loadAnns(ids); an annotation is
    {'id', 'image_id', 'category_id', 'bbox': [x, y, w, h], 'area', 'iscrowd'}.  Annotations of a category that getCatIds() does
    not list are left out, as the reference's evaluation leaves them out.  ValueError for annotation id 0 (the reference uses
    the id as the match flag and would count such a match as a miss), for a negative category id and for an image with more
    than MAX_PER_IMAGE annotations."""
    img_ids = sorted(int(i) for i in dataset_like.getImgIds())
    cat_ids = sorted(int(c) for c in dataset_like.getCatIds())
    if not img_ids or not cat_ids:
        raise ValueError("pack_ground_truth: a split needs at least one image and one category")
    if cat_ids[0] < 0 or len(set(img_ids)) != len(img_ids):
        raise ValueError("pack_ground_truth: category ids are class indices >= 0 and image ids are unique")
    cats = set(cat_ids)
    img_off, box, area, cat, crowd, ann_img, ann_id = [0], [], [], [], [], [], []
    for slot, img in enumerate(img_ids):
        anns = [a for a in dataset_like.loadAnns(dataset_like.getAnnIds(imgIds=[img])) if int(a['category_id']) in cats]
        if len(anns) > MAX_PER_IMAGE:
            raise ValueError("pack_ground_truth: image %d has %d annotations, the evaluation kernel takes %d" % (img, len(anns), MAX_PER_IMAGE))
        for a in sorted(anns, key=lambda a: int(a['category_id'])):  # stable: annotation order within a category
            if int(a['id']) == 0:
                raise ValueError("pack_ground_truth: annotation id 0 (image %d) cannot be told from 'unmatched'" % img)
            box.append([float(v) for v in a['bbox']])
            area.append(float(a['area']))
            cat.append(int(a['category_id']))
            crowd.append(1 if a.get('iscrowd', 0) else 0)
            ann_img.append(slot)
            ann_id.append(int(a['id']))
        img_off.append(len(cat))
    return PackedGroundTruth(img_ids, cat_ids, np.asarray(img_off, np.int32), np.asarray(box, np.float64).reshape(-1, 4),
                             np.asarray(area, np.float64), np.asarray(cat, np.int32), np.asarray(crowd, np.uint8),
                             np.asarray(ann_img, np.int32), np.asarray(ann_id, np.int64))


def pack_ground_truth_attr(dataset_like, num_attr):
    """The attribute split of the Visual Genome protocol as a PackedGroundTruth whose classes are the attributes 0 .. num_attr - 1:
    an object contributes one row (class = a, its box) for every attribute a it carries, so the matching kernel is the same for
    objects and attributes.  dataset_like: getImgIds(), getAnnIds(imgIds=[...]), loadAnns(ids) and loadImgs(ids); an annotation
    carries 'attributes', a list of attribute ids (absent or empty: none; an id listed twice counts once), an image 'has_attr'
    (absent: True).  An image with has_attr False is not part of the split (DeviceGroundTruth.slots_of gives it -1, so neither its
    rows nor its detections count).  An image's rows are sorted by attribute and are in annotation order within an attribute;
    area = w * h, crowd = 0, ann_id = the object's id.  ValueError for an attribute id outside [0, num_attr), for a split without
    images and for an image with more than MAX_PER_IMAGE rows."""
    num_attr = int(num_attr)
    if num_attr <= 0:
        raise ValueError("pack_ground_truth_attr: num_attr must be positive")
    ids = sorted(int(i) for i in dataset_like.getImgIds())
    if len(set(ids)) != len(ids):
        raise ValueError("pack_ground_truth_attr: image ids are unique")
    img_ids = [i for i in ids if dataset_like.loadImgs([i])[0].get('has_attr', True)]
    if not img_ids:
        raise ValueError("pack_ground_truth_attr: no image of the split has attributes")
    img_off, box, cat, ann_img, ann_id = [0], [], [], [], []
    for slot, img in enumerate(img_ids):
        rows = []
        for a in dataset_like.loadAnns(dataset_like.getAnnIds(imgIds=[img])):
            for attr in sorted(set(int(v) for v in a.get('attributes', ()))):
                if not 0 <= attr < num_attr:
                    raise ValueError("pack_ground_truth_attr: attribute %d of annotation %s is outside [0, %d)" % (attr, a['id'], num_attr))
                rows.append((attr, a))
        if len(rows) > MAX_PER_IMAGE:
            raise ValueError("pack_ground_truth_attr: image %d has %d attribute rows, the evaluation kernel takes %d"
                             % (img, len(rows), MAX_PER_IMAGE))
        for attr, a in sorted(rows, key=lambda r: r[0]):  # stable: annotation order within an attribute
            box.append([float(v) for v in a['bbox']])
            cat.append(attr)
            ann_img.append(slot)
            ann_id.append(int(a['id']))
        img_off.append(len(cat))
    box = np.asarray(box, np.float64).reshape(-1, 4)
    return PackedGroundTruth(img_ids, np.arange(num_attr), np.asarray(img_off, np.int32), box, box[:, 2] * box[:, 3],
                             np.asarray(cat, np.int32), np.zeros(len(cat), np.uint8), np.asarray(ann_img, np.int32),
                             np.asarray(ann_id, np.int64))


class DeviceGroundTruth(object):
    """A PackedGroundTruth on the device, and the grit_det_gt that points into it.  Every array has one padding element, so that
    a split without annotations is no null pointer."""

    def __init__(self, packed, device='cuda'):
        import torch
        self.packed, self.device = packed, torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.GritHipError("Not implemented on the CPU: the GRIT kernels need HIP device tensors")
        pad = lambda a, shape=(1,): np.concatenate([a, np.zeros(shape, a.dtype)])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.img_off, self.box, self.area = up(packed.img_off), up(pad(packed.box, (1, 4))), up(pad(packed.area))
        self.cat, self.crowd, self.cat_valid = up(pad(packed.cat)), up(pad(packed.crowd)), up(pad(packed.cat_valid))
        self.img_ids = up(packed.img_ids)
        self.struct = _lib.DetGt()
        for name in ('img_off', 'box', 'area', 'cat', 'crowd', 'cat_valid'):
            setattr(self.struct, name, getattr(self, name).data_ptr())
        self.struct.n_img, self.struct.n_cat, self.struct.max_per_img = packed.n_img, packed.n_cat, packed.max_per_img

    def slots_of(self, image_ids):
        """image_ids [B] int64 on the device -> their slots [B] int32, -1 for an id the split does not have.  No synchronisation."""
        import torch
        ids = image_ids.to(torch.int64)
        at = torch.searchsorted(self.img_ids, ids).clamp_(max=self.packed.n_img - 1)
        return torch.where(self.img_ids[at] == ids, at, torch.full_like(at, -1)).to(torch.int32)

    def slots_for(self, image_ids):
        """slots_of for whatever a batch carries: a tensor of ids or a list of 0-d tensors (looked up on the device, no
        synchronisation), or a list of host integers (looked up on the host and uploaded)."""
        import torch
        if isinstance(image_ids, torch.Tensor):
            return self.slots_of(image_ids.to(self.device))
        if all(isinstance(i, torch.Tensor) for i in image_ids):
            return self.slots_of(torch.stack([i.reshape(()) for i in image_ids]).to(self.device))
        ids, wanted = self.packed.img_ids, np.asarray([int(i) for i in image_ids], np.int64)
        at = np.minimum(np.searchsorted(ids, wanted), len(ids) - 1)
        host = torch.from_numpy(np.where(ids[at] == wanted, at, -1).astype(np.int32))
        return host.pin_memory().to(self.device, non_blocking=True)


class EvalRecords(object):
    """The per-detection records of a split (include/grit_hip.h, grit_det_eval_img), on the device: flags [I * N, A] uint32 (as
    int32 storage), rank [I * N] int32 filled with -1, score [I * N] fp32, label [I * N] int32, seen [I] uint8."""

    def __init__(self, n_img, n_det, n_rng, device):
        import torch
        self.n_img, self.n_det, self.n_rng = n_img, n_det, n_rng
        self.flags = torch.zeros((n_img * n_det, n_rng), dtype=torch.int32, device=device)
        self.rank = torch.full((n_img * n_det,), -1, dtype=torch.int32, device=device)
        self.score = torch.zeros(n_img * n_det, dtype=torch.float32, device=device)
        self.label = torch.full((n_img * n_det,), -1, dtype=torch.int32, device=device)
        self.seen = torch.zeros(n_img, dtype=torch.uint8, device=device)

    def to_host(self):
        """(flags uint32, rank, score, label, seen) as numpy arrays: the one device-to-host copy of an evaluation."""
        return (self.flags.cpu().numpy().view(np.uint32), self.rank.cpu().numpy(), self.score.cpu().numpy(), self.label.cpu().numpy(),
                self.seen.cpu().numpy())


VocHostRecords = collections.namedtuple("VocHostRecords", "flag gt iou score label seen")


class VocRecords(object):
    """The per-detection records of a split under the Visual Genome protocol (include/grit_hip.h, grit_det_voc_img), on the device:
    flag [I * N] uint8 (0), gt [I * N] int32 (-1), iou [I * N] float64 (-inf), score [I * N] fp32 (0), label [I * N] int32 (-1),
    seen [I] uint8 (0); in brackets what a row holds until its image has been matched."""

    def __init__(self, n_img, n_det, device):
        import torch
        self.n_img, self.n_det = n_img, n_det
        self.flag = torch.zeros(n_img * n_det, dtype=torch.uint8, device=device)
        self.gt = torch.full((n_img * n_det,), -1, dtype=torch.int32, device=device)
        self.iou = torch.full((n_img * n_det,), float('-inf'), dtype=torch.float64, device=device)
        self.score = torch.zeros(n_img * n_det, dtype=torch.float32, device=device)
        self.label = torch.full((n_img * n_det,), -1, dtype=torch.int32, device=device)
        self.seen = torch.zeros(n_img, dtype=torch.uint8, device=device)

    def to_host(self):
        """VocHostRecords of numpy arrays: the one device-to-host copy of an evaluation."""
        return VocHostRecords(*(getattr(self, name).cpu().numpy() for name in VocHostRecords._fields))


def det_topk(logits, boxes, sizes):
    """logits [B, Q, K], boxes [B, Q, 4] cxcywh, sizes [B, 2] (height, width), fp32 on the device -> top_logit [B, N] fp32,
    top_index [B, N] int32 (q * K + k), corners [B, N, 4] fp32 absolute, N = min(TOPK, Q * K); an image's rows ordered by logit
    descending, then index ascending.  Two launches, no synchronisation."""
    import torch
    _lib.require_device(logits, boxes, sizes)
    if logits.dim() != 3 or tuple(boxes.shape) != tuple(logits.shape[:2]) + (4,) or tuple(sizes.shape) != (logits.shape[0], 2):
        raise _lib.GritHipError("det topk: logits [B, Q, K], boxes [B, Q, 4], sizes [B, 2], got %s, %s, %s"
                                % (tuple(logits.shape), tuple(boxes.shape), tuple(sizes.shape)))
    if logits.dtype != torch.float32 or boxes.dtype != torch.float32 or sizes.dtype != torch.float32:
        raise _lib.GritHipError("det topk: fp32 only, got %s / %s / %s" % (logits.dtype, boxes.dtype, sizes.dtype))
    B, Q, K = logits.shape
    if B == 0 or Q * K == 0:
        raise _lib.GritHipError("det topk: an empty batch or an empty score map has no best detections")
    logits, boxes, sizes = (x if x.is_contiguous() else x.contiguous() for x in (logits.detach(), boxes.detach(), sizes))
    N, dev = min(TOPK, Q * K), logits.device
    work = torch.empty(B * _lib.DET_TOPK_CHUNKS * TOPK, dtype=torch.int64, device=dev)
    top_logit = torch.empty((B, N), dtype=torch.float32, device=dev)
    top_index = torch.empty((B, N), dtype=torch.int32, device=dev)
    corners = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    p = _lib.ptr
    with _lib.device_guard(dev):
        st = _lib.load().grit_det_topk_f32(p(logits), p(boxes), p(sizes), B, Q, K, p(work), p(top_logit), p(top_index), p(corners),
                                           _lib.current_stream_ptr())
    _lib.check(st, "grit_det_topk_f32")
    return top_logit, top_index, corners


def eval_images(scores, labels, boxes, slots, gt, iou_thr, area_rng, records):
    """scores [B, N] fp32, labels [B, N] int64, boxes [B, N, 4] fp32 absolute corners (an image's rows in score order), slots [B]
    int32; gt: DeviceGroundTruth; iou_thr [T], area_rng [A, 2]: float64 device tensors of the host's numbers -> the images'
    rows of `records`.  One launch, no synchronisation."""
    import torch
    _lib.require_device(scores, labels, boxes, slots, iou_thr, area_rng)
    B, N = scores.shape
    if tuple(labels.shape) != (B, N) or tuple(boxes.shape) != (B, N, 4) or tuple(slots.shape) != (B,):
        raise _lib.GritHipError("det eval: scores / labels [B, N], boxes [B, N, 4], slots [B], got %s, %s, %s, %s"
                                % (tuple(scores.shape), tuple(labels.shape), tuple(boxes.shape), tuple(slots.shape)))
    if (scores.dtype, labels.dtype, boxes.dtype, slots.dtype) != (torch.float32, torch.int64, torch.float32, torch.int32):
        raise _lib.GritHipError("det eval: scores fp32, labels int64, boxes fp32, slots int32")
    if iou_thr.dtype != torch.float64 or area_rng.dtype != torch.float64 or area_rng.dim() != 2 or area_rng.shape[1] != 2:
        raise _lib.GritHipError("det eval: iou_thr [T] and area_rng [A, 2] must be float64")
    if N != records.n_det or area_rng.shape[0] != records.n_rng or records.n_img != gt.packed.n_img:
        raise _lib.GritHipError("det eval: %d detections per image and %d area ranges for records of %d and %d"
                                % (N, area_rng.shape[0], records.n_det, records.n_rng))
    scores, labels, boxes, slots, iou_thr, area_rng = (x if x.is_contiguous() else x.contiguous()
                                                       for x in (scores, labels, boxes, slots, iou_thr, area_rng))
    p = _lib.ptr
    with _lib.device_guard(scores.device):
        st = _lib.load().grit_det_eval_img(p(scores), p(labels), p(boxes), p(slots), B, N, ctypes.c_void_p(ctypes.addressof(gt.struct)),
                                           p(iou_thr), iou_thr.numel(), p(area_rng), area_rng.shape[0], p(records.flags),
                                           p(records.rank), p(records.score), p(records.label), p(records.seen),
                                           _lib.current_stream_ptr())
    _lib.check(st, "grit_det_eval_img")


def voc_images(scores, labels, boxes, slots, gt, iou_thr, records):
    """The matching of the Visual Genome protocol (grit_det_voc_img): scores [B, N] fp32, labels [B, N] int64, boxes [B, N, 4] fp32
    absolute corners (an image's rows in score order), slots [B] int32; gt: DeviceGroundTruth of the object split
    (pack_ground_truth) or of the attribute split (pack_ground_truth_attr); iou_thr: one host number (the protocol's 0.5) -> the
    images' rows of `records` (VocRecords).  One launch, no synchronisation."""
    import torch
    _lib.require_device(scores, labels, boxes, slots)
    if scores.dim() != 2:
        raise _lib.GritHipError("det voc: scores [B, N], got %s" % (tuple(scores.shape),))
    B, N = scores.shape
    if tuple(labels.shape) != (B, N) or tuple(boxes.shape) != (B, N, 4) or tuple(slots.shape) != (B,):
        raise _lib.GritHipError("det voc: scores / labels [B, N], boxes [B, N, 4], slots [B], got %s, %s, %s, %s"
                                % (tuple(scores.shape), tuple(labels.shape), tuple(boxes.shape), tuple(slots.shape)))
    if (scores.dtype, labels.dtype, boxes.dtype, slots.dtype) != (torch.float32, torch.int64, torch.float32, torch.int32):
        raise _lib.GritHipError("det voc: scores fp32, labels int64, boxes fp32, slots int32")
    if not isinstance(records, VocRecords) or N != records.n_det or records.n_img != gt.packed.n_img:
        raise _lib.GritHipError("det voc: %d detections per image over %d images for VocRecords of %s and %s"
                                % (N, gt.packed.n_img, getattr(records, 'n_det', None), getattr(records, 'n_img', None)))
    if records.flag.device != scores.device or gt.img_off.device != scores.device:
        raise _lib.GritHipError("det voc: detections, ground truth and records must be on one device")
    iou_thr = float(iou_thr)
    if iou_thr != iou_thr:
        raise _lib.GritHipError("det voc: the overlap threshold is NaN")
    if B == 0:
        return
    scores, labels, boxes, slots = (x if x.is_contiguous() else x.contiguous() for x in (scores, labels, boxes, slots))
    p = _lib.ptr
    with _lib.device_guard(scores.device):
        st = _lib.load().grit_det_voc_img(p(scores), p(labels), p(boxes), p(slots), B, N, ctypes.c_void_p(ctypes.addressof(gt.struct)),
                                          iou_thr, p(records.flag), p(records.gt), p(records.iou), p(records.score), p(records.label),
                                          p(records.seen), _lib.current_stream_ptr())
    _lib.check(st, "grit_det_voc_img")
