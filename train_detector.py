"""Detector pre-training, the first stage of the published recipe (the reference's train_detector.py).

    python train_detector.py --synthetic [--augment] [--attr] --steps 3 [--batch-size 2] [--size 224] [--bf16] [--eval [--eval-protocol vg]] [key=value ...]

The Visual Genome / LMDB readers and the hook-based solver are out of scope of this build, so the only data source here is
`--synthetic`: seeded random images and targets.  It runs the real model, the device matcher and criterion
(grit_amd/models/detection/od_losses.py) and engine.det_engine.train_step, and prints the loss dictionary of every step.
`--augment` feeds the input pipeline of the recipe instead of noise tensors: seeded uint8 images of mixed sizes with pixel boxes go
through datasets.detection.make_transforms('train', 'train') -- flip, random resize, ratio resize + crop + resize -- and
collate_detection, which resamples the batch on the device (`--size` does not apply: the recipe decides the sizes).
`--bf16` trains on the path the captioner uses (grit_amd.amp.Bf16Compute: bf16 compute copies, fp32 masters, flat AdamW and gradient
clipping on the device, the reference's four parameter groups and MultiStepLR; engine.det_engine.build_optimizers_schedulers).
`--attr` trains the attribute head as well (model.has_attr_head, models/detection/heads.py): every other image carries seeded
multi-hot attributes, attr_loss_coef is 1, the head has its own AdamW (optimizer.sp_names=['attr_head']) and `loss_attr` is printed
with the other losses.
`--eval` evaluates after the steps (engine.det_engine.evaluate: PostProcess and the COCO-style box evaluation on the device,
datasets.detection.metrics.CocoEvaluator) on `--eval-batches` seeded synthetic batches and prints the losses and the box mAP table.
`--eval-protocol vg` (default `coco`) also runs the Visual Genome protocol in the same loop (datasets.detection.metrics.VGEvaluator:
PASCAL-VOC AP at IoU 0.5 per class) and prints the mean and the weighted mean AP over the object classes and, with `--attr`, over the
attribute classes (PostProcessAttr's detections; the split's targets then carry attributes on every other image).
Configuration: grit_amd.config.detection_config (the keys of configs/detection/train_config.yaml), dotted key=value overrides.
"""
import argparse
import random

import torch

from grit_amd.config import detection_config
from engine.det_engine import build_optimizers_schedulers, evaluate, train_step
from models.detection.detector import build_detector
from utils.misc import NestedTensor


def synthetic_batch(generator, batch_size, size, num_classes, max_targets, device):
    """Images ~ N(0, 1) and, per image, 1..max_targets boxes (cxcywh inside the unit square) with uniform labels."""
    images = torch.randn(batch_size, 3, size, size, generator=generator)
    mask = torch.zeros(batch_size, size, size, dtype=torch.bool)
    targets = []
    for _ in range(batch_size):
        n = int(torch.randint(1, max_targets + 1, (1,), generator=generator))
        wh = 0.05 + 0.4 * torch.rand(n, 2, generator=generator)
        centre = wh / 2 + (1 - wh) * torch.rand(n, 2, generator=generator)
        targets.append({'labels': torch.randint(0, num_classes, (n,), generator=generator).to(device),
                        'boxes': torch.cat([centre, wh], 1).to(device)})
    return NestedTensor(images.to(device), mask.to(device), any_padding=False), targets


def add_synthetic_attributes(generator, targets, num_attr, device):
    """--attr: every other image of the batch gets has_attr=True and a multi-hot 'attributes' [T, num_attr] uint8 with about 2 % ones
    (Visual Genome annotates a few attributes per object); the others has_attr=False and no attributes."""
    for i, t in enumerate(targets):
        t['has_attr'] = i % 2 == 0
        if t['has_attr']:
            n = int(t['labels'].shape[0])
            t['attributes'] = (torch.rand(n, num_attr, generator=generator) < 0.02).to(torch.uint8).to(device)
    return targets


def synthetic_split(generator, batches, batch_size, size, num_classes, max_targets, device, num_attr=0):
    """`batches` synthetic batches as an evaluation split: every target also carries 'image_id' and 'orig_size' (device tensors),
    and the annotations -- the same boxes in pixels, (x, y, w, h), area w * h, ids from 1 -- come back as a COCO dataset dictionary.
    With num_attr > 0 the targets carry attributes as the training batches do (add_synthetic_attributes: every other image), the
    images of the dictionary 'has_attr' and the annotations 'attributes', the list of an object's attribute ids."""
    split, images, annotations = [], [], []
    for _ in range(batches):
        samples, targets = synthetic_batch(generator, batch_size, size, num_classes, max_targets, device)
        if num_attr > 0:
            add_synthetic_attributes(generator, targets, num_attr, device)
        for t in targets:
            image_id = len(images) + 1
            images.append({'id': image_id, 'height': size, 'width': size})
            t['image_id'] = torch.tensor(image_id, device=device)
            t['orig_size'] = torch.tensor([size, size], device=device)
            first = len(annotations)
            for label, (cx, cy, w, h) in zip(t['labels'].tolist(), (t['boxes'].double() * size).tolist()):
                annotations.append({'id': len(annotations) + 1, 'image_id': image_id, 'category_id': label,
                                    'bbox': [cx - 0.5 * w, cy - 0.5 * h, w, h], 'area': w * h, 'iscrowd': 0})
            if num_attr > 0:
                images[-1]['has_attr'] = bool(t['has_attr'])
                if t['has_attr']:
                    for ann, row in zip(annotations[first:], t['attributes'].tolist()):
                        ann['attributes'] = [a for a, on in enumerate(row) if on]
        split.append((samples, targets))
    return split, {'images': images, 'categories': [{'id': c} for c in range(num_classes)], 'annotations': annotations}


SOURCE_SIZES = ((500, 375), (375, 500), (500, 333), (640, 480), (480, 640), (400, 300))  # (w, h) of the synthetic "photos"


def augmented_batch(generator, batch_size, num_classes, max_targets, device, transform):
    """Per image: uint8 noise of one of SOURCE_SIZES and 1..max_targets boxes in pixels (xyxy) -> `transform` (which draws from the
    global `random` and torch generators and finishes the targets on the host) -> collate_detection.  An image whose crop removed
    every box is drawn again; no pixel has been touched by then."""
    from grit_amd.datasets.detection import collate_detection
    items = []
    while len(items) < batch_size:
        w, h = SOURCE_SIZES[int(torch.randint(0, len(SOURCE_SIZES), (1,), generator=generator))]
        image = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=generator)
        n = int(torch.randint(1, max_targets + 1, (1,), generator=generator))
        extent = torch.tensor([w, h], dtype=torch.float32)
        wh = (0.05 + 0.4 * torch.rand(n, 2, generator=generator)) * extent
        corner = (extent - wh) * torch.rand(n, 2, generator=generator)
        target = {'boxes': torch.cat([corner, corner + wh], 1), 'labels': torch.randint(0, num_classes, (n,), generator=generator),
                  'area': wh.prod(1), 'iscrowd': torch.zeros(n, dtype=torch.int64), 'size': torch.tensor([h, w]),
                  'orig_size': torch.tensor([h, w])}
        record, target = transform(image.numpy(), target)
        if len(target['labels']):
            items.append((record, target))
    return collate_detection(items, device=device)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--synthetic', action='store_true', help='seeded random images and targets (the only data source of this build)')
    ap.add_argument('--augment', action='store_true', help="with --synthetic: uint8 images through the recipe's transforms and the device collator")
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--batch-size', type=int, default=None)
    ap.add_argument('--size', type=int, default=224, help='image side')
    ap.add_argument('--max-targets', type=int, default=30)
    ap.add_argument('--bf16', action='store_true', help='bf16 compute + fp32 masters: flat AdamW and device gradient clipping')
    ap.add_argument('--attr', action='store_true',
                    help='with the attribute head (model.has_attr_head): synthetic attributes on every other image, attr_loss_coef 1, '
                         "and the reference's second optimizer for the head (optimizer.sp_names=['attr_head'])")
    ap.add_argument('--steps-per-epoch', type=int, default=0,
                    help='with --bf16: step the lr schedulers once per this many steps (0: never within a run)')
    ap.add_argument('--eval', action='store_true', help='after the steps: losses and COCO-style box mAP on seeded synthetic batches')
    ap.add_argument('--eval-batches', type=int, default=2)
    ap.add_argument('--eval-protocol', choices=('coco', 'vg'), default='coco',
                    help="with --eval: 'vg' adds the Visual Genome protocol (VOC AP at IoU 0.5: mean and weighted mean over the object "
                         'classes and, with --attr, over the attribute classes; the split then carries attributes on every other image)')
    ap.add_argument('overrides', nargs='*', help='dotted key=value configuration overrides')
    args = ap.parse_args()
    if not args.synthetic:
        ap.error("only --synthetic is available: the Visual Genome readers are not part of this build")
    over = {'model.backbone.pre_trained': 'none'}
    if args.attr:
        over.update({'model.has_attr_head': True, 'model.det_module.loss.attr_loss_coef': 1.0, 'optimizer.sp_names': ['attr_head']})
    for item in args.overrides:
        key, _, value = item.partition('=')
        try:
            value = int(value)
        except ValueError:
            try:
                value = float(value)
            except ValueError:
                value = {'true': True, 'false': False}.get(value.lower(), value)
        over[key] = value
    config = detection_config(**over)
    torch.manual_seed(config.exp.seed)
    device = torch.device('cuda')
    model, criterion, postprocessors = build_detector(config)
    model.to(device)
    schedulers = []
    if args.bf16:
        from grit_amd.amp import Bf16Compute
        model = Bf16Compute(model)
        optimizer, schedulers = build_optimizers_schedulers(model, config)
    elif args.attr:  # the recipe's grouping: the head's own AdamW at sp_lr beside the main one
        optimizer, schedulers = build_optimizers_schedulers(model, config)
    else:
        optimizer = _plain_optimizer(model, config)
    g = torch.Generator().manual_seed(config.exp.seed)
    batch_size = args.batch_size or config.optimizer.batch_size
    if args.augment:
        from grit_amd.datasets.detection import make_transforms
        random.seed(config.exp.seed)
        transform = make_transforms('train', 'train')
    for step in range(args.steps):
        if args.augment:
            samples, targets = augmented_batch(g, batch_size, config.model.det_module.num_classes, args.max_targets, device, transform)
        else:
            samples, targets = synthetic_batch(g, batch_size, args.size, config.model.det_module.num_classes, args.max_targets, device)
        if args.attr:
            add_synthetic_attributes(g, targets, config.model.num_attr_classes, device)
        total, losses = train_step(model, criterion, optimizer, samples, targets, config.optimizer.clip_max_norm)
        print('step %d  loss %.5f  %s' % (step, float(total), {k: round(float(v), 5) for k, v in sorted(losses.items())}))
        if args.steps_per_epoch > 0 and (step + 1) % args.steps_per_epoch == 0:
            for sch in schedulers:
                sch.step()
    if args.eval:
        from datasets.detection.metrics import AnnotationIndex, CocoEvaluator
        vg = args.eval_protocol == 'vg'
        num_attr = config.model.num_attr_classes if vg and args.attr else 0
        split, dataset = synthetic_split(g, args.eval_batches, batch_size, args.size, config.model.det_module.num_classes, args.max_targets,
                                         device, num_attr=num_attr)
        index = AnnotationIndex(dataset)
        vg_evaluator = None
        if vg:
            from datasets.detection.metrics import VGEvaluator
            vg_evaluator = VGEvaluator(index, ('obj', 'attr') if args.attr else ('obj',), num_attr=num_attr, device=device)
        result = evaluate(model, criterion, postprocessors, split, CocoEvaluator(index, ('bbox',), device=device), vg_evaluator=vg_evaluator)
        text = result.pop('result_text') + result.pop('vg_text', '')
        print('eval  %s' % {k: round(v, 5) for k, v in sorted(result.items())})
        print(text, end='')


def _plain_optimizer(model, config):
    backbone = [p for n, p in model.named_parameters() if n.startswith('backbone.') and p.requires_grad]
    rest = [p for n, p in model.named_parameters() if not n.startswith('backbone.') and p.requires_grad]
    return torch.optim.AdamW([{'params': rest, 'lr': config.optimizer.lr}, {'params': backbone, 'lr': config.optimizer.lr_backbone}],
                             weight_decay=config.optimizer.weight_decay)


if __name__ == '__main__':
    main()
