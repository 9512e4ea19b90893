"""Transforms of the detection datasets for image + boxes (reference datasets/detection/transforms.py:107-466).

The reference applies every transform to a PIL image inside the dataset worker.  Here a transform only DRAWS: it appends a
step -- ('hflip',), ('resize', oh, ow) or ('crop', top, left, h, w) -- to the plan of a `Planned` record, keeps track of the
current (w, h) and transforms the target on the host, right then, with the reference's torch float32 expressions.  The pixels
are resampled for the whole batch on the device (grit_amd/ops/image_batch.py: image_batch_geo, Pillow's BILINEAR, which is what
torchvision's `resize` does to a PIL image), bit-identically to the PIL chain.  Targets are final when the plan is, so a
dataset can redraw an item that lost all its boxes without touching a pixel.

The draws consume Python's global `random` in the reference's order; the crop origin comes from torch's global CPU generator
as in torchvision's RandomCrop.get_params (`crop_params`).  `pad`, RandomPad, PadOrCrop, RandomErasing and masks are not used
by `make_transforms` and are not provided: they raise."""
import random

import numpy as np
import torch

from grit_amd.ops.image_batch import MEAN, STD, image_batch_geo
from grit_amd.utils.box_ops import box_xyxy_to_cxcywh
from grit_amd.utils.misc import NestedTensor


class Planned(object):
    """A decoded RGB image ([h, w, 3] uint8) with the plan of what the device is to do with it.  `size`, `width` and `height`
    are those of the image as it stands after the plan, named as on a PIL image.  Plain data: picklable for dataset workers."""
    __slots__ = ('pixels', 'plan', 'size', 'to_tensor', 'normalize')

    def __init__(self, pixels, plan=(), size=None, to_tensor=False, normalize=None):
        self.pixels, self.plan, self.to_tensor, self.normalize = pixels, tuple(plan), to_tensor, normalize
        self.size = (int(pixels.shape[1]), int(pixels.shape[0])) if size is None else (int(size[0]), int(size[1]))

    width = property(lambda self: self.size[0])
    height = property(lambda self: self.size[1])

    def then(self, step, size):
        return Planned(self.pixels, self.plan + (step,), size, self.to_tensor, self.normalize)

    def __getstate__(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __setstate__(self, state):
        for k, v in zip(self.__slots__, state):
            setattr(self, k, v)


def planned(image):
    if isinstance(image, Planned):
        return image
    if not hasattr(image, 'shape'):
        image = np.asarray(image)  # PIL image -> [h, w, 3] uint8 view of the decoded pixels
    if len(image.shape) != 3 or image.shape[2] != 3:
        raise ValueError("expected a decoded RGB image as [h, w, 3] uint8, got shape %s" % (tuple(image.shape),))
    return Planned(image)


def _no_masks(target):
    if target is not None and 'masks' in target:
        raise NotImplementedError("targets with 'masks' are not provided: the device pipeline resamples the image only")


def crop(image, target, region):
    image = planned(image)
    _no_masks(target)
    i, j, h, w = (int(v) for v in region)
    image = image.then(('crop', i, j, h, w), (w, h))
    target = target.copy()
    target["size"] = torch.tensor([h, w])
    fields = ["labels", "area", "iscrowd", "attributes"]
    if "boxes" in target:
        boxes = target["boxes"]
        max_size = torch.as_tensor([w, h], dtype=torch.float32)
        cropped_boxes = boxes - torch.as_tensor([j, i, j, i])
        cropped_boxes = torch.min(cropped_boxes.reshape(-1, 2, 2), max_size)
        cropped_boxes = cropped_boxes.clamp(min=0)
        area = (cropped_boxes[:, 1, :] - cropped_boxes[:, 0, :]).prod(dim=1)
        target["boxes"] = cropped_boxes.reshape(-1, 4)
        target["area"] = area
        fields.append("boxes")
        # elements whose box has no area left are removed
        corners = target['boxes'].reshape(-1, 2, 2)
        keep = torch.all(corners[:, 1, :] > corners[:, 0, :], dim=1)
        for field in fields:
            if field in target:
                target[field] = target[field][keep]
    return image, target


def hflip(image, target):
    image = planned(image)
    _no_masks(target)
    w, h = image.size
    image = image.then(('hflip',), (w, h))
    target = target.copy()
    if "boxes" in target:
        boxes = target["boxes"]
        target["boxes"] = boxes[:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
    return image, target


def get_size_with_aspect_ratio(image_size, size, max_size=None):
    w, h = image_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        return (int(size * h / w), size)
    return (size, int(size * w / h))


def resize(image, target, size, max_size=None):
    """size: the short side (scalar), or a (w, h) pair."""
    image = planned(image)
    _no_masks(target)
    if isinstance(size, (list, tuple)):
        oh, ow = size[::-1]
    else:
        oh, ow = get_size_with_aspect_ratio(image.size, size, max_size)
    rescaled = image.then(('resize', int(oh), int(ow)), (ow, oh))
    if target is None:
        return rescaled, None
    ratio_width, ratio_height = (float(s) / float(s_orig) for s, s_orig in zip(rescaled.size, image.size))
    target = target.copy()
    if "boxes" in target:
        target["boxes"] = target["boxes"] * torch.as_tensor([ratio_width, ratio_height, ratio_width, ratio_height])
    if "area" in target:
        target["area"] = target["area"] * (ratio_width * ratio_height)
    target["size"] = torch.tensor([oh, ow])
    return rescaled, target


def crop_params(image, output_size):
    """torchvision.transforms.RandomCrop.get_params (0.8 and later) restated, torchvision not being a dependency: no draw and
    (0, 0) when the crop equals the image, else the top then the left edge from torch's global CPU generator."""
    w, h = image.size
    th, tw = output_size
    if h + 1 < th or w + 1 < tw:
        raise ValueError("Required crop size %s is larger then input image size %s" % ((th, tw), (h, w)))
    if w == tw and h == th:
        return 0, 0, h, w
    i = torch.randint(0, h - th + 1, size=(1,)).item()
    j = torch.randint(0, w - tw + 1, size=(1,)).item()
    return i, j, th, tw


def pad(image, target, padding):
    raise NotImplementedError("pad is not provided: make_transforms does not use it and the device pipeline only pads the batch")


class RandomCrop(object):

    def __init__(self, size):
        self.size = size

    def __call__(self, img, target):
        img = planned(img)
        return crop(img, target, crop_params(img, self.size))


class RandomSizeCrop(object):

    def __init__(self, min_size: int, max_size: int):
        self.min_size = min_size
        self.max_size = max_size

    def __call__(self, img, target):
        img = planned(img)
        w = random.randint(min(self.min_size, img.width), min(img.width, self.max_size))
        h = random.randint(min(self.min_size, img.height), min(img.height, self.max_size))
        return crop(img, target, crop_params(img, [h, w]))


class CenterCrop(object):

    def __init__(self, size):
        self.size = size

    def __call__(self, img, target):
        img = planned(img)
        image_width, image_height = img.size
        crop_height, crop_width = self.size
        crop_top = int(round((image_height - crop_height) / 2.))
        crop_left = int(round((image_width - crop_width) / 2.))
        return crop(img, target, (crop_top, crop_left, crop_height, crop_width))


class RandomHorizontalFlip(object):

    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, img, target):
        if random.random() < self.p:
            return hflip(img, target)
        return planned(img), target


class RandomResize(object):

    def __init__(self, sizes, max_size=None):
        assert isinstance(sizes, (list, tuple))
        self.sizes = sizes
        self.max_size = max_size

    def __call__(self, img, target=None):
        size = random.choice(self.sizes)
        return resize(img, target, size, self.max_size)


class RandomRatioResize(object):

    def __init__(self, ratio_range, max_size=None):
        assert isinstance(ratio_range, (list, tuple))
        self.ratio_range = ratio_range
        self.max_size = max_size

    def __call__(self, img, target=None):
        img = planned(img)
        ratio = random.uniform(*self.ratio_range)
        w = int(img.width * ratio)
        h = int(img.height * ratio)
        return resize(img, target, (w, h), self.max_size)


class RandomSelect(object):
    """transforms1 with probability p, else transforms2."""

    def __init__(self, transforms1, transforms2, p=0.5):
        self.transforms1 = transforms1
        self.transforms2 = transforms2
        self.p = p

    def __call__(self, img, target):
        if random.random() < self.p:
            return self.transforms1(img, target)
        return self.transforms2(img, target)


class ToTensor(object):
    """Marks the record: /255 is part of the device's lookup table."""

    def __call__(self, img, target):
        img = planned(img)
        return Planned(img.pixels, img.plan, img.size, True, img.normalize), target


class Normalize(object):
    """Marks the record with (mean, std) for the device's lookup table; boxes xyxy -> cxcywh relative to the image size."""

    def __init__(self, mean, std):
        self.mean = mean
        self.std = std

    def __call__(self, image, target=None):
        image = planned(image)
        if not image.to_tensor:
            raise TypeError("Normalize follows ToTensor")
        image = Planned(image.pixels, image.plan, image.size, True, (tuple(self.mean), tuple(self.std)))
        if target is None:
            return image, None
        target = target.copy()
        w, h = image.size
        if "boxes" in target:
            boxes = box_xyxy_to_cxcywh(target["boxes"])
            target["boxes"] = boxes / torch.tensor([w, h, w, h], dtype=torch.float32)
        return image, target


class _NotProvided(object):

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("%s is not provided: make_transforms does not use it and the device pipeline has no kernel for it"
                                  % type(self).__name__)


class PadOrCrop(_NotProvided):
    pass


class RandomPad(_NotProvided):
    pass


class RandomErasing(_NotProvided):
    pass


class Compose(object):

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target

    def __repr__(self):
        return "%s(%s\n)" % (type(self).__name__, "".join("\n    %s" % (t,) for t in self.transforms))


TRAIN_SCALES = list(range(480, 801, 16))


def make_transforms(split, phase='train'):
    normalize = Compose([ToTensor(), Normalize(list(MEAN), list(STD))])
    recipes = {
        ('train', 'train'): lambda: [RandomHorizontalFlip(),
                                     RandomSelect(RandomResize(TRAIN_SCALES, max_size=1333),
                                                  Compose([RandomRatioResize((0.5, 1.5)), RandomSizeCrop(384, 800),
                                                           RandomResize(TRAIN_SCALES, max_size=1333)]))],
        ('train', 'valid'): lambda: [RandomResize([800], max_size=1333)],
        ('pretrain-od', 'train'): lambda: [RandomHorizontalFlip(), RandomResize([384, 400, 416, 432, 448], max_size=800)],
        ('pretrain-od', 'valid'): lambda: [RandomResize([800], max_size=1333)],
        ('pretrain-vl', 'train'): lambda: [RandomResize(list(range(480, 641, 16)), max_size=900)],
        ('pretrain-vl', 'valid'): lambda: [RandomResize([640], max_size=900)],
    }
    key = ('train' if phase == 'finetune' else phase, split)
    if key not in recipes:
        raise ValueError(f'unknown {split}')
    return Compose(recipes[key]() + [normalize])


def collate_detection(batch, device=None, pad_to=None):
    """List of (Planned record, target) as make_transforms' transforms return them -> (NestedTensor, targets) on the device,
    what engine.det_engine.train_step takes: the device counterpart of the PIL chain + ToTensor + Normalize per image and
    nested_tensor_from_tensor_list(images).to(device), with every tensor of the targets moved to the device."""
    records = [item[0] for item in batch]
    for r in records:
        if not isinstance(r, Planned) or not r.to_tensor or r.normalize is None:
            raise TypeError("collate_detection expects the records of a transform that ends in ToTensor and Normalize")
    stats = set(r.normalize for r in records)
    if len(stats) != 1:
        raise ValueError("the images of a batch share one Normalize")
    mean, std = stats.pop()
    tensors, mask = image_batch_geo([r.pixels for r in records], [r.plan for r in records], mean, std, device, pad_to)
    sizes = set(r.size for r in records)
    padded = len(sizes) > 1 or (pad_to is not None and (int(pad_to[1]), int(pad_to[0])) != records[0].size)
    targets = [{k: v.to(tensors.device, non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in item[1].items()}
               for item in batch]
    return NestedTensor(tensors, mask, any_padding=padded), targets
