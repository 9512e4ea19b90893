"""`get_transform(cfg)` of the captioning datasets (reference datasets/caption/transforms/__init__.py:6-32).

train / valid transforms = resize policy only: ToTensor and Normalize are applied on the device together with the
resampling and the batch padding (`collate_images`), so a transform returns a `Deferred` image, not a tensor.
RandAugment: `cfg.randaug = 'device'` makes the train transform draw the reference's four random operations per image
(transforms/randaug.py) and the device apply them between the resize and ToTensor, bit-identically to Pillow.  The
reference's `randaug: True` (PIL in the dataset worker) is not provided and raises.
`resize_name = 'normal'` is torchvision's Resize((h, w)) = PIL BILINEAR: a `FixedResize` whose records ask for bilinear taps, which
`collate_images` resamples through the plan path of the device pipeline (image_batch_geo); it has no augmented variant."""
from grit_amd.ops.image_batch import MEAN, STD, image_batch, image_batch_geo
from grit_amd.utils.misc import NestedTensor

from .randaug import RandAugment, augment_list
from .utils import Deferred, FixedResize, MaxWHResize, MinMaxResize

RESIZE = {'minmax': MinMaxResize, 'maxwh': MaxWHResize, 'normal': FixedResize}  # 'normal': torchvision Resize = PIL BILINEAR


class Sequence(object):
    """torchvision's Compose for the `Deferred` transforms: each one is called on the previous one's result."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def get_transform(cfg):
    randaug = getattr(cfg, 'randaug', False)
    if randaug and randaug != 'device':
        raise NotImplementedError("randaug=True is the reference's host-side PIL augmentation, which this build does not run; "
                                  "set transform_cfg.randaug = 'device' for the same operations on the GPU")
    if randaug == 'device' and cfg.resize_name == 'normal':
        raise NotImplementedError("randaug='device' follows a bicubic resize ('maxwh', 'minmax'); the bilinear 'normal' policy has no augmented path")
    resize = RESIZE[cfg.resize_name](cfg.size)
    if randaug == 'device':
        return {'train': Sequence([resize, RandAugment()]), 'valid': resize}
    return {'train': resize, 'valid': resize}


def collate_images(items, device=None, pad_to=None):
    """List of `Deferred` (what the transforms return) -> NestedTensor on the device; the device counterpart of
    Compose([resize, (RandAugment(),) ToTensor(), normalize()]) per image + nested_tensor_from_tensor_list(imgs).to(device)."""
    for it in items:
        if not isinstance(it, Deferred):
            raise TypeError("collate_images expects the Deferred images returned by get_transform()'s transforms")
    sizes = [it.size for it in items]
    plans = [it.augment for it in items]
    augment = None if all(p is None for p in plans) else [p or () for p in plans]
    filters = set(it.filter for it in items)
    if filters == {'bilinear'}:  # the bilinear taps run on the plan path: one resize per image
        if augment is not None:
            raise NotImplementedError("RandAugment after a bilinear resize is not provided: the augmented path resamples with bicubic taps")
        tensors, mask = image_batch_geo([it.pixels for it in items], [(('resize',) + tuple(s),) for s in sizes], MEAN, STD, device, pad_to)
    elif filters == {'bicubic'}:
        tensors, mask = image_batch([it.pixels for it in items], sizes, MEAN, STD, device, pad_to, augment=augment)
    else:
        raise ValueError("the images of a batch share one resampling filter, got %s" % sorted(filters))
    padded = len(set(sizes)) > 1 or (pad_to is not None and tuple(pad_to) != tuple(sizes[0]))
    return NestedTensor(tensors, mask, any_padding=padded)
