"""`get_transform(cfg)` of the captioning datasets (reference datasets/caption/transforms/__init__.py:6-32).

train / valid transforms = resize policy only: ToTensor and Normalize are applied on the device together with the
resampling and the batch padding (`collate_images`), so a transform returns a `Deferred` image, not a tensor.
RandAugment: `cfg.randaug = 'device'` makes the train transform draw the reference's four random operations per image
(transforms/randaug.py) and the device apply them between the resize and ToTensor, bit-identically to Pillow.  The
reference's `randaug: True` (PIL in the dataset worker) is not provided and raises."""
from grit_amd.ops.image_batch import MEAN, STD, image_batch
from grit_amd.utils.misc import NestedTensor

from .randaug import RandAugment, augment_list
from .utils import Deferred, FixedResize, MaxWHResize, MinMaxResize

RESIZE = {'minmax': MinMaxResize, 'maxwh': MaxWHResize}


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
    if cfg.resize_name == 'normal':
        # the reference's 'normal' policy is torchvision Resize = PIL BILINEAR; the device resampler implements Pillow's
        # BICUBIC taps only, and silently resampling with another filter would change the input pixels
        raise NotImplementedError("resize_name='normal' (bilinear torchvision Resize) is not provided; use 'maxwh' or 'minmax'")
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
    tensors, mask = image_batch([it.pixels for it in items], sizes, MEAN, STD, device, pad_to, augment=augment)
    padded = len(set(sizes)) > 1 or (pad_to is not None and tuple(pad_to) != tuple(sizes[0]))
    return NestedTensor(tensors, mask, any_padding=padded)
