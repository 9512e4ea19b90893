"""RandAugment of the captioning datasets (reference datasets/caption/transforms/randaug.py:74-104), planned on the host,
applied on the device.

The reference picks four of eleven PIL operations per training image and applies them in the dataset worker.  Here the
transform only *draws*: from Python's global `random`, in the reference's order -- `random.choices(augment_list(), k=n)`,
then per operation `random.random() * (max - min) + min` and, for the five geometric operations, one more
`random.random()` whose value `> 0.5` negates the magnitude -- so that after `random.seed(s)` the plan equals what the
reference's class does to the image.  The plan rides on the `Deferred` image; the pixels are touched by
grit_image_batch_aug_fwd (grit_amd/ops/image_batch.py) after the resize, bit-identically to Pillow."""
import random

from .utils import Deferred

GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXabs', 'TranslateYabs')


def augment_list():
    """(operation, smallest, largest magnitude) in the reference's order (randaug.py:74-88)."""
    return [
        ('Identity', 0, 100),
        ('AutoContrast', 0, 100),
        ('Rotate', 0, 8),
        ('Color', 0.5, 1.5),
        ('Contrast', 0.5, 1.5),
        ('Brightness', 0.5, 1.5),
        ('Sharpness', 0.5, 1.5),
        ('ShearX', 0.0, 0.12),
        ('ShearY', 0.0, 0.12),
        ('TranslateXabs', 0.0, 80),
        ('TranslateYabs', 0.0, 80),
    ]


class RandAugment(object):
    """`RandAugment()(deferred)` -> a `Deferred` carrying the plan ((name, magnitude, negate), ...); touches no pixels."""

    def __init__(self, n_augments=4):
        self.n_augments = n_augments
        self.augment_list = augment_list()

    def draw(self):
        plan = []
        for name, minval, maxval in random.choices(self.augment_list, k=self.n_augments):
            val = random.random() * (maxval - minval) + minval
            negate = random.random() > 0.5 if name in GEOMETRIC else False
            plan.append((name, val, negate))
        return tuple(plan)

    def __call__(self, x):
        if not isinstance(x, Deferred):
            raise TypeError("RandAugment follows the resize policy: it expects the Deferred image a policy returns")
        if x.augment is not None:
            raise ValueError("image already carries an augmentation plan")
        return Deferred(x.pixels, x.size, self.draw(), x.filter)
