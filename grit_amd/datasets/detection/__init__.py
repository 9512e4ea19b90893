"""Detection datasets: the transforms of detector pre-training and the collator that carries them out on the device."""
from .transforms import (CenterCrop, Compose, Normalize, Planned, RandomCrop, RandomHorizontalFlip, RandomRatioResize, RandomResize,
                         RandomSelect, RandomSizeCrop, ToTensor, collate_detection, crop, hflip, make_transforms, resize)
