"""Host-side mask generators of CAE pre-training.

Reference: tasks/ssl/cae/util/masking_generator.py — MaskingGenerator :22-93 (BEiT's block-wise masking) and
RandomMaskingGenerator :96-118.  Both draw from the process-wide generators (``random`` for the blocks, ``np.random`` for
the shuffle) in the reference's order, so equal seeds give equal masks.  A mask is a numpy array, 1 = masked: int32
[height, width] from the block generator, float64 [height * width] from the random one, as the reference returns them.
"""
import math
import random

import numpy as np

__all__ = ['MaskingGenerator', 'RandomMaskingGenerator']


def _pair(size):
    return size if isinstance(size, tuple) else (size, size)


class MaskingGenerator:
    """Rectangles of random area and aspect ratio are laid over the grid until exactly ``num_masking_patches`` cells are
    masked; a rectangle counts only for the cells it newly covers, and is retried (ten times) when it covers none or
    more than are still missing."""

    def __init__(self, input_size, num_masking_patches, min_num_patches=4, max_num_patches=None, min_aspect=0.3,
                 max_aspect=None):
        self.height, self.width = _pair(input_size)
        self.num_patches = self.height * self.width
        self.num_masking_patches = num_masking_patches
        self.min_num_patches = min_num_patches
        self.max_num_patches = num_masking_patches if max_num_patches is None else max_num_patches
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))

    def __repr__(self):
        return 'Generator(%d, %d -> [%d ~ %d], max = %d, %.3f ~ %.3f)' % (
            self.height, self.width, self.min_num_patches, self.max_num_patches, self.num_masking_patches,
            self.log_aspect_ratio[0], self.log_aspect_ratio[1])

    def get_shape(self):
        return self.height, self.width

    def _mask(self, mask, max_mask_patches):
        """One rectangle (up to ten attempts); returns the number of newly masked cells."""
        for _ in range(10):
            # the order of the four draws is the reference's: area, aspect, then (only for a box that fits) top, left
            target_area = random.uniform(self.min_num_patches, max_mask_patches)
            aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if not (w < self.width and h < self.height):
                continue
            top = random.randint(0, self.height - h)
            left = random.randint(0, self.width - w)
            box = mask[top:top + h, left:left + w]
            fresh = h * w - int(box.sum())
            if 0 < fresh <= max_mask_patches:
                box[...] = 1
                return fresh
        return 0

    def __call__(self):
        mask = np.zeros(self.get_shape(), dtype=np.int32)
        count = 0
        while count != self.num_masking_patches:
            count += self._mask(mask, min(self.num_masking_patches - count, self.max_num_patches))
        return mask


class RandomMaskingGenerator:
    """``int(ratio * patches)`` ones among zeros, shuffled by ``np.random.shuffle``."""

    def __init__(self, input_size, ratio_masking_patches):
        self.height, self.width = _pair(input_size)
        self.num_patches = self.height * self.width
        self.num_masking_patches = int(ratio_masking_patches * self.num_patches)

    def __repr__(self):
        return 'Mask: total patches %d, mask patches %d' % (self.num_patches, self.num_masking_patches)

    def __call__(self):
        mask = np.hstack([np.zeros(self.num_patches - self.num_masking_patches), np.ones(self.num_masking_patches)])
        np.random.shuffle(mask)
        return mask
