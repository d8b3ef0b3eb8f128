"""``src/utils/utils.py``'s post-processing on the device."""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K
from .metric import to_device


def keep_largest_connected_components(mask):
    """``utils.py:43-65``: for each ``struc_id`` in ``1..mask.shape[1]`` (sic: the second axis' size, not the class
    count) keep only the largest face-connected component of ``mask == struc_id``; labels absent from the mask are
    skipped and every other voxel becomes 0.  Among components of equal size the one whose first voxel comes first in
    raster order wins (the reference's ``np.argmax`` over ``regionprops``).  uint8 result: a device tensor for a
    device tensor, numpy for numpy.  One divergence: label values >= 256 that the loop would visit raise ValueError
    where the reference wraps them in its uint8 output silently."""
    if torch.is_tensor(mask):
        return K.largest_components(to_device(mask))
    a = np.asarray(mask)
    if a.ndim >= 2 and a.shape[1] >= 256 and np.issubdtype(a.dtype, np.integer):
        if np.any((a >= 256) & (a <= a.shape[1])):
            raise ValueError("keep_largest_connected_components: label values 256..%d do not fit the uint8 output"
                             % a.shape[1])
    return K.largest_components(to_device(a)).cpu().numpy()
