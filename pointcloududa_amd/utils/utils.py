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


def resize_volume(img_volume, w=256, h=256):
    """``utils.py:83-92``: ``cv2.resize(im, dsize=(w, h), interpolation=cv2.INTER_AREA)`` of every fp32 plane of ``img_volume
    [N,H,W]`` -> ``[N,h,w]`` on the device (``K.area_resize``): a device tensor for a device tensor, numpy for numpy.  The rule
    is the build's own, written after OpenCV's ``resize.cpp``; its parity with OpenCV is not pinned.  Other
    dtypes and multi-channel images are not built."""
    if torch.is_tensor(img_volume):
        return K.area_resize(img_volume, int(h), int(w))
    a = np.asarray(img_volume)
    if a.dtype != np.float32 or a.ndim != 3:
        raise TypeError("resize_volume: float32 planes [N,H,W], got %s with %d dimensions" % (a.dtype, a.ndim))
    if not torch.cuda.is_available():
        raise RuntimeError("resize_volume: pointcloududa_amd kernels run on a HIP device; none is available (no CPU fallback)")
    return K.area_resize(torch.from_numpy(np.ascontiguousarray(a)).cuda(), int(h), int(w)).cpu().numpy()
