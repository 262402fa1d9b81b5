"""What the tools on int32 label stacks share (LabelMatcher, LabelExpander, IntensityMeasurer; the limits also CellExtractor and
ThresholdSegmenter): the limits of csrc/stage_host.hpp, the argument checks of a label plane and of a stack's shape, and the
ownership of the preprocess handle."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib as L
from .preprocess import Preprocessor

MAX_SIDE = 4096
MAX_BATCH = 65535
MAX_LABEL = 1 << 20                     # per image


def _is_tensor(a) -> bool:
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def check_label_plane(name, a, device_id, noun):
    """a: int32 [B,H,W], a C-contiguous numpy array or a contiguous CUDA tensor of device_id; noun: the tool in the message."""
    if _is_tensor(a):
        import torch
        if a.dtype != torch.int32:
            raise TypeError(f"{name} tensor dtype {a.dtype}: int32 expected")
        if not a.is_cuda:
            raise ValueError(f"{name} is a CPU tensor; pass numpy arrays or CUDA tensors")
        if a.device.index != device_id:
            raise ValueError(f"{name} is on {a.device}, {noun} on cuda:{device_id}")
        if not a.is_contiguous():
            raise ValueError(f"{name} is not contiguous")
    elif isinstance(a, np.ndarray):
        if a.dtype != np.int32:
            raise TypeError(f"{name} dtype {a.dtype}: int32 expected")
        if not a.flags.c_contiguous:
            raise ValueError(f"{name} must be C-contiguous")
    else:
        raise TypeError(f"unsupported input type {type(a)} for {name}")
    if a.ndim != 3:
        raise ValueError(f"{name} must be [B,H,W], got shape {tuple(a.shape)}")


def check_stack_shape(B, H, W, shape, channels=1):
    """The limits of a stack of B images of H x W; shape: what the message shows of an empty one."""
    if B < 1 or H < 1 or W < 1 or channels < 1:
        raise ValueError(f"empty batch or image: shape {tuple(shape)}")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"image sides above {MAX_SIDE} are not supported, got {H}x{W}")
    if B > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} images per call, got {B}")


class LabelTool:
    """A tool on one preprocess handle (one GPU, one stream): its own, made by the first call after that call's argument checks,
    or that of `extractor` (a CellExtractor or a ThresholdSegmenter), so that what the owner left on the device is read in stream
    order.  _noun: the tool in the messages."""
    _noun = "the tool"

    def __init__(self, device_id: int = 0, extractor=None):
        if extractor is not None and extractor.device_id != device_id:
            raise ValueError(f"extractor is on device {extractor.device_id}, {self._noun} on {device_id}")
        self._lib = L.load_library()
        self.device_id = device_id
        self._ext = extractor
        self._pre: Optional[Preprocessor] = None

    @property
    def _handle(self):
        if self._ext is not None:
            return self._ext._handle
        if self._pre is None:
            self._pre = Preprocessor(self.device_id)
        return self._pre._h

    def close(self):
        """Frees the tool's own handle (a shared one stays its owner's); a later call makes a new one."""
        if self._pre is not None:
            self._pre.close()
            self._pre = None
