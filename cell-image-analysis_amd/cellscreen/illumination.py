"""Flat-field correction from a plate's own images on the device (cs_illum_tile_stats, cs_illum_reduce and cs_illum_apply,
include/cellscreen.h): one multiplicative illumination function per channel, estimated from all fields of a plate,
since cells lie elsewhere in every field, and divided out of every field -- CellProfiler's CorrectIlluminationCalculate and
CorrectIlluminationApply.

    ic = IlluminationCorrector(extractor=seg)                    # or IlluminationCorrector(device_id=0)
    for batch in plate:                                          # [B,H,W] or [B,H,W,C] uint8 / uint16, C <= 4
        ic.add_batch(batch, tile=64)
    fn = ic.finish(offset=100)                                   # an IlluminationFunction; fn.save("plate.npz")
    flat = ic.apply_batch(batch, fn)                             # same dtype, layout and memory kind; pass it on to the tools

All integers, no tolerance, bit-identical run to run; tests/illumination_reference.py restates the rule.  The mesh is
threshold="noise"'s: tile side T a power of two in 16..256, max(1, n // T) tiles per axis, the last one takes the remainder.

  1. per image, channel and tile the value of rank (q_num (N - 1)) // q_den among the tile's N sorted pixels;
  2. per channel and node the value of rank (a_num (n - 1)) // a_den across the n images (or the rounded mean), then
     F8 = 256 max(value - offset_c, floor), then the optional 3 x 3 mesh median and Gaussian (both off by default: they flatten a
     curved function at the mesh's edges);
  3. G8_c: the rounded mean, the lower median, the max or the min of F8_c, or the caller's integer (normalize);
  4. N = max(sum wy wx F8, 256 floor D) between the tile centres, continued linearly outside the outer ones;
  5. y = clamp(pedestal_c + floor((2 (v - offset_c) G8_c D + N) / (2 N)), 0, top).
2-D only, at most 4 channels per call; the corrected stack is passed on to the segmenter and the measurers by the caller."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_SIDE, LabelTool, _is_tensor, check_stack_shape  # noqa: F401
from .preprocess import PIX_U8, PIX_U16
from .segment import smooth_weights

MAX_CHANNELS = 4
MAX_IMAGES = 16384                      # meshes of a stack
MAX_STACK = 1 << 28                     # values of a stack
TILES = (16, 32, 64, 128, 256)
F8_MIN, F8_END = 256, 1 << 24
FLOOR_MAX = 4095
SIGMA_MAX = 16.0                        # nodes: radius int(4 sigma + 0.5) <= 64
NORMALIZE = ("mean", "median", "max", "min")


def _integer(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
    if not lo <= int(v) <= hi:
        raise ValueError(f"{name} {int(v)} outside {lo}..{hi}")
    return int(v)


def _fraction(name, q):
    if isinstance(q, (str, bytes)) or not hasattr(q, "__len__") or len(q) != 2:
        raise TypeError(f"{name} must be a pair (num, den) of integers, got {q!r}")
    den = _integer(f"{name} den", q[1], 1, 65536)
    return _integer(f"{name} num", q[0], 0, den), den


def _per_channel(name, v, nc, lo, hi):
    """One integer for every channel, or one per channel."""
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
        v = [v] * nc
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__"):
        raise TypeError(f"{name} must be an integer or one integer per channel, got {type(v).__name__}")
    if len(v) != nc:
        raise ValueError(f"{name} has {len(v)} values for {nc} channels")
    return [_integer(name, x, lo, hi) for x in v]


def mesh_shape(H: int, W: int, tile: int):
    return max(1, H // tile), max(1, W // tile)


def tile_params(tile=64, quantile=(1, 2)):
    """(tile, q_num, q_den) of the Python arguments; anything out of range raises before a handle exists."""
    if isinstance(tile, (bool, np.bool_)) or not isinstance(tile, (int, np.integer)):
        raise TypeError(f"tile must be an integer, got {type(tile).__name__}")
    if int(tile) not in TILES:
        raise ValueError(f"tile {tile}: a power of two in 16..256")
    return (int(tile),) + _fraction("quantile", quantile)


def reduce_params(nc, across=(1, 2), offset=0, floor=1, mesh_median=False, smooth_sigma=0) -> L.CSIllumReduceParams:
    """cs_illum_reduce_params from finish's arguments; anything out of range raises before a handle exists."""
    p = L.CSIllumReduceParams()
    if isinstance(across, str):
        if across != "mean":
            raise ValueError(f"across {across!r}: a pair (num, den) or 'mean'")
        p.a_num, p.a_den, p.mean = 1, 2, 1
    else:
        p.a_num, p.a_den = _fraction("across", across)
        p.mean = 0
    for c, v in enumerate(_per_channel("offset", offset, nc, 0, 65535)):
        p.offset[c] = v
    p.floor = _integer("floor", floor, 1, FLOOR_MAX)
    if not isinstance(mesh_median, (bool, np.bool_)):
        raise TypeError(f"mesh_median must be a bool, got {type(mesh_median).__name__}")
    p.mesh_median = 1 if mesh_median else 0
    if isinstance(smooth_sigma, (bool, np.bool_)) or not isinstance(smooth_sigma, (int, float, np.integer, np.floating)):
        raise TypeError(f"smooth_sigma must be a number (mesh nodes), got {type(smooth_sigma).__name__}")
    s = float(smooth_sigma)
    if not 0.0 <= s <= SIGMA_MAX:                       # NaN fails both
        raise ValueError(f"smooth_sigma {smooth_sigma} outside 0..{SIGMA_MAX}")
    w = smooth_weights(s) if s > 0.0 else [65536]
    p.radius = len(w) - 1                               # a sigma below 1 / 8 has radius 0: no Gaussian
    if p.radius:
        for k, v in enumerate(w):
            p.weights[k] = v
    return p


def scale_of(F8c: np.ndarray, normalize="mean") -> int:
    """G8 of one channel's F8 [my,mx], in Python ints: the rounded mean (2 sum + n) // (2 n), the lower median, the max, the
    min, or the caller's integer in [1, 2^24)."""
    v = sorted(int(x) for x in np.asarray(F8c).ravel())
    if isinstance(normalize, str):
        if normalize not in NORMALIZE:
            raise ValueError(f"normalize {normalize!r}: one of {NORMALIZE} or an integer")
        n = len(v)
        return {"mean": (2 * sum(v) + n) // (2 * n), "median": v[(n - 1) // 2], "max": v[-1], "min": v[0]}[normalize]
    return _integer("normalize", normalize, 1, F8_END - 1)


@dataclass(eq=False)
class IlluminationFunction:
    """The illumination function of a plate: F8 in 1/256 counts on the tile mesh, G8 the scale it is normalised to."""
    tile: int
    shape: tuple                        # (H, W) of the fields
    channels: int
    dtype: np.dtype                     # uint8 or uint16
    F8: np.ndarray                      # [C,my,mx] int32, 256 <= F8 < 2^24
    G8: list                            # [C] Python ints, 1 <= G8 < 2^24
    offset: list                        # [C] counts
    floor: int = 1
    n_images: int = 0
    params: dict = field(default_factory=dict)    # quantile, across, mesh_median, smooth_sigma, normalize
    _dev: object = None                 # F8 on a device, made by an apply_batch of a tensor ...
    _dev_src: object = None             # ... and the F8 it was made from: a changed F8 is uploaded again

    def __post_init__(self):
        self.tile = tile_params(self.tile)[0]
        self.dtype = np.dtype(self.dtype)
        if self.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise TypeError(f"dtype {self.dtype}: uint8 or uint16 expected")
        H, W = (_integer("shape", s, 1, MAX_SIDE) for s in self.shape)
        self.shape = (H, W)
        self.channels = _integer("channels", self.channels, 1, MAX_CHANNELS)
        F8 = np.asarray(self.F8)
        if F8.dtype != np.int32:
            raise TypeError(f"F8 dtype {F8.dtype}: int32 expected")
        if F8.shape != (self.channels,) + mesh_shape(H, W, self.tile):
            raise ValueError(f"F8 {F8.shape}: [{self.channels},{mesh_shape(H, W, self.tile)}] expected for fields of {H} x {W} at tile {self.tile}")
        if F8.min() < F8_MIN or F8.max() >= F8_END:
            raise ValueError("F8 outside [256, 2^24)")
        self.F8 = np.ascontiguousarray(F8)
        self.G8 = _per_channel("G8", list(self.G8), self.channels, 1, F8_END - 1)
        self.offset = _per_channel("offset", list(self.offset), self.channels, 0, 65535)
        self.floor = _integer("floor", self.floor, 1, FLOOR_MAX)

    def save(self, path):
        """A plain .npz: arrays and integers only."""
        p = self.params
        np.savez(path, tile=self.tile, shape=np.array(self.shape, np.int64), channels=self.channels, dtype=str(self.dtype), F8=self.F8,
                 G8=np.array(self.G8, np.int64), offset=np.array(self.offset, np.int64), floor=self.floor, n_images=self.n_images,
                 params=np.array(sorted(f"{k}={v!r}" for k, v in p.items())))

    @classmethod
    def load(cls, path) -> "IlluminationFunction":
        import ast
        with np.load(path, allow_pickle=False) as z:
            params = dict((s.split("=", 1)[0], ast.literal_eval(s.split("=", 1)[1])) for s in z["params"].tolist())
            return cls(tile=int(z["tile"]), shape=tuple(int(s) for s in z["shape"]), channels=int(z["channels"]), dtype=np.dtype(str(z["dtype"])),
                       F8=z["F8"], G8=[int(g) for g in z["G8"]], offset=[int(o) for o in z["offset"]], floor=int(z["floor"]),
                       n_images=int(z["n_images"]), params=params)

    def maps(self, channel: int):
        """(N, D) of every pixel of a field, int64 [H,W]: the function in 1/256 counts times D, with its floor."""
        c = _integer("channel", channel, 0, self.channels - 1)
        H, W = self.shape
        ys, xs = _axis(H, self.tile), _axis(W, self.tile)
        a = self.F8[c].astype(np.int64)
        (y0, y1, wy0, wy1, Dy), (x0, x1, wx0, wx1, Dx) = ys, xs
        N = (wy0[:, None] * (wx0[None, :] * a[y0][:, x0] + wx1[None, :] * a[y0][:, x1]) +
             wy1[:, None] * (wx0[None, :] * a[y1][:, x0] + wx1[None, :] * a[y1][:, x1]))
        D = Dy[:, None] * Dx[None, :]
        return np.maximum(N, F8_MIN * self.floor * D), D

    def gain_map(self, channel: int) -> np.ndarray:
        """float64 [H,W]: G D / N, what a pixel above the dark level is multiplied by.  For plots, on the host."""
        N, D = self.maps(channel)
        return self.G8[int(channel)] * D.astype(np.float64) / N.astype(np.float64)


def _axis(n: int, T: int):
    """(i0, i1, w0, w1, D) per pixel of one axis, int64 [n]: the two nodes and their weights between the tile centres at the doubled
    coordinates C2_i = start_i + end_i - 1; w1 = 2 p - C2_i0 is not clamped, so the function continues linearly outside the outer
    centres.  One node: D = 1, w0 = 1, w1 = 0."""
    m = max(1, n // T)
    z = np.zeros(n, np.int64)
    if m == 1:
        return z, z, z + 1, z, z + 1
    c2 = np.array([2 * i * T + T - 1 if i < m - 1 else i * T + n - 1 for i in range(m)], np.int64)
    p2 = 2 * np.arange(n, dtype=np.int64)
    i0 = np.clip(np.searchsorted(c2, p2, side="right") - 1, 0, m - 2)
    D = c2[i0 + 1] - c2[i0]
    w1 = p2 - c2[i0]
    return i0, i0 + 1, D - w1, w1, D


class IlluminationCorrector(LabelTool):
    """cs_illum_* on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter) whose
    handle and stream to share, so that the corrected stack is read by its stages in stream order.  The stack of meshes that
    add_batch fills lives on the device."""
    _noun = "the corrector"

    def __init__(self, device_id: int = 0, extractor=None):
        super().__init__(device_id, extractor)
        self.reset()

    # ---- argument checks: everything is refused before the device is touched ----
    def _check_image(self, image, name="images"):
        if not (_is_tensor(image) or isinstance(image, np.ndarray)):
            raise TypeError(f"unsupported input type {type(image)} for {name}")
        on_dev = _is_tensor(image)
        if image.ndim not in (3, 4):
            raise ValueError(f"{name} must be [B,H,W] or [B,H,W,C], got shape {tuple(image.shape)}")
        B, H, W = (int(x) for x in image.shape[:3])
        nc = int(image.shape[3]) if image.ndim == 4 else 1
        check_stack_shape(B, H, W, image.shape, nc)
        if nc > MAX_CHANNELS:
            raise ValueError(f"{nc} channels: at most {MAX_CHANNELS} are corrected per call, split the stack")
        if on_dev:
            import torch
            if image.dtype == torch.uint8:
                ptype, dtype = PIX_U8, np.dtype(np.uint8)
            elif image.dtype in (torch.uint16, torch.int16):
                ptype, dtype = PIX_U16, np.dtype(np.uint16)
            else:
                raise TypeError(f"{name} tensor dtype {image.dtype}: uint8 or uint16 expected")
            if not image.is_cuda:
                raise ValueError(f"{name} is a CPU tensor; pass a numpy array or a CUDA tensor")
            if image.device.index != self.device_id:
                raise ValueError(f"{name} is on {image.device}, the corrector on cuda:{self.device_id}")
            if not image.is_contiguous():
                raise ValueError(f"{name} is not contiguous")
        else:
            if image.dtype == np.uint8:
                ptype, dtype = PIX_U8, np.dtype(np.uint8)
            elif image.dtype == np.uint16:
                ptype, dtype = PIX_U16, np.dtype(np.uint16)
            else:
                raise TypeError(f"{name} dtype {image.dtype}: uint8 or uint16 expected")
            if not image.flags.c_contiguous:
                raise ValueError(f"{name} must be C-contiguous")
        return B, H, W, nc, ptype, dtype, on_dev

    # ---- step 1 ----
    def _tile_stats(self, images, dims, tile, q_num, q_den, mesh):
        """cs_illum_tile_stats into mesh, a numpy array or a CUDA tensor [B,C,my,mx] int32."""
        B, H, W, nc, ptype, _, on_dev = dims
        if on_dev or _is_tensor(mesh):
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, images if on_dev else None, mesh if _is_tensor(mesh) else None)
        L.check(self._lib.cs_illum_tile_stats(self._handle, L._ptr(images), ptype, nc, B, H, W, L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST,
                                              tile, q_num, q_den, L._ptr(mesh), L.CS_MEM_DEVICE if _is_tensor(mesh) else L.CS_MEM_HOST))
        return mesh

    def tile_stats_batch(self, images, tile=64, quantile=(1, 2)) -> np.ndarray:
        """int32 [B,C,my,mx] on the host: per image, channel and tile the value of rank (q_num (N - 1)) // q_den among the tile's N
        sorted pixels (1 / 2: the lower median; 0: the minimum, CellProfiler's "Background" method)."""
        dims = self._check_image(images)
        tile, q_num, q_den = tile_params(tile, quantile)
        B, H, W, nc = dims[:4]
        return self._tile_stats(images, dims, tile, q_num, q_den, np.empty((B, nc) + mesh_shape(H, W, tile), np.int32))

    def add_batch(self, images, tile=64, quantile=(1, 2)) -> int:
        """Appends the batch's meshes to the stack on the device; returns n_images.  The first batch after reset() fixes the
        shape, dtype, channels, tile and quantile; a batch that differs is refused."""
        dims = self._check_image(images)
        B, H, W, nc, _, dtype, _ = dims
        key = ((H, W), nc, dtype) + tile_params(tile, quantile)
        if self._key is not None and key != self._key:
            raise ValueError(f"the stack holds fields of {self._key}, this batch is {key}: reset() first")
        if self.n_images + B > MAX_IMAGES:
            raise ValueError(f"{self.n_images} + {B} images: at most {MAX_IMAGES} per function")
        my, mx = mesh_shape(H, W, key[3])
        if (self.n_images + B) * nc * my * mx > MAX_STACK:
            raise ValueError(f"{self.n_images + B} meshes of {nc} x {my} x {mx}: the stack is capped at {MAX_STACK} values")
        import torch
        self._handle                                    # made here at the latest: without a device it raises before torch is asked for memory
        dev = torch.device("cuda", self.device_id)
        if self._stack is None or self._stack.shape[0] < self.n_images + B:
            cap = min(MAX_IMAGES, max(self.n_images + B, 2 * (self._stack.shape[0] if self._stack is not None else 32)))
            grown = torch.empty((cap, nc, my, mx), dtype=torch.int32, device=dev)
            if self._stack is not None:
                self._wait()                            # the stack is complete before torch copies it
                grown[:self.n_images] = self._stack[:self.n_images]
            self._stack = grown
        self._tile_stats(images, dims, key[3], key[4], key[5], self._stack[self.n_images:self.n_images + B])
        self._key = key
        self.n_images += B
        return self.n_images

    def _wait(self):
        """Until the handle's stream has finished: reading the times waits for a result that was left on the device."""
        self.last_timing()

    def reset(self):
        self._stack, self._key, self.n_images = None, None, 0

    # ---- steps 2 and 3 ----
    def reduce_stack(self, stack, params: L.CSIllumReduceParams) -> np.ndarray:
        """cs_illum_reduce of a stack [n,C,my,mx] int32, a numpy array or a CUDA tensor: F8 int32 [C,my,mx] on the host."""
        if _is_tensor(stack):
            import torch
            if stack.dtype != torch.int32 or not stack.is_cuda or stack.device.index != self.device_id or not stack.is_contiguous():
                raise ValueError("stack: a contiguous int32 CUDA tensor of the corrector's device expected")
        elif not (isinstance(stack, np.ndarray) and stack.dtype == np.int32 and stack.flags.c_contiguous):
            raise TypeError("stack: a C-contiguous int32 numpy array or a CUDA tensor expected")
        if stack.ndim != 4:
            raise ValueError(f"stack must be [n,C,my,mx], got shape {tuple(stack.shape)}")
        n, nc, my, mx = (int(s) for s in stack.shape)
        if n < 1 or not 1 <= nc <= MAX_CHANNELS or my < 1 or mx < 1:
            raise ValueError(f"stack shape {tuple(stack.shape)}: [n >= 1, 1..{MAX_CHANNELS}, my >= 1, mx >= 1] expected")
        if n > MAX_IMAGES or n * nc * my * mx > MAX_STACK:
            raise ValueError(f"stack of {n} meshes: at most {MAX_IMAGES} meshes and {MAX_STACK} values")
        F8 = np.empty((nc, my, mx), np.int32)
        on_dev = _is_tensor(stack)
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, stack)
        L.check(self._lib.cs_illum_reduce(self._handle, L._ptr(stack), n, nc, my, mx, L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST,
                                          C.byref(params), L._ptr(F8), L.CS_MEM_HOST))
        return F8

    def finish(self, across=(1, 2), offset=0, floor=1, mesh_median=False, smooth_sigma=0, normalize="mean") -> IlluminationFunction:
        """The function of the images added so far (the stack stays: more may be added).  across: the rank (num, den) across the
        images, default the lower median, or "mean"; offset: the camera's dark level per channel in counts; floor: the least
        value of the function above the offset, counts; mesh_median, smooth_sigma (mesh nodes): the optional filters, off by
        default; normalize: "mean", "median", "max", "min" ("min": a gain <= 1, the output never clips) or an integer G8."""
        if self._key is None:
            raise ValueError("no image was added")
        (H, W), nc, dtype, tile, q_num, q_den = self._key
        rp = reduce_params(nc, across, offset, floor, mesh_median, smooth_sigma)
        if not isinstance(normalize, str):
            _integer("normalize", normalize, 1, F8_END - 1)
        elif normalize not in NORMALIZE:
            raise ValueError(f"normalize {normalize!r}: one of {NORMALIZE} or an integer")
        F8 = self.reduce_stack(self._stack[:self.n_images], rp)
        return IlluminationFunction(tile=tile, shape=(H, W), channels=nc, dtype=dtype, F8=F8, G8=[scale_of(F8[c], normalize) for c in range(nc)],
                                    offset=[int(rp.offset[c]) for c in range(nc)], floor=int(rp.floor), n_images=self.n_images,
                                    params=dict(quantile=(q_num, q_den), across="mean" if rp.mean else (int(rp.a_num), int(rp.a_den)),
                                                mesh_median=bool(rp.mesh_median), smooth_sigma=float(smooth_sigma),
                                                normalize=normalize if isinstance(normalize, str) else int(normalize)))

    # ---- steps 4 and 5 ----
    def apply_batch(self, images, function: IlluminationFunction, pedestal=None, out=None, return_clipped=False):
        """The corrected stack: the images' dtype, layout and memory kind.  pedestal: what is added back per channel, default the
        function's offset, so that noise below the dark level is not clipped away.  out: None (a new stack), or where to write
        it, images itself for in place.  return_clipped: also int64 [B,C,2] on the host, the pixels clamped at 0 and at top (one
        host synchronisation; without it a device stack is complete in the handle's stream order only)."""
        dims = self._check_image(images)
        B, H, W, nc, ptype, dtype, on_dev = dims
        if not isinstance(function, IlluminationFunction):
            raise TypeError(f"function must be an IlluminationFunction, got {type(function).__name__}")
        if (function.shape, function.channels, function.dtype) != ((H, W), nc, dtype):
            raise ValueError(f"the function is of {function.channels}-channel {function.dtype} fields of {function.shape}, "
                             f"the images are {nc}-channel {dtype} fields of {(H, W)}")
        ped = function.offset if pedestal is None else _per_channel("pedestal", pedestal, nc, 0, 65535)
        if not isinstance(return_clipped, (bool, np.bool_)):
            raise TypeError(f"return_clipped must be a bool, got {type(return_clipped).__name__}")
        if out is not None:
            if _is_tensor(out) != on_dev or tuple(out.shape) != tuple(images.shape) or out.dtype != images.dtype:
                raise ValueError("out must have the images' type, shape and memory kind")
            self._check_image(out, "out")
        ap = L.CSIllumApplyParams()
        ap.tile, ap.floor = function.tile, function.floor
        for c in range(nc):
            ap.g8[c], ap.offset[c], ap.pedestal[c] = function.G8[c], function.offset[c], ped[c]
        my, mx = function.F8.shape[1:]
        clipped = np.empty((B, nc, 2), np.int64) if return_clipped else None
        if on_dev:
            import torch
            if function._dev is None or function._dev.device != images.device or not np.array_equal(function._dev_src, function.F8):
                function._dev_src = np.array(function.F8, np.int32)
                function._dev = torch.from_numpy(function._dev_src).to(images.device)
            f8, mesh_kind, kind = function._dev, L.CS_MEM_DEVICE, L.CS_MEM_DEVICE
            if out is None:
                out = torch.empty_like(images)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, images, out, f8)
        else:
            f8, mesh_kind, kind = function.F8, L.CS_MEM_HOST, L.CS_MEM_HOST
            if out is None:
                out = np.empty_like(images)
        L.check(self._lib.cs_illum_apply(self._handle, L._ptr(images), ptype, nc, B, H, W, kind, L._ptr(f8), my, mx, mesh_kind, C.byref(ap),
                                         L._ptr(out), L._ptr(clipped)))
        return (out, clipped) if return_clipped else out

    def last_timing(self):
        """Device milliseconds of the last tile statistics, reduction and apply on the handle: stats_ms, reduce_ms, apply_ms.
        Waits for a call that left its result on the device, and raises CellScreenError (CS_ERR_INVALID) if such a call met a value
        of a device stack or function outside its range, which it cut to the range."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.check(self._lib.cs_illum_last_timing(self._handle, C.byref(a), C.byref(b), C.byref(c)))
        return dict(stats_ms=a.value, reduce_ms=b.value, apply_ms=c.value)
