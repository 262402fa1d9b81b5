"""Quality-cell extraction from segmentation label images on the GPU: the reference's extract_quality_cells
(improved_detection.py:61-111, CAE_improved_modeltrain.py:54-107) after its StarDist call,

    for prop in regionprops(labels):
        border / area / eccentricity rules             (:69-81)
        cell_image = green_channel[minr:maxr, minc:maxc]
        mean / std rule on the bbox rectangle          (:84-91)
        equalize_adapthist + resize                    (:98-99)
        stats: area, eccentricity, solidity, mean_intensity, std_intensity   (:100-106)

for a whole batch of label images in two library calls (csrc/extract.hip, then the preprocess kernel of
csrc/preprocess.hip).  The segmenter stays the caller's: any function from the segmentation channel to an int32
label image (StarDist's predict_instances, a threshold + scipy.ndimage.label, labels kept on disk).

Eccentricity and solidity follow scikit-image 0.18.3's definitions as restated in tests/extract_reference.py (scikit-image
itself is not a dependency); the cells are bit-identical to Preprocessor on the same crops cut on the host, which the
preprocess golden pins to scikit-image."""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, List, NamedTuple, Optional

import numpy as np

from . import _lib as L
from ._labels import MAX_LABEL, MAX_SIDE, _is_tensor  # noqa: F401
from .preprocess import CLIP_LIMIT, MAX_RATIO, OUT_SIDE, PIX_U8, PIX_U16, Preprocessor, check_out_hw

QC_BORDER, QC_AREA, QC_ECCENTRICITY, QC_INTENSITY = 1, 2, 4, 8          # cs_region.failed bits
IMAGE_OK, IMAGE_NO_CELLS, IMAGE_UNSUPPORTED = 0, 1, 2                   # per-image status
MAX_SLOTS = 1 << 22                                                     # batch * max_label

# the reference's thresholds (improved_detection.py:69-91) and clip limit (:98)
REFERENCE_QC = dict(border=10, min_area=200, max_area=8000, max_eccentricity=0.95, min_mean=0.5, min_std=0.1,
                    clip_limit=CLIP_LIMIT)
STAT_KEYS = ("area", "eccentricity", "solidity", "mean_intensity", "std_intensity")    # :100-106


def qc_params(**kw) -> L.CSQcParams:
    bad = set(kw) - set(REFERENCE_QC)
    if bad:
        raise ValueError(f"unknown QC parameter(s) {sorted(bad)}; known: {sorted(REFERENCE_QC)}")
    v = dict(REFERENCE_QC, **kw)
    q = L.CSQcParams()
    q.border, q.min_area, q.max_area, q.reserved = int(v["border"]), int(v["min_area"]), int(v["max_area"]), 0
    q.max_eccentricity, q.min_mean, q.min_std = float(v["max_eccentricity"]), float(v["min_mean"]), float(v["min_std"])
    q.clip_limit = float(v["clip_limit"])
    return q


class Extraction(NamedTuple):
    cells: object               # float32 [n,out_h,out_w]: numpy, or a torch CUDA tensor
    cell_image: np.ndarray      # int32 [n]: image index of each cell
    regions: np.ndarray         # L.REGION_DTYPE [n_regions]: every region, passing or not, in (image, label) order
    status: np.ndarray          # int32 [B]: IMAGE_OK / IMAGE_NO_CELLS / IMAGE_UNSUPPORTED


def region_stats(regions: np.ndarray) -> List[dict]:
    """The reference's per-cell stats dicts (:100-106) for the passing regions of a table."""
    out = []
    for r in regions[regions["cell"] >= 0]:
        out.append({"area": int(r["area"]), "eccentricity": float(r["eccentricity"]), "solidity": float(r["solidity"]),
                    "mean_intensity": float(r["mean_intensity"]), "std_intensity": float(r["std_intensity"])})
    return out


class CellExtractor:
    """One preprocess handle (one GPU, one stream) that turns label images into screened-ready cells of
    out_hw = (out_h, out_w): 64 x 64 by default, (H, W) for a model built with input_shape=(H, W, 1)."""

    def __init__(self, device_id: int = 0, out_hw=(OUT_SIDE, OUT_SIDE), **qc):
        self.out_hw = check_out_hw(out_hw)
        self._lib = L.load_library()
        self.device_id = device_id
        self.qc = dict(REFERENCE_QC, **qc)
        self._qc = qc_params(**qc)
        self._pre: Optional[Preprocessor] = None        # the handle is created by the first call, after its argument checks

    @property
    def _handle(self):
        if self._pre is None:
            self._pre = Preprocessor(self.device_id, self.out_hw)
        return self._pre._h

    def close(self):
        if self._pre is not None:
            self._pre.close()

    # ---- argument checks: everything is refused before the device is touched ---------------------------------------
    def _check(self, images, labels, channel):
        tens = _is_tensor(images), _is_tensor(labels)
        if tens[0] != tens[1]:
            raise TypeError("images and labels must both be numpy arrays or both be torch tensors")
        if not tens[0] and not (isinstance(images, np.ndarray) and isinstance(labels, np.ndarray)):
            raise TypeError(f"unsupported input types {type(images)}, {type(labels)}")
        if labels.ndim != 3:
            raise ValueError(f"labels must be [B,H,W], got shape {tuple(labels.shape)}")
        if images.ndim not in (3, 4):
            raise ValueError(f"images must be [B,H,W] or [B,H,W,C], got shape {tuple(images.shape)}")
        if tuple(images.shape[:3]) != tuple(labels.shape):
            raise ValueError(f"images {tuple(images.shape)} and labels {tuple(labels.shape)} differ in batch or height x width")
        B, H, W = (int(x) for x in labels.shape)
        if B < 1 or H < 1 or W < 1:
            raise ValueError(f"empty batch or image: labels shape {tuple(labels.shape)}")
        if H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f"image sides above {MAX_SIDE} are not supported, got {H}x{W}")
        Cn = int(images.shape[3]) if images.ndim == 4 else 1
        if channel is None:
            if Cn == 1:
                channel = 0
            elif Cn >= 3:
                channel = 1                                         # the analysis (green) channel, improved_detection.py:57
            else:
                raise ValueError(f"{Cn} channels: pass channel= explicitly")
        if not 0 <= channel < Cn:
            raise ValueError(f"channel {channel} outside [0, {Cn})")
        if tens[0]:
            import torch
            if images.dtype == torch.uint8:
                ptype = PIX_U8
            elif images.dtype in (torch.uint16, torch.int16):
                ptype = PIX_U16
            else:
                raise TypeError(f"image tensor dtype {images.dtype}: uint8 or uint16 expected")
            if labels.dtype != torch.int32:
                raise TypeError(f"label tensor dtype {labels.dtype}: int32 expected")
            for name, t in (("images", images), ("labels", labels)):
                if not t.is_cuda:
                    raise ValueError(f"{name} is a CPU tensor; pass numpy arrays or CUDA tensors")
                if t.device.index != self.device_id:
                    raise ValueError(f"{name} is on {t.device}, the extractor on cuda:{self.device_id}")
                if not t.is_contiguous():
                    raise ValueError(f"{name} is not contiguous")
        else:
            if images.dtype == np.uint8:
                ptype = PIX_U8
            elif images.dtype == np.uint16:
                ptype = PIX_U16
            else:
                raise TypeError(f"image dtype {images.dtype}: uint8 or uint16 expected")
            if not np.issubdtype(labels.dtype, np.integer):
                raise TypeError(f"label dtype {labels.dtype}: an integer label image expected")
            if not (images.flags.c_contiguous and labels.flags.c_contiguous):
                raise ValueError("images and labels must be C-contiguous")
        return B, H, W, Cn, channel, ptype, tens[0]

    @staticmethod
    def _relabel_host(labels: np.ndarray):
        """int32 labels + the map back to the caller's ids (None when the ids are used as they are).  Sparse ids are renumbered
        per image with np.unique(return_inverse=True), which keeps their order and so every result."""
        B = labels.shape[0]
        lo, hi = (int(labels.min()), int(labels.max())) if labels.size else (0, 0)
        if lo < 0:
            raise ValueError(f"negative label {lo}: 0 is background, regions are > 0")
        if hi <= MAX_LABEL and B * hi <= MAX_SLOTS:
            return np.ascontiguousarray(labels, np.int32), hi, None
        out = np.empty(labels.shape, np.int32)
        maps, mx = [], 0
        for b in range(B):
            u, inv = np.unique(labels[b], return_inverse=True)
            if u[0] != 0:                                  # keep 0 as background
                u = np.concatenate([[0], u])
                inv = inv + 1
            out[b] = inv.reshape(labels.shape[1:])
            maps.append(u.astype(np.int64))
            mx = max(mx, len(u) - 1)
        return out, mx, maps

    @staticmethod
    def _relabel_device(labels):
        import torch
        lo, hi = (int(x) for x in torch.aminmax(labels))
        if lo < 0:
            raise ValueError(f"negative label {lo}: 0 is background, regions are > 0")
        B = labels.shape[0]
        if hi <= MAX_LABEL and B * hi <= MAX_SLOTS:
            return labels, hi, None
        out = torch.empty_like(labels)
        maps, mx = [], 0
        for b in range(B):
            u, inv = torch.unique(labels[b], return_inverse=True)
            u = u.cpu().numpy().astype(np.int64)
            if u[0] != 0:
                u = np.concatenate([[0], u])
                inv = inv + 1
            out[b] = inv.to(torch.int32)
            maps.append(u)
            mx = max(mx, len(u) - 1)
        return out.contiguous(), mx, maps

    # ---- the two calls ---------------------------------------------------------------------------------------------------
    def extract_batch(self, images, labels, out=None, channel: Optional[int] = None) -> Extraction:
        """images: [B,H,W] or [B,H,W,C] uint8/uint16 (the analysis channel is `channel`, default 1 of >= 3 channels as
        improved_detection.py:57, 0 of one); labels: [B,H,W] integer, 0 = background.  numpy arrays or CUDA tensors of the
        extractor's device.  out: None -- cells as numpy for numpy inputs, as a CUDA float32 tensor for tensor inputs -- or a
        CUDA float32 tensor [>= n,out_h,out_w] to fill (the result is its first n cells)."""
        B, H, W, Cn, channel, ptype, on_dev = self._check(images, labels, channel)
        oh, ow = self.out_hw
        if out is not None:
            import torch
            if not (_is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
                    and tuple(out.shape[1:]) == (oh, ow) and out.device.index == self.device_id):
                raise ValueError(f"out must be a contiguous CUDA float32 tensor [n,{oh},{ow}] on the extractor's device")
        if on_dev:
            lab, max_label, maps = self._relabel_device(labels)
        else:
            lab, max_label, maps = self._relabel_host(labels)
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, images, lab)
        nreg, ncell = C.c_int64(), C.c_int64()
        L.check(self._lib.cs_extract_measure(self._handle, L._ptr(images), ptype, Cn, channel, L._ptr(lab), B, H, W,
                                             L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST, max_label, C.byref(self._qc),
                                             C.byref(nreg), C.byref(ncell)))
        n_reg, n = nreg.value, ncell.value
        regions = np.zeros(n_reg, L.REGION_DTYPE)
        status = np.zeros(B, np.int32)
        if out is not None or on_dev:
            import torch
            dev = torch.device("cuda", self.device_id)
            if out is not None:
                if out.shape[0] < n:
                    raise ValueError(f"out holds {out.shape[0]} cells, the batch yields {n}")
                cells = out[:n]
            else:
                cells = torch.empty((n, oh, ow), dtype=torch.float32, device=dev)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, cells)
            L.check(self._lib.cs_extract_fill(self._handle, regions.ctypes.data, status.ctypes.data, L.CS_MEM_HOST,
                                              cells.data_ptr() if n else None, None, L.CS_MEM_DEVICE))
            cell_image = regions["image"][regions["cell"] >= 0].astype(np.int32)     # the same indices, from the host table
        else:
            cells = np.empty((n, oh, ow), np.float32)
            cell_image = np.empty(n, np.int32)
            L.check(self._lib.cs_extract_fill(self._handle, regions.ctypes.data, status.ctypes.data, L.CS_MEM_HOST,
                                              cells.ctypes.data, cell_image.ctypes.data, L.CS_MEM_HOST))
        if maps is not None:
            # the table is in (image, label) order: one slice per image, not one pass over the table per image
            edge = np.searchsorted(regions["image"], np.arange(B + 1))
            for b, u in enumerate(maps):
                m = slice(edge[b], edge[b + 1])
                regions["label"][m] = u[regions["label"][m]]
        return Extraction(cells, cell_image, regions, status)

    def extract(self, image, labels):
        """One image ([H,W] or [H,W,C]) and its [H,W] labels -> (cells float32 [n,out_h,out_w], stats dicts), the return value of
        the reference's extract_quality_cells.  An image whose status is not OK raises, as the reference's extraction does
        inside its per-file try (improved_detection.py:113-115)."""
        r = self.extract_batch(image[None], labels[None])
        st = int(r.status[0])
        if st == IMAGE_NO_CELLS:
            raise ValueError("a passing region has a bounding-box side below 8 px: equalize_adapthist raises on it")
        if st == IMAGE_UNSUPPORTED:
            raise ValueError(self._unsupported_text() + ": beyond the preprocess kernel")
        return r.cells, region_stats(r.regions)

    def _unsupported_text(self) -> str:
        oh, ow = self.out_hw
        if (oh, ow) == (OUT_SIDE, OUT_SIDE):
            return "a passing region has a bounding-box side above 1024 px"
        return (f"a passing region has a bounding-box side above 1024 px or above {MAX_RATIO} x the output size "
                f"{oh}x{ow} on its axis")

    def last_timing(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.check(self._lib.cs_extract_last_timing(self._handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"label_ms": a.value, "region_ms": b.value, "cells_ms": c.value}


def read_image(path: str) -> np.ndarray:
    """.npy, or .tif / .tiff through tifffile (imported only then; the reference reads with tiff.imread, :51)."""
    if path.endswith(".npy"):
        return np.load(path)
    if path.lower().endswith((".tif", ".tiff")):
        import tifffile
        return tifffile.imread(path)
    raise ValueError(f"{os.path.basename(path)}: .npy or .tif expected")


def split_channels(image: np.ndarray):
    """(seg_channel, analysis image, analysis channel index) as improved_detection.py:54-60: channel 2 segments, channel 1 is
    analysed; a 2-D image is both.  A 3-D image with fewer than 3 channels raises (the reference falls through to using
    the 3-D image as a 2-D one, which fails in its segmentation)."""
    if image.ndim == 3 and image.shape[-1] >= 3:
        return image[..., 2], image, 1
    if image.ndim == 2:
        return image, image, 0
    raise ValueError(f"image of shape {image.shape}: a 2-D image or [H,W,>=3] channels expected")


def label_cell_extractor(segment: Callable[[np.ndarray], np.ndarray], device_id: int = 0, out_hw=(OUT_SIDE, OUT_SIDE),
                         expand_distance=None, **qc):
    """The `cell_extractor(image_path) -> (cells, stats)` that ProductionMutantScreening accepts, from a segmenter
    `segment(seg_channel) -> labels`.  The seg channel is handed over untouched (csbdeep's normalize belongs to the
    segmenter), e.g. label_cell_extractor(lambda seg: model.predict_instances(normalize(seg))[0]).  Errors raise; the
    screening driver's try turns them into the reference's "Error processing" line and ([], []).
    out_hw: the size of the cells, 64 x 64 as the reference's resize by default; for a model built with
    input_shape=(H, W, 1) pass out_hw=(H, W).
    expand_distance (None, or a number of pixels in 1..127): for a segmenter of nuclei, such as StarDist's 2D_versatile_fluo,
    whose labels cover the stain and not the cell.  The labels are uploaded, grown by that distance on the extractor's handle
    (cellscreen/expand.py: every label spreads outwards and stops halfway to its neighbours, ids unchanged) and extracted
    without coming back to the host; integer labels are cast to int32, and ids that do not fit raise.  The QC numbers among
    **qc stay the caller's: a grown nucleus is judged by the same min_area and max_area unless they are changed to fit it."""
    out_hw = check_out_hw(out_hw)
    if expand_distance is not None:
        from .expand import expand_params                # expand.py imports this module
        expand_params(expand_distance)
    ext = {}

    def cell_extractor(image_path: str):
        image = read_image(image_path)
        seg, img, ch = split_channels(image)
        labels = np.asarray(segment(seg))
        if labels.shape != img.shape[:2]:
            raise ValueError(f"segmenter returned labels of shape {labels.shape} for an image of {img.shape[:2]}")
        if "x" not in ext:
            ext["x"] = CellExtractor(device_id, out_hw, **qc)
        if expand_distance is None:
            r = ext["x"].extract_batch(np.ascontiguousarray(img)[None], np.ascontiguousarray(labels)[None], channel=ch)
        else:
            r = _extract_grown(ext, img, labels, ch, expand_distance)
        st = int(r.status[0])
        if st != IMAGE_OK:
            raise ValueError("a passing region has a bounding-box side below 8 px (equalize_adapthist raises)" if st == IMAGE_NO_CELLS
                             else ext["x"]._unsupported_text() + " (beyond the preprocess kernel)")
        return list(r.cells), region_stats(r.regions)

    return cell_extractor


def _extract_grown(ext: dict, img: np.ndarray, labels: np.ndarray, ch: int, expand_distance) -> Extraction:
    """label_cell_extractor with expand_distance: image and labels go up once, the labels are grown in place on the
    extractor's handle and extracted where they are; only the cells come back.  ext: the closure's state, the CellExtractor
    "x" and the expander "e"."""
    import torch

    from .expand import LabelExpander
    if img.dtype not in (np.uint8, np.uint16):
        raise TypeError(f"image dtype {img.dtype}: uint8 or uint16 expected")
    if not np.issubdtype(labels.dtype, np.integer):
        raise TypeError(f"label dtype {labels.dtype}: an integer label image expected")
    if labels.size and (int(labels.min()) < -(1 << 31) or int(labels.max()) >= 1 << 31):
        raise ValueError(f"label ids {int(labels.min())}..{int(labels.max())} do not fit int32")
    if "e" not in ext:
        ext["e"] = LabelExpander(ext["x"].device_id, extractor=ext["x"])
    dev = torch.device("cuda", ext["x"].device_id)
    host = np.ascontiguousarray(img)[None]
    d_img = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
    d_lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)[None]).to(dev)
    ext["e"].expand_batch(d_lab, expand_distance, out=d_lab)
    r = ext["x"].extract_batch(d_img, d_lab, channel=ch)
    return r._replace(cells=r.cells.cpu().numpy())
