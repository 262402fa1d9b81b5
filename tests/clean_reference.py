"""CPU restatement of the segmenter's mask cleanup (cs_segment_clean in csrc/segment.hip,
ThresholdSegmenter(open_radius=..., min_area=...)): what the device kernels are compared against.  Numpy only in this file; the
components are tests/segment_reference.py's (scipy.ndimage.label).

  erode / dilate  one elementary step by the 3 x 3 cross (k = 1) or square (k = 2) on a bool image padded with background:
                  outside the image is 0 for the erosion, and for the dilation it does not matter
  opening         r erosions, then r dilations: scipy.ndimage.binary_opening(mask, generate_binary_structure(2, k),
                  iterations=r) (border_value 0), which equals one opening by the iterated structure: the diamond of radius r
                  for k = 1, the square of side 2r + 1 for k = 2
  drop_small      components (connectivity 1: 4 neighbours, 2: 8) of fewer than `a` pixels become background; a component of
                  exactly `a` pixels stays.  This is skimage.morphology.remove_small_objects(mask, min_size=a,
                  connectivity=c), whose definition is label + bincount + a comparison `size < min_size`; scikit-image is not
                  needed for it, and the restatement is scipy.ndimage.label + numpy.bincount
  clean           opening (r = None or 0: none), then drop_small (a = None or 0: none), in that order
tests/golden/golden_clean.npz (tools/make_golden_clean.py) pins both steps to SciPy 1.15.3."""
import numpy as np

import segment_reference as R

MAX_R, MAX_AREA = 15, 1 << 24


def _shifted(p: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """The neighbour at (dy, dx) of every pixel of an image that was padded by one."""
    H, W = p.shape[0] - 2, p.shape[1] - 2
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def _offsets(k: int):
    if k not in (1, 2):
        raise ValueError("open connectivity: 1 (cross) or 2 (square)")
    return [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if k == 2 or dy == 0 or dx == 0]


def erode(m: np.ndarray, k: int) -> np.ndarray:
    p = np.pad(m.astype(bool), 1)
    out = np.ones(m.shape, bool)
    for dy, dx in _offsets(k):
        out &= _shifted(p, dy, dx)
    return out


def dilate(m: np.ndarray, k: int) -> np.ndarray:
    p = np.pad(m.astype(bool), 1)
    out = np.zeros(m.shape, bool)
    for dy, dx in _offsets(k):
        out |= _shifted(p, dy, dx)
    return out


def opening(mask: np.ndarray, r: int, k: int = 2) -> np.ndarray:
    """uint8 0 / 1 plane of one 2-D mask (anything non-zero is foreground)."""
    if mask.ndim != 2:
        raise TypeError("2-D mask expected")
    if not 1 <= r <= MAX_R:
        raise ValueError(f"open radius outside 1..{MAX_R}")
    m = mask.astype(bool)
    for _ in range(r):
        m = erode(m, k)
    for _ in range(r):
        m = dilate(m, k)
    return m.astype(np.uint8)


def drop_small(mask: np.ndarray, a: int, connectivity: int = 1) -> np.ndarray:
    if mask.ndim != 2:
        raise TypeError("2-D mask expected")
    if not 1 <= a <= MAX_AREA:
        raise ValueError(f"min area outside 1..{MAX_AREA}")
    lab, _ = R.label_mask(mask.astype(bool), connectivity)
    sizes = np.bincount(lab.ravel())
    small = sizes < a
    small[0] = True                                     # the background stays background
    return (~small[lab]).astype(np.uint8)


def clean(mask: np.ndarray, r=None, k: int = 2, a=None, connectivity: int = 1) -> np.ndarray:
    m = (mask != 0).astype(np.uint8)
    if r:
        m = opening(m, r, k)
    if a:
        m = drop_small(m, a, connectivity)
    return m


def mask_inputs(shape, seed=0):
    """(name, uint8 0 / 1 mask) of one shape: noise at densities 0.5 and 0.9, blobs joined by bridges one and two pixels thick,
    all foreground, all background, a checkerboard, a one-pixel frame on the border and a thick one."""
    H, W = shape
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    rad = max(2, min(H, W, 64) // 4)                                            # 10 at 40 rows: holds a 15 x 15 square
    pitch = 3 * rad
    cy, cx = yy // pitch * pitch + pitch // 2, xx // pitch * pitch + pitch // 2
    blobs = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
    blobs |= yy % pitch == pitch // 2                                           # rows of blobs joined by a 1-pixel bridge
    blobs |= (xx % pitch == pitch // 2) | (xx % pitch == pitch // 2 + 1)        # columns by a 2-pixel one
    frame = np.zeros(shape, bool)
    frame[[0, -1], :] = frame[:, [0, -1]] = True
    t = min(5, (min(H, W) + 1) // 2)
    thick = np.ones(shape, bool)
    thick[t:H - t, t:W - t] = False
    named = [("noise50", rng.random(shape) < 0.5), ("noise90", rng.random(shape) < 0.9), ("bridged", blobs),
             ("full", np.ones(shape, bool)), ("empty", np.zeros(shape, bool)), ("checker", (yy + xx) % 2 == 0), ("frame", frame),
             ("thick", thick)]
    return [(n, m.astype(np.uint8)) for n, m in named]
