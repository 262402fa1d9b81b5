"""CPU restatement of the whole segmenter, ThresholdSegmenter.segment_batch with any combination of its stages, built only by
composing the stage restatements under tests/ in the order the class documents:

  smoothing (smooth_reference) -> top-hat (background_reference) -> the rule: Otsu / fixed (segment_reference), "local"
  (local_reference), either under a weak rule (hysteresis_reference), or "noise" (noise_reference) -> hole filling -> opening and
  minimum area (clean_reference) -> labels (segment_reference), or the split (split_reference on the mask, or
  split_intensity_reference on the plane the rule saw) -> growth (expand_reference).

The rules that no stage restatement holds are restated here: the 3 x 3 median runs once, in the first of smoothing, correction and
local rule; the thresholds reported are the strong rule's, -1 for "local" and "noise"; the holes are filled once, behind the rule
(or its weak form) and in front of the cleanup; n_labels and the height plane are what they are without the growth.

  segment_batch   the restatement; `planes` of its result holds every intermediate plane by the name of the method that returns it
  scene           the batches of two images the cases run on
  FACTORS, CASES  the option combinations of tests/test_gpu_pipeline.py: a literal list that covers every pair of levels of
                  FACTORS which the package's own *_params functions accept, plus one full chain per rule; `generate` is the
                  greedy cover it was written out from, and tests/test_pipeline_reference_cpu.py holds the two together
  options         a case's ThresholdSegmenter keyword arguments, its shape and its pixel type"""
import itertools

import numpy as np
from scipy import ndimage

import background_reference as BR
import clean_reference as CR
import expand_reference as ER
import hysteresis_reference as HR
import local_reference as LR
import noise_reference as NR
import segment_reference as R
import smooth_reference as MR
import split_intensity_reference as IR
import split_reference as SR

DEFAULTS = dict(threshold="otsu", connectivity=1, fill_holes=True, split_touching=False, split_h=3, background_radius=None,
                denoise=False, local_radius=None, local_delta=0, local_floor=-1, open_radius=None, open_connectivity=2, min_area=None,
                smooth_sigma=None, split_by="distance", split_depth=16, split_contrast=0, weak_threshold=None, weak_delta=None,
                noise_k=5.0, noise_tile=64, noise_floor=1.0, weak_k=None, expand_distance=None)


def expand_windows(lab: np.ndarray, max_d2: int, side: int = 32):
    """expand_reference.expand of one image, (grown, d2), window by window: what a pixel gets depends on the labels within
    sqrt(max_d2) of it alone, so each side x side window is cut from the expansion of itself with that margin around it.  The
    restatement compares every background pixel with every labelled one, which on whole images costs the tests minutes."""
    H, W = lab.shape
    m = int(np.sqrt(max_d2)) + 1
    out, d2 = np.empty((H, W), np.int32), np.empty((H, W), np.uint16)
    for y in range(0, H, side):
        for x in range(0, W, side):
            y0, x0 = max(0, y - m), max(0, x - m)
            g, d = ER.expand(lab[y0:y + side + m, x0:x + side + m], max_d2)
            out[y:y + side, x:x + side] = g[y - y0:y - y0 + side, x - x0:x - x0 + side]
            d2[y:y + side, x:x + side] = d[y - y0:y - y0 + side, x - x0:x - x0 + side]
    return out, d2


def segment_one(raw: np.ndarray, **opts):
    """(labels, n_labels, threshold, heights or None, planes) of one 2-D image; opts: ThresholdSegmenter's keyword arguments."""
    unknown = set(opts) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"not a ThresholdSegmenter argument: {sorted(unknown)}")
    o = dict(DEFAULTS, **opts)
    conn, planes = o["connectivity"], {}
    x = np.ascontiguousarray(raw)
    median = bool(o["denoise"])                           # runs once, inside the first stage that exists
    if o["smooth_sigma"] is not None:
        x, median = MR.smooth_sigma(x, float(o["smooth_sigma"]), median), False
        planes["smooth_batch"] = x
    if o["background_radius"] is not None:
        x, median = BR.correct(x, int(o["background_radius"]), median), False
        planes["correct_batch"] = x
    guide = x                                             # what the rule sees, and split_by="intensity" after it
    rule = o["threshold"]
    if isinstance(rule, str) and rule == "noise":
        weak8 = None if o["weak_k"] is None else NR.k8_of(o["weak_k"])
        m = NR.noise_mask(x, o["noise_tile"], NR.k8_of(o["noise_k"]), weak8, NR.k8_of(o["noise_floor"]), conn)
        planes["noise_mask_batch"], t = m, -1
    elif isinstance(rule, str) and rule == "local":
        r, delta, floor = o["local_radius"], o["local_delta"], o["local_floor"]
        planes["local_mask_batch"] = m = LR.local_mask(x, r, delta, floor, median)
        if o["weak_delta"] is not None:
            planes["hysteresis_mask_batch"] = m = HR.hysteresis(HR.levels_local(x, r, delta, o["weak_delta"], floor, median), conn)
        t = -1
    else:
        if median:
            raise ValueError("denoise needs smooth_sigma, background_radius or threshold='local'")
        t = R.otsu(x) if rule == "otsu" else int(rule)
        if o["weak_threshold"] is not None:
            planes["hysteresis_mask_batch"] = m = HR.hysteresis(HR.levels_global(x, t, HR.weak_of(t, o["weak_threshold"])), conn)
        else:
            m = x > t
    m = np.asarray(m) > 0
    if o["fill_holes"]:
        m = ndimage.binary_fill_holes(m)
    if o["open_radius"] is not None or o["min_area"] is not None:
        planes["clean_mask_batch"] = c = CR.clean(m.astype(np.uint8), o["open_radius"], o["open_connectivity"], o["min_area"], conn)
        m = c > 0                                         # labelled as it is: no second hole filling
    heights = None
    if not o["split_touching"]:
        lab, n = R.label_mask(m, conn)
    elif o["split_by"] == "intensity":
        lab, n, heights = IR.split_intensity(m, guide, conn, o["split_depth"], o["split_contrast"])
    else:
        lab, n, heights = SR.split_mask(m, conn, o["split_h"])
    if o["expand_distance"] is not None:
        lab = expand_windows(lab, ER.max_d2_of(o["expand_distance"]))[0]
    return lab.astype(np.int32), n, t, heights, planes


def segment_batch(images: np.ndarray, channel=None, return_distance: bool = False, **opts):
    """What ThresholdSegmenter(**opts).segment_batch(images, channel, return_distance) returns, and after it `planes`: the
    [B,H,W] plane of every stage that is on, under the name of the method that returns it."""
    if images.ndim == 3:
        chan = images
    else:
        chan = images[..., channel if channel is not None else (2 if images.shape[3] >= 3 else 0)]
    if return_distance and not opts.get("split_touching", False):
        raise ValueError("return_distance needs split_touching=True")
    out = [segment_one(c, **opts) for c in chan]
    planes = {k: np.stack([o[4][k] for o in out]) for k in out[0][4]}
    head = (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32))
    return head + ((np.stack([o[3] for o in out]),) if return_distance else ()) + (planes,)


# ---- the scene ---------------------------------------------------------------------------------------------------------------
PITCH = 20                                               # one object (or touching pair) per PITCH x PITCH cell of the field
KINDS = ("gauss pair", "ring", "flat pair", "small", "gauss", "speck")


def scene(shape, dtype, seed=0) -> np.ndarray:
    """[2,H,W] of `dtype`, the two images different.  On a PITCH grid (every other cell of it in fields of more than 12 cells, so
    that the noise rule's mesh sees background), in an order that turns with the image: pairs of Gaussian blobs with an intensity
    valley between them, shallow or deep enough to survive the smoothing; flat disks with a hole wider than twice the growth;
    pairs of flat disks joined by a neck, or parted by a gap that only a weak rule on the smoothed plane closes; groups of small
    objects; single blobs; and single 3 x 3 squares, which survive the opening and stay under the minimum area whatever the
    rule makes of them.  Under them a slow illumination gradient, along another axis in each image, and Gaussian speckle; on top
    isolated bright pixels.  tests/test_pipeline_reference_cpu.py holds that with this content no stage of any case is idle."""
    H, W = shape
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((2, H, W), dtype)
    rows, cols = max(1, H // PITCH), max(1, W // PITCH)
    for b in range(2):
        f = 0.08 + 0.10 * (xx / max(W - 1, 1) if b == 0 else yy / max(H - 1, 1)) + 0.02 * (yy / H) * (xx / W)
        k = 2 * b
        for i in range(rows):
            for j in range(cols):
                cy = (i * H) // rows + H // (2 * rows) + int(rng.integers(-1, 2))
                cx = (j * W) // cols + W // (2 * cols) + int(rng.integers(-1, 2))
                if rows * cols > 12 and (i + j + b) % 2:                 # room for the noise rule's mesh to see background
                    continue
                kind = KINDS[k % len(KINDS)]
                k += 1
                d2 = lambda y, x: (yy - y) ** 2 + (xx - x) ** 2
                if kind == "gauss pair":
                    gap = 4 + (i + j + b) % 2                              # a shallow valley, or one that survives the smoothing
                    f += 0.5 * np.exp(-d2(cy, cx - gap) / 18.0) + 0.42 * np.exp(-d2(cy, cx + gap) / 18.0)
                elif kind == "ring":
                    f += 0.5 * ((d2(cy, cx) <= 81) & (d2(cy, cx) > 30))         # the hole is wider than twice the growth
                elif kind == "flat pair":
                    far = ((i + j + b) // 2) % 2                           # a neck, or a gap that only a smoothed weak rule closes
                    f += 0.45 * ((d2(cy, cx - 5) <= 30) | (d2(cy + 1, cx + 5 + 2 * far) <= 30))
                elif kind == "small":
                    f += 0.55 * (d2(cy, cx) <= 8) + 0.5 * np.exp(-d2(cy + 1, cx - 7) / 8.0)
                    f += 0.8 * ((abs(yy - cy + 5) <= 1) & (abs(xx - cx - 6) <= 1))
                elif kind == "gauss":
                    f += 0.6 * np.exp(-d2(cy, cx) / 24.5)
                else:
                    f += 0.8 * ((abs(yy - cy) <= 1) & (abs(xx - cx) <= 1))
        f += rng.normal(0.0, 0.012, (H, W))
        hot = rng.random((H, W)) < 0.004
        f[hot] += 0.6
        out[b] = np.clip(np.rint(f * top), 0, top).astype(dtype)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
FACTORS = (("smooth", (0, 1)), ("correct", (0, 1)), ("denoise", (0, 1)), ("rule", ("otsu", "fixed", "local", "noise")),
           ("weak", (0, 1)), ("clean", ("off", "open", "area", "both")), ("connectivity", (1, 2)), ("fill", (0, 1)),
           ("split", ("off", "distance", "intensity")), ("expand", (0, 1)), ("dtype", ("uint8", "uint16")))
NAMES = tuple(n for n, _ in FACTORS)
# the smallest shapes that cross the stages' tiles, taken in rotation, each with the noise tile that keeps two mesh tiles a side
SHAPES = (((47, 61), 16), ((67, 261), 32), ((131, 200), 32), ((40, 1030), 16))
SIGMA, RADIUS, LOCAL_RADIUS, OPEN_RADIUS, MIN_AREA, EXPAND = 1.5, 11, 13, 2, 90, 3
# in parts of the pixel type's top: the fixed strong and weak thresholds, the local rule's strong and weak deltas
FIXED, FIXED_WEAK, DELTA, DELTA_WEAK = 0.34, 0.26, 0.12, 0.05

CASES = [
    # smooth correct denoise rule weak clean connectivity fill split expand dtype
    (1, 1, 1, "otsu", 1, "both", 1, 1, "intensity", 1, "uint16"),
    (1, 1, 1, "fixed", 1, "both", 2, 1, "distance", 1, "uint8"),
    (1, 1, 1, "local", 1, "both", 1, 1, "distance", 1, "uint8"),
    (1, 1, 1, "noise", 1, "both", 2, 1, "intensity", 1, "uint16"),
    (0, 0, 0, "otsu", 0, "open", 2, 0, "off", 0, "uint8"),
    (0, 0, 0, "fixed", 0, "area", 1, 0, "distance", 1, "uint16"),
    (0, 0, 1, "local", 1, "off", 1, 1, "off", 0, "uint16"),
    (1, 1, 0, "noise", 0, "off", 1, 0, "intensity", 0, "uint8"),
    (1, 1, 0, "local", 1, "area", 2, 1, "off", 1, "uint8"),
    (0, 1, 1, "local", 0, "open", 1, 1, "intensity", 1, "uint16"),
    (1, 0, 1, "noise", 1, "open", 1, 0, "distance", 0, "uint8"),
    (0, 0, 0, "fixed", 0, "both", 1, 0, "intensity", 0, "uint8"),
    (1, 1, 1, "otsu", 1, "off", 2, 1, "distance", 1, "uint8"),
    (0, 1, 1, "noise", 1, "area", 1, 1, "intensity", 0, "uint8"),
    (1, 1, 1, "fixed", 1, "both", 1, 1, "off", 1, "uint8"),
    (1, 1, 1, "otsu", 1, "area", 1, 1, "distance", 1, "uint8"),
    (1, 1, 1, "fixed", 1, "open", 1, 1, "distance", 1, "uint8"),
    (1, 1, 1, "local", 1, "both", 1, 0, "distance", 1, "uint8"),
    (1, 1, 1, "noise", 1, "both", 1, 1, "off", 1, "uint8"),
    (1, 1, 1, "fixed", 1, "off", 1, 1, "distance", 1, "uint8"),
]


def options(case, index):
    """(ThresholdSegmenter keyword arguments, shape, dtype) of case number `index`; the shapes go in rotation."""
    c = dict(zip(NAMES, case))
    dtype = np.dtype(c["dtype"]).type
    top = int(np.iinfo(dtype).max)
    shape, tile = SHAPES[index % len(SHAPES)]
    kw = dict(connectivity=c["connectivity"], fill_holes=bool(c["fill"]))
    if c["smooth"]:
        kw["smooth_sigma"] = SIGMA
    if c["correct"]:
        kw["background_radius"] = RADIUS
    if c["denoise"]:
        kw["denoise"] = True
    if c["rule"] == "fixed":
        kw["threshold"] = int(FIXED * top)
        if c["weak"]:
            kw["weak_threshold"] = int(FIXED_WEAK * top)                 # counts
    elif c["rule"] == "otsu":
        if c["weak"]:
            kw["weak_threshold"] = 0.6                                   # a fraction of Otsu's threshold
    elif c["rule"] == "local":
        kw.update(threshold="local", local_radius=LOCAL_RADIUS, local_delta=int(DELTA * top))
        if c["weak"]:
            kw["weak_delta"] = int(DELTA_WEAK * top)
    else:
        kw.update(threshold="noise", noise_tile=tile, noise_k=6.0)
        if c["weak"]:
            kw["weak_k"] = 3.0
    if c["clean"] in ("open", "both"):
        kw["open_radius"] = OPEN_RADIUS
    if c["clean"] in ("area", "both"):
        kw["min_area"] = MIN_AREA
    if c["split"] != "off":
        kw["split_touching"] = True
        if c["split"] == "intensity":
            kw["split_by"] = "intensity"
    if c["expand"]:
        kw["expand_distance"] = EXPAND
    return kw, shape, dtype


def allowed(case) -> bool:
    """Whether the package's own argument checks, which need no device, accept the case."""
    from cellscreen import segment as S
    kw = options(case, 0)[0]
    g = lambda k: kw.get(k, DEFAULTS[k])
    try:
        S._threshold_mode(g("threshold"), g("connectivity"), g("fill_holes"), g("local_radius"), g("local_delta"), g("local_floor"),
                          g("background_radius"), g("denoise"), g("smooth_sigma"))
        if S._noise_mode(g("threshold"), g("connectivity"), g("noise_k"), g("noise_tile"), g("noise_floor"), g("weak_k"),
                         g("weak_threshold"), g("weak_delta")) is None:
            S.hysteresis_params(g("threshold"), g("weak_threshold"), g("weak_delta"), g("local_delta"))
        S.smooth_params(g("smooth_sigma"), g("denoise"))
        S.split_params(g("split_touching"), g("split_h"))
        S.split_intensity_params(g("split_touching"), g("split_by"), g("split_h"), g("split_depth"), g("split_contrast"))
        S.clean_params(g("open_radius"), g("open_connectivity"), g("min_area"))
    except (ValueError, TypeError):
        return False
    return True


def pairs_of(case):
    return {((a, case[a]), (b, case[b])) for a, b in itertools.combinations(range(len(case)), 2)}


def all_allowed_pairs():
    """Every pair of levels of two factors that at least one allowed combination holds."""
    found = set()
    for case in itertools.product(*(levels for _, levels in FACTORS)):
        if allowed(case):
            found |= pairs_of(case)
    return found


def full_chains():
    """One case per rule with every stage on; connectivity, the kind of split and the pixel type alternate."""
    turn = lambda k, pair: pair[((k + 1) // 2) % 2]
    return [(1, 1, 1, rule, 1, "both", 1 + k % 2, 1, turn(k, ("intensity", "distance")), 1, turn(k, ("uint16", "uint8")))
            for k, rule in enumerate(FACTORS[3][1])]


def stages_on(case) -> int:
    """How many stages of a case do something: the chain's length."""
    c = dict(zip(NAMES, case))
    return (c["smooth"] + c["correct"] + c["denoise"] + c["weak"] + c["fill"] + c["expand"] + (c["clean"] != "off") + (c["clean"] == "both") +
            (c["split"] != "off"))


def generate():
    """The full chains, then a greedy cover: again and again the allowed combination that holds the most pairs not yet covered,
    among equals the longest chain, and among those the first in the order of itertools.product."""
    cases = full_chains()
    todo = all_allowed_pairs()
    for c in cases:
        todo -= pairs_of(c)
    pool = [c for c in itertools.product(*(levels for _, levels in FACTORS)) if allowed(c)]
    while todo:
        best = max(pool, key=lambda c: (len(pairs_of(c) & todo), stages_on(c)))          # max keeps the first of equals
        cases.append(best)
        todo -= pairs_of(best)
    return cases
