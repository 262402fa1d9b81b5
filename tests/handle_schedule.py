"""Who calls what on one shared preprocess handle, in which order and with which input: the schedule of
tests/test_gpu_shared_handle.py, and the CPU restatement of every call in it.  Nothing here touches a device.

  ACTORS     the tools that share one SegmentState: two split segmenters (the second with smoothing and background correction, so
             that the median, smoothing and top-hat planes are dirty too), the label expander, the eight measurers, the matcher,
             the cell extractor, the propagator, the spot detector and the image quality and focus records, each with cheap but
             non-default parameters
  circuit    an Eulerian circuit of the complete directed graph on n vertices: n (n - 1) + 1 stops, every ordered pair of
             different vertices adjacent exactly once
  schedule   the circuit on the actors as (actor, input, on_device, exclude) steps; every actor has a counter of its own that
             takes it through the three INPUTS (large, small, medium: a small call lands inside the buffers a large one left, a
             large one forces a free and a new allocation), then numpy / CUDA tensors, then without / with an exclude plane
  inputs_of  the images and labels of one input, from the generators of the tools' own restatements
  expected   the restatement of one (actor, input, exclude), computed once and kept"""
import functools

import numpy as np

import colocalize_reference as CO
import expand_reference as ER
import extract_reference as XR
import granularity_reference as GR
import intensity_reference as IR
import match_reference as MA
import neighbors_reference as NB
import pipeline_reference as P
import propagate_reference as PG
import quality_reference as QY
import quantile_reference as QR
import radial_reference as RR
import shape_reference as SH
import smooth_reference as SM
import spots_reference as SR
import texture_reference as TR

ACTORS = ("split", "split_intensity", "expand", "intensity", "quantiles", "texture", "shape", "neighbors", "colocalize", "radial",
          "granularity", "match", "extract", "propagate", "spots", "quality", "focus")
SEGMENTERS = {"split": dict(split_touching=True, split_h=2, connectivity=2, fill_holes=False),
              "split_intensity": dict(split_touching=True, split_by="intensity", split_depth=24, smooth_sigma=1.0, denoise=True,
                                      background_radius=9)}
HAS_EXCLUDE = ("intensity", "quantiles", "texture", "shape", "colocalize", "radial", "granularity", "spots", "focus")
RANGE_CHECKED = HAS_EXCLUDE + ("neighbors", "match")     # the tools that take a largest label and refuse one above it with status -1
INPUTS = ((2, 130, 520), (1, 33, 67), (1, 64, 256))
DTYPES = (np.uint16, np.uint8, np.uint16)
EXPAND_DISTANCE, QUANTILES, TEXTURE, NEIGHBOR_D2 = 4, ((1, 10), (1, 2)), (2, 8), 25         # TEXTURE: distance, levels
COLOC_THRESHOLD, RADIAL_BINS, GRANULARITY = (20, 50), 3, (4, 2)                             # GRANULARITY: steps, subsample
PROPAGATE = dict(metric="cityblock", lam=2, guide_channel=1)          # and a max_cost per input: inputs_of()["max_cost"]
# the spot detector: a difference of Gaussians of sigma 1 and 1.6 in channel 1 (the plain noise), a window of 7 x 7, the response
# plane asked for, and per input a threshold in counts that cuts into the noise's own peaks
SPOTS = dict(sigma=1.0, min_distance=3, channel=1)
SPOT_THRESHOLDS = (1000.0, 4.0, 1000.0)
QUALITY_TILE = 16                                        # the image quality records: both channels, a mesh, and per input
SAT_LEVELS = ((40000, 3000), (150, 11), (32768, 1))      # a saturation level for either channel that is not the dtype's top


def circuit(n):
    """Vertices 0..n-1 in an order that starts and ends at 0 and walks every edge (a, b), a != b, exactly once: Hierholzer's
    algorithm, taking at every vertex the unused edge to the smallest vertex."""
    if n < 2:
        return [0] * n
    unused = {a: [b for b in range(n - 1, -1, -1) if b != a] for a in range(n)}        # pop() takes the smallest
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def schedule():
    """[(actor, input index, on_device, exclude)]: the circuit, each actor on its own counter."""
    seen, out = dict.fromkeys(ACTORS, 0), []
    for v in circuit(len(ACTORS)):
        a = ACTORS[v]
        c = seen[a]
        seen[a] += 1
        out.append((a, c % 3, bool((c // 3) % 2), bool((c // 6) % 2) and a in HAS_EXCLUDE))
    return out


@functools.lru_cache(maxsize=None)
def inputs_of(k):
    """One input: image [B,H,W,2] of DTYPES[k] (uniform noise, bright on the objects in channel 0), labels int32 [B,H,W] (random
    disks, the images different), exclude int32 [B,H,W] (smaller disks from other seeds), truth (the labels shifted), centres of
    the radial measurer int32 [B,max_label,2], and the largest label; for the propagator seeds (the labels eroded three times by the
    4-neighbourhood: the few pixels of an object three steps inside it, none of a small one), mask (labels > 0 dilated by three
    such steps) and max_cost (about four of the guide's noise steps, so that part of the mask stays unreached)."""
    B, H, W = INPUTS[k]
    dtype = DTYPES[k]
    top = int(np.iinfo(dtype).max)
    labels = np.stack([IR.contents((H, W), 11 * k + b)[0][1] for b in range(B)])
    exclude = np.stack([ER.disks((H, W), max(2, H * W // 300), 50 + 7 * k + b, radii=(1, 3)) for b in range(B)])
    image = IR.noise((B, H, W), 2, dtype, 3 + k, 0, top // 4 + 1)
    image[..., 0] += ((labels > 0) * (top // 2)).astype(dtype)
    truth = np.stack([MA.shifted(x, 1, -2) for x in labels])
    m = int(labels.max())
    rng = np.random.default_rng(90 + k)
    centers = np.stack([rng.integers(0, H, (B, m)), rng.integers(0, W, (B, m))], axis=-1).astype(np.int32)
    seeds = labels
    for _ in range(3):
        seeds = np.where(_all_neighbours(seeds, lambda q, s=seeds: q == s), seeds, 0).astype(np.int32)
    mask = labels > 0
    for _ in range(3):
        mask = ~_all_neighbours(mask, lambda q: ~q)
    mask = mask.astype(np.uint8)
    for a in (image, labels, exclude, truth, centers, seeds, mask):
        a.setflags(write=False)
    return dict(image=image, labels=labels, exclude=exclude, truth=truth, centers=centers, max_label=m,
                plane=np.ascontiguousarray(image[..., 0]), seeds=seeds, mask=mask, max_cost=top // 4 + 1)


def _all_neighbours(a, pred):
    """[B,H,W] bool: pred holds of all four neighbours of a pixel of the stack a; outside the image the plane repeats its edge."""
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)), mode="edge")
    H, W = a.shape[1:]
    return pred(p[:, :H, 1:W + 1]) & pred(p[:, 2:, 1:W + 1]) & pred(p[:, 1:H + 1, :W]) & pred(p[:, 1:H + 1, 2:])


@functools.lru_cache(maxsize=None)
def expected(actor, k, exclude=False):
    """The integer tables of one call, as tuples in the order the tool returns them (test_gpu_shared_handle.call)."""
    x = inputs_of(k)
    image, labels, ex = x["image"], x["labels"], (x["exclude"] if exclude else None)
    if actor in SEGMENTERS:
        return P.segment_batch(x["plane"], return_distance=True, **SEGMENTERS[actor])[:4]
    if actor == "expand":
        out = [P.expand_windows(lab, ER.max_d2_of(EXPAND_DISTANCE)) for lab in labels]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    if actor == "intensity":
        return IR.measure(image, labels, ex)
    if actor == "quantiles":
        return QR.measure(image, labels, QUANTILES, True, ex)
    if actor == "texture":
        c, marg, sumsq, _, glcm = TR.measure(image, labels, TEXTURE[0], TEXTURE[1], TR.full_range(image.dtype.type, 2), ex, None, True)
        return c, marg, sumsq, glcm                       # clogc is a float64: the integers are what this schedule compares
    if actor == "shape":
        return SH.measure(labels, ex, None, True)
    if actor == "neighbors":
        return NB.measure(labels, NEIGHBOR_D2)
    if actor == "colocalize":
        return CO.measure(image, labels, ex, None, COLOC_THRESHOLD, None, True)
    if actor == "radial":
        return RR.measure(image, labels, ex, None, RADIAL_BINS, x["centers"])[:4]
    if actor == "granularity":
        return GR.measure(image, labels, ex, GRANULARITY[0], GRANULARITY[1], False)[:3]
    if actor == "match":
        return MA.tables(labels, x["truth"], x["max_label"], max(1, int(x["truth"].max())))
    if actor == "extract":
        status, rows = [], []
        for b in range(labels.shape[0]):
            _, regs, st = XR.extract(labels[b], x["plane"][b], None)
            status.append(st)
            rows += [(b,) + tuple(int(r[f]) for f in EXTRACT_FIELDS) for r in regs]
        return np.array(status, np.int32), np.array(rows, np.int64).reshape(len(rows), 1 + len(EXTRACT_FIELDS))
    if actor == "propagate":
        return PG.propagate(x["seeds"], x["mask"], image, max_cost=x["max_cost"], **PROPAGATE)
    if actor == "spots":                                 # counts, offsets, the list, geom, records, the response
        w_a, w_b = SM.smooth_weights(SPOTS["sigma"]), SM.smooth_weights(SPOTS["sigma"] * 1.6)
        T = int(round(256 * SPOT_THRESHOLDS[k]))
        return SR.detect(image, [T] * image.shape[0], w_a, w_b, SPOTS["min_distance"], SPOTS["channel"], labels, ex, x["max_label"])
    if actor == "quality":
        return QY.measure_image(image, QUALITY_TILE, SAT_LEVELS[k])
    if actor == "focus":
        return QY.measure_objects(image, labels, ex, x["max_label"])
    raise KeyError(actor)


EXTRACT_FIELDS = ("label", "minr", "minc", "maxr", "maxc", "area", "convex_area", "failed")
