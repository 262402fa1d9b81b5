"""The label tools and the segmenter at the caps they accept: the caps read out of the sources, one entry per tool, four families
of scenes and the segmenter's cases, with the CPU restatement of every scene.  Nothing here touches a device;
tests/test_label_caps_cpu.py holds this file to the sources and to itself, tests/test_gpu_label_caps.py runs the scenes.

  CAPS       every limit the entry points on the preprocess handle publish, by its name in csrc/ (read_caps: a regex per file)
  TOOLS      per tool: its entry point, the caps that bind it, its cheapest legal parameters, how many cells one (image, label)
             row costs under them (`factor`), and its restatement from the tool's own *_reference.py
  FAMILIES   batch   kMaxBatch images of 8 x 8 from at most 24 prototypes, ids <= 8: grid.y / grid.z = 65535 and the bases
                     b * max_label and b * H * W of the last image
             labels  two images of 40 x 300 with max_label = kMaxLabel and the ids 1, 2, 1000, kMaxLabel - 1, kMaxLabel
             rows    the tool's own row, cell or byte cap met exactly: 4096 images of 16 x 16 from prototypes, max_label = cap /
                     (4096 * factor); four images with max_label = kMaxLabel where factor is 1 ("rows4"); and the byte caps of the
                     ring table, the granularity sums and the colocalization rank tables under the parameters that reach them
             sides   (1, 4096), (4096, 1), (3, 4096) and (4096, 3), two images each
             The three tools that are no cs_label_* add their own caps to `rows`: the spot list's (spots-list: 4096 images of
             64 x 64 with 1024 spots and 1024 objects each, 2^22 of either) and the response scratch's (scratch: 21845 images of
             64 x 64), the focus cells with four channels (rows-channels) and the mesh's (tiles: 32768 images of 17 x 49 x 4
             under a 2 x 4 mesh); the image quality records take no labels, so their scenes hold an image alone.
             A family is a function from a tool's name to a list of scenes, or to a reason string where the tool has no such scene.
  expected   the restatement of a scene: directly, or of its prototypes gathered by the scene's index map
  SEGMENT_CASES, segment_scene, segment_expected    cs_segment_* at kMaxBatch images of 8 x 8, the same way

A scene is a dict: name, the tool's inputs (image, labels, max_label; truth and max_truth for the matcher; seeds, mask and guide for
the propagator), params (the tool's parameters where the scene changes them), cap (the cap it sits on), and for a gathered scene
protos (the scene of its prototypes), index (the prototype of every image) and batch in place of the planes, which full() spreads."""
import functools
import os
import re

import numpy as np

import colocalize_reference as CO
import expand_reference as ER
import granularity_reference as GR
import handle_schedule as HS
import helpers as H
import intensity_reference as IR
import match_reference as MA
import neighbors_reference as NB
import pipeline_reference as P
import propagate_reference as PG
import quantile_reference as QR
import radial_reference as RR
import quality_reference as QY
import shape_reference as SH
import smooth_reference as SM
import spots_reference as SR
import texture_reference as TR

CSRC = os.path.join(H.ROOT, "cell-image-analysis_amd", "csrc")
PKG = os.path.join(H.ROOT, "cell-image-analysis_amd", "cellscreen")

# name -> (file, the C++ type it is declared with)
CAP_SOURCES = {"kMaxSide": ("stage_host.hpp", "int"), "kMaxBatch": ("stage_host.hpp", "int"), "kMaxLabel": ("stage_host.hpp", "int"),
               "kLiMaxCells": ("intensity.hip", "int64_t"), "kLqMaxCells": ("quantile.hip", "int64_t"),
               "kShMaxRows": ("shape.hip", "int64_t"), "kNbMaxRows": ("neighbors.hip", "int64_t"),
               "kLcMaxCells": ("colocalize.hip", "int64_t"), "kLrMaxCells": ("radial.hip", "int64_t"),
               "kGrMaxCells": ("granularity.hip", "int64_t"), "kLmMaxRows": ("match.hip", "int64_t"),
               "kTxMaxCells": ("texture.hip", "int64_t"), "kLrMaxRing": ("radial.hip", "size_t"),
               "kGrMaxBytes": ("granularity.hip", "size_t"), "kLcMaxScratch": ("colocalize.hip", "size_t"),
               "kPgMaxBytes": ("propagate.hip", "size_t"), "LC_LEVELS": ("colocalize.hip", "int"),
               "kSdMaxRows": ("spots.hip", "int64_t"), "kSdMaxSpots": ("spots.hip", "int64_t"), "kSdMaxScratch": ("spots.hip", "size_t"),
               "kIqMaxTiles": ("quality.hip", "int64_t"), "kLfMaxCells": ("quality.hip", "int64_t"), "kIqMaxChannels": ("quality.hip", "int")}


def read_caps():
    """{name: value}: `static constexpr <type> <name> = <a literal or a shift>;` as the sources declare it."""
    out, text = {}, {}
    for name, (fname, ctype) in CAP_SOURCES.items():
        if fname not in text:
            with open(os.path.join(CSRC, fname)) as f:
                text[fname] = f.read()
        m = re.search(rf"static constexpr {ctype} {name} = (?:\(size_t\))?(\d+)(?: << (\d+))?;", text[fname])
        assert m, f"{name} is not declared in {fname} as the suite reads it"
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def read_python_limits():
    """MAX_SIDE, MAX_BATCH and MAX_LABEL of cellscreen/_labels.py, read as text: no device library is loaded here."""
    with open(os.path.join(PKG, "_labels.py")) as f:
        text = f.read()
    out = {}
    for name in ("MAX_SIDE", "MAX_BATCH", "MAX_LABEL"):
        m = re.search(rf"^{name} = (\d+)(?: << (\d+))?\b", text, re.M)
        assert m, name
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def read_tool_limits():
    """The limits cellscreen/spots.py and cellscreen/quality.py repeat for their own argument checks, read as text."""
    out = {}
    for fname, names in (("spots.py", ("MAX_ROWS", "MAX_SPOTS", "MAX_SCRATCH")), ("quality.py", ("MAX_TILES", "MAX_CHANNELS"))):
        with open(os.path.join(PKG, fname)) as f:
            text = f.read()
        for name in names:
            m = re.search(rf"^{name} = (\d+)(?: << (\d+))?\b", text, re.M)
            assert m, (fname, name)
            out[fname[:-3], name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def defined_entry_points():
    """{name: body}: every `int cs_*(...)` csrc/*.hip defines at file scope, with its text up to the closing brace in column 0."""
    out = {}
    for fname in sorted(os.listdir(CSRC)):
        if not fname.endswith(".hip"):
            continue
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        lines = text.split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"int (cs_\w+)\(", line)
            if not m:
                continue
            j = i
            while not (lines[j].startswith("}") or (j == i and "{" in line and line.rstrip().endswith("}"))):    # or a one-line body
                j += 1
            out[m.group(1)] = "\n".join(lines[i:j + 1])
    return out


def declared_entry_points():
    """The entry points of cellscreen/_lib.py that run a batch on the preprocess handle: the tools themselves.  A name alone does
    not say so (cs_image_quality, cs_object_focus and cs_spot_detect are no cs_label_*), so the rule reads the definitions: every
    declared entry point whose definition under csrc/ calls state_begin(, the door to the SegmentState the tools share, and every
    cs_label_* that is neither a *_last_* reader nor the pair list's copy (the matcher keeps a state of its own and never calls
    state_begin).  Left out on purpose: the cs_segment_* stages, which SEGMENT_CASES covers."""
    with open(os.path.join(PKG, "_lib.py")) as f:
        names = re.findall(r'^\s*"(cs_\w+)":', f.read(), re.M)
    body = defined_entry_points()
    other = {n for n in names if n.endswith("_free")} | {"cs_status_string", "cs_last_error", "cs_profile_kernel_name"}   # no int
    assert set(names) - other <= set(body), sorted(set(names) - other - set(body))             # the rule has read every definition
    label = {n for n in names if n.startswith("cs_label_") and "_last_" not in n and n != "cs_label_neighbors_pairs"}
    state = {n for n in names if n in body and "state_begin(" in body[n]}
    return sorted(n for n in label | state if not n.startswith("cs_segment_"))


CAPS = read_caps()
MAX_SIDE, MAX_BATCH, MAX_LABEL = CAPS["kMaxSide"], CAPS["kMaxBatch"], CAPS["kMaxLabel"]
LC_SCRATCH_PER = 3 * CAPS["LC_LEVELS"]                   # colocalize.hip, kLcScratchPer: bytes per image and channel with rwc

# ---- the tools -----------------------------------------------------------------------------------------------------------------
EXPAND_DISTANCE, NEIGHBOR_D2, TEXTURE_LEVELS = 2, 1, 8
PROPAGATE = dict(metric="cityblock", lam=1, guide_channel=0)


def _restate_expand(x, p):
    return ER.expand(x["labels"], ER.max_d2_of(EXPAND_DISTANCE))


def _restate_intensity(x, p):
    return IR.measure(x["image"], x["labels"], None, x["max_label"])


def _restate_quantiles(x, p):
    return QR.measure(x["image"], x["labels"], p["quantiles"], False, None, x["max_label"])[:2]


SPARSE_ABOVE = 4096


def _restate_texture(x, p):
    """texture_reference.measure builds one matrix per table row and direction, which at kMaxLabel rows costs seconds and half a
    gigabyte a time.  An object's records depend on its own pixels alone, never on its id, so above SPARSE_ABOVE rows the ids that
    occur are renumbered 1..n, measured, and the n rows put where the ids say into tables of zeros: the encoding of an absent
    object.  tests/test_label_caps_cpu.py holds this to the direct form."""
    img, lab, M = x["image"], x["labels"], x["max_label"]
    ranges = TR.full_range(img.dtype.type, 1 if img.ndim == 3 else img.shape[3])
    ids = np.unique(lab)
    ids = ids[ids > 0]
    if M <= SPARSE_ABOVE or not len(ids):
        return TR.measure(img, lab, p["distance"], p["levels"], ranges, None, M, False)[:4]
    dense = np.where(lab > 0, np.searchsorted(ids, lab) + 1, 0).astype(np.int32)
    small = TR.measure(img, dense, p["distance"], p["levels"], ranges, None, len(ids), False)[:4]
    out = []
    for t in small:
        full = np.zeros((t.shape[0], M) + t.shape[2:], t.dtype)
        full[:, ids - 1] = t
        out.append(full)
    return tuple(out)


def _restate_shape(x, p):
    return SH.measure(x["labels"], None, x["max_label"], False)[:4]


def _restate_neighbors(x, p):
    return NB.measure(x["labels"], NEIGHBOR_D2, x["max_label"])


def _restate_colocalize(x, p):
    return CO.measure(x["image"], x["labels"], None, x["max_label"], p["threshold"], None, p["rwc"])


def _restate_radial(x, p):
    return RR.measure(x["image"], x["labels"], None, x["max_label"], p["bins"], None)[:4]


def _restate_granularity(x, p):
    return GR.measure(x["image"], x["labels"], None, p["steps"], p["subsample"], False, x["max_label"])[:3]


def _restate_propagate(x, p):
    return PG.propagate(x["seeds"], x["mask"], x["guide"], p["guide_channel"], p["metric"], p["lam"])


def _restate_match(x, p):
    return MA.tables(x["labels"], x["truth"], x["max_label"], x["max_truth"])


SPOTS = dict(sigma=0, sigma_coarse=1.0, min_distance=1, threshold=1.0)        # the identity against sigma 1: radii 0 and 4
SPOTS_WIDE = dict(sigma=15.9, sigma_coarse=16.1, min_distance=8, threshold=1.0)            # both radii 64, the widest window


def spot_tables(p):
    """(w_a, w_b, m, T) of a spots scene's parameters as spots_reference takes them: cellscreen.spots.spot_params builds the same
    tables from the same sigmas (tests/test_label_caps_cpu.py holds them together); T in 1/256 counts."""
    w_a = None if p["sigma"] == 0 else SM.smooth_weights(p["sigma"])
    return w_a, SM.smooth_weights(p["sigma_coarse"]), p["min_distance"], int(round(256 * p["threshold"]))


def _restate_spots(x, p):
    """counts, offsets, the list, geom, records (both None without labels) and the response, which is always asked for."""
    w_a, w_b, m, T = spot_tables(p)
    lab = x.get("labels")
    out = SR.detect(x["image"], [T] * len(x["image"]), w_a, w_b, m, 0, lab, None, x["max_label"] if lab is not None else None)
    return tuple(t for t in out if t is not None)


def _restate_focus(x, p):
    return QY.measure_objects(x["image"], x["labels"], None, x["max_label"])


def _restate_quality(x, p):
    """records and, with a mesh, the mesh."""
    return tuple(t for t in QY.measure_image(x["image"], p["tile"], p["sat_level"]) if t is not None)


# entry: the C entry point; caps: what binds it besides kMaxSide and kMaxBatch; channels: of its cheapest image (0: it takes none);
# factor: cells of the row cap per (image, label) under params; float_outputs: the indices of what is compared with a bound
TOOLS = {
    "expand": dict(entry="cs_label_expand", caps=(), channels=0, factor=0, params=dict(distance=EXPAND_DISTANCE), restate=_restate_expand),
    "intensity": dict(entry="cs_label_intensity", caps=("kMaxLabel", "kLiMaxCells"), channels=1, factor=1, params={},
                      restate=_restate_intensity),
    "quantiles": dict(entry="cs_label_quantiles", caps=("kMaxLabel", "kLqMaxCells"), channels=1, factor=1,
                      params=dict(quantiles=((1, 2),), mad=False), restate=_restate_quantiles),
    "texture": dict(entry="cs_label_texture", caps=("kMaxLabel", "kTxMaxCells"), channels=1, factor=TEXTURE_LEVELS,
                    params=dict(distance=1, levels=TEXTURE_LEVELS, glcm=False), restate=_restate_texture, float_outputs=(3,)),
    "shape": dict(entry="cs_label_shape", caps=("kMaxLabel", "kShMaxRows"), channels=0, factor=1, params=dict(hull=False),
                  restate=_restate_shape),
    "neighbors": dict(entry="cs_label_neighbors", caps=("kMaxLabel", "kNbMaxRows"), channels=0, factor=1, params=dict(distance=1.0),
                      restate=_restate_neighbors),
    "colocalize": dict(entry="cs_label_colocalize", caps=("kMaxLabel", "kLcMaxCells", "kLcMaxScratch"), channels=2, factor=2,
                       params=dict(threshold=(15, 100), rwc=False), restate=_restate_colocalize),
    "radial": dict(entry="cs_label_radial", caps=("kMaxLabel", "kLrMaxCells", "kLrMaxRing"), channels=1, factor=1, params=dict(bins=1),
                   restate=_restate_radial),
    "granularity": dict(entry="cs_label_granularity", caps=("kMaxLabel", "kGrMaxCells", "kGrMaxBytes"), channels=1, factor=1,
                        params=dict(steps=1, subsample=1), restate=_restate_granularity),
    "propagate": dict(entry="cs_label_propagate", caps=("kPgMaxBytes",), channels=1, factor=0, params=dict(PROPAGATE),
                      restate=_restate_propagate),
    "match": dict(entry="cs_label_match", caps=("kMaxLabel", "kLmMaxRows"), channels=0, factor=1, params={}, restate=_restate_match),
    # cs_spot_detect with cs_spot_fill behind it: one tool.  cs_image_quality takes no labels: its scenes hold an image alone.
    "spots": dict(entry="cs_spot_detect", caps=("kMaxLabel", "kSdMaxRows", "kSdMaxSpots", "kSdMaxScratch"), channels=1, factor=1,
                  params=dict(SPOTS), restate=_restate_spots),
    "focus": dict(entry="cs_object_focus", caps=("kMaxLabel", "kLfMaxCells", "kIqMaxChannels"), channels=1, factor=1, params={},
                  restate=_restate_focus),
    "quality": dict(entry="cs_image_quality", caps=("kIqMaxTiles", "kIqMaxChannels"), channels=1, factor=0,
                    params=dict(tile=0, sat_level=None), restate=_restate_quality),
}
ROW_CAP = {"intensity": "kLiMaxCells", "quantiles": "kLqMaxCells", "texture": "kTxMaxCells", "shape": "kShMaxRows",
           "neighbors": "kNbMaxRows", "colocalize": "kLcMaxCells", "radial": "kLrMaxCells", "granularity": "kGrMaxCells",
           "match": "kLmMaxRows", "spots": "kSdMaxRows", "focus": "kLfMaxCells"}
NO_TABLE = "no max_label table: its outputs are planes of the image's size"
NO_CAP = "no cap of its own: the image limits are all that binds it, and the batch and sides families sit on those"
NO_LABELS = "takes no labels: its records are per image, channel and mesh tile"
LABEL_FREE = ("quality",)                                # the tools whose scenes are images without labels


def _frozen(x):
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def _pixels(tool, shape, seed):
    """The image a tool measures on labels of `shape` [B,H,W]: uint16 noise, [B,H,W] for one channel and [B,H,W,C] above."""
    c = TOOLS[tool]["channels"]
    if c == 0:
        return None
    img = IR.noise(shape, c, np.uint16, seed)
    return np.ascontiguousarray(img[..., 0]) if c == 1 else img


def _scene(tool, name, labels, max_label, seed, cap, **more):
    """The inputs of `tool` on a label stack: what each tool needs besides the labels is made from them."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    x = dict(name=name, tool=tool, labels=labels, max_label=int(max_label), image=_pixels(tool, labels.shape, seed), cap=cap,
             params=dict(TOOLS[tool]["params"]))
    if tool == "match":
        x["truth"] = np.ascontiguousarray(labels[:, :, ::-1])                 # mirrored: same ids, other overlaps
        x["max_truth"] = int(max_label)
    x.update(more)
    return _frozen(x)


def _image_scene(tool, name, image, cap, **params):
    """The scene of a tool that takes no labels: an image stack and the parameters that differ from the tool's cheapest."""
    return _frozen(dict(name=name, tool=tool, image=np.ascontiguousarray(image), cap=cap, params=dict(TOOLS[tool]["params"], **params)))


def planes_of(x):
    """The stack a scene is made on, with all its images: the image of a tool without labels, the propagator's seeds, else the
    labels."""
    return full(x)["image" if x["tool"] in LABEL_FREE else "seeds" if x["tool"] == "propagate" else "labels"]


def _gathered(protos, index, name, cap):
    """The scene of len(index) images whose image b is prototype index[b] of the scene `protos`.  It holds the prototypes and the
    map only; full() spreads them, so that listing the scenes costs nothing."""
    x = {k: a for k, a in protos.items() if not isinstance(a, np.ndarray)}
    x.update(name=name, cap=cap, protos=protos, index=index, batch=len(index))
    return _frozen(x)


def full(x, lo=None, hi=None):
    """A scene with all its planes: itself, or for a gathered scene the prototypes' planes spread by the index map; lo, hi: the
    images lo..hi-1 only, as a scene of their own without a gather."""
    if "index" not in x:
        if lo is None:
            return x
        return {k: (a[lo:hi] if isinstance(a, np.ndarray) else a) for k, a in x.items()}
    index = x["index"] if lo is None else x["index"][lo:hi]
    y = {k: a for k, a in x.items() if k not in ("index", "protos", "batch")}
    y.update({k: a[index] for k, a in x["protos"].items() if isinstance(a, np.ndarray)})
    return y


def index_map(batch, n_protos, last, seed):
    """The prototype of every image: drawn from a seeded generator, so periodic with no period; the first and the last image
    are prototype `last`, a non-empty one."""
    p = np.random.default_rng(seed).integers(0, n_protos, batch)
    p[0] = p[-1] = last
    return p


# ---- batch ----------------------------------------------------------------------------------------------------------------------
BATCH_SIDE, BATCH_MAX_LABEL, BATCH_VARIANTS = 8, 8, 5
BATCH_KINDS = 4                                          # empty, corners, touching blocks, covered


def batch_label_kinds():
    k = np.zeros((BATCH_KINDS, BATCH_SIDE, BATCH_SIDE), np.int32)
    k[1, 0, 0], k[1, 7, 7] = 1, BATCH_MAX_LABEL
    k[2, 2:5, 1:4], k[2, 2:6, 4:7] = 3, 4
    k[3] = 6
    return k


def _propagate_planes(labels, seed):
    """(mask, guide) of the propagator on seeds `labels` [P,h,w]: three pixels in four open, a noise guide."""
    rng = np.random.default_rng(seed)
    mask = (rng.integers(0, 4, labels.shape) > 0).astype(np.uint8)
    guide = rng.integers(0, 4000, labels.shape).astype(np.uint16)
    return mask, guide


def batch_protos(tool):
    """The 20 prototypes of a tool: prototype kind * BATCH_VARIANTS + variant, the variants differing in the pixels."""
    labs = np.repeat(batch_label_kinds(), BATCH_VARIANTS, axis=0)
    if tool == "propagate":
        mask, guide = _propagate_planes(labs, 11)
        return _frozen(dict(name="batch prototypes", tool=tool, seeds=labs, mask=mask, guide=guide, params=dict(PROPAGATE), cap=None))
    return _scene(tool, "batch prototypes", labs, BATCH_MAX_LABEL, 12, None)


def family_batch(tool):
    index = index_map(MAX_BATCH, BATCH_KINDS * BATCH_VARIANTS, 2 * BATCH_VARIANTS + 4, 21)
    if tool == "quality":                                # one channel, and the most there are: iq_close then runs 4 * 65535 workgroups
        n, top = BATCH_KINDS * BATCH_VARIANTS, CAPS["kIqMaxChannels"]
        one = _image_scene(tool, "batch prototypes", QY.noise((n, BATCH_SIDE, BATCH_SIDE), 1, np.uint16, 13)[..., 0], None)
        many = _image_scene(tool, "batch prototypes", QY.noise((n, BATCH_SIDE, BATCH_SIDE), top, np.uint16, 14), None)
        return [_gathered(one, index, "batch", "kMaxBatch"), _gathered(many, index, "batch-channels", "kIqMaxChannels")]
    return [_gathered(batch_protos(tool), index, "batch", "kMaxBatch")]


# ---- labels ---------------------------------------------------------------------------------------------------------------------
LABELS_SHAPE = (2, 40, 300)


def labels_planes(top):
    lab = np.zeros(LABELS_SHAPE, np.int32)
    lab[0, 3:9, 5:11], lab[0, 3:9, 11:20] = 1, 2                              # 1 and 2 touch
    lab[0, 20:25, 100:140] = 1000
    lab[0, 30:40, 280:290], lab[0, 30:40, 290:300] = top - 1, top             # the two largest touch, in the last corner
    lab[1, :, 0] = top                                                         # a strip down column 0
    lab[1, 10:30, 150:170] = 2
    return lab


def bright_inside(image, labels):
    """A copy of image [B,H,W] with the dtype's top at one pixel of every object: the middle one of its pixels in raster order."""
    out = image.copy()
    for b in range(len(labels)):
        for i in np.unique(labels[b]):
            if i > 0:
                at = np.argwhere(labels[b] == i)
                out[(b,) + tuple(at[len(at) // 2])] = np.iinfo(out.dtype).max
    return out


def family_labels(tool):
    if tool in ("expand", "propagate"):
        return NO_TABLE
    if tool in LABEL_FREE:
        return NO_LABELS
    lab = labels_planes(MAX_LABEL)
    if tool == "spots":                                  # a spot inside every object: the records of the largest labels are not empty
        return [_scene(tool, "labels", lab, MAX_LABEL, 31, "kMaxLabel", image=bright_inside(_pixels(tool, lab.shape, 31), lab))]
    return [_scene(tool, "labels", lab, MAX_LABEL, 31, "kMaxLabel")]


# ---- rows -----------------------------------------------------------------------------------------------------------------------
ROWS_SIDE, ROWS_BATCH, ROWS_VARIANTS, ROWS_KINDS = 16, 4096, 3, 4
PG_ROWS_SIDE = 64                                       # the propagator's: kPgMaxBytes / 8 pixels as 32768 images of 64 x 64


def rows_label_kinds(top):
    """Four 16 x 16 planes with sparse ids that include 1 and top."""
    k = np.zeros((ROWS_KINDS, ROWS_SIDE, ROWS_SIDE), np.int32)
    k[1, 0, 0], k[1, 15, 15] = 1, top
    k[2, 1:5, 1:6], k[2, 1:5, 6:9], k[2, 9:14, 3:8], k[2, 9:14, 8:15] = 1, 2, top - 1, top
    k[3, :, :7], k[3, 4:9, 10:14] = top, max(1, top // 2)
    return k


def rows4_planes(top):
    k = rows_label_kinds(top)
    return k[[2, 0, 3, 1]]                                                    # the last image holds `top` in the last pixel


LIST_SIDE, LIST_BATCH, LIST_VARIANTS = 64, 4096, 6       # the spot list's cap: 4096 images of 64 x 64 with 1024 spots each
SCRATCH_SIDE = 64                                        # the response scratch's cap: images of 64 x 64, 12 bytes a pixel
TILES_SHAPE, TILES_TILE, TILES_VARIANTS = (17, 49), 16, 8                 # the mesh cap: a 2 x 4 mesh off the pixel grid


def spots_list_protos():
    """uint8 [6,64,64]: noise below 40 with 200 more on the (even, even) lattice, and labels that give every 2 x 2 block an id of
    its own, 1..1024.  Under SPOTS every lattice pixel is a spot and nothing else is: 1024 spots an image, one in each object."""
    n, s = LIST_VARIANTS, LIST_SIDE
    img = np.random.default_rng(51).integers(0, 40, (n, s, s)).astype(np.uint8)
    img[:, ::2, ::2] += 200
    rr, cc = np.mgrid[0:s, 0:s]
    lab = np.broadcast_to(((rr // 2) * (s // 2) + cc // 2 + 1).astype(np.int32), (n, s, s))
    return _scene("spots", "spots-list prototypes", lab, (s // 2) ** 2, 0, None, image=img)


def spots_list_index():
    return index_map(LIST_BATCH, LIST_VARIANTS, 4, 52)


def spots_over_the_list():
    """The images of the spots-list scene and one more with a single bright pixel, without labels: 2^22 + 1 spots, which
    cs_spot_detect refuses once it has counted them."""
    protos = spots_list_protos()
    one = np.zeros((1, LIST_SIDE, LIST_SIDE), np.uint8)
    one[0, 33, 21] = 250
    return _frozen(dict(name="spots-list + 1", tool="spots", image=np.concatenate([protos["image"][spots_list_index()], one]),
                        params=dict(SPOTS), cap="kSdMaxSpots"))


def scratch_batch():
    """The most images of 64 x 64 cs_spot_detect takes: 12 bytes of scratch a pixel stay under kSdMaxScratch."""
    return (CAPS["kSdMaxScratch"] - 1) // (12 * SCRATCH_SIDE * SCRATCH_SIDE)


def spots_scratch_protos():
    """uint16 [6,64,64]: flat planes with no, two, five, one, sixteen and two equal adjacent bright pixels, and a few objects."""
    s = SCRATCH_SIDE
    img = np.full((6, s, s), 300, np.uint16)
    img[1, 0, 0] = img[1, s - 1, s - 1] = 9000
    for r, c, v in ((5, 7, 4000), (20, 40, 8000), (33, 33, 700), (50, 3, 65535), (63, 30, 5000)):
        img[2, r, c] = v
    img[3, 31, 32] = 2000
    img[4, 40, ::4] = 3000
    img[5, 10, 10] = img[5, 10, 11] = 6000
    lab = np.zeros((6, s, s), np.int32)
    lab[1, :4, :4], lab[1, 60:, 60:] = 1, 8
    lab[2, 0:10, 0:20], lab[2, 15:25, 30:50], lab[2, 45:55, 0:8] = 2, 3, 8
    lab[3] = 5
    lab[4, 38:43, 0:32], lab[4, 38:43, 32:64] = 6, 7
    lab[5, 5:15, 5:11], lab[5, 5:15, 11:20] = 1, 2
    return _scene("spots", "scratch prototypes", lab, 8, 0, None, image=img)


def family_rows(tool):
    t = TOOLS[tool]
    if tool == "expand":
        return NO_CAP
    if tool == "quality":                                # its own cap is the mesh's: batch * channels * mesh tiles
        C = CAPS["kIqMaxChannels"]
        m_r, m_c = QY.mesh_dims(*TILES_SHAPE, TILES_TILE)
        B = CAPS["kIqMaxTiles"] // (C * m_r * m_c)
        assert B * C * m_r * m_c == CAPS["kIqMaxTiles"] and B <= MAX_BATCH and (m_r, m_c) == (2, 4)
        assert TILES_SHAPE[0] % m_r and TILES_SHAPE[1] % m_c              # the mesh lies off the pixel grid
        protos = _image_scene(tool, "tiles prototypes", QY.noise((TILES_VARIANTS,) + TILES_SHAPE, C, np.uint8, 53), None, tile=TILES_TILE)
        return [_gathered(protos, index_map(B, TILES_VARIANTS, 3, 54), "tiles", "kIqMaxTiles")]
    if tool == "propagate":
        B = CAPS["kPgMaxBytes"] // 8 // (PG_ROWS_SIDE * PG_ROWS_SIDE)
        assert B * PG_ROWS_SIDE * PG_ROWS_SIDE * 8 == CAPS["kPgMaxBytes"] and B <= MAX_BATCH
        seeds = np.zeros((6, PG_ROWS_SIDE, PG_ROWS_SIDE), np.int32)
        seeds[1, 0, 0], seeds[1, 63, 63] = 1, MAX_LABEL
        seeds[2, 30:33, 10:13], seeds[2, 5, 60] = 7, 9
        seeds[3, ::9, ::11] = np.arange(1, 8 * 6 + 1, dtype=np.int32).reshape(8, 6)
        seeds[4, 63, 0] = 5
        seeds[5] = 3
        mask, _ = _propagate_planes(seeds, 41)
        protos = _frozen(dict(name="rows prototypes", tool=tool, seeds=seeds, mask=mask, guide=None, params=dict(PROPAGATE), cap=None))
        return [_gathered(protos, index_map(B, 6, 1, 42), "rows", "kPgMaxBytes")]
    cap = CAPS[ROW_CAP[tool]]
    top = cap // (ROWS_BATCH * t["factor"])
    assert ROWS_BATCH * top * t["factor"] == cap and 4 <= top <= MAX_LABEL, (tool, top)
    protos = _scene(tool, "rows prototypes", np.repeat(rows_label_kinds(top), ROWS_VARIANTS, axis=0), top, 43, None)
    index = index_map(ROWS_BATCH, ROWS_KINDS * ROWS_VARIANTS, 2 * ROWS_VARIANTS + 2, 44)         # touching blocks first and last
    out = [_gathered(protos, index, "rows", ROW_CAP[tool])]
    if t["factor"] == 1:                                 # the same cap as four images of kMaxLabel labels
        assert 4 * MAX_LABEL == cap
        out.append(_scene(tool, "rows4", rows4_planes(MAX_LABEL), MAX_LABEL, 45, ROW_CAP[tool]))
    # two byte caps that the cheapest parameters stay under are met by dearer ones, at the cell cap as well: two rings make the
    # ring table kLrMaxRing bytes, 31 steps make the sums table kGrMaxBytes
    for name, key, value, bytes_per_row, cap_name in (("radial", "bins", 2, 8 * 2 * 8 * 2, "kLrMaxRing"),
                                                      ("granularity", "steps", 31, 32 * 8, "kGrMaxBytes")):
        if tool == name:
            assert ROWS_BATCH * top * bytes_per_row == CAPS[cap_name]
            dear = dict(protos, params=dict(t["params"], **{key: value}))
            out.append(_gathered(_frozen(dear), index, "rows-bytes", cap_name))
    if tool == "colocalize":                             # with rwc the rank tables bind before the cells do
        B = CAPS["kLcMaxScratch"] // (2 * LC_SCRATCH_PER)
        assert B < ROWS_BATCH and (B + 1) * 2 * LC_SCRATCH_PER > CAPS["kLcMaxScratch"]
        p8 = _scene(tool, "rows prototypes", np.repeat(rows_label_kinds(8), ROWS_VARIANTS, axis=0), 8, 46, None,
                    params=dict(t["params"], rwc=True))
        out.append(_gathered(p8, index_map(B, ROWS_KINDS * ROWS_VARIANTS, 2 * ROWS_VARIANTS + 1, 47), "rows-scratch", "kLcMaxScratch"))
    if tool == "spots":                                  # the list's cap and the scratch's, each met exactly
        lp = spots_list_protos()
        assert LIST_BATCH * lp["max_label"] == CAPS["kSdMaxRows"] and LIST_BATCH * (LIST_SIDE // 2) ** 2 == CAPS["kSdMaxSpots"]
        out.append(_gathered(lp, spots_list_index(), "spots-list", "kSdMaxSpots"))
        B, per = scratch_batch(), 12 * SCRATCH_SIDE * SCRATCH_SIDE
        assert B * per < CAPS["kSdMaxScratch"] <= (B + 1) * per and B <= MAX_BATCH and B * 8 <= CAPS["kSdMaxRows"]
        out.append(_gathered(spots_scratch_protos(), index_map(B, 6, 2, 55), "scratch", "kSdMaxScratch"))
    if tool == "focus":                                  # the cells are rows x channels: the same 4096 images with four channels
        C = CAPS["kIqMaxChannels"]
        top4 = cap // (ROWS_BATCH * C)
        assert ROWS_BATCH * top4 * C == cap and top4 == ROWS_SIDE * ROWS_SIDE
        # a fifth kind: every pixel an object of its own, as many objects as lf_pass's table has slots above one channel (256), so
        # that some find no slot within its 16 probes and go straight to the dense tables
        own = np.arange(1, top4 + 1, dtype=np.int32).reshape(1, ROWS_SIDE, ROWS_SIDE)
        labs = np.repeat(np.concatenate([rows_label_kinds(top4), own]), ROWS_VARIANTS, axis=0)
        p4 = _scene(tool, "rows prototypes", labs, top4, 48, None, image=IR.noise(labs.shape, C, np.uint16, 48))
        out.append(_gathered(p4, index_map(ROWS_BATCH, len(labs), 2 * ROWS_VARIANTS + 2, 49), "rows-channels", ROW_CAP[tool]))
    return out


# ---- sides ----------------------------------------------------------------------------------------------------------------------
SIDES = ((1, 4096), (4096, 1), (3, 4096), (4096, 3))


def corridor(shape):
    """(seeds, mask) [2,H,W] of the propagator on a thin plane: a seed at either end of the long side, in the second image at
    opposite corners; where the plane is three wide the middle line is shut over its central half."""
    H, W = shape
    seeds, mask = np.zeros((2, H, W), np.int32), np.ones((2, H, W), np.uint8)
    seeds[0, 0, 0], seeds[0, H - 1, W - 1] = 2, 1
    seeds[1, H - 1, 0], seeds[1, 0, W - 1] = MAX_LABEL, 3
    if min(H, W) == 3:
        n = max(H, W)
        if W > H:
            mask[:, 1, n // 4:3 * n // 4] = 0
        else:
            mask[:, n // 4:3 * n // 4, 1] = 0
    return seeds, mask


def family_sides(tool):
    out = []
    for k, shape in enumerate(SIDES):
        name = f"sides {shape[0]}x{shape[1]}"
        if tool == "propagate":
            seeds, mask = corridor(shape)
            out.append(_frozen(dict(name=name, tool=tool, seeds=seeds, mask=mask, guide=None, params=dict(PROPAGATE), cap="kMaxSide")))
            continue
        if tool == "quality":                            # without a mesh, and with one of 256 tiles along the long side
            img = QY.noise((2,) + shape, 1, np.uint16, 70 + k)[..., 0]
            out += [_image_scene(tool, name, img, "kMaxSide"), _image_scene(tool, name + " tile16", img, "kMaxSide", tile=16)]
            continue
        lab = np.stack([IR.contents(shape, 50 + k)[0][1], IR.contents(shape, 60 + k)[1][1]])          # disks, then single pixels
        # the spots' widest tables: both radii 64 fold many times over the short side, and at H = 4096 sd_cols asks for its most LDS
        more = dict(params=dict(SPOTS_WIDE)) if tool == "spots" else {}
        out.append(_scene(tool, name, lab, max(1, int(lab.max())), 70 + k, "kMaxSide", **more))
    return out


@functools.lru_cache(maxsize=None)
def small_scene(tool):
    """The ordinary call behind a cap run: input 1 of handle_schedule.INPUTS (one image of 33 x 67, uint8) under the tool's
    cheapest parameters."""
    k = HS.inputs_of(1)
    if tool == "propagate":
        return _frozen(dict(name="small", tool=tool, seeds=k["seeds"], mask=k["mask"], guide=k["plane"], params=dict(PROPAGATE), cap=None))
    if tool in LABEL_FREE:
        return _image_scene(tool, "small", k["plane"], None)
    c = TOOLS[tool]["channels"]
    return _scene(tool, "small", k["labels"], k["max_label"], 0, None, image=None if c == 0 else k["plane"] if c == 1 else k["image"])


FAMILIES = {"batch": family_batch, "labels": family_labels, "rows": family_rows, "sides": family_sides}
REASONS = (NO_TABLE, NO_CAP, NO_LABELS)


@functools.lru_cache(maxsize=None)
def scenes(tool, family):
    """The scenes of a tool in a family, or the reason there are none."""
    return FAMILIES[family](tool)


def nodes():
    """[(tool, family, n)]: every scene there is, n its place in scenes(tool, family)."""
    return [(t, f, n) for t in TOOLS for f in FAMILIES if not isinstance(scenes(t, f), str) for n in range(len(scenes(t, f)))]


# ---- the restatement of a scene -------------------------------------------------------------------------------------------------
def restate(x):
    """The tool's tables on the scene's own planes, image by image: no gather."""
    return tuple(TOOLS[x["tool"]]["restate"](x, x["params"]))


def gather(tool, tables, index):
    """The tables of the images index[b] of a batch whose tables are `tables`: every table has the image first, but the
    neighbours' CSR offsets and pair list and the spots' offsets and list, which run through the whole batch (RUNNING)."""
    if tool == "spots":                                  # counts, offsets, the list, then geom and records (with labels), the response
        counts, offsets, lst = tables[:3]
        per = [lst[offsets[p]:offsets[p + 1]] for p in range(len(counts))]
        ends = np.concatenate([[0], np.cumsum(counts[index, 0])]).astype(offsets.dtype)
        spread = np.concatenate([per[p] for p in index]).astype(lst.dtype).reshape(-1, lst.shape[1])
        return (counts[index], ends, spread) + tuple(t[index] for t in tables[3:])
    if tool != "neighbors":
        return tuple(t[index] for t in tables)
    geom, objects, offsets, pairs = tables
    M = geom.shape[1]
    deg = np.diff(offsets).reshape(-1, M)[index].reshape(-1)
    per = [pairs[offsets[p * M]:offsets[(p + 1) * M]] for p in range(geom.shape[0])]
    return geom[index], objects[index], np.concatenate([[0], np.cumsum(deg)]).astype(offsets.dtype), \
        np.concatenate([per[p] for p in index]).astype(pairs.dtype).reshape(-1, pairs.shape[1])


def expected(x, lo=None, hi=None):
    """The tables the device must return on scene x; lo, hi: of the images lo..hi-1 of a gathered scene only."""
    if "index" not in x:
        return restate(x)
    index = x["index"] if lo is None else x["index"][lo:hi]
    return gather(x["tool"], restate(x["protos"]), index)


def absent_rows(x):
    """bool [B,max_label]: the rows of the labels that image b does not hold (for the matcher: of `labels`, the predicted side)."""
    lab, M = full(x)["labels"], x["max_label"]
    present = np.zeros((lab.shape[0], M + 1), bool)
    present[np.repeat(np.arange(lab.shape[0]), lab[0].size), lab.reshape(-1)] = True
    return ~present[:, 1:]


def table_bytes(x):
    """The bytes of the largest table the scene's call returns, and of all of them, from the documented shapes."""
    tool, p = x["tool"], x["params"]
    key = "image" if tool in LABEL_FREE else "seeds" if tool == "propagate" else "labels"
    images = x["batch"] if "index" in x else x[key].shape[0]
    one = (x["protos"] if "index" in x else x)
    if tool in ("expand", "propagate"):
        n = images * one[key][0].size
        sizes = [4 * n, (8 if tool == "propagate" else 2) * n]
    elif tool == "quality":                              # records, and the mesh where there is one
        H, W = one["image"].shape[1:3]
        C = one["image"].shape[3] if one["image"].ndim == 4 else 1
        m_r, m_c = QY.mesh_dims(H, W, p["tile"])
        sizes = [104 * images * C] + ([64 * images * C * m_r * m_c] if p["tile"] else [])
    elif tool == "spots":                                # geom, records, the response, and the list at the most it can hold
        pixels, rows = images * one["labels"][0].size, images * x["max_label"]
        sizes = [24 * rows, 48 * rows, 4 * pixels, 32 * min(CAPS["kSdMaxSpots"], pixels), 16 * images]
    elif tool == "focus":
        rows = images * x["max_label"]
        sizes = [24 * rows, 40 * rows * (one["image"].shape[3] if one["image"].ndim == 4 else 1)]
    else:
        rows = images * x["max_label"]
        C = TOOLS[tool]["channels"]
        sizes = {"intensity": [24, 48 * C], "quantiles": [4, 8 * C], "texture": [4, 4 * C * 16 * p.get("levels", 0), 32 * C, 32 * C],
                 "shape": [80, 16, 64, 12], "neighbors": [24, 12, 8], "colocalize": [24, 40 * C, 72], "radial": [24, 16, 64 * (1 + C) * p.get("bins", 0), 32 * C],
                 "granularity": [24, 8 * C * (p.get("steps", 0) + 1)], "match": [16, 16]}[tool]
        sizes = [s * rows for s in sizes]
    return max(sizes), sum(sizes)


# ---- the segmenter --------------------------------------------------------------------------------------------------------------
SEGMENT_CASES = {"default": {}, "split": dict(split_touching=True), "split_intensity": dict(HS.SEGMENTERS["split_intensity"]),
                 "local": dict(threshold="local", local_radius=1), "noise": dict(threshold="noise", noise_tile=16)}
SEGMENT_VARIANTS = 4


def segment_protos():
    """uint16 [24,8,8]: six kinds (flat; one blob; two touching blobs; bright opposite corners; a ring with a hole; a bright last
    pixel on a ramp) under four noises."""
    yy, xx = np.mgrid[0:8, 0:8]
    kinds = np.zeros((6, 8, 8))
    kinds[1] = 3000.0 * np.exp(-((yy - 3) ** 2 + (xx - 4) ** 2) / 4.0)
    kinds[2] = 3000.0 * (np.exp(-((yy - 3) ** 2 + (xx - 2) ** 2) / 2.5) + np.exp(-((yy - 4) ** 2 + (xx - 5.5) ** 2) / 2.5))
    kinds[3, :2, :2] = kinds[3, 6:, 6:] = 2500.0
    kinds[4, 1:7, 1:7] = 2000.0
    kinds[4, 3:5, 3:5] = 0.0
    kinds[5] = 20.0 * (yy + xx)
    kinds[5, 7, 7] = 4000.0
    rng = np.random.default_rng(81)
    noise = rng.integers(0, 120, (SEGMENT_VARIANTS, 8, 8))
    out = (300.0 + kinds[:, None] + noise[None]).reshape(-1, 8, 8)
    out = np.rint(out).astype(np.uint16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def segment_scene():
    """(images uint16 [kMaxBatch,8,8], index): the prototypes spread over the batch, an image with two bright corners, which every
    case's rule finds, first and last."""
    index = index_map(MAX_BATCH, 6 * SEGMENT_VARIANTS, 3 * SEGMENT_VARIANTS + 3, 82)
    images = segment_protos()[index]
    images.setflags(write=False)
    return images, index


def segment_restate(images, case):
    opts = SEGMENT_CASES[case]
    out = P.segment_batch(images, return_distance=bool(opts.get("split_touching")), **opts)
    return tuple(np.asarray(o) for o in out[:-1])


@functools.lru_cache(maxsize=None)
def _segment_proto_tables(case):
    return segment_restate(segment_protos(), case)


def segment_expected(case, lo=None, hi=None):
    """(labels, n_labels, thresholds[, heights]) of the whole batch, or of its images lo..hi-1."""
    index = segment_scene()[1]
    return tuple(t[index if lo is None else index[lo:hi]] for t in _segment_proto_tables(case))
