"""The segmenter and every label tool lending each other one preprocess handle (the SegmentState of csrc/segment_internal.hpp):
about twenty device buffers that only grow, nearly all reused under another element type by another entry point, so that a call
works inside whatever the one before left.  Each tool's own test runs it alone, or behind a plain segmenter and the expander; here
every tool follows every other one (tests/handle_schedule.py: an Eulerian circuit of the complete directed graph on the tools), on
inputs that shrink and grow, and follows every other tool's refused call; and the neighbour pair list and the spot list are fetched
after other stages ran on their handle.  All tables compared are integers: np.array_equal against each tool's own CPU restatement."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import handle_schedule as HS
from cellscreen import _lib as L
from cellscreen import colocalize as CO
from cellscreen import expand as EX
from cellscreen import extract as X
from cellscreen import granularity as GR
from cellscreen import intensity as IN
from cellscreen import neighbors as NB
from cellscreen import propagate as PG
from cellscreen.preprocess import PIX_U16
from cellscreen import quality as Q
from cellscreen import quantile as QU
from cellscreen import radial as RA
from cellscreen import score as SC
from cellscreen import segment as S
from cellscreen import shape as SH
from cellscreen import spots as SP
from cellscreen import texture as TX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tools():
    """Every actor on one handle: the extractor's, which a plain segmenter passes on to the tools."""
    ext = X.CellExtractor(0)
    seg = S.ThresholdSegmenter(0, extractor=ext)
    made = {name: S.ThresholdSegmenter(0, extractor=ext, **kw) for name, kw in HS.SEGMENTERS.items()}
    made.update(expand=EX.LabelExpander(0, extractor=seg), intensity=IN.IntensityMeasurer(0, extractor=seg),
                quantiles=QU.QuantileMeasurer(0, extractor=seg), texture=TX.TextureMeasurer(0, extractor=seg),
                shape=SH.ShapeMeasurer(0, extractor=seg), neighbors=NB.NeighborMeasurer(0, extractor=seg),
                colocalize=CO.ColocalizationMeasurer(0, extractor=seg), radial=RA.RadialMeasurer(0, extractor=seg),
                granularity=GR.GranularityMeasurer(0, extractor=seg), match=SC.LabelMatcher(0, extractor=seg), extract=ext,
                propagate=PG.LabelPropagator(0, extractor=seg), spots=SP.SpotDetector(0, extractor=seg),
                quality=Q.ImageQualityMeasurer(0, extractor=seg), focus=Q.ImageQualityMeasurer(0, extractor=seg))
    assert set(made) == set(HS.ACTORS) and all(t._handle is ext._handle for t in made.values())
    yield made
    assert all(t._pre is None for name, t in made.items() if name != "extract")   # nobody made a handle of its own
    ext.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a.view(np.int16).copy() if a.dtype == np.uint16 else a.copy()).to(torch.device("cuda", 0))


def to_host(x):
    if x is None or not hasattr(x, "is_cuda"):
        return x
    x = x.cpu().numpy()
    return x.view(np.uint16) if x.dtype == np.int16 else x


_DEVICE = {}


def on(k, name, on_device):
    """An array of input k where the call wants it; the device copies are made once."""
    a = HS.inputs_of(k)[name]
    if not on_device:
        return a
    if (k, name) not in _DEVICE:
        _DEVICE[k, name] = as_tensor(a)
    return _DEVICE[k, name]


def call(tools, actor, k, on_device=False, exclude=False, labels=None, max_label=None):
    """One call of one actor on input k, its integer tables in the order of handle_schedule.expected.  labels, max_label: in the
    input's place, for the calls that must fail (the propagator takes `labels` as its seeds)."""
    t = tools[actor]
    image = on(k, "image", on_device)
    lab = on(k, "labels", on_device) if labels is None else labels
    ex = on(k, "exclude", on_device) if exclude else None
    if actor in HS.SEGMENTERS:
        out = t.segment_batch(on(k, "plane", on_device), return_distance=True)
    elif actor == "expand":
        out = t.expand_batch(lab, HS.EXPAND_DISTANCE, return_d2=True)
    elif actor == "intensity":
        out = t.measure_dense(image, lab, exclude=ex, max_label=max_label)
    elif actor == "quantiles":
        out = t.measure_dense(image, lab, HS.QUANTILES, True, exclude=ex, max_label=max_label)
    elif actor == "texture":
        c, marg, sumsq, _, glcm = t.measure_dense(image, lab, HS.TEXTURE[0], HS.TEXTURE[1], exclude=ex, max_label=max_label, glcm=True)
        out = c, marg, sumsq, glcm
    elif actor == "shape":
        out = t.measure_dense(lab, exclude=ex, max_label=max_label, hull=True)
    elif actor == "neighbors":
        out = t.measure_dense(lab, math.sqrt(HS.NEIGHBOR_D2), max_label=max_label)
    elif actor == "colocalize":
        out = t.measure_dense(image, lab, exclude=ex, max_label=max_label, threshold=HS.COLOC_THRESHOLD, rwc=True)
    elif actor == "radial":
        out = t.measure_dense(image, lab, exclude=ex, max_label=max_label, bins=HS.RADIAL_BINS, centers=HS.inputs_of(k)["centers"])
    elif actor == "granularity":
        out = t.measure_dense(image, lab, exclude=ex, steps=HS.GRANULARITY[0], subsample=HS.GRANULARITY[1], max_label=max_label)
    elif actor == "match":
        m = t.match_batch(lab, on(k, "truth", on_device), max_pred=max_label)
        out = m.pred, m.truth, m.n_pairs
    elif actor == "propagate":
        out = t.propagate_batch(on(k, "seeds", on_device) if labels is None else labels, mask=on(k, "mask", on_device), guide=image,
                                max_cost=HS.inputs_of(k)["max_cost"], return_cost=True, **HS.PROPAGATE)
    elif actor == "spots":
        out = t.detect_dense(image, HS.SPOT_THRESHOLDS[k], lab, ex, max_label, SP.spot_params(**HS.SPOTS), True)
    elif actor == "quality":
        out = t.measure_batch_dense(image, tile=HS.QUALITY_TILE, sat_level=list(HS.SAT_LEVELS[k]))
    elif actor == "focus":
        out = t.measure_objects_dense(image, lab, exclude=ex, max_label=max_label)
    else:
        r = t.extract_batch(on(k, "plane", on_device), lab)
        reg = r.regions
        rows = np.stack([reg[f].astype(np.int64) for f in ("image",) + HS.EXTRACT_FIELDS], axis=1).reshape(len(reg), -1)
        out = r.status, rows
    return tuple(to_host(o) for o in out)


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, i, int((g != w).sum()))


def test_every_tool_behind_every_other_on_one_handle(tools):
    steps = HS.schedule()
    assert len(steps) == len(HS.ACTORS) * (len(HS.ACTORS) - 1) + 1
    for actor, k, _, exclude in steps:                                            # the restatements, outside the time below
        HS.expected(actor, k, exclude)
    t0 = time.perf_counter()
    for n, (actor, k, on_device, exclude) in enumerate(steps):
        got = call(tools, actor, k, on_device, exclude)
        before = steps[n - 1][:2] if n else None
        same(got, HS.expected(actor, k, exclude), f"step {n}: {actor} on input {k} {HS.INPUTS[k]}, tensor={on_device}, "
                                                  f"exclude={exclude}, behind {before}")
    print(f"\n{len(steps)} calls on one handle in {time.perf_counter() - t0:.2f} s")
    for name, t in tools.items():
        timing = t.last_timing()
        assert timing and all(math.isfinite(v) and v >= 0.0 for v in timing.values()), (name, timing)


def test_a_refused_call_leaks_nothing_into_the_next_tool(tools):
    """Every tool that range-checks its labels is handed one label above max_label and refuses it with status -1, and the
    propagator one seed above the largest label there is; the very next call goes to another of the tools that share its status
    words (the control buffer), with good input."""
    k = 1
    x = HS.inputs_of(k)
    m = x["max_label"]
    bad = x["labels"].copy()
    bad[0, 20, 40] = m + 1
    bad_seed = x["seeds"].copy()
    bad_seed[0, 20, 40] = PG.MAX_LABEL + 1
    nexts = HS.RANGE_CHECKED + ("expand", "propagate") + tuple(HS.SEGMENTERS)        # all of them keep their status words in ctrl
    for n, failing in enumerate(HS.RANGE_CHECKED + ("propagate",)):
        wrong, text = (bad_seed, "a seed is negative or exceeds") if failing == "propagate" else (bad, "exceeds max_")
        for j, after in enumerate(a for a in nexts if a != failing):
            on_device = bool((n + j) % 2)
            with pytest.raises(L.CellScreenError) as ei:
                call(tools, failing, k, on_device, labels=as_tensor(wrong) if on_device else wrong, max_label=m)
            assert ei.value.status == -1 and text in str(ei.value), (failing, str(ei.value))
            exclude = after in HS.HAS_EXCLUDE and bool(j % 2)
            same(call(tools, after, k, not on_device, exclude), HS.expected(after, k, exclude), f"{after} behind a refused {failing}")
    # and once on the large input, where the refused call has written most before it is found out
    big = HS.inputs_of(0)["labels"].copy()
    big[1, 129, 519] = HS.inputs_of(0)["max_label"] + 1
    for failing, after in zip(HS.RANGE_CHECKED, HS.RANGE_CHECKED[1:] + HS.RANGE_CHECKED[:1]):
        with pytest.raises(L.CellScreenError):
            call(tools, failing, 0, labels=big, max_label=HS.inputs_of(0)["max_label"])
        same(call(tools, after, 1), HS.expected(after, 1), f"{after}, small, behind a refused large {failing}")


def test_spot_list_survives_other_stages(tools):
    """The spot list "stays on the handle until the next cs_spot_detect" (include/cellscreen.h).  cs_spot_detect works in the
    planes of cs_segment_smooth and of the split, in the mask, count and chunk buffers and in the staging area; between it and
    cs_spot_fill a smoothing intensity split, the granularity spectrum, a propagation, the image quality and focus records and a
    small split run on the handle.  The list is then fetched twice: to the host, and into CUDA tensors."""
    import torch
    lib, h = tools["spots"]._lib, tools["spots"]._handle
    prm = SP.spot_params(**HS.SPOTS)
    for k in (2, 0):
        x = HS.inputs_of(k)
        img, lab, m = x["image"], x["labels"], x["max_label"]
        B, H, W = lab.shape
        want = HS.expected("spots", k)
        thr = np.full(B, int(round(256 * HS.SPOT_THRESHOLDS[k])), np.int32)
        counts, geom, records = np.empty((B, 2), np.int64), np.empty((B, m, 3), np.int64), np.empty((B, m, 6), np.int64)
        n = C.c_int64(-1)
        assert img.dtype == np.uint16
        assert lib.cs_spot_detect(h, img.ctypes.data, PIX_U16, img.shape[3], lab.ctypes.data, None, B, H, W, L.CS_MEM_HOST, m, C.byref(prm),
                                  thr.ctypes.data, counts.ctypes.data, geom.ctypes.data, records.ctypes.data, None, L.CS_MEM_HOST, C.byref(n)) == 0
        assert n.value == len(want[2]) > 0
        for actor, kk in (("split_intensity", 0), ("granularity", 0), ("propagate", 0), ("quality", 0), ("focus", 0), ("split", 1)):
            exclude = actor in HS.HAS_EXCLUDE
            same(call(tools, actor, kk, False, exclude), HS.expected(actor, kk, exclude), f"{actor} between the two calls")
        lst, offsets = np.full((n.value, 8), -1, np.int32), np.full(B + 1, -1, np.int64)
        assert lib.cs_spot_fill(h, lst.ctypes.data, n.value, offsets.ctypes.data, L.CS_MEM_HOST) == 0
        same((counts, offsets, lst, geom, records), want[:5], f"the spot list of input {k} after other stages, on the host")
        dev = torch.device("cuda", 0)
        d_lst, d_off = torch.full((n.value, 8), -1, dtype=torch.int32, device=dev), torch.full((B + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()                         # the fills are done before the handle's own stream writes
        assert lib.cs_spot_fill(h, d_lst.data_ptr(), n.value, d_off.data_ptr(), L.CS_MEM_DEVICE) == 0
        same((d_off.cpu().numpy(), d_lst.cpu().numpy()), want[1:3], f"the spot list of input {k} after other stages, on the device")


def test_pair_list_survives_other_stages(tools):
    """cs_label_neighbors leaves its sorted pair list on the handle "until cs_label_neighbors_pairs copies it out, whatever other
    stage runs between": here a split segmentation, the granularity spectrum and the radial distribution, which use the same
    buffers as the pair table for their own planes and keys, and a propagation, which writes the key, queue and mask planes, run
    between the two calls."""
    lib, h = tools["neighbors"]._lib, tools["neighbors"]._handle
    for k in (2, 0):
        x = HS.inputs_of(k)
        lab, m = x["labels"], x["max_label"]
        B, H, W = lab.shape
        want = HS.expected("neighbors", k)
        prm = L.CSNeighborsParams()
        prm.max_d2 = HS.NEIGHBOR_D2
        geom, objects = np.empty((B, m, 3), np.int64), np.empty((B, m, 3), np.int32)
        offsets, n = np.empty(B * m + 1, np.int64), C.c_int64(-1)
        assert lib.cs_label_neighbors(h, lab.ctypes.data, B, H, W, L.CS_MEM_HOST, m, C.byref(prm), geom.ctypes.data, objects.ctypes.data,
                                      offsets.ctypes.data, L.CS_MEM_HOST, C.byref(n)) == 0
        assert n.value == len(want[3]) > 0
        for actor, kk in (("split", 0), ("granularity", 0), ("propagate", 0), ("radial", 0), ("split_intensity", 1), ("propagate", 1),
                          ("granularity", 1)):
            exclude = actor in HS.HAS_EXCLUDE
            same(call(tools, actor, kk, False, exclude), HS.expected(actor, kk, exclude), f"{actor} between the two calls")
        pairs = np.full((n.value, 3), -1, np.int32)
        assert lib.cs_label_neighbors_pairs(h, pairs.ctypes.data, n.value, L.CS_MEM_HOST) == 0
        same((geom, objects, offsets, pairs), want, f"the pair list of input {k} after other stages")
