"""The segmenter's stages chained on the device (ThresholdSegmenter.segment_batch and the scaffold under it, _front) against the
composed CPU restatement of tests/pipeline_reference.py, which tests/test_pipeline_reference_cpu.py holds to the per-stage
restatements and to non-idle inputs.

Every result is an integer plane or vector: np.array_equal throughout.  CASES covers every pair of option levels and one full
chain per rule; the shapes, taken in rotation, are the smallest that cross the stages' tiles: 47 x 61 inside one tile everywhere,
67 x 261 across the 16- and 64-row tiles, the 64- and 256-column tiles and the cleanup's 32 x 256 tile with a width no multiple of
4, 131 x 200 across the smoothing's 128-row column tile, 40 x 1030 across the 768- and 1024-pixel row segments of the smoothing,
the top-hat and the local sums."""
import functools
import math

import numpy as np
import pytest

import pipeline_reference as P
from cellscreen import extract as X
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

IDS = [f"{i}-" + "-".join(str(v) for v in c) for i, c in enumerate(P.CASES)]


@pytest.fixture(scope="module")
def shared():
    ext = X.CellExtractor(0)
    yield ext
    ext.close()


def as_tensor(imgs):
    import torch
    return torch.from_numpy(imgs.view(np.int16).copy() if imgs.dtype == np.uint16 else imgs.copy()).to(torch.device("cuda", 0))


def to_host(x):
    if not hasattr(x, "is_cuda"):
        return x
    x = x.cpu().numpy()
    return x.view(np.uint16) if x.dtype == np.int16 else x              # a uint16 plane travels as an int16 tensor


@functools.lru_cache(maxsize=None)
def case_of(index):
    """(keyword arguments, images, whether the case has a height plane, the restatement's result) of one case, computed once."""
    kw, shape, dtype = P.options(P.CASES[index], index)
    imgs = P.scene(shape, dtype, index)
    heights = bool(kw.get("split_touching", False))
    want = P.segment_batch(imgs, return_distance=heights, **kw)
    for a in (imgs,) + tuple(want[:-1]) + tuple(want[-1].values()):
        a.setflags(write=False)
    return kw, imgs, heights, want


def timing_keys(kw):
    """The keys that last_timing's docstring promises for a combination of options."""
    if not kw.get("split_touching"):
        keys = {"threshold_ms", "label_ms"}
    else:
        keys = {"threshold_ms", "height_ms" if kw.get("split_by") == "intensity" else "distance_ms", "seed_ms", "flood_ms"}
    if "smooth_sigma" in kw:
        keys |= {"smooth_ms"} | ({"smooth_median_ms"} if kw.get("denoise") else set())
    if "background_radius" in kw:
        keys |= {"median_ms", "background_ms"}
    if kw.get("threshold") == "noise":
        keys |= {"noise_mesh_ms", "noise_cut_ms", "noise_link_ms"}
    elif any(k in kw for k in ("weak_threshold", "weak_delta")):
        keys |= {"hysteresis_level_ms", "hysteresis_link_ms"}            # in the local rule's place: no local_ms
    elif kw.get("threshold") == "local":
        keys |= {"local_median_ms", "local_ms"}
    if "open_radius" in kw or "min_area" in kw:
        keys |= {"open_ms", "min_area_ms"}
    if "expand_distance" in kw:
        keys |= {"expand_columns_ms", "expand_rows_ms"}
    return keys


def same(got, want, heights, what):
    names = ("labels", "n_labels", "thresholds", "heights")[:3 + heights]
    assert len(got) == len(names), what
    for name, g, w in zip(names, got, want):
        g = to_host(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:3].tolist())


def check_timing(seg, kw, what):
    t = seg.last_timing()
    assert set(t) == timing_keys(kw), (what, sorted(t))
    assert all(math.isfinite(v) and v >= 0.0 for v in t.values()), (what, t)


def run(seg, x, kw, heights, want, what):
    got = seg.segment_batch(x, return_distance=True) if heights else seg.segment_batch(x)
    if hasattr(x, "is_cuda"):
        assert got[0].is_cuda and (not heights or got[3].is_cuda), what            # the planes stay on the device
        assert isinstance(got[1], np.ndarray) and isinstance(got[2], np.ndarray), what
    same(got, want, heights, what)
    check_timing(seg, kw, what)


def check_planes(seg, x, want, what):
    for name, plane in want[-1].items():
        got = getattr(seg, name)(x)
        assert hasattr(got, "is_cuda") == hasattr(x, "is_cuda"), (what, name)
        got = to_host(got)
        assert got.dtype == plane.dtype and np.array_equal(got, plane), (what, name, int((got != plane).sum()))


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=IDS)
def test_case_equals_the_restatement(shared, index):
    kw, imgs, heights, want = case_of(index)
    assert set(want[-1]) == {m for m, on in (("smooth_batch", "smooth_sigma" in kw), ("correct_batch", "background_radius" in kw),
                                             ("local_mask_batch", kw.get("threshold") == "local"),
                                             ("hysteresis_mask_batch", "weak_threshold" in kw or "weak_delta" in kw),
                                             ("noise_mask_batch", kw.get("threshold") == "noise"),
                                             ("clean_mask_batch", "open_radius" in kw or "min_area" in kw)) if on}
    dev = as_tensor(imgs)
    own = S.ThresholdSegmenter(0, **kw)
    try:
        run(own, imgs, kw, heights, want, "numpy")
        check_planes(own, imgs, want, "numpy")
        run(own, dev, kw, heights, want, "tensor")
        run(own, imgs, kw, heights, want, "numpy after the planes")
    finally:
        own.close()
    seg = S.ThresholdSegmenter(0, extractor=shared, **kw)
    assert seg._handle is shared._handle
    run(seg, dev, kw, heights, want, "shared handle, tensor")
    check_planes(seg, dev, want, "shared handle, tensor")
    run(seg, imgs, kw, heights, want, "shared handle, numpy")
    assert seg._pre is None


def test_one_handle_through_every_case_there_and_back(shared):
    """Every case on one handle, in order and then in reverse, so that each follows two different predecessors, on shapes that
    grow three times and then shrink (and the reverse), numpy and tensor input in turn: a stage that is off in one case leaves
    nothing that the next one reads, and none reads the larger buffers of the one before."""
    segs = [S.ThresholdSegmenter(0, extractor=shared, **case_of(i)[0]) for i in range(len(P.CASES))]
    order = list(range(len(P.CASES))) + list(range(len(P.CASES) - 1))[::-1]
    tensors = {}
    for step, i in enumerate(order):
        kw, imgs, heights, want = case_of(i)
        if step % 2 and i not in tensors:
            tensors[i] = as_tensor(imgs)
        x = tensors[i] if step % 2 else imgs
        run(segs[i], x, kw, heights, want, f"step {step}: case {i} {P.CASES[i]}")
    for i, seg in enumerate(segs):                                               # and every one's times are still its own
        check_timing(seg, case_of(i)[0], f"afterwards: case {i}")
