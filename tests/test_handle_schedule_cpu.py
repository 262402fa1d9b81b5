"""tests/handle_schedule.py without a device: in the schedule of tests/test_gpu_shared_handle.py every actor follows every other
one, and every actor meets every input, both kinds of memory and, where it has one, the exclude plane."""
import numpy as np

import expand_reference as ER
import handle_schedule as HS
import pipeline_reference as P


def test_circuit_walks_every_edge_once():
    for n in (2, 3, 5, len(HS.ACTORS)):
        walk = HS.circuit(n)
        edges = list(zip(walk, walk[1:]))
        assert walk[0] == walk[-1] == 0 and len(edges) == n * (n - 1) == len(set(edges))
        assert set(edges) == {(a, b) for a in range(n) for b in range(n) if a != b}
    assert HS.circuit(len(HS.ACTORS)) == HS.circuit(len(HS.ACTORS))               # the same walk every time


def test_every_actor_follows_every_other_and_meets_every_input():
    steps = HS.schedule()
    names = [s[0] for s in steps]
    assert set(zip(names, names[1:])) == {(a, b) for a in HS.ACTORS for b in HS.ACTORS if a != b}
    assert len(steps) == len(HS.ACTORS) * (len(HS.ACTORS) - 1) + 1
    for a in HS.ACTORS:
        mine = {s[1:] for s in steps if s[0] == a}
        want = {(k, dev, ex) for k in range(3) for dev in (False, True) for ex in ((False, True) if a in HS.HAS_EXCLUDE else (False,))}
        assert mine == want, a
    # a small call behind a large one, and a large one behind a small one
    sizes = [int(np.prod(HS.INPUTS[s[1]])) for s in steps]
    assert any(a > 4 * b for a, b in zip(sizes, sizes[1:])) and any(b > 4 * a for a, b in zip(sizes, sizes[1:]))


def test_inputs_are_what_the_tools_accept():
    for k, (B, H, W) in enumerate(HS.INPUTS):
        x = HS.inputs_of(k)
        assert x["image"].shape == (B, H, W, 2) and x["image"].dtype == HS.DTYPES[k] and x["plane"].flags.c_contiguous
        for name in ("labels", "exclude", "truth"):
            assert x[name].shape == (B, H, W) and x[name].dtype == np.int32 and x[name].min() == 0
        assert x["max_label"] == x["labels"].max() >= 3 and x["centers"].shape == (B, x["max_label"], 2)
        assert ((x["exclude"] > 0) & (x["labels"] > 0)).any() and (x["truth"] != x["labels"]).any()
        seeds, mask = x["seeds"], x["mask"]                             # the propagator's: a few pixels inside the objects, a wider mask
        assert seeds.dtype == np.int32 and mask.dtype == np.uint8 and seeds.shape == mask.shape == (B, H, W)
        assert 0 < (seeds > 0).sum() < (x["labels"] > 0).sum() // 3 and len(np.unique(seeds)) > 3
        assert np.array_equal(seeds[seeds > 0], x["labels"][seeds > 0])
        assert mask[x["labels"] > 0].all() and mask.sum() > (x["labels"] > 0).sum()
        grown, cost = HS.expected("propagate", k)
        assert (grown > 0).sum() > 2 * (seeds > 0).sum() and ((mask > 0) & (grown == 0)).any() and cost.max() <= x["max_cost"]
    for name, kw in HS.SEGMENTERS.items():
        n = HS.expected(name, 1)[1]
        assert (n >= 2).all(), (name, n)


def test_the_three_newest_actors_have_something_to_find():
    assert len(HS.ACTORS) == 17 and HS.ACTORS[-3:] == ("spots", "quality", "focus") and len(HS.schedule()) == 17 * 16 + 1 == 273
    assert {"spots", "focus"} <= set(HS.HAS_EXCLUDE) <= set(HS.RANGE_CHECKED) and "quality" not in HS.RANGE_CHECKED
    for k, (B, H, W) in enumerate(HS.INPUTS):
        x = HS.inputs_of(k)
        top = int(np.iinfo(HS.DTYPES[k]).max)
        plain = HS.expected("spots", k)
        for exclude in (False, True):
            counts, offsets, lst, geom, records, response = HS.expected("spots", k, exclude)
            assert offsets[-1] == len(lst) > 0 and (lst[:, 2] > 0).any() and response.shape == (B, H, W)      # a spot on a labelled pixel
            assert geom.shape == (B, x["max_label"], 3) and records[..., 0].sum() == (lst[:, 2] > 0).sum()
            assert (lst[:, 3] >= 256 * HS.SPOT_THRESHOLDS[k]).all()
        assert (response >= 256 * HS.SPOT_THRESHOLDS[k]).sum() > len(lst)          # the window prunes, and the threshold cuts:
        assert (response >= 256).sum() > (response >= 256 * HS.SPOT_THRESHOLDS[k]).sum()      # not every positive pixel passes
        assert not np.array_equal(HS.expected("spots", k, True)[3], plain[3])     # the exclude plane takes pixels from the objects
        records, mesh = HS.expected("quality", k)
        assert records.shape == (B, 2, 13) and mesh.shape == (B, 2, -(-H // 16), -(-W // 16), 8)
        assert all(0 < s < top for s in HS.SAT_LEVELS[k]) and (records[:, :, 7] > 0).all() and (records[:, :, 7] < records[:, :, 0]).all()
        g0, f0 = HS.expected("focus", k)
        g1, f1 = HS.expected("focus", k, True)
        assert f0.shape == (B, x["max_label"], 2, 5) and f0.any() and not np.array_equal(f0, f1) and np.array_equal(g0, plain[3])


def test_windowed_expansion_is_the_whole_image_s():
    lab = np.stack([ER.disks((45, 70), 9, 4), ER.disks((45, 70), 3, 5)])
    for distance, side in ((3, 32), (4, 16), (11, 20)):
        max_d2 = ER.max_d2_of(distance)
        want = ER.expand(lab, max_d2)
        for b in range(2):
            got = P.expand_windows(lab[b], max_d2, side)
            assert np.array_equal(got[0], want[0][b]) and np.array_equal(got[1], want[1][b]) and (got[0] != lab[b]).any()
