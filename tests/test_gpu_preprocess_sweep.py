"""cs_preprocess (csrc/preprocess.hip) over every crop side it accepts: the families of tests/preprocess_plans.py on the device.
For every crop the CLAHE plane is the oracle's bit for bit and the output lies within 6e-8, one float32 rounding below 1.0, of the
float64 restatement (oracle/preprocess_oracle.py at 64 x 64, tests/preprocess_sized_reference.py at another size); then the things a
list of crops cannot show: crops of very different LDS needs in one chunk, both input kinds, a handle whose buffers grow and are
reused, the pixel-span rule of the chunk loop, and the refusals next to the cases that are accepted.
tests/test_preprocess_envelope_cpu.py proves what the families cover and that each can fail."""
import numpy as np
import pytest

import preprocess_plans as PL
from cellscreen import _lib as L
from cellscreen import preprocess as pp

pytestmark = pytest.mark.gpu

TOL_OUT = PL.TOL_OUT


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(proc, crops, clip=0.02):
    pix, off, hs, ws = pp.pack_crops(crops)
    out, cl = proc.run_packed(pix, off, hs, ws, clip, want_clahe=True)
    return out, pp.split_clahe(cl, off, hs, ws)


def _groups(cases):
    """The cases of a node by what one call shares: dtype, output size, clip limit."""
    out = {}
    for c in cases:
        out.setdefault((c["dtype"], c["hw"], c["clip"]), []).append(c)
    return out


def _check(cases, what):
    """Runs the cases, one call per (dtype, output size, clip limit), and holds every crop to its restatement."""
    assert cases, what
    worst, worst_name = 0.0, None
    for (dt, hw, clip), group in _groups(cases).items():
        p = pp.Preprocessor(0, out_hw=hw)
        try:
            out, cl = _run(p, [PL.crop(c) for c in group], clip)
        finally:
            p.close()
        assert out.dtype == np.float32 and out.shape == (len(group),) + hw
        assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
        for i, c in enumerate(group):
            plane, ref = PL.expected(c)
            assert cl[i].dtype == np.uint16 and cl[i].shape == c["shape"]
            assert np.array_equal(cl[i], plane), f"CLAHE plane of {c['name']}: {(cl[i] != plane).sum()} of {plane.size} pixels differ"
            err = np.abs(out[i].astype(np.float64) - ref).max()
            if err > worst:
                worst, worst_name = err, c["name"]
            assert err <= TOL_OUT, f"{c['name']}: {err:.3e}"
    print(f"{what}: {len(cases)} crops, worst {worst:.3e} ({worst_name})")


def _half(c, part):
    return (PL.TILE_SIDES.index(c["shape"][0]) < 10) == (part == 0)


NODES = {}
for _dt in ("uint8", "uint16"):
    for _part in (0, 1):
        NODES[f"tiles-{_dt}-{'ab'[_part]}"] = ("tiles", lambda c, dt=_dt, part=_part: c["dtype"] == dt and _half(c, part))
    NODES[f"large-{_dt}"] = ("large", lambda c, dt=_dt: c["dtype"] == dt and c["hw"] == (64, 64))
    NODES[f"radius-{_dt}"] = ("radius", lambda c, dt=_dt: c["dtype"] == dt)
    NODES[f"ties-{_dt}"] = ("ties", lambda c, dt=_dt: c["dtype"] == dt)
    NODES[f"clip-small-{_dt}"] = ("clip", lambda c, dt=_dt: c["dtype"] == dt and c["shape"] == (120, 88))
NODES["large-sized"] = ("large", lambda c: c["hw"] != (64, 64))
for _content in ("const", "two", "low", "noise"):
    NODES[f"clip-1024-{_content}"] = ("clip", lambda c, k=_content: c["shape"] == (1024, 1024) and c["content"] == k)


def test_the_nodes_run_every_case_once():
    seen = [c["name"] for family, pick in NODES.values() for c in PL.cases(family) if pick(c)]
    want = [c["name"] for f in PL.FAMILIES if f != "mixed" for c in PL.cases(f)]
    assert sorted(seen) == sorted(want)


@pytest.mark.parametrize("node", list(NODES))
def test_family(node):
    family, pick = NODES[node]
    _check([c for c in PL.cases(family) if pick(c)], node)


# ---- crops of very different LDS needs in one chunk -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["uint8", "uint16"])
def test_mixed_one_chunk_equals_every_crop_alone_in_both_orders(dt):
    """A chunk's dynamic LDS is the maximum over its crops: 225 tiles (15 x 15), 64 tiles, and the 64 KB line of a 1024-wide crop."""
    cases = [c for c in PL.cases("mixed") if c["dtype"] == dt]
    crops = [PL.crop(c) for c in cases]
    p = pp.Preprocessor(0)
    try:
        out, cl = _run(p, crops)
        rout, rcl = _run(p, crops[::-1])
    finally:
        p.close()
    worst = 0.0
    for i, c in enumerate(cases):
        q = pp.Preprocessor(0)                           # a fresh handle: its launch asks for this crop's LDS alone
        try:
            aout, acl = _run(q, [crops[i]])
        finally:
            q.close()
        j = len(crops) - 1 - i
        assert np.array_equal(_bits(out[i]), _bits(aout[0])) and np.array_equal(cl[i], acl[0]), c["name"]
        assert np.array_equal(_bits(rout[j]), _bits(aout[0])) and np.array_equal(rcl[j], acl[0]), c["name"]
        plane, ref = PL.expected(c)
        assert np.array_equal(cl[i], plane), c["name"]
        worst = max(worst, np.abs(out[i].astype(np.float64) - ref).max())
    print(f"mixed-{dt}: worst {worst:.3e}")
    assert worst <= TOL_OUT


# ---- input kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["uint8", "uint16"])
def test_large_crops_host_and_device_give_the_same_bits(dt):
    """Host pixels to a host result (the staging path) and device pixels to a device result, CLAHE tap included; uint16 tensors
    go in as int16 views."""
    import torch
    for (_, hw, clip), group in _groups([c for c in PL.cases("large") if c["dtype"] == dt]).items():
        pix, off, hs, ws = pp.pack_crops([PL.crop(c) for c in group])
        p = pp.Preprocessor(0, out_hw=hw)
        try:
            host, hcl = p.run_packed(pix, off, hs, ws, clip, want_clahe=True)
            d_pix = torch.from_numpy(pix.view(np.int16) if dt == "uint16" else pix).cuda()
            d_out = torch.full((len(group),) + hw, -1.0, dtype=torch.float32, device="cuda")
            _, dcl = p.run_packed(d_pix, off, hs, ws, clip, out=d_out, want_clahe=True)
            torch.cuda.synchronize()
        finally:
            p.close()
        assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(host)), hw
        assert np.array_equal(dcl.cpu().numpy().view(np.uint16), hcl), hw
        assert host.min() >= 0.0 and host.max() <= 1.0


# ---- one handle: its buffers grow and are reused -----------------------------------------------------------------------------------
def test_small_then_the_largest_crop_then_small_again_on_one_handle():
    small = [PL.crop(c) for c in PL.cases("tiles")[0::98]]
    big = PL.crop(PL.cases("large")[0])
    assert big.shape == (1024, 1024) and big.dtype == small[0].dtype == np.uint8 and len(small) >= 4
    p = pp.Preprocessor(0)
    try:
        first, fcl = _run(p, small)
        bout, bcl = _run(p, [big])
        again, acl = _run(p, small)
        bout2, bcl2 = _run(p, [big])
    finally:
        p.close()
    assert np.array_equal(_bits(first), _bits(again)) and all(np.array_equal(a, b) for a, b in zip(fcl, acl))
    assert np.array_equal(_bits(bout), _bits(bout2)) and np.array_equal(bcl[0], bcl2[0])
    assert np.array_equal(bcl[0], PL.expected(PL.cases("large")[0])[0])
    for i, c in enumerate(PL.cases("tiles")[0::98]):
        assert np.array_equal(fcl[i], PL.expected(c)[0]), c["name"]


# ---- the pixel-span rule of the chunk loop ----------------------------------------------------------------------------------------
def test_a_chunk_ends_where_its_pixel_span_would_exceed_the_limit():
    """Crops spread over a device buffer slightly longer than kChunkPixels: the first chunk's span is the limit exactly, the
    next crop would make it one pixel more, the last crop ends with the buffer.  Each crop's cell and CLAHE plane are the bits of
    the same crops packed densely, and the pixels of last_timing are the two chunks' spans."""
    import torch
    limit = PL.CHUNK_PIXELS
    n_pix = limit + 300000
    picks = [PL.cases("tiles")[k] for k in (6, 200, 440, 700, 880)]
    assert all(c["dtype"] == "uint8" for c in picks)
    crops = [PL.crop(c) for c in picks]
    sizes = [c.size for c in crops]
    # crop 2 ends on the limit: with it the span is the limit itself, which a chunk may have; crop 3 lies beyond and opens the second
    off = np.array([0, 5000, limit - sizes[2], limit + 17, n_pix - sizes[4]], np.int64)
    assert off[2] + sizes[2] == limit and off[3] + sizes[3] > limit and off[4] + sizes[4] == n_pix and (np.diff(off) > 0).all()
    hs = np.array([c.shape[0] for c in crops], np.int32)
    ws = np.array([c.shape[1] for c in crops], np.int32)
    d_pix = torch.zeros(n_pix, dtype=torch.uint8, device="cuda")
    for o, c in zip(off, crops):
        d_pix[int(o):int(o) + c.size] = torch.from_numpy(np.array(c).ravel()).cuda()
    p = pp.Preprocessor(0)
    try:
        d_out = torch.full((len(crops), 64, 64), -1.0, dtype=torch.float32, device="cuda")
        _, d_cl = p.run_packed(d_pix, off, hs, ws, out=d_out, want_clahe=True)
        torch.cuda.synchronize()
        _, px = p.last_timing()
        spans = (off[2] + sizes[2] - off[0], off[4] + sizes[4] - off[3])
        assert spans[0] == limit and px == sum(int(s) for s in spans) and px < n_pix
        dense, dense_cl = _run(p, crops)
        assert p.last_timing()[1] == sum(sizes)
    finally:
        p.close()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(dense))
    for o, c, want in zip(off, crops, dense_cl):
        got = d_cl[int(o):int(o) + c.size].cpu().numpy().view(np.uint16).reshape(c.shape)
        assert np.array_equal(got, want), (int(o), c.shape)
    # between the crops the tap reads what the caller put there
    for a, b in ((off[1] + sizes[1], off[2]), (off[2] + sizes[2], off[3]), (off[3] + sizes[3], off[4])):
        assert int(torch.count_nonzero(d_cl[int(a):int(b)])) == 0


# ---- the refusals stay refusals ---------------------------------------------------------------------------------------------------
def test_sides_outside_the_limits_are_refused_and_the_handle_goes_on():
    good = [PL.crop(c) for c in PL.cases("radius") if c["hw"] == (8, 8) and c["dtype"] == "uint8"][:6]
    big = PL.crop(PL.cases("large")[14])
    assert big.shape == (512, 1024)
    for hw, ok, refused in (((64, 64), [PL.crop(PL.cases("large")[4]), PL.crop(PL.cases("large")[6])],
                             [((1025, 8), "above 1024"), ((8, 1025), "above 1024"), ((7, 8), "below 8 px"), ((8, 7), "below 8 px")]),
                            ((8, 8), good, [((129, 8), "16 times"), ((8, 129), "16 times"), ((1025, 8), "above 1024"), ((7, 9), "below 8 px")]),
                            ((32, 64), [big], [((513, 64), "16 times"), ((32, 1025), "above 1024"), ((7, 64), "below 8 px")])):
        p = pp.Preprocessor(0, out_hw=hw)
        try:
            want = p(ok)
            assert want.shape == (len(ok),) + hw
            for shape, text in refused:
                with pytest.raises(L.CellScreenError, match=text) as ei:
                    p([ok[0], np.zeros(shape, ok[0].dtype)])
                assert "crop 1" in str(ei.value) and f"{shape[0]}x{shape[1]}" in str(ei.value)
                assert ei.value.status == (-6 if text != "below 8 px" else -1), str(ei.value)
                assert np.array_equal(_bits(p(ok)), _bits(want)), (hw, shape)      # the handle takes a good call
        finally:
            p.close()
