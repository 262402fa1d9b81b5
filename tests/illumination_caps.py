"""The flat-field correction at the caps it accepts (cs_illum_tile_stats, cs_illum_reduce, cs_illum_apply): the caps
read out of csrc/illumination.hip, one entry per tool, and the scenes that sit on them, in the manner of tests/label_caps.py,
whose tables hold the tools that were there before these.  Nothing here touches a device: tests/test_illumination_cpu.py holds
this file to the sources, tests/test_gpu_illumination_caps.py runs the scenes against tests/illumination_reference.py.

  CAPS     kIlMaxChannels, kIlMaxImages, kIlMaxMesh, kIlMaxStack as illumination.hip declares them; kMaxSide and kMaxBatch are
           label_caps'
  TOOLS    per tool its entry point and the caps that bind it besides the sides and the batch
  SCENES   sides      one 4096 x 4096 field at T = 16: a mesh of kIlMaxMesh x kIlMaxMesh nodes, 65536 workgroups of il_stats, the
                      last pixel's index H * W - 1 in il_apply
           channels   kIlMaxChannels channels: 4096 x 4096 at T = 256 for the statistic (tiles of 65536 pixels, read again in every
                      pass), 4096 x 512 for the correction
           batch      kMaxBatch fields of 16 x 17: grid.z and grid.y = 65535, the base b * H * W * C of the last field
           images     kIlMaxImages meshes of kIlMaxChannels x 2 x 2 nodes
           mesh       16 meshes of kIlMaxChannels x kIlMaxMesh x kIlMaxMesh nodes, with both filters at the widest radius
The stack cap kIlMaxStack (2^28 values, 1 GiB) is met by no scene: the refusal one past it is in tests/test_illumination_cpu.py, and
il_across indexes with size_t, k * nodes + node < 2^28."""
import os
import re

import numpy as np

import label_caps as LC

CSRC = LC.CSRC
CAP_SOURCES = {"kIlMaxChannels": "int", "kIlMaxImages": "int", "kIlMaxMesh": "int", "kIlMaxStack": "int64_t"}


def _source():
    with open(os.path.join(CSRC, "illumination.hip")) as f:
        return f.read()


def read_caps():
    """{name: value}: `static constexpr <type> <name> = <a literal or a shift>;` as illumination.hip declares it."""
    out, text = {}, _source()
    for name, ctype in CAP_SOURCES.items():
        m = re.search(rf"static constexpr {ctype} {name} = (?:\(int64_t\))?(\d+)(?: << (\d+))?;", text)
        assert m, f"{name} is not declared in illumination.hip as the suite reads it"
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def declared_entry_points():
    """The cs_illum_* entry points of cellscreen/_lib.py that run a batch on the handle: those whose definition opens the shared
    state through il_begin(."""
    with open(os.path.join(LC.PKG, "_lib.py")) as f:
        names = re.findall(r'^\s*"(cs_illum_\w+)":', f.read(), re.M)
    body = LC.defined_entry_points()
    assert set(names) <= set(body)
    return sorted(n for n in names if "il_begin(" in body[n])


CAPS = read_caps()
MAX_SIDE, MAX_BATCH = LC.MAX_SIDE, LC.MAX_BATCH
TOOLS = {
    "tile_stats": dict(entry="cs_illum_tile_stats", caps=("kIlMaxChannels",)),
    "reduce": dict(entry="cs_illum_reduce", caps=("kIlMaxChannels", "kIlMaxImages", "kIlMaxMesh", "kIlMaxStack")),
    "apply": dict(entry="cs_illum_apply", caps=("kIlMaxChannels", "kIlMaxMesh")),
}


def _noise(shape, dtype, seed):
    return np.random.default_rng(seed).integers(0, int(np.iinfo(dtype).max) + 1, shape, dtype=dtype)


# name -> (tool, the cap it sits on, a function that makes its inputs)
SCENES = {
    "sides": dict(tools=("tile_stats", "reduce", "apply"), cap="kMaxSide", tile=16,
                  image=lambda: _noise((1, MAX_SIDE, MAX_SIDE), np.uint16, 1)),
    "channels-stats": dict(tools=("tile_stats",), cap="kIlMaxChannels", tile=256,
                           image=lambda: _noise((1, MAX_SIDE, MAX_SIDE, CAPS["kIlMaxChannels"]), np.uint8, 2)),
    "channels-apply": dict(tools=("tile_stats", "reduce", "apply"), cap="kIlMaxChannels", tile=256,
                           image=lambda: _noise((1, MAX_SIDE, 512, CAPS["kIlMaxChannels"]), np.uint8, 3)),
    "batch": dict(tools=("tile_stats", "reduce", "apply"), cap="kMaxBatch", tile=16, image=lambda: _noise((MAX_BATCH, 16, 17), np.uint8, 4)),
    "images": dict(tools=("reduce",), cap="kIlMaxImages",
                   stack=lambda: _noise((CAPS["kIlMaxImages"], CAPS["kIlMaxChannels"], 2, 2), np.uint16, 5).astype(np.int32)),
    "mesh": dict(tools=("reduce",), cap="kIlMaxMesh", filters=True,
                 stack=lambda: _noise((16, CAPS["kIlMaxChannels"], CAPS["kIlMaxMesh"], CAPS["kIlMaxMesh"]), np.uint16, 6).astype(np.int32)),
}
