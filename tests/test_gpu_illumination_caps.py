"""The flat-field correction at its caps on the device: the scenes of tests/illumination_caps.py, every output np.array_equal to
tests/illumination_reference.py.  A scene with an image runs the tile statistic, the function of its own meshes and the
correction with its counts, as its entry names; a scene with a stack runs the reduction by rank and by the mean."""
import numpy as np
import pytest

import illumination_caps as IC
import illumination_reference as IR
import smooth_reference as SR
from cellscreen import illumination as IL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ic():
    c = IL.IlluminationCorrector(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", [n for n, s in IC.SCENES.items() if "image" in s])
def test_image_scenes_at_the_caps(ic, name):
    scene = IC.SCENES[name]
    image, T = scene["image"](), scene["tile"]
    Cn = image.shape[3] if image.ndim == 4 else 1
    want = IR.tile_stats(image, T)
    got = ic.tile_stats_batch(image, T)
    assert got.shape == want.shape and np.array_equal(got, want)
    if name == "sides":
        assert want.shape[2:] == (IC.CAPS["kIlMaxMesh"],) * 2
    if "apply" not in scene["tools"]:
        return
    stack = np.ascontiguousarray(want[:64])                              # the function of the first fields' meshes
    F8 = IR.reduce(stack, (1, 2), 3, 1)
    assert np.array_equal(ic.reduce_stack(stack, IL.reduce_params(Cn, (1, 2), 3, 1)), F8)
    fn = IL.IlluminationFunction(tile=T, shape=image.shape[1:3], channels=Cn, dtype=image.dtype, F8=F8, G8=IR.scale(F8), offset=[3] * Cn)
    out, clipped = ic.apply_batch(image, fn, return_clipped=True)
    want_out, want_clipped = IR.apply(image, F8, fn.G8, T, 3)
    assert np.array_equal(out, want_out) and np.array_equal(clipped, want_clipped)
    assert np.array_equal(out[-1].ravel()[-8:], want_out[-1].ravel()[-8:])          # the last pixels of the last field


@pytest.mark.parametrize("name", [n for n, s in IC.SCENES.items() if "stack" in s])
def test_stack_scenes_at_the_caps(ic, name):
    scene = IC.SCENES[name]
    stack = scene["stack"]()
    Cn = stack.shape[1]
    off = list(range(Cn))
    assert np.array_equal(ic.reduce_stack(stack, IL.reduce_params(Cn, (1, 2), off, 2)), IR.reduce(stack, (1, 2), off, 2))
    assert np.array_equal(ic.reduce_stack(stack, IL.reduce_params(Cn, "mean", off, 2)), IR.reduce(stack, "mean", off, 2))
    if scene.get("filters"):
        got = ic.reduce_stack(stack, IL.reduce_params(Cn, (1, 4), off, 2, True, 16.0))       # radius 64
        assert np.array_equal(got, IR.reduce(stack, (1, 4), off, 2, True, SR.smooth_weights(16.0)))
