"""Seeded weight families for the inference tests, for any instance (hw, channels, n_enc) of the layer grammar.

synth.random_cae draws what Keras initialises: Glorot kernels, zero biases, BN gains near 1.  A trained checkpoint has a
non-zero bias in every layer, dead filters, and BN gains that differ by orders of magnitude between channels.

* trained_like(seed, hw, channels, n_enc): such a weight set, calibrated by the float64 forward of this file alone so that
  every hidden layer's output has an RMS in [0.5, 2) and the sigmoid's argument stays within +-8 on the calibration crops
  (the absolute reconstruction bar then means something).
* compensated(w, k, seed): the same function with a third of every hidden layer's channels moved 2^-k below their
  neighbours (BN gain and shift times 2^-k, the next kernel's input channel times 2^k).
* forward64 / plain32_layer / channel_budget: the float64 forward with its pre-activations, one layer in plain float32,
  and the per-channel magnitude budget of a layer.

Test code only; nothing here touches the device."""
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from cellscreen import synth
from cellscreen.spec import CAEWeights

DEAD_MARGIN = 8.0            # |bias| of a dead / never-clipped filter >= this x max|response| on the calibration crops
FILTER_LOG2 = (-4, 2)        # per-filter powers of two on every kernel's output filters
GAMMA_LOG2 = (-4.0, 4.0)     # |gamma| log-uniform over 2^-4 .. 2^4
VAR_LOG10 = (-4.0, 2.0)      # variance log-uniform over 1e-4 .. 1e2
Z7_MAX = 8.0
REF_SEED = 2024              # the reference-graph draw test_gpu_weight_families.py runs
# The per-channel bar: |got - ref| <= PER_CHANNEL_TOL * B_c (channel_budget).  Plain float32 numpy, each layer from the
# oracle's input to it, on trained_like(REF_SEED) and edge_crops(): worst |err| / B_c per layer 1.2e-7, 1.2e-7, 1.4e-7,
# 1.6e-7, 9.8e-8, 1.1e-7 -- no layer exceeds 1e-5, so no layer needs a bar of its own.
PER_CHANNEL_TOL = 1e-5


@dataclass
class Family:
    """What trained_like put where: per hidden layer the filters with a special role (absent where the layer is too narrow)."""
    dead: List[np.ndarray] = field(default_factory=list)
    never_clipped: List[np.ndarray] = field(default_factory=list)
    gamma_zero: List[np.ndarray] = field(default_factory=list)
    var_zero: List[np.ndarray] = field(default_factory=list)
    var_tiny: List[np.ndarray] = field(default_factory=list)
    response_rms: List[np.ndarray] = field(default_factory=list)      # fp64 RMS of conv(x, k) per filter, every conv
    response_max: List[np.ndarray] = field(default_factory=list)      # max |conv(x, k)| per filter, every conv


def calibration_crops(seed, hw, n=4):
    """n counter-hash noise crops and n blob crops."""
    return np.concatenate([synth.synth_crops(seed, 0, n, hw=hw), synth.blob_crops(seed, n, hw=hw)])


# ---------------------------------------------------------------- a layer in float64 (and in plain float32)
def _conv3x3(x, k):
    """'same' 3x3 convolution, NHWC x HWIO, in the dtype of its arguments (no bias)."""
    n, h, w, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    z = np.zeros((n, h, w, k.shape[3]), x.dtype)
    for dy in range(3):
        for dx in range(3):
            z += xp[:, dy:dy + h, dx:dx + w, :] @ k[dy, dx]
    return z


def _pool(a):
    n, h, w, c = a.shape
    return a.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


def _ups(a):
    return a.repeat(2, axis=1).repeat(2, axis=2)


def layer_input(w, l, prev, dtype=np.float64):
    """What conv l reads: the crops (l = 0) or the previous layer's output, upsampled behind the bottleneck."""
    x = np.asarray(prev, dtype)
    if x.ndim == 3:
        x = x[..., None]
    return _ups(x) if l > w.n_enc else x


def _epilogue(w, l, z, s, t):
    if l == w.n_conv - 1:
        return 1.0 / (1.0 + np.exp(-z))
    a = np.maximum(z, 0) * s + t
    return _pool(a) if l < w.n_enc else a


def forward64(w, x, upto=None):
    """The float64 forward from float32 parameters (BN as the float32 scale and shift the library and the C oracle use):
    per layer dict(z=pre-activation with bias, out=the layer's output)."""
    s, t = w.bn_scale_shift()
    out, a = [], x
    for l in range(w.n_conv if upto is None else upto + 1):
        z = _conv3x3(layer_input(w, l, a), w.kernels[l].astype(np.float64)) + w.biases[l].astype(np.float64)
        hidden = l < w.n_conv - 1
        a = _epilogue(w, l, z, s[l].astype(np.float64) if hidden else None, t[l].astype(np.float64) if hidden else None)
        out.append(dict(z=z, out=a))
    return out


def plain32_layer(w, l, prev):
    """Layer l in plain float32 numpy -- float32 products, float32 accumulation -- from the float32 tensor `prev`."""
    s, t = w.bn_scale_shift()
    f = np.float32
    z = _conv3x3(layer_input(w, l, prev, f), w.kernels[l].astype(f)) + w.biases[l].astype(f)
    if l == w.n_conv - 1:
        return (f(1) / (f(1) + np.exp(-z))).astype(f)
    return _epilogue(w, l, z, s[l], t[l]).astype(f)


def channel_budget(w, l, prev):
    """B_c = |bn_scale_c| * max over pixels of (sum |a||w| + |b_c|) + |bn_shift_c| in float64, per filter of hidden layer
    l, from the tensor that layer reads: the magnitude every rounding of the channel's evaluation is relative to.  Never
    below the channel's own range."""
    s, t = w.bn_scale_shift()
    m = _conv3x3(np.abs(layer_input(w, l, prev)), np.abs(w.kernels[l].astype(np.float64))) + np.abs(w.biases[l].astype(np.float64))
    return np.abs(s[l].astype(np.float64)) * m.max(axis=(0, 1, 2)) + np.abs(t[l].astype(np.float64))


# ---------------------------------------------------------------- the families
def _pow2_into(v, lo):
    """The power of two p with v * p in [lo, 2 lo); 1 for v = 0."""
    return 2.0 ** -np.floor(np.log2(v / lo)) if v > 0 else 1.0


def trained_like(seed, hw=(64, 64), channels=(32, 64, 32, 32, 64, 32, 1), n_enc=3, with_info=False):
    """A CAEWeights as a trained checkpoint looks to the kernels (see the module docstring), drawn layer by layer:

    * every kernel's output filters times a power of two from 2^-4 .. 2^2;
    * every bias non-zero, mixed signs, 0.05 .. 1 times the float64 RMS of that filter's bias-free response conv(x, k)
      on the calibration crops; per hidden layer two dead filters (bias <= -8 max|response|: the output is the BN shift
      everywhere) and two that never clip (bias >= +8 max|response|);
    * gamma of mixed sign, |gamma| log-uniform over 2^-4 .. 2^4, one filter exactly 0; variance log-uniform over
      1e-4 .. 1e2, one filter 0 and one 1e-6; mean in +-2 RMS(response); beta in +-1;
    * then gamma and beta of each hidden layer times ONE power of two that puts the layer's float64 output RMS into [1, 2),
      and conv7's kernel and bias times one power of two that puts max|z7| into [4, 8).

    A layer narrower than 8 filters takes as many of the seven special roles as leave it one ordinary filter, in the
    order dead, never-clipped, gamma 0, variance 0, variance 1e-6, dead, never-clipped."""
    hw, channels = tuple(hw), tuple(channels)
    base = synth.random_cae(seed, hw=hw, channels=channels, n_enc=n_enc)
    rng = np.random.default_rng([seed, 0x7261])
    x = calibration_crops(seed, hw)
    w = CAEWeights([k.copy() for k in base.kernels], [b.copy() for b in base.biases], [g.copy() for g in base.bn_gamma],
                   [b.copy() for b in base.bn_beta], [m.copy() for m in base.bn_mean], [v.copy() for v in base.bn_var],
                   hw, n_enc, base.bn_eps)
    info = Family()
    n_conv = len(channels)
    a = x
    for l, cout in enumerate(channels):
        f32 = np.float32
        w.kernels[l] = (w.kernels[l] * (2.0 ** rng.integers(FILTER_LOG2[0], FILTER_LOG2[1] + 1, cout))).astype(f32)
        resp = _conv3x3(layer_input(w, l, a), w.kernels[l].astype(np.float64))
        rms = np.sqrt((resp * resp).mean(axis=(0, 1, 2)))
        top = np.abs(resp).max(axis=(0, 1, 2))
        info.response_rms.append(rms); info.response_max.append(top)
        unit = np.where(rms > 0, rms, 1.0)                     # a filter that reads only constant-zero channels
        bias = rng.choice([-1.0, 1.0], cout) * rng.uniform(0.05, 1.0, cout) * unit
        if l == n_conv - 1:
            z = resp + bias
            p = _pow2_into(np.abs(z).max(), Z7_MAX / 2)
            w.kernels[l] = (w.kernels[l] * p).astype(f32)
            w.biases[l] = (bias * p).astype(f32)
            info.response_rms[l], info.response_max[l] = rms * p, top * p
            break
        roles = rng.permutation(cout)[:max(0, min(7, cout - 1))]
        role = lambda i: roles[i:i + 1] if i < len(roles) else roles[:0]
        dead, never = np.concatenate([role(0), role(5)]), np.concatenate([role(1), role(6)])
        g0, v0, v6 = role(2), role(3), role(4)
        big = np.maximum(top, unit)
        bias[dead] = -(DEAD_MARGIN + rng.uniform(0.5, 2.0, len(dead))) * big[dead]
        bias[never] = (DEAD_MARGIN + rng.uniform(0.5, 2.0, len(never))) * big[never]
        w.biases[l] = bias.astype(f32)
        gamma = rng.choice([-1.0, 1.0], cout) * 2.0 ** rng.uniform(*GAMMA_LOG2, cout)
        var = 10.0 ** rng.uniform(*VAR_LOG10, cout)
        gamma[g0], var[v0], var[v6] = 0.0, 0.0, 1e-6
        w.bn_gamma[l], w.bn_var[l] = gamma.astype(f32), var.astype(f32)
        w.bn_mean[l] = (rng.uniform(-2.0, 2.0, cout) * unit).astype(f32)
        w.bn_beta[l] = rng.uniform(-1.0, 1.0, cout).astype(f32)
        for lst, idx in ((info.dead, dead), (info.never_clipped, never), (info.gamma_zero, g0), (info.var_zero, v0), (info.var_tiny, v6)):
            lst.append(np.sort(idx))
        # one power of two on gamma and beta: BN's scale and shift, hence the whole layer, scale by exactly that
        s, t = w.bn_scale_shift()
        out = _epilogue(w, l, resp + w.biases[l].astype(np.float64), s[l].astype(np.float64), t[l].astype(np.float64))
        p = _pow2_into(np.sqrt((out * out).mean()), 1.0)
        w.bn_gamma[l] = (w.bn_gamma[l] * f32(p)).astype(f32)
        w.bn_beta[l] = (w.bn_beta[l] * f32(p)).astype(f32)
        a = out * p
    w.validate()
    return (w, info) if with_info else w


def compensated_channels(w, seed):
    """The third of every hidden layer's channels that compensated() moves, per layer."""
    rng = np.random.default_rng([seed, 0x636f])
    return [np.sort(rng.choice(c, max(1, c // 3), replace=False)) for c in w.channels[:-1]]


def compensated(w, k, seed=0):
    """The same function as w: for a third of the channels c of every hidden layer l, bn_gamma[l][c] and bn_beta[l][c]
    times 2^-k and kernels[l + 1][:, :, c, :] times 2^k -- all exact in float32.  Channel c then sits 2^-k below its
    cell's maximum and the boosted weights are their layer's largest."""
    c = CAEWeights([a.copy() for a in w.kernels], [a.copy() for a in w.biases], [a.copy() for a in w.bn_gamma],
                   [a.copy() for a in w.bn_beta], [a.copy() for a in w.bn_mean], [a.copy() for a in w.bn_var],
                   w.input_hw, w.n_enc, w.bn_eps)
    down, up = np.float32(2.0 ** -k), np.float32(2.0 ** k)
    for l, ch in enumerate(compensated_channels(w, seed)):
        c.bn_gamma[l][ch] *= down
        c.bn_beta[l][ch] *= down
        c.kernels[l + 1][:, :, ch, :] *= up
    return c.validate()


def uncompensate(layer_out, l, w, k, seed=0):
    """A hidden layer's output under compensated(w, k, seed) brought back to w's scale (exact: a power of two)."""
    out = np.array(layer_out, copy=True)
    shape = out.shape
    out = out.reshape(shape[0], -1, w.channels[l])
    out[..., compensated_channels(w, seed)[l]] *= out.dtype.type(2.0 ** k)
    return out.reshape(shape)


def edge_crops(hw=(64, 64), n=12, seed=3):
    """n >= 6 crops: a zero cell, an all-ones cell, row stripes, column stripes, then blobs and noise in turn."""
    x = synth.synth_crops(seed, 50, n, hw=hw)
    x[2::2] = synth.blob_crops(seed, len(x[2::2]), hw=hw)
    x[0] = 0.0
    x[1] = 1.0
    x[2, ::2] = 0.0
    x[3, :, ::2] = 0.0
    return x


# ---------------------------------------------------------------- the run-time-shaped cases of test_gpu_weight_families.py
# A subset of generic_plans.SWEEP_CASES that reaches every (kernel instantiation, precision) the whole list reaches,
# chosen greedily (most of those not yet reached first, the fewest multiply-adds per cell among equals):
# greedy_cover() returns exactly this list, test_weight_families_cpu.py checks it.
GENERIC_CASES = [
    ((64, 128), (32, 64, 128, 128, 64, 32, 1), 3),
    ((128, 128), (4, 12, 20, 40, 20, 12, 1), 3),
    ((8, 64), (32, 72, 1), 1),
    ((48, 96), (12, 100, 1), 1),
    ((112, 64), (32, 64, 128, 64, 1), 2),
    ((8, 32), (20, 16, 1), 1),
    ((32, 64), (16, 64, 32, 16, 1), 2),
    ((8, 32), (128, 128, 1), 1),
    ((16, 128), (32, 32, 32, 1, 32, 32, 1), 3),
    ((272, 128), (16, 32, 1), 1),
]
# compensated(k = 12) runs on these: between them conv_generic_x3_kernel plain and folded, conv_last_x3_kernel<32> and <64>
GENERIC_COMPENSATED = [GENERIC_CASES[0], GENERIC_CASES[4]]


def greedy_cover(cases):
    """(the chosen (hw, channels, n_enc) in order, every (instantiation, precision) `cases` reach)."""
    import generic_plans as G
    from cellscreen import spec
    pts = [tuple(c[:3]) for c in cases]
    reach = {p: {(k, prec) for prec in ("split16", "fp32_exact") for k in G.instantiations(points=[p], precisions=(prec,))}
             for p in pts}
    macs = {p: sum(r["macs"] for r in spec.layer_table(*p)) for p in pts}
    full = set().union(*reach.values())
    left, chosen = set(full), []
    while left:
        best = max(pts, key=lambda p: (len(reach[p] & left), -macs[p]))
        chosen.append(best)
        left -= reach[best]
    return chosen, full
