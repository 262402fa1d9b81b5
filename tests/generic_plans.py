"""A plain restatement of how libcellscreen serves a non-reference instance of the layer grammar: which shapes it accepts
(engine and trainer), and for each conv which run-time-shaped kernel runs, at which template width, with which plan,
how many work items per cell and how many workgroups.  Test code only: it is tied to the library by
test_generic_envelope_cpu.py (acceptance) and test_gpu_generic_sweep.py (which kernel class ran), never by a C ABI.

Each function cites the lines of cell-image-analysis_amd/csrc/ that it restates; a change there must change this file.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

CUS = 256                       # MI355X compute units (hipDeviceAttributeMultiprocessorCount)
GEN_SR = 2                      # conv_generic.hip:21
REF = ((64, 64), (32, 64, 32, 32, 64, 32, 1), 3)        # api_internal.hpp kH, kW, kRefChannels, kNEnc
KB = 1024


# ---------------------------------------------------------------- acceptance
def conv_generic_supported(H, W, cin, cout) -> Optional[str]:
    """conv_generic.hip:714-726.  None or the rule that refuses."""
    if W % 16 != 0 or W < 16 or W > 128 or H % 2 != 0:
        return "grid"
    if not (cin == 1 or cin % 4 == 0):
        return "cin"
    if cout < 1:
        return "cout"
    if 4 * (W + 2) * (cin + 4) * 4 > 160 * KB:
        return "lds"
    return None


@dataclass
class Arch:
    hw: Tuple[int, int]
    ch: Tuple[int, ...]
    n_enc: int
    gh: List[int] = field(default_factory=list)
    gw: List[int] = field(default_factory=list)

    @property
    def n_conv(self):
        return len(self.ch)

    def cin(self, l):
        return 1 if l == 0 else self.ch[l - 1]

    @property
    def ref(self):
        return (tuple(self.hw), tuple(self.ch), self.n_enc) == REF


@dataclass
class Refused:
    layer: int          # -1: the whole architecture
    rule: str


def grids(hw, channels, n_enc) -> Arch:
    """api.hip:170-176 (the stored size of the tensor each conv reads; the trainer's is the same, train_api.hip:81-89)."""
    a = Arch(tuple(hw), tuple(channels), n_enc)
    h, w = hw
    for l in range(len(channels)):
        if l > n_enc:
            h, w = h * 2, w * 2
        a.gh.append(h); a.gw.append(w)
        if l < n_enc:
            h, w = h // 2, w // 2
    return a


def _grammar(hw, channels, n_enc, max_conv):
    """api.hip:159-169 / train_api.hip:74-92: the checks both share, in their order."""
    H, W = hw
    n_conv = len(channels)
    if n_conv < 3 or n_conv > max_conv or n_enc < 1 or n_conv != 2 * n_enc + 1:
        return Refused(-1, "grammar")
    if H <= 0 or W <= 0 or H % (1 << n_enc) or W % (1 << n_enc):
        return Refused(-1, "divisible")
    if any(c <= 0 for c in channels):
        return Refused(-1, "filters")
    if channels[-1] != 1:
        return Refused(-1, "last")
    return None


def describe_arch(hw, channels, n_enc):
    """api.hip:155-190 (CS_MAX_CONV = 16): an Arch or a Refused."""
    r = _grammar(hw, channels, n_enc, 16)
    if r:
        return r
    a = grids(hw, channels, n_enc)
    if not a.ref:
        for l in range(a.n_conv):
            why = conv_generic_supported(a.gh[l], a.gw[l], a.cin(l), a.ch[l])
            if why:
                return Refused(l, why)
    return a


def wgrad_generic_lds_bytes(W, cin, cout):
    """train_generic.hip:206-210."""
    pad = lambda c: c + ((48 - (c & 31)) & 31)
    return (3 * (W + 2) * pad(cin) + W * pad(cout)) * 4


def describe_trainer(hw, channels, n_enc):
    """train_api.hip:70-115 (TR_MAXL = 7): None (accepted) or a Refused."""
    r = _grammar(hw, channels, n_enc, 7)
    if r:
        return r
    a = grids(hw, channels, n_enc)
    if a.ref:
        return None
    pow2 = lambda v: v > 0 and (v & (v - 1)) == 0
    for l in range(a.n_conv):
        why = conv_generic_supported(a.gh[l], a.gw[l], a.cin(l), a.ch[l])
        if why:
            return Refused(l, why)
        if l > 0 and conv_generic_supported(a.gh[l], a.gw[l], a.ch[l], a.cin(l)):
            return Refused(l, "backward-data " + conv_generic_supported(a.gh[l], a.gw[l], a.ch[l], a.cin(l)))
        if l < a.n_conv - 1 and (not pow2(a.gh[l]) or not pow2(a.gw[l]) or not pow2(a.ch[l]) or a.ch[l] < 4 or a.ch[l] > 256):
            return Refused(l, "pow2")
        if wgrad_generic_lds_bytes(a.gw[l], a.cin(l), a.ch[l]) > 160 * KB:
            return Refused(l, "wgrad-lds")
    return None


# ---------------------------------------------------------------- plans
def gen2_plan(H, W, cin, cout, ups):
    """conv_generic.hip:729-748: (SR, nmg, nslw, tpw, lds) or None."""
    if not (cin % 16 == 0 or (cin == 1 and not ups)) or W not in (16, 32, 64, 128) or cout < 16:
        return None
    slices = (cout + 15) // 16
    ns = 1
    while ns * 2 <= slices and ns < 8:
        ns *= 2
    mg, TPR, Ws, ps = 8 // ns, W // 16, W // 2 if ups else W, 1 if cin == 1 else cin + 4
    for t in (16, 8, 4):
        pairs = (t // 2) * mg
        if pairs % TPR:
            continue
        sr = 2 * pairs // TPR
        if sr < 2 or H % sr:
            continue
        R = sr // 2 + 2 if ups else sr + 2
        lds = R * (Ws + 2) * ps * 4
        if lds > 100 * KB:
            continue
        return sr, mg, ns, t, lds
    return None


def gen2f_plan(H, W, cin, cout):
    """conv_generic.hip:751-769."""
    Ws = W // 2
    if cin % 16 != 0 or Ws not in (16, 32, 64) or cout < 32:
        return None
    slices = (cout + 15) // 16
    ns = 2
    while ns * 2 <= slices and ns < 8:
        ns *= 2
    mg, TPRs, ps = 8 // ns, Ws // 16, cin + 4
    for t in (16, 8, 4):
        if t % TPRs:
            continue
        srs = t // TPRs
        if srs < 1 or (H // 2) % srs:
            continue
        lds = (srs + 2) * (Ws + 2) * ps * 4
        if lds > 100 * KB:
            continue
        return 2 * srs, mg, ns, t, lds
    return None


X3_MAX_LDS = 150 * KB           # conv_generic_x3.hip:443


def x3_plan(H, W, cin, cout):
    """conv_generic_x3.hip:447-466."""
    if cin not in (32, 64, 128) or W not in (16, 32, 64, 128) or cout < 16:
        return None
    slices = (cout + 15) // 16
    ns = 1
    while ns * 2 <= slices and ns < 8:
        ns *= 2
    mg, TPR, psb = 8 // ns, W // 16, 6 * cin + 32
    for t in (8, 4):
        pairs = (t // 2) * mg
        if pairs % TPR:
            continue
        sr = 2 * pairs // TPR
        if sr < 2 or H % sr:
            continue
        lds = (sr + 2) * (W + 2) * psb
        if lds > X3_MAX_LDS:
            continue
        return sr, mg, ns, t, lds
    return None


def x3f_plan(H, W, cin, cout):
    """conv_generic_x3.hip:469-488."""
    Ws = W // 2
    if cin not in (32, 64, 128) or Ws not in (16, 32, 64) or cout < 32:
        return None
    slices = (cout + 15) // 16
    ns = 2
    while ns * 2 <= slices and ns < 8:
        ns *= 2
    mg, TPRs, psb = 8 // ns, Ws // 16, 6 * cin + 32
    for t in (8, 4):
        if t % TPRs:
            continue
        srs = t // TPRs
        if srs < 1 or (H // 2) % srs:
            continue
        lds = (srs + 2) * (Ws + 2) * psb
        if lds > X3_MAX_LDS:
            continue
        return 2 * srs, mg, ns, t, lds
    return None


def last_x3_plan(H, W, cin):
    """conv_generic_x3.hip:597-612: (SRS, NT, P, lds) or None."""
    if cin not in (32, 64) or H % 2 or W % 2:
        return None
    Hs, Ws, psb = H // 2, W // 2, 6 * cin + 32
    for srs in (8, 4, 2, 1):
        if Hs % srs:
            continue
        npx = (srs + 2) * (Ws + 2)
        nt = (npx + 15) // 16
        p = ((nt * 16 + 7) & ~7) + 4
        lds = nt * 16 * psb + 16 * p * 4
        if lds > 150 * KB:
            continue
        return srs, nt, p, lds
    return None


@dataclass
class LayerPlan:
    layer: int
    kernel: str          # the instantiation the launcher picks, e.g. "conv_generic2_kernel<8>"
    grid_hw: Tuple[int, int]
    cin: int
    cout: int
    split: bool          # a 16-bit-pipe split kernel (cs_profile_bf16_mfma_per_cell > 0 at this position)
    sr: int              # conv rows (SR) or stored rows (SRS) per strip
    tpw: int             # tiles per wave (0: no such parameter)
    nslw: int            # 16-filter slices per pass (0: none)
    items_per_cell: int
    cap: int             # the launch's grid = min(items, cap)

    def grid(self, n):
        return min(n * self.items_per_cell, self.cap)


def _layer_plan(a: Arch, l: int, split16: bool, cus: int) -> LayerPlan:
    H, W, cin, cout = a.gh[l], a.gw[l], a.cin(l), a.ch[l]
    last, ups = l == a.n_conv - 1, l > a.n_enc
    epi_sigmoid, epi_bn = last, not last and l >= a.n_enc
    mk = lambda k, split, sr, tpw, nslw, ipc, cap: LayerPlan(l, k, (H, W), cin, cout, split, sr, tpw, nslw, ipc, cap)
    # pack_generic, api.hip:318-347: which forms a layer is packed in
    folded = ups and ((not last and gen2f_plan(H, W, cin, cout) is not None) or (last and cout == 1 and cin % 4 == 0))
    x3 = False
    if folded:
        if split16 and last and cout == 1 and last_x3_plan(H, W, cin):
            x3 = True
        if split16 and not last and x3f_plan(H, W, cin, cout):
            x3 = True
    elif split16 and l <= a.n_enc and not last and x3_plan(H, W, cin, cout):
        x3 = True
    # run_convs_generic, api.hip:503-518
    if x3 and last:                                       # launch_conv_last_x3, conv_generic_x3.hip:637-660
        srs, _, _, lds = last_x3_plan(H, W, cin)
        return mk(f"conv_last_x3_kernel<{cin}>", True, srs, 0, 0, (H // 2) // srs, cus * (2 if lds <= 76 * KB else 1))
    if x3:                                                # launch_conv_generic_x3, conv_generic_x3.hip:544-594 (H2 form:
        sr, _, ns, tpw, _ = (x3f_plan(H, W, cin, cout) if ups else x3_plan(H, W, cin, cout))   # h2_inv != 0 always)
        Ws, R = (W // 2, sr // 2 + 2) if ups else (W, sr + 2)
        lds = R * (Ws + 2) * (4 * cin + 32) + 16
        per_cu = 2 if tpw <= 8 and lds <= 76 * KB else 1
        form = "fold" if ups else "plain"
        return mk(f"conv_generic_x3_kernel<{cin},{tpw},{form}>", True, sr, tpw, ns,
                  (H // sr) * ((cout + ns * 16 - 1) // (ns * 16)), cus * per_cu)
    # launch_conv_generic, conv_generic.hip:801-926
    ps = 1 if cin == 1 else cin + 4
    if cout == 1 and epi_sigmoid and ups and folded and cin % 4 == 0 and cin >= 4:
        Hs, Ws = H // 2, W // 2
        srs = 4 if Hs % 4 == 0 else (2 if Hs % 2 == 0 else 1)
        if ((srs + 2) * (Ws + 2) * ps + 16 * cin) * 4 <= 64 * KB:
            return mk("conv_last_folded_kernel", False, srs, 0, 0, Hs // srs, cus * 8)
    if cout == 1 and epi_sigmoid and cin % 4 == 0 and cin >= 4:
        sr = 4 if H % 4 == 0 else 2
        Ws, R = (W // 2, sr // 2 + 2) if ups else (W, sr + 2)
        if (R * (Ws + 2) * ps + 9 * cin) * 4 <= 64 * KB:
            return mk("conv_last_generic_kernel", False, sr, 0, 0, H // sr, cus * 8)
    p = gen2f_plan(H, W, cin, cout) if ups and folded and epi_bn else None
    if p:
        sr, _, ns, tpw, lds = p
        return mk(f"conv_generic2f_kernel<{tpw}>", False, sr, tpw, ns, (H // sr) * ((cout + ns * 16 - 1) // (ns * 16)),
                  cus * (2 if lds <= 76 * KB else 1))
    p = gen2_plan(H, W, cin, cout, ups)
    if p:
        sr, _, ns, tpw, lds = p
        name = "conv_generic_c1_kernel" if cin == 1 else "conv_generic2_kernel"
        return mk(f"{name}<{tpw}>", False, sr, tpw, ns, (H // sr) * ((cout + ns * 16 - 1) // (ns * 16)),
                  cus * (2 if lds <= 76 * KB else 1))
    tps = GEN_SR * W // 16
    assert tps in (2, 4, 6, 8, 10, 12, 14, 16), tps
    return mk(f"conv_generic_kernel<{tps}>", False, GEN_SR, 0, 0, (H // GEN_SR) * ((cout + 63) // 64), cus * 8)


def plan(hw, channels, n_enc, precision="split16", cus=CUS):
    """A Refused, the string "reference" (the fixed 64x64 graph, not this module's business), or one LayerPlan per conv."""
    assert precision in ("split16", "fp32_exact")
    a = describe_arch(hw, channels, n_enc)
    if isinstance(a, Refused):
        return a
    if a.ref:
        return "reference"
    return [_layer_plan(a, l, precision == "split16", cus) for l in range(a.n_conv)]


def final_round_cells(lp: LayerPlan, n):
    """Cells that a workgroup reaches only on the launch's last, ragged trip round the grid-stride loop (items are
    cell-major in every kernel: item = (cell * strips + strip) * slices + slice)."""
    items, g = n * lp.items_per_cell, lp.grid(n)
    first = (items // g) * g
    return sorted({i // lp.items_per_cell for i in range(first, items)})


# ---------------------------------------------------------------- the enumerated envelope
HW_STEPS = range(8, 273, 8)
N_ENCS = (1, 2, 3)
PROBE = (1, 4, 12, 20, 40, 72, 76, 100, 128, 256)


def channel_sets(n_enc):
    """Filter counts per conv: every probe value as all hidden layers, as the first layer alone (the rest 16), and as the
    bottleneck alone, plus two mixed sets; the last conv always has 1 filter."""
    nh = 2 * n_enc
    out = []
    for c in PROBE:
        out.append((c,) * nh + (1,))
        out.append((c,) + (16,) * (nh - 1) + (1,))
        out.append((32,) * (n_enc) + (c,) + (32,) * (n_enc - 1) + (1,))
    out.append(tuple([32, 64, 128, 128, 64, 32][:n_enc] + [128, 64, 32, 32, 16, 16][:n_enc]) + (1,))
    out.append(tuple(([8, 16, 32][:n_enc] + [32, 16, 8][-n_enc:])) + (1,))
    return sorted(set(out))


# off the grid: the rules it cannot reach (odd filter counts, sizes not divisible by 2^n_enc, the grammar, H = 4 mod 8)
EXTRA = [((64, 64), (16, 18, 1), 1), ((64, 64), (18, 16, 1), 1), ((20, 128), (16, 32, 64, 64, 32, 16, 1), 3),
         ((64, 64), (16, 32, 16, 1), 1), ((64, 64), (16, 16, 4), 1), ((44, 64), (32, 64, 1), 1), ((52, 128), (16, 32, 1), 1)]


def envelope():
    """Every (hw, channels, n_enc) point of the enumerated grid, then EXTRA."""
    yield from EXTRA
    for n_enc in N_ENCS:
        sets = channel_sets(n_enc)
        for H in HW_STEPS:
            for W in HW_STEPS:
                for ch in sets:
                    yield (H, W), ch, n_enc


def instantiations(points=None, precisions=("split16", "fp32_exact")):
    """{kernel instantiation: first (hw, channels, n_enc, precision, layer) that reaches it} over the enumerated grid."""
    seen = {}
    for hw, ch, ne in (points if points is not None else envelope()):
        for prec in precisions:
            p = plan(hw, ch, ne, prec)
            if isinstance(p, list):
                for lp in p:
                    seen.setdefault(lp.kernel, (hw, ch, ne, prec, lp.layer))
    return seen


# ---------------------------------------------------------------- the GPU sweep's case list (test_gpu_generic_sweep.py)
# (hw, channels, n_enc, why).  test_generic_envelope_cpu.py checks that these reach every instantiation of the grid above.
SWEEP_CASES = [
    ((48, 128), (16, 72, 1), 1, "n_enc 1; cin 72 at grid 128, the largest accepted there; H 48"),
    ((16, 128), (148, 16, 1), 1, "cin 148 at grid 64, the largest accepted there"),
    ((48, 96), (12, 100, 1), 1, "W 96: grids 96 and 48; cin 100 at grid 96 (the largest); cout 12"),
    ((80, 96), (200, 20, 1), 1, "cin 200 at grid 48 (the largest); H 80"),
    ((32, 128), (16, 296, 564, 16, 16, 16, 1), 3, "cin 296 at grid 32 and 564 at grid 16 (the largest)"),
    ((64, 64), (32, 100, 1, 100, 1), 2, "cout 100; hidden cout 1; cin 1 behind an upsample; conv_last_generic"),
    ((32, 64), (1, 16, 1), 1, "first conv with 1 filter, cin 1 after it"),
    ((112, 64), (32, 64, 128, 64, 1), 2, "H 112; conv_last_x3<64>"),
    ((144, 128), (32, 64, 1), 1, "H 144; conv_last_x3<64> with its smallest strip"),
    ((44, 64), (32, 64, 1), 1, "H 44: the last conv's strips of 2 stored rows"),
    ((8, 32), (32, 128, 1), 1, "tiny grids: 4-tile plans"),
    ((8, 128), (32, 32, 128, 32, 1), 2, "4-tile plain and folded plans"),
    ((8, 32), (20, 16, 1), 1, "cout 20 on the cin-1 kernel"),
    ((8, 32), (72, 16, 1), 1, "cout 72 on the cin-1 kernel"),
    ((8, 32), (128, 128, 1), 1, "cin 128 split kernel, 4 tiles"),
    ((16, 128), (32, 32, 32, 1, 32, 32, 1), 3, "a 1-filter bottleneck"),
    ((8, 64), (32, 64, 128, 64, 1), 2, "n_enc 2, 8-row input"),
    ((8, 64), (32, 32, 1, 32, 1), 2, "n_enc 2, 1-filter bottleneck"),
    ((8, 64), (32, 72, 1), 1, "cin 72 into the last conv"),
    ((64, 128), (32, 64, 128, 128, 64, 32, 1), 3, "the 8-tile split plans (BASELINE.json configs[4] filters)"),
    ((128, 128), (4, 12, 20, 40, 20, 12, 1), 3, "filters below 16 everywhere"),
    ((272, 128), (16, 32, 1), 1, "the tallest input of the grid"),
    ((96, 96), (40, 40, 1), 1, "W 96, cin 40 into the last conv"),
    ((64, 128), (8, 16, 1), 1, "n_enc 1, trainer-sized"),
    ((32, 64), (16, 64, 32, 16, 1), 2, "n_enc 2, trainer-sized"),
    ((48, 64), (64, 32, 1), 1, "H 48, cin 64 split kernel, 4 tiles"),
]

# just outside the envelope: (hw, channels, n_enc, the rule the restatement names)
ENGINE_REFUSALS = [
    ((48, 128), (16, 76, 1), 1, "lds"),                              # cin 76 at grid 128
    ((64, 64), (16, 32, 64, 64, 32, 16, 1), 3, "grid"),              # a grid 8 wide
    ((42, 64), (16, 32, 1), 1, "grid"),                              # grid 21 high
]
TRAINER_REFUSALS = [
    ((48, 64), (16, 32, 1), 1, "pow2"),                              # engine-accepted, grid 48 high
    ((32, 64), (2, 16, 1), 1, "pow2"),                               # 2 filters
    ((32, 64), (512, 16, 1), 1, "pow2"),                             # 512 filters
    ((8, 128), (256, 16, 1), 1, "wgrad-lds"),                        # the first conv's weight gradient
]


def persistent_n(hw, channels, n_enc, cus=CUS):
    """The smallest cell count at which every launch of both precisions has at least 3 items per workgroup and a
    ragged last round (items mod grid != 0)."""
    lps = [lp for prec in ("split16", "fp32_exact") for lp in plan(hw, channels, n_enc, prec, cus)]
    n = max(-(-3 * lp.cap // lp.items_per_cell) for lp in lps)
    while any((n * lp.items_per_cell) % lp.cap == 0 for lp in lps):
        n += 1
    return n


def oracle_cells(hw, channels, n_enc, n, seed=0, cus=CUS, sample=4):
    """The cells checked against the oracle at n: the first, the last, the first and last cell that each launch
    reaches only in its final round, and a seeded sample."""
    import random
    cells = {0, n - 1}
    for prec in ("split16", "fp32_exact"):
        for lp in plan(hw, channels, n_enc, prec, cus):
            fr = final_round_cells(lp, n)
            cells |= {fr[0], fr[-1]}
    cells |= set(random.Random(seed).sample(range(n), min(sample, n)))
    return sorted(cells)
