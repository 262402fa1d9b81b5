"""A plain restatement of how libcellscreen shapes the detector tail (csrc/detector.hip): which detectors it accepts, the
padded sizes it derives, when the split form of a small call runs, how the fixed DET_RANGES ranges partition the features
and the support-vector blocks, and which kernel instantiation each call reaches.  Test code only: it is tied to the
library by test_detector_envelope_cpu.py (the GPU case list reaches every instantiation and partition class) and by
test_gpu_detector_sweep.py (profile counters, bit identities), never by a C ABI.

Each function cites the lines of cell-image-analysis_amd/csrc/ that it restates; a change there must change this file.
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import generic_plans as G
from cellscreen import spec

DET_RANGES = 8                  # detector.hip:147
DET_SPLIT_MAX_CELLS = 16384     # common.hpp:195
PCA_KC = 256                    # detector.hip:23  (scaler_pca_kernel: features per LDS chunk)
PX_KC = 128                     # detector.hip:136 (scaler_pca_x3_kernel: features per LDS chunk)
PCA_CELLS = 64                  # detector.hip:22  (cells per PCA workgroup)
SVMM_CELLS = 256                # detector.hip:315 (cells per SVM workgroup)
C_MAX = 128                     # api.hip:782


# ---------------------------------------------------------------- acceptance and derived sizes
def accept(encoder_width: int, n_features: int, n_components: int, n_sv: Tuple[int, int]) -> Optional[str]:
    """api.hip:777-786 and pack_svm, api.hip:378-381: None or the rule that refuses."""
    if n_features != encoder_width:
        return "n_features"
    if n_components <= 0 or n_components > C_MAX:
        return "n_components"
    if any(s <= 0 for s in n_sv):
        return "n_sv"
    return None


def fpad(F):
    """api.hip:788: features padded to whole 512-feature blocks (a multiple of PCA_KC and of PX_KC)."""
    return (F + 511) // 512 * 512


def cpad(C):
    """api.hip:790."""
    return (C + 15) // 16 * 16


def tiles(C):
    """detector.hip:38, 160: 16-component tiles; wave w owns tiles w and w + 4, so tiles 5..8 use the second slot."""
    return cpad(C) // 16


def ks(C):
    """detector.hip:619-626: the K steps of 4 components of ocsvm_mfma_kernel<KS, *>."""
    return 25 if C <= 100 else 32


def nsv_pad(n_sv):
    """api.hip:383."""
    return (n_sv + 15) // 16 * 16


def nblk(n_sv):
    """detector.hip:388: 16-SV blocks."""
    return nsv_pad(n_sv) // 16


def pca_chunks(F):
    """detector.hip:168: PX_KC-feature chunks of scaler_pca_x3_kernel."""
    return fpad(F) // PX_KC


def pca_ranges(F) -> List[Tuple[int, int]]:
    """detector.hip:168-171: range j = chunks [nch j / 8, nch (j + 1) / 8), as (first, end) FEATURE indices."""
    nch = pca_chunks(F)
    return [(nch * j // DET_RANGES * PX_KC, nch * (j + 1) // DET_RANGES * PX_KC) for j in range(DET_RANGES)]


def svm_ranges(n_sv) -> List[Tuple[int, int]]:
    """detector.hip:388-390: range j = blocks [nblk j / 8, nblk (j + 1) / 8), as (first, end) BLOCK indices."""
    nb = nblk(n_sv)
    return [(nb * j // DET_RANGES, nb * (j + 1) // DET_RANGES) for j in range(DET_RANGES)]


def pca_class(F):
    """The partition class of the PCA ranges: 'empty' (nch < 8: some ranges hold no chunk), 'even' (nch a multiple of
    8) or 'ragged' (nch > 8, not a multiple)."""
    nch = pca_chunks(F)
    return "empty" if nch < DET_RANGES else ("even" if nch % DET_RANGES == 0 else "ragged")


def svm_class(n_sv):
    nb = nblk(n_sv)
    if nb == 1:
        return "1"
    if nb < DET_RANGES:
        return "<8"
    if nb == DET_RANGES:
        return "=8"
    return ">8 even" if nb % DET_RANGES == 0 else ">8 ragged"


# ---------------------------------------------------------------- passes
def device_chunk(hw, channels, n_enc):
    """eff_chunk, api.hip:410-419, for device-resident input: cells a ~28 GB workspace holds, in [1024, 65536]."""
    rows = spec.layer_table(hw, channels, n_enc)
    per_cell = hw[0] * hw[1] * 4 + sum(r["out_hw"][0] * r["out_hw"][1] * r["cout"] * 4 for r in rows[:-1])
    c = int(28e9) // per_cell // 1024 * 1024
    return min(max(c, 1024), 65536)


def eff_chunk(kind, chunk=0, arch=None):
    """api.hip:410-419: cs_model_set_chunk's value if set, 16,384 for host input, device_chunk otherwise.
    arch = (hw, channels, n_enc) of the engine's CAE, needed for device input only."""
    if chunk > 0:
        return chunk
    if kind == "host":
        return 16384
    return device_chunk(*arch)


def passes(n, kind="host", chunk=0, arch=None) -> List[int]:
    """The cells per internal pass of a call (cs_screen, cs_scaler_pca, cs_svm_decision: ch = min(n, eff_chunk),
    api.hip:990-991, 1190-1191, 1222-1223)."""
    ch = min(n, eff_chunk(kind, chunk, arch))
    return [min(ch, n - off) for off in range(0, n, ch)]


def split_runs(nc, small_split=True):
    """detector.hip:606, 635; api.hip:959: the split form runs for a pass of <= 16,384 cells when the range-sum workspace
    exists, which it does unless CS_DEBUG_NO_SMALL_SPLIT (api.hip:432, 751)."""
    return small_split and nc <= DET_SPLIT_MAX_CELLS


# ---------------------------------------------------------------- instantiations
def pca_kernels(precision, nc, small_split=True):
    """api.hip:951-958, 1197-1204; detector.hip:606-616: the PCA launches of one pass."""
    if precision == "fp32_exact":
        return ["scaler_pca_kernel"]                         # no split form
    if split_runs(nc, small_split):
        return ["scaler_pca_x3_kernel<true>", "pca_split_sum_kernel"]
    return ["scaler_pca_x3_kernel<false>"]


def svm_kernels(call, C, nc, small_split=True):
    """The SVM launches of one pass.  cs_screen (run_tail, api.hip:959-972): a split pass runs both detectors in ONE
    launch (launch_ocsvm_pair_split, blockIdx.z = detector, detector.hip:646-658), otherwise one launch per detector.
    cs_svm_decision (api.hip:1230-1235): always one launch_ocsvm per detector (detector.hip:628-643), split or not.
    '[z=2]' names the pair launch, '[z=1]' a single detector's."""
    k = ks(C)
    if split_runs(nc, small_split):
        if call == "screen":
            return [f"ocsvm_mfma_kernel<{k},true>[z=2]", "svm_split_sum_kernel[y=2]"]
        return [f"ocsvm_mfma_kernel<{k},true>[z=1]", "svm_split_sum_kernel[y=1]"] * 2
    return [f"ocsvm_mfma_kernel<{k},false>[z=1]"] * 2


def call_kernels(call, precision, C, n, kind="host", chunk=0, small_split=True, arch=None) -> List[str]:
    """Every detector-tail launch of a call, pass after pass.  call: 'screen', 'scaler_pca' or 'svm_decision'."""
    out = []
    for nc in passes(n, kind, chunk, arch):
        if call in ("screen", "scaler_pca"):
            out += pca_kernels(precision, nc, small_split)
        if call in ("screen", "svm_decision"):
            out += svm_kernels(call, C, nc, small_split)
        if call == "screen":
            out.append("finalize_kernel")
    return out


def mfma_per_cell(precision, F, C):
    """cs_profile_mfma_per_cell / cs_profile_bf16_mfma_per_cell for the scaler_pca family (api.hip:1307-1310, 1343-1345):
    (fp32 MFMAs, bf16 MFMAs) per cell."""
    if precision == "fp32_exact":
        return fpad(F) * cpad(C) / 1024.0, 0.0
    return 0.0, (cpad(C) // 16) * (fpad(F) // 32) * 6.0 / 16.0


# ---------------------------------------------------------------- encoders of a given width
def arch_for_width(F):
    """The cheapest accepted generic architecture (describe_arch) whose encoder emits F features: F = (H >> n_enc) *
    (W >> n_enc) * channels[n_enc - 1] (api.hip:66, 175).  Returns (hw, channels, n_enc) or None."""
    best = None
    for ne in (1, 2, 3):
        for ws in range(16, 129, 16):
            for c in (1, 4, 8, 16, 32):
                if F % (ws * c):
                    continue
                hs = F // (ws * c)
                if hs < 2 or hs % 2:
                    continue
                hw = (hs << ne, ws << ne)
                hidden = [16] * (2 * ne)
                hidden[ne - 1] = c
                ch = tuple(hidden) + (1,)
                a = G.describe_arch(hw, ch, ne)
                if not isinstance(a, G.Arch) or a.ref:
                    continue
                cost = (hw[0] * hw[1] * max(ch), sum(ch))
                if best is None or cost < best[0]:
                    best = (cost, (hw, ch, ne))
    return best[1] if best else None


def encoder_width(hw, channels, n_enc):
    a = G.grids(hw, channels, n_enc)
    h, w = a.gh[n_enc - 1] // 2, a.gw[n_enc - 1] // 2
    return h * w * channels[n_enc - 1]


# ---------------------------------------------------------------- the GPU sweep's case list (test_gpu_detector_sweep.py)
@dataclass(frozen=True)
class Case:
    F: int
    C: int
    n_sv: Tuple[int, int]           # (conservative, moderate)
    gamma_mult: Tuple[float, float]  # x 1 / (C var) of the PCA outputs
    n: int                          # cells
    why: str

    @property
    def id(self):
        return f"F{self.F}-C{self.C}-sv{self.n_sv[0]}.{self.n_sv[1]}-n{self.n}"


SWEEP_CASES = [
    Case(32, 1, (1, 17), (1.0, 30.0), 16347, "C 1, one SV; 4 chunks: empty ranges; nblk 1 / 2; just below 16,384 cells"),
    Case(96, 128, (129, 256), (1.0, 1e-3), 17391, "C 128 > F: KS 32, 8 tiles; nblk 9 ragged / 16 even; above 16,384 cells"),
    Case(128, 101, (17, 129), (30.0, 1.0), 1000, "C 101: the smallest KS 32; 7 tiles"),
    Case(480, 100, (55, 61), (1e-3, 1.0), 777, "C 100: the largest KS 25; the golden model's SV counts"),
    Case(512, 64, (113, 128), (1.0, 1.0), 4097, "4 tiles: the second tile slot idle; nblk 8 = DET_RANGES"),
    Case(544, 59, (33, 48), (1.0, 30.0), 513, "F 544: fpad 1024, 8 chunks; D = 3 mod 4; nblk 3"),
    Case(1344, 18, (7, 100), (30.0, 1.0), 255, "12 chunks: ragged ranges; 2 tiles; D = 2 mod 4"),
    Case(2112, 35, (16, 300), (1.0, 1e-3), 301, "20 chunks; 3 tiles; nblk 1 / 19"),
    Case(2048, 127, (64, 200), (1.0, 1.0), 1, "one cell; C 127; nblk 4 / 13"),
    Case(2560, 90, (400, 33), (1e-3, 30.0), 2049, "2560: 20 chunks, no padding; 6 tiles; nblk 25"),
    Case(4096, 80, (8, 1000), (1.0, 1.0), 63, "32 chunks; 5 tiles; nblk 63"),
    Case(32768, 113, (50, 90), (1.0, 1.0), 300, "256 chunks; 8 tiles with C = 1 mod 16; KS 32"),
]

# A one-hot PCA at a ragged width: every column a component reads, including the last feature and the first of ranges
ONE_HOT_F, ONE_HOT_C = 1344, 128


def sweep_calls(case: Case):
    """The tail calls test_gpu_detector_sweep.py makes per case and precision, as (call, n, input kind, set_chunk,
    small_split): the default host calls, the same with CS_DEBUG_NO_SMALL_SPLIT, device-resident input, an odd pass
    size and, above 16,384 cells, a host pass size that keeps the whole call in one unsplit pass."""
    n = case.n
    calls = [(c, n, "host", 0, s) for s in (True, False) for c in ("scaler_pca", "svm_decision", "screen")]
    calls += [("screen", n, "device", 0, True), ("scaler_pca", n, "device", 0, True), ("svm_decision", n, "device", 0, True),
              ("screen", n, "host", n // 3 | 1, True), ("scaler_pca", n, "host", n // 3 | 1, True)]
    if n > DET_SPLIT_MAX_CELLS:
        calls += [("screen", n, "host", n, True), ("scaler_pca", n, "host", n, True)]
    return calls


def sweep_kernels(cases=None, precisions=("split16", "fp32_exact")):
    """{instantiation: first (case id, precision, call) that reaches it} over the sweep's calls."""
    seen = {}
    for c in (cases if cases is not None else SWEEP_CASES):
        arch = arch_for_width(c.F)
        for prec in precisions:
            for call, n, kind, chunk, ss in sweep_calls(c):
                for k in call_kernels(call, prec, c.C, n, kind, chunk, ss, arch):
                    seen.setdefault(k, (c.id, prec, call, kind, chunk, ss))
    return seen


ALL_KERNELS = {"scaler_pca_kernel", "scaler_pca_x3_kernel<false>", "scaler_pca_x3_kernel<true>", "pca_split_sum_kernel",
               "svm_split_sum_kernel[y=1]", "svm_split_sum_kernel[y=2]", "finalize_kernel"} | {
    f"ocsvm_mfma_kernel<{k},{s}>[z={z}]" for k in (25, 32) for s, z in (("false", 1), ("true", 1), ("true", 2))}
