// extract.hip -- quality-cell extraction from segmentation label images on gfx950: what the reference does between
// StarDist and the crop preprocess (improved_detection.py:61-111, CAE_improved_modeltrain.py:54-107):
//
//     for prop in regionprops(labels):            border / area / eccentricity rules on the region
//         cell_image = green_channel[minr:maxr, minc:maxc]
//         mean / std rule on the bbox rectangle, then equalize_adapthist + resize (preprocess.hip)
//
// Four kernels per batch, then the preprocess kernel itself:
//   ex_label_pass   ONE read of the int32 label images, on the tile of label_tile.hpp.  A lane keeps the bbox of the
//                   label it is in and flushes (four integer atomics) only when the label changes.  At the end the 64
//                   lanes of a wave merge their open labels (merge_open_runs), one set of atomics per distinct label.
//   ex_region_pass  one workgroup per (image, label) slot over the region's bbox window: exact int64 moment sums
//                   (area, first and second moments), exact intensity sums of the analysis channel over the whole
//                   rectangle, each row's extreme pixels (LDS), the convex hull of the pixel-edge midpoints as two
//                   monotone chains in LDS and the exact count of pixel centres inside or on it; then the QC bits.
//   ex_scan         one workgroup: exclusive scan, in (image, label) order, of region presence, of the cell flags
//                   (passing region of an image whose status is OK) and of the crop sizes.
//   ex_compact      the region table and the crop descriptors in scan order; ex_gather cuts the crops out of the
//                   analysis channel into the ragged layout preprocess.hip reads.
// Integers throughout up to the final quotients; no float atomics, so every output is bit-identical run to run and
// independent of which other images share the batch (a slot's work reads nothing but its own image).
#include "hull_chain.hpp"
#include "label_tile.hpp"
#include "stage_host.hpp"

#include <algorithm>
#include <climits>

namespace cs {

static constexpr int EX_THREADS = LT_THREADS;           // of the region pass, the sweeps and the gather too
static constexpr int EX_WAVES = EX_THREADS / 64;
static constexpr int64_t kMaxSlots = 1 << 22;           // batch * max_label
static constexpr int SCAN_THREADS = 1024;

struct ExQc {
    int border, min_area, max_area;
    double max_ecc, min_mean, min_std;
};

// totals the host reads after the scan
struct ExCounts {
    long long n_regions, n_cells, crop_px, lds;
    unsigned int err;                                   // 1: a negative label, 2: a label above max_label
    unsigned int pad;
};

struct SlotIdx {
    int region, cell;
    long long off;                                      // element offset of the cell's crop in the ragged buffer
};

struct GatherDesc {
    int image, minr, minc, pad;
};

// a*b - c*d for a, b, c, d >= 0 whose products stay below 2^85 and whose difference is >= 0, as the correctly rounded double
// (the rounding Python's float(int) applies): the exact difference in 128 bits, then one fp64 addition of two exact parts
__device__ inline double exact_diff_to_double(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d)
{
    const unsigned long long plo = a * b, phi = __umul64hi(a, b);
    const unsigned long long qlo = c * d, qhi = __umul64hi(c, d);
    const unsigned long long lo = plo - qlo;
    const unsigned long long hi = phi - qhi - (plo < qlo ? 1ull : 0ull);
    const unsigned long long top = (hi << 32) | (lo >> 32);            // < 2^53
    const unsigned long long bot = lo & 0xffffffffull;
    return __dadd_rn(__dmul_rn((double)top, 4294967296.0), (double)bot);
}

// n*s2 - s1a*s1b for the window's moment sums (all >= 0: window coordinates), exact; negative only for the mixed moment
__device__ inline double central_num(long long n, long long s2, long long s1a, long long s1b)
{
    const unsigned long long un = (unsigned long long)n, u2 = (unsigned long long)s2;
    const unsigned long long ua = (unsigned long long)s1a, ub = (unsigned long long)s1b;
    const unsigned long long plo = un * u2, phi = __umul64hi(un, u2);
    const unsigned long long qlo = ua * ub, qhi = __umul64hi(ua, ub);
    const bool ge = phi > qhi || (phi == qhi && plo >= qlo);
    return ge ? exact_diff_to_double(un, u2, ua, ub) : -exact_diff_to_double(ua, ub, un, u2);
}

// ---- init: empty bbox table, flags, counters ----------------------------------------------------------------------------
__global__ __launch_bounds__(EX_THREADS) void ex_init(int4* __restrict__ bbox, int64_t nslots, unsigned int* __restrict__ img_flags, int batch,
                                                      ExCounts* __restrict__ counts)
{
    const int64_t stride = (int64_t)gridDim.x * EX_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x; s < nslots; s += stride) bbox[s] = make_int4(INT_MAX, INT_MAX, -1, -1);
    if (blockIdx.x == 0) {
        for (int b = threadIdx.x; b < batch; b += EX_THREADS) img_flags[b] = 0u;
        if (threadIdx.x == 0) *counts = ExCounts{0, 0, 0, 0, 0u, 0u};
    }
}

// ---- label pass -----------------------------------------------------------------------------------------------------------
// grid (ceil(W/256), ceil(H/64), B).  bbox[slot] = {minr, minc, maxr, maxc} (max inclusive), slot = b * max_label + label - 1.
__device__ inline void bbox_flush(int4* bbox, int64_t slot, int r0, int c0, int r1, int c1)
{
    atomicMin(&bbox[slot].x, r0);
    atomicMin(&bbox[slot].y, c0);
    atomicMax(&bbox[slot].z, r1);
    atomicMax(&bbox[slot].w, c1);
}

__global__ __launch_bounds__(EX_THREADS) void ex_label_pass(const int* __restrict__ labels, int H, int W, int max_label,
                                                            int4* __restrict__ bbox, ExCounts* __restrict__ counts)
{
    const LabelTile tile = label_tile();
    const int r_base = tile.r_base, c_base = tile.c_base;
    const int* lab = labels + (size_t)tile.b * H * W;
    const int64_t slot0 = (int64_t)tile.b * max_label - 1;
    const bool vec = (W & 3) == 0 && ((uintptr_t)labels & 15) == 0 && c_base + 3 < W;

    int v[LT_ROWS][4];
#pragma unroll
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = r_base + i;
        label_load4(lab + (size_t)r * W + c_base, r < H ? W - c_base : 0, vec && r < H, v[i]);
    }
    unsigned int err = 0u;
    int L = 0, r0 = 0, c0 = 0, r1 = 0, c1 = 0;
#pragma unroll
    for (int i = 0; i < LT_ROWS; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = v[i][k];
            if (x == 0) continue;
            if (x < 0 || x > max_label) { err |= x < 0 ? 1u : 2u; continue; }
            const int r = r_base + i, c = c_base + k;
            if (x != L) {
                if (L) bbox_flush(bbox, slot0 + L, r0, c0, r1, c1);
                L = x; r0 = r1 = r; c0 = c1 = c;
            } else {
                r1 = r; c0 = min(c0, c); c1 = max(c1, c);
            }
        }
    }
    if (err) atomicOr(&counts->err, err);
    // the open label of every lane: one set of atomics per distinct label of the wave
    merge_open_runs(L != 0, L, tile.lane, [&](int Lw, bool mine, bool leader) {
        const int a = wave_min(mine ? r0 : INT_MAX), bmin = wave_min(mine ? c0 : INT_MAX);
        const int cmax = wave_max(mine ? r1 : -1), dmax = wave_max(mine ? c1 : -1);
        if (leader) bbox_flush(bbox, slot0 + Lw, a, bmin, cmax, dmax);
    });
}

// ---- per-region pass -------------------------------------------------------------------------------------------------------
// One workgroup per slot.  Dynamic LDS: rowL / rowR (int16, [H] each) + the two chains (packed (y+1) << 16 | (x+1), [2H+2] each).
// Coordinates inside the bbox window: row i, column j; doubled coordinates of the hull: y = 2i, x = 2j, pixel-edge
// midpoints at (2i +- 1, 2j) and (2i, 2j +- 1).  The chains and their packing are hull_chain.hpp's, which shape.hip shares.
template <typename PIX>
__global__ __launch_bounds__(EX_THREADS) void ex_region_pass(const int* __restrict__ labels, const PIX* __restrict__ image, int C, int ch,
                                                             int H, int W, int max_label, const int4* __restrict__ bbox, ExQc qc,
                                                             int out_h, int out_w, cs_region* __restrict__ rec,
                                                             unsigned int* __restrict__ img_flags)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ex_lds[];
    short* rowL = (short*)ex_lds;
    short* rowR = rowL + H;
    int* chL = (int*)(ex_lds + (((size_t)4 * H + 15) & ~(size_t)15));
    int* chR = chL + 2 * H + 2;
    __shared__ long long red[EX_WAVES][9];
    __shared__ int nch[2];

    const int64_t s = blockIdx.x;
    const int b = (int)(s / max_label), L = (int)(s - (int64_t)b * max_label) + 1;
    const int4 bb = bbox[s];
    if (bb.x == INT_MAX) {
        if (threadIdx.x == 0) rec[s].label = 0;         // no such label in this image
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = bb.z - bb.x + 1, w = bb.w - bb.y + 1;
    const int* lab = labels + ((size_t)b * H + bb.x) * W + bb.y;
    const PIX* img = image + (((size_t)b * H + bb.x) * W + bb.y) * C + ch;

    long long n = 0, si = 0, sj = 0, sii = 0, sjj = 0, sij = 0;
    unsigned long long sx = 0, sxx = 0;
    for (int i = wave; i < h; i += EX_WAVES) {
        const int* lrow = lab + (size_t)i * W;
        const PIX* irow = img + (size_t)i * W * C;
        int jmin = 0x7fff, jmax = -1;
        for (int j = lane; j < w; j += 64) {
            const unsigned int x = (unsigned int)irow[(size_t)j * C];
            sx += x;
            sxx += (unsigned long long)x * x;
            if (lrow[j] == L) {
                ++n; si += i; sj += j;
                sii += i * i; sjj += j * j; sij += i * j;
                jmin = min(jmin, j); jmax = max(jmax, j);
            }
        }
        jmin = wave_min(jmin);
        jmax = wave_max(jmax);
        if (lane == 0) { rowL[i] = (short)jmin; rowR[i] = (short)jmax; }
    }
    long long v[8] = {n, si, sj, sii, sjj, sij, (long long)sx, (long long)sxx};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) red[wave][k] = v[k];
    }
    __syncthreads();                                    // rowL / rowR and the partial sums are complete
    if (tid == 0) nch[0] = build_chain(rowL, h, false, chL);
    if (tid == 64) nch[1] = build_chain(rowR, h, true, chR);
    __syncthreads();

    // convex area: for each pixel row, the columns j with x_left(2i) <= 2j <= x_right(2i)
    const int nl = nch[0], nr = nch[1];
    long long cnt = 0;
    for (int i = tid; i < h; i += EX_THREADS) {
        const int y = 2 * i;
        int k = chain_segment(chL, nl, y);
        long long y0 = pt_y(chL[k]), x0 = pt_x(chL[k]), dy = pt_y(chL[k + 1]) - y0, dx = pt_x(chL[k + 1]) - x0;
        const long long jl = ceil_div(x0 * dy + dx * (y - y0), 2 * dy);
        k = chain_segment(chR, nr, y);
        y0 = pt_y(chR[k]); x0 = pt_x(chR[k]); dy = pt_y(chR[k + 1]) - y0; dx = pt_x(chR[k + 1]) - x0;
        const long long jr = floor_div(x0 * dy + dx * (y - y0), 2 * dy);
        const long long a = max(jl, 0ll), e = min(jr, (long long)w - 1);
        if (e >= a) cnt += e - a + 1;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) red[wave][8] = cnt;
    __syncthreads();
    if (tid != 0) return;

    long long t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        t[k] = 0;
        for (int q = 0; q < EX_WAVES; ++q) t[k] += red[q][k];
    }
    const long long area = t[0], convex = t[8];
    // inertia tensor of the central moments (skimage 0.18.3 _moments.inertia_tensor): [[mu02, -mu11], [-mu11, mu20]] / mu00,
    // each entry num / n^2 with the exact integer num = n * S2 - S1 * S1'
    const double n2 = (double)area * (double)area;                                      // < 2^48: exact
    const double trr = __ddiv_rn(central_num(area, t[3], t[1], t[1]), n2);
    const double tcc = __ddiv_rn(central_num(area, t[4], t[2], t[2]), n2);
    const double trc = __ddiv_rn(central_num(area, t[5], t[1], t[2]), n2);
    const double mean2 = __dmul_rn(__dadd_rn(tcc, trr), 0.5);
    const double half = __dmul_rn(__dsub_rn(tcc, trr), 0.5);
    const double rad = __dsqrt_rn(__dadd_rn(__dmul_rn(half, half), __dmul_rn(trc, trc)));
    const double l1 = __dadd_rn(mean2, rad);
    const double l2 = __dsub_rn(mean2, rad);
    // sqrt(1 - l2/l1) with 1 - l2/l1 = 2 rad / l1 (no cancellation near a circle); l2 clipped at 0 gives 1
    const double ecc = l1 == 0.0 ? 0.0 : (l2 <= 0.0 ? 1.0 : __dsqrt_rn(__ddiv_rn(__dmul_rn(2.0, rad), l1)));
    const long long nb = (long long)h * w;
    const double mean = __ddiv_rn((double)t[6], (double)nb);
    const double var = __ddiv_rn(exact_diff_to_double((unsigned long long)nb, (unsigned long long)t[7], (unsigned long long)t[6],
                                                      (unsigned long long)t[6]),
                                 (double)nb * (double)nb);
    const double sd = __dsqrt_rn(var);
    const int minr = bb.x, minc = bb.y, maxr = bb.z + 1, maxc = bb.w + 1;
    unsigned int failed = 0u;
    if (minr < qc.border || minc < qc.border || maxr > H - qc.border || maxc > W - qc.border) failed |= CS_QC_BORDER;
    if (area < qc.min_area || area > qc.max_area) failed |= CS_QC_AREA;
    if (ecc > qc.max_ecc) failed |= CS_QC_ECCENTRICITY;
    if (mean < qc.min_mean || sd < qc.min_std) failed |= CS_QC_INTENSITY;
    cs_region r;
    r.image = b; r.label = L;
    r.minr = minr; r.minc = minc; r.maxr = maxr; r.maxc = maxc;
    r.area = area; r.convex_area = convex;
    r.eccentricity = ecc;
    r.solidity = __ddiv_rn((double)area, (double)convex);
    r.mean_intensity = mean; r.std_intensity = sd;
    r.failed = failed; r.cell = -1;
    rec[s] = r;
    if (failed == 0u) {
        if (min(h, w) < kPreprocMin) atomicOr(&img_flags[b], 1u);
        if (preproc_side_beyond(h, out_h) || preproc_side_beyond(w, out_w)) atomicOr(&img_flags[b], 2u);   // cs_preprocess's rule
    }
}

__device__ inline int image_status(unsigned int f) { return (f & 1u) ? CS_IMAGE_NO_CELLS : (f & 2u) ? CS_IMAGE_UNSUPPORTED : CS_IMAGE_OK; }

// dynamic LDS of the preprocess kernel for one crop (cs_preprocess's rule)
__device__ inline long long preprocess_lds(int H, int W)
{
    const int kh = H / 8, kw = W / 8;
    const long long tiles = (long long)((H + kh - 1) / kh) * ((W + kw - 1) / kw);
    return max(tiles * 256 * 2, 8ll * W * 8);
}

// ---- scan (one workgroup) ----------------------------------------------------------------------------------------------------
__device__ inline void block_excl_scan3(long long& a, long long& b, long long& c, long long* buf /* [3][SCAN_THREADS] */,
                                        long long& ta, long long& tb, long long& tc)
{
    const int t = threadIdx.x;
    buf[t] = a; buf[SCAN_THREADS + t] = b; buf[2 * SCAN_THREADS + t] = c;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const long long xa = t >= d ? buf[t - d] : 0, xb = t >= d ? buf[SCAN_THREADS + t - d] : 0,
                        xc = t >= d ? buf[2 * SCAN_THREADS + t - d] : 0;
        __syncthreads();
        buf[t] += xa; buf[SCAN_THREADS + t] += xb; buf[2 * SCAN_THREADS + t] += xc;
        __syncthreads();
    }
    const long long ia = buf[t], ib = buf[SCAN_THREADS + t], ic = buf[2 * SCAN_THREADS + t];
    ta = buf[SCAN_THREADS - 1]; tb = buf[2 * SCAN_THREADS - 1]; tc = buf[3 * SCAN_THREADS - 1];
    a = ia - a; b = ib - b; c = ic - c;
}

__global__ __launch_bounds__(SCAN_THREADS) void ex_scan(cs_region* __restrict__ rec, int64_t nslots, int max_label,
                                                        const unsigned int* __restrict__ img_flags, int batch, int* __restrict__ status,
                                                        SlotIdx* __restrict__ idx, ExCounts* __restrict__ counts)
{
    __shared__ long long buf[3 * SCAN_THREADS];
    __shared__ long long lmax[SCAN_THREADS / 64];
    const int t = threadIdx.x;
    for (int b = t; b < batch; b += SCAN_THREADS) status[b] = image_status(img_flags[b]);
    const int64_t per = (nslots + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t s0 = min((int64_t)t * per, nslots), s1 = min(s0 + per, nslots);
    long long nreg = 0, ncell = 0, px = 0, lds = 0;
    for (int64_t s = s0; s < s1; ++s) {
        if (rec[s].label == 0) continue;
        ++nreg;
        const int b = (int)(s / max_label);
        if (rec[s].failed == 0u && image_status(img_flags[b]) == CS_IMAGE_OK) {
            const int h = rec[s].maxr - rec[s].minr, w = rec[s].maxc - rec[s].minc;
            ++ncell;
            px += (long long)h * w;
            lds = max(lds, preprocess_lds(h, w));
        }
    }
    long long tr, tcl, tpx;
    block_excl_scan3(nreg, ncell, px, buf, tr, tcl, tpx);
    for (int64_t s = s0; s < s1; ++s) {
        if (rec[s].label == 0) continue;
        const int b = (int)(s / max_label);
        SlotIdx q{(int)nreg++, -1, 0};
        if (rec[s].failed == 0u && image_status(img_flags[b]) == CS_IMAGE_OK) {
            const int h = rec[s].maxr - rec[s].minr, w = rec[s].maxc - rec[s].minc;
            q.cell = (int)ncell++;
            q.off = px;
            px += (long long)h * w;
        }
        rec[s].cell = q.cell;
        idx[s] = q;
    }
    // largest preprocess LDS over the cells
    long long m = wave_max(lds);
    if ((t & 63) == 0) lmax[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < SCAN_THREADS / 64; ++q) m = max(m, lmax[q]);
        counts->n_regions = tr;
        counts->n_cells = tcl;
        counts->crop_px = tpx;
        counts->lds = m;
    }
}

// ---- compaction + crop gather ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_THREADS) void ex_compact(const cs_region* __restrict__ rec, const SlotIdx* __restrict__ idx, int64_t nslots,
                                                         cs_region* __restrict__ regions, CropDesc* __restrict__ desc,
                                                         GatherDesc* __restrict__ gat, int* __restrict__ cell_image)
{
    const int64_t stride = (int64_t)gridDim.x * EX_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x; s < nslots; s += stride) {
        if (rec[s].label == 0) continue;
        const cs_region r = rec[s];
        const SlotIdx q = idx[s];
        if (regions) regions[q.region] = r;
        if (q.cell >= 0) {
            desc[q.cell] = CropDesc{q.off, r.maxr - r.minr, r.maxc - r.minc};
            gat[q.cell] = GatherDesc{r.image, r.minr, r.minc, 0};
            if (cell_image) cell_image[q.cell] = r.image;
        }
    }
}

template <typename PIX>
__global__ __launch_bounds__(EX_THREADS) void ex_gather(const PIX* __restrict__ image, int C, int ch, int H, int W,
                                                        const CropDesc* __restrict__ desc, const GatherDesc* __restrict__ gat,
                                                        PIX* __restrict__ pix)
{
    const CropDesc d = desc[blockIdx.x];
    const GatherDesc g = gat[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PIX* src = image + (((size_t)g.image * H + g.minr) * W + g.minc) * C + ch;
    PIX* dst = pix + d.off;
    for (int i = wave; i < d.H; i += EX_WAVES)
        for (int j = lane; j < d.W; j += 64) dst[(size_t)i * d.W + j] = src[((size_t)i * W + j) * C];
}

// ---- host state between the two calls -------------------------------------------------------------------------------------
struct ExtractState {
    DevBuf lab, img;                                    // uploads of host inputs
    DevBuf bbox, rec, idx, flags, status, counts;
    DevBuf regions, cell_image, desc, gat, cpix, clahe, cells;
    StageClock clk;                                     // spans: label, region, between the two calls (no step), cells
    bool measured = false;
    const void* d_img = nullptr;
    int ptype = 0, C = 1, ch = 0, batch = 0, H = 0, W = 0, max_label = 0;
    int out_h = 64, out_w = 64;                         // the handle's output size at the measure: sizes the fill's cells
    int64_t nslots = 0;
    double clip_limit = 0.02;
    ExCounts host{};
};

void extract_state_free(ExtractState* s) { delete s; }

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_extract_measure(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, const int32_t* labels,
                       int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, const cs_qc_params* qc,
                       int64_t* n_regions, int64_t* n_cells)
{
    if (n_regions) *n_regions = 0;
    if (n_cells) *n_cells = 0;
    if (!image || !labels || !n_regions || !n_cells) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind)) return fail(CS_ERR_INVALID, "in_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1 || channel < 0 || channel >= channels)
        return fail(CS_ERR_INVALID, "channel %d of %d: need 0 <= channel < channels", (int)channel, (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width)) || (rc = side_limits(height, width))) return rc;   // the region pass keeps ~20 B of LDS per row
    if (max_label < 0) return fail(CS_ERR_INVALID, "max_label is negative");
    if ((rc = label_cap("max_label", max_label, batch, 0, kMaxSlots, "per-label tables", "per batch; relabel sparse ids in order first")))
        return rc;
    cs_qc_params q{10, 200, 8000, 0, 0.95, 0.5, 0.1, 0.02};
    if (qc) {
        q = *qc;
        if (q.reserved != 0) return fail(CS_ERR_INVALID, "cs_qc_params.reserved must be 0");
        if (!(q.clip_limit == q.clip_limit) || !(q.max_eccentricity == q.max_eccentricity) || !(q.min_mean == q.min_mean) ||
            !(q.min_std == q.min_std))
            return fail(CS_ERR_INVALID, "cs_qc_params holds a NaN");
    }
    if ((rc = handle_check(p))) return rc;
    HIPCHK(hipSetDevice(p->device));
    if (!p->ext) p->ext = new ExtractState();
    ExtractState& S = *p->ext;
    S.measured = false;
    p->extract_pending = false;
    const int out_h = p->out_h, out_w = p->out_w;

    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const size_t npx = (size_t)batch * height * width;
    const int* d_lab;
    const void* d_img;
    if (in_kind == CS_MEM_DEVICE) {
        d_lab = labels;
        d_img = image;
    } else {
        if ((rc = S.lab.ensure(npx * sizeof(int32_t))) || (rc = S.img.ensure(npx * channels * esz))) return rc;
        HIPCHK(hipMemcpyAsync(S.lab.p, labels, npx * sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipMemcpyAsync(S.img.p, image, npx * channels * esz, hipMemcpyHostToDevice, p->stream));
        d_lab = S.lab.as<int>();
        d_img = S.img.p;
    }
    const int64_t nslots = (int64_t)batch * max_label;
    const int64_t ns = std::max<int64_t>(nslots, 1);
    if ((rc = S.bbox.ensure(ns * sizeof(int4))) || (rc = S.rec.ensure(ns * sizeof(cs_region))) || (rc = S.idx.ensure(ns * sizeof(SlotIdx))) ||
        (rc = S.flags.ensure(batch * sizeof(unsigned int))) || (rc = S.status.ensure(batch * sizeof(int))) ||
        (rc = S.counts.ensure(sizeof(ExCounts))))
        return rc;
    const ExQc eq{q.border, q.min_area, q.max_area, q.max_eccentricity, q.min_mean, q.min_std};
    const unsigned init_blocks = (unsigned)std::min<int64_t>((ns + EX_THREADS - 1) / EX_THREADS, 4096);
    hipLaunchKernelGGL(ex_init, dim3(init_blocks), dim3(EX_THREADS), 0, p->stream, S.bbox.as<int4>(), nslots, S.flags.as<unsigned int>(),
                       (int)batch, S.counts.as<ExCounts>());
    HIPCHK(hipGetLastError());
    if ((rc = S.clk.record(0, p->stream))) return rc;
    hipLaunchKernelGGL(ex_label_pass, label_tile_grid(batch, height, width), dim3(EX_THREADS), 0, p->stream, d_lab, (int)height, (int)width, (int)max_label,
                       S.bbox.as<int4>(), S.counts.as<ExCounts>());
    HIPCHK(hipGetLastError());
    if ((rc = S.clk.record(1, p->stream))) return rc;
    if (nslots > 0) {
        const size_t lds = (((size_t)4 * height + 15) & ~(size_t)15) + (size_t)2 * (2 * height + 2) * sizeof(int);
        if (pixel_type == CS_PIX_U8) {
            HIPCHK(hipFuncSetAttribute((const void*)ex_region_pass<unsigned char>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(ex_region_pass<unsigned char>, dim3((unsigned)nslots), dim3(EX_THREADS), lds, p->stream, d_lab,
                               (const unsigned char*)d_img, (int)channels, (int)channel, (int)height, (int)width, (int)max_label,
                               S.bbox.as<int4>(), eq, out_h, out_w, S.rec.as<cs_region>(), S.flags.as<unsigned int>());
        } else {
            HIPCHK(hipFuncSetAttribute((const void*)ex_region_pass<unsigned short>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(ex_region_pass<unsigned short>, dim3((unsigned)nslots), dim3(EX_THREADS), lds, p->stream, d_lab,
                               (const unsigned short*)d_img, (int)channels, (int)channel, (int)height, (int)width, (int)max_label,
                               S.bbox.as<int4>(), eq, out_h, out_w, S.rec.as<cs_region>(), S.flags.as<unsigned int>());
        }
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(ex_scan, dim3(1), dim3(SCAN_THREADS), 0, p->stream, S.rec.as<cs_region>(), nslots, (int)std::max(max_label, 1),
                       S.flags.as<unsigned int>(), (int)batch, S.status.as<int>(), S.idx.as<SlotIdx>(), S.counts.as<ExCounts>());
    HIPCHK(hipGetLastError());
    if ((rc = S.clk.record(2, p->stream))) return rc;
    HIPCHK(hipMemcpyAsync(&S.host, S.counts.p, sizeof(ExCounts), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));              // host synchronisation 1 of 2: the counts
    if ((rc = S.clk.finish())) return rc;
    S.clk.ms[3] = 0.0;                                    // the cells of an earlier fill are not this measure's
    if (S.host.err & 1u) return fail(CS_ERR_INVALID, "negative label in the label images");
    if (S.host.err & 2u) return fail(CS_ERR_INVALID, "a label exceeds max_label = %d", (int)max_label);
    S.d_img = d_img;
    S.ptype = pixel_type; S.C = channels; S.ch = channel; S.batch = batch; S.H = height; S.W = width; S.max_label = max_label;
    S.nslots = nslots;
    S.clip_limit = q.clip_limit;
    S.out_h = out_h; S.out_w = out_w;
    S.measured = true;
    p->extract_pending = true;
    *n_regions = S.host.n_regions;
    *n_cells = S.host.n_cells;
    return CS_OK;
}

int cs_extract_fill(cs_preproc* p, cs_region* regions, int32_t* image_status, int table_kind, float* cells, int32_t* cell_image,
                    int cells_kind)
{
    if (!mem_kind(table_kind) || !mem_kind(cells_kind)) return fail(CS_ERR_INVALID, "table_kind / cells_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    int rc;
    if ((rc = handle_check(p))) return rc;
    if (!p->ext || !p->ext->measured) return fail(CS_ERR_INVALID, "cs_extract_fill without a successful cs_extract_measure on this handle");
    HIPCHK(hipSetDevice(p->device));
    ExtractState& S = *p->ext;
    const int64_t nreg = S.host.n_regions, ncell = S.host.n_cells;
    const bool tdev = table_kind == CS_MEM_DEVICE, dev = cells_kind == CS_MEM_DEVICE;
    const size_t cell = (size_t)S.out_h * S.out_w;       // floats of one cell, as measured
    cs_region* d_reg = nullptr;
    if (regions && nreg > 0) {
        if (tdev) d_reg = regions;
        else {
            if ((rc = S.regions.ensure(nreg * sizeof(cs_region)))) return rc;
            d_reg = S.regions.as<cs_region>();
        }
    }
    int* d_cimg = nullptr;
    if (cell_image && ncell > 0) {
        if (dev) d_cimg = cell_image;
        else {
            if ((rc = S.cell_image.ensure(ncell * sizeof(int)))) return rc;
            d_cimg = S.cell_image.as<int>();
        }
    }
    const size_t esz = S.ptype == CS_PIX_U8 ? 1 : 2;
    float* d_cells = nullptr;
    if (ncell > 0) {
        if ((rc = S.desc.ensure(ncell * sizeof(CropDesc))) || (rc = S.gat.ensure(ncell * sizeof(GatherDesc)))) return rc;
        if (cells) {
            if ((rc = S.cpix.ensure((size_t)S.host.crop_px * esz)) || (rc = S.clahe.ensure((size_t)S.host.crop_px * sizeof(uint16_t)))) return rc;
            if (dev) d_cells = cells;
            else {
                if ((rc = S.cells.ensure((size_t)ncell * cell * sizeof(float)))) return rc;
                d_cells = S.cells.as<float>();
            }
        }
    }
    if (S.nslots > 0 && nreg > 0) {
        const unsigned blocks = (unsigned)std::min<int64_t>((S.nslots + EX_THREADS - 1) / EX_THREADS, 4096);
        hipLaunchKernelGGL(ex_compact, dim3(blocks), dim3(EX_THREADS), 0, p->stream, S.rec.as<cs_region>(), S.idx.as<SlotIdx>(), S.nslots,
                           d_reg, S.desc.as<CropDesc>(), S.gat.as<GatherDesc>(), d_cimg);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk.record(3, p->stream, false))) return rc;      // since the measure's last event: no step of this clock
    if (d_cells) {
        if (S.ptype == CS_PIX_U8)
            hipLaunchKernelGGL(ex_gather<unsigned char>, dim3((unsigned)ncell), dim3(EX_THREADS), 0, p->stream, (const unsigned char*)S.d_img,
                               S.C, S.ch, S.H, S.W, S.desc.as<CropDesc>(), S.gat.as<GatherDesc>(), S.cpix.as<unsigned char>());
        else
            hipLaunchKernelGGL(ex_gather<unsigned short>, dim3((unsigned)ncell), dim3(EX_THREADS), 0, p->stream, (const unsigned short*)S.d_img,
                               S.C, S.ch, S.H, S.W, S.desc.as<CropDesc>(), S.gat.as<GatherDesc>(), S.cpix.as<unsigned short>());
        HIPCHK(hipGetLastError());
        HIPCHK(launch_preprocess(S.cpix.p, S.ptype, S.desc.as<CropDesc>(), ncell, S.clip_limit, (size_t)S.host.lds, S.clahe.as<uint16_t>(),
                                 d_cells, S.out_h, S.out_w, p->stream));
    }
    if ((rc = S.clk.record(4, p->stream))) return rc;
    if (image_status) {
        if (tdev) HIPCHK(hipMemcpyAsync(image_status, S.status.p, S.batch * sizeof(int), hipMemcpyDeviceToDevice, p->stream));
        else HIPCHK(hipMemcpyAsync(image_status, S.status.p, S.batch * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    }
    if (!tdev && d_reg) HIPCHK(hipMemcpyAsync(regions, d_reg, nreg * sizeof(cs_region), hipMemcpyDeviceToHost, p->stream));
    if (!dev) {
        if (d_cimg) HIPCHK(hipMemcpyAsync(cell_image, d_cimg, ncell * sizeof(int), hipMemcpyDeviceToHost, p->stream));
        if (d_cells) HIPCHK(hipMemcpyAsync(cells, d_cells, (size_t)ncell * cell * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    }
    HIPCHK(hipStreamSynchronize(p->stream));              // host synchronisation 2 of 2: the table and the cells
    if ((rc = S.clk.finish())) return rc;
    p->extract_pending = false;                           // the handle's output size may change again
    return CS_OK;
}

int cs_extract_last_timing(const cs_preproc* p, double* label_ms, double* region_ms, double* cells_ms)
{
    return clock_read(p, p && p->ext ? &p->ext->clk : nullptr, {label_ms, region_ms, nullptr, cells_ms});
}
