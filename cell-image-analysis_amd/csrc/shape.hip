// shape.hip -- per-object size and shape of a label image on gfx950: the exact integer records that area, bounding box, central
// moments, axes, orientation, Hu moments, perimeter, Euler numbers, convex area and Feret diameters follow from (include/cellscreen.h,
// cs_label_shape; the rule and the sizing: DESIGN 3x, restated in tests/shape_reference.py).
//
// Per object (cs_label_intensity's: a label > 0 of an image, less the pixels where `exclude` is non-zero); no image is read.
// Two steps, and the kernel boundary is the only ordering between workgroups:
//   sh_moments   lb_pass<true> of label_boxes.hpp, which cs_label_texture shares: one read of labels and exclude on the tile of
//                label_tile.hpp; a run per lane with its count, extent and nine power sums in tile coordinates, merged per wave,
//                then per workgroup in a table of 256 labels in LDS; only the distinct labels of a tile reach the global tables,
//                ten 64-bit integer adds and four integer maxima each.
//   sh_outline   one workgroup per present object.  It walks the object's box in strips of rows; a strip's membership goes into a
//                bitmap in LDS first, a bit per pixel of the strip with a halo of 2 rows and 3 columns, a 64-bit word per wave
//                and load (__ballot), so that every pixel of the box is read from memory once per strip that holds it, and the
//                5 x 5 neighbourhoods come from LDS.  Then a thread per pixel: the code of the 2 x 2 quad whose top-left corner it
//                is (the box with a halo of 1 holds every quad with a bit set), and for a pixel of the object whether it is a
//                border pixel and which of skimage.measure.perimeter's classes its 3 x 3 of border pixels falls into.  Counts stay
//                in registers, 15 + 3 of them, and meet once at the end: no atomics at all.  With want_hull the strips also leave
//                each row's first and last pixel in LDS; then the two chains of hull_chain.hpp (shared with extract.hip), the
//                count of pixel centres inside or on the hull, and two brute-force searches over the hull's vertices: the largest
//                squared distance, and per edge the largest cross product, the edges compared as quotients w^2 / |b - a|^2 by
//                cross-multiplication in 128 bits (they reach 2^81).
// The hull's LDS grows with the box's height, 20 bytes a row, so the objects are served by two launches of the same kernel: boxes
// up to 256 rows with 5 KB, where many workgroups share a CU, and the taller ones, where there are any rows for them, with what the
// image's height asks for (82 KB at 4096 rows, above the 64 KB default: the launch raises the limit as extract's does).  A
// workgroup whose object belongs to the other launch leaves at once.
// No floating point; every result is a sum, a maximum or a minimum under a total order of integers, bit-identical run to run.  A
// label is range-checked before it is a key or an index, a box is clamped to the image before it is walked, and a pixel outside
// the box is never read: its bit is 0 by rule, since the box holds the whole object.
#include "hull_chain.hpp"
#include "label_boxes.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int SH_THREADS = LT_THREADS;
static constexpr int64_t kShMaxRows = 1 << 22;          // batch * max_label
static constexpr int SH_BM_WORDS = 2048;                // the strip's bitmap: 16 KB
static constexpr int SH_HALO_R = 2, SH_HALO_C = 3;      // the bitmap starts 2 rows above the strip and 3 columns left of the box
static constexpr int SH_SMALL_ROWS = 256;               // the tallest box of the first launch
static constexpr int SH_LOADS = 4;                      // words of the bitmap whose loads a wave keeps in flight together
static constexpr int SH_COUNTS = 18;                    // quads 1..15, then the three perimeter classes

static constexpr auto sh_moments = lb_pass<true>;

// bits x0 .. x0 + 4 of a bitmap row; the row has a spare word behind its last
__device__ inline unsigned int sh_bits5(const unsigned long long* rowp, int x0)
{
    const int wd = x0 >> 6, sh = x0 & 63;
    unsigned long long v = rowp[wd] >> sh;
    if (sh > 59) v |= rowp[wd + 1] << (64 - sh);
    return (unsigned int)v & 31u;
}

// whether the quotient w1^2 / d1 is below w2^2 / d2, or equal to it with d1 < d2; w < 2^28, d < 2^28, d > 0
__device__ inline bool sh_narrower(unsigned long long w1, unsigned long long d1, unsigned long long w2, unsigned long long d2)
{
    const unsigned long long a = w1 * w1, b = w2 * w2;                   // below 2^56
    const unsigned long long plo = a * d2, phi = __umul64hi(a, d2), qlo = b * d1, qhi = __umul64hi(b, d1);
    if (phi != qhi) return phi < qhi;
    if (plo != qlo) return plo < qlo;
    return d1 < d2;
}

// dynamic LDS of sh_outline for boxes of up to `rows` rows: rowL / rowR (int16 each) and the two chains
inline size_t sh_hull_lds(int rows) { return (((size_t)4 * rows + 15) & ~(size_t)15) + (size_t)2 * (2 * rows + 2) * sizeof(int); }

// grid (B * max_label).  labels, exclude (or null): [B][H][W] int.  mom: [rows][10], ebox: [rows][4] (LbExtent) from sh_moments.
// Serves the objects whose box has more than h_lo and at most h_hi rows; dynamic LDS: sh_hull_lds(h_hi) with want_hull, else none.
// box: [rows][4], quads: [rows][16], perim: [rows][3], hull (with want_hull): [rows][4], all cleared.
__global__ __launch_bounds__(SH_THREADS) void sh_outline(const int* __restrict__ labels, const int* __restrict__ exclude, int H, int W, int max_label,
                                                         const unsigned long long* __restrict__ mom, const int* __restrict__ ebox, int h_lo, int h_hi,
                                                         int want_hull, int* __restrict__ box, int* __restrict__ quads, int* __restrict__ perim,
                                                         long long* __restrict__ hull)
{
    const size_t row = blockIdx.x;
    if (mom[row * LB_MOMENTS] == 0ull) return;          // an absent object keeps its zeros
    const int* bx = ebox + row * 4;
    const int r0 = max(kMaxSide - bx[0], 0), r1 = min(bx[1], H) - 1, c0 = max(kMaxSide - bx[2], 0), c1 = min(bx[3], W) - 1;
    if (r0 > r1 || c0 > c1) return;                     // cannot be, with a count above 0
    const int h = r1 - r0 + 1, w = c1 - c0 + 1;
    if (h <= h_lo || h > h_hi) return;                  // the other launch's; all of this is uniform over the workgroup

    extern __shared__ __attribute__((aligned(16))) unsigned char sh_lds[];
    __shared__ unsigned long long bm[SH_BM_WORDS];
    __shared__ unsigned int red[LT_WAVES][SH_COUNTS];
    __shared__ long long redc[LT_WAVES];
    __shared__ int nch[2];
    short* rowL = (short*)sh_lds;                       // touched with want_hull only
    short* rowR = rowL + h_hi;
    int* chL = (int*)(sh_lds + (((size_t)4 * h_hi + 15) & ~(size_t)15));
    int* chR = chL + 2 * h_hi + 2;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)(row / (size_t)max_label), lab = (int)(row - (size_t)b * max_label) + 1;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    if (tid == 0) {
        int* o = box + row * 4;
        o[0] = r0; o[1] = c0; o[2] = r1 + 1; o[3] = c1 + 1;
    }
    // bit x of a bitmap row is column c0 - 3 + x, x = 0 .. w + 4; a spare word behind, so that sh_bits5 may look one further
    const int nw = (w + 2 * SH_HALO_C - 1 + 63) >> 6, wpr = nw + 1;      // at most 65 + 1
    const int SR = min(SH_BM_WORDS / wpr - 2 * SH_HALO_R, h + 1);        // centre rows of a strip: at least 27
    const size_t home = (size_t)r0 * W + c0;            // a pixel of the box: what a lane without a pixel reads
    unsigned int cnt[SH_COUNTS];
#pragma unroll
    for (int k = 0; k < SH_COUNTS; ++k) cnt[k] = 0u;

    for (int s = r0 - 1; s <= r1; s += SR) {            // the centres are rows s .. s + SR - 1, row y of the bitmap is s - 2 + y
        const int ntask = (SR + 2 * SH_HALO_R) * wpr;
        for (int t0 = wave * SH_LOADS; t0 < ntask; t0 += LT_WAVES * SH_LOADS) {       // uniform over the wave
            bool ok[SH_LOADS];
            int vl[SH_LOADS], ve[SH_LOADS];
#pragma unroll
            for (int u = 0; u < SH_LOADS; ++u) {
                const int t = t0 + u, y = t / wpr, k = t - y * wpr;
                const int r = s - SH_HALO_R + y, c = c0 - SH_HALO_C + 64 * k + lane;
                ok[u] = t < ntask && r >= r0 && r <= r1 && c >= c0 && c <= c1;          // inside the box, so inside the image
                const size_t at = ok[u] ? (size_t)r * W + c : home;
                vl[u] = ll[at];
                ve[u] = ee ? ee[at] : 0;
            }
#pragma unroll
            for (int u = 0; u < SH_LOADS; ++u) {
                const unsigned long long m = __ballot(ok[u] && vl[u] == lab && ve[u] == 0);
                if (lane == 0 && t0 + u < ntask) bm[t0 + u] = m;
            }
        }
        __syncthreads();
        const int rows = min(SR, r1 - s + 1);           // the centres that are rows of the box, or the one above it
        if (want_hull) {
            for (int i = tid; i < rows; i += SH_THREADS) {
                const int r = s + i;
                if (r < r0) continue;
                const unsigned long long* rp = bm + (size_t)(i + SH_HALO_R) * wpr;
                int first = 0x7fff, last = -1;
                for (int k = 0; k < nw; ++k) {
                    const unsigned long long m = rp[k];
                    if (m == 0ull) continue;
                    if (first == 0x7fff) first = 64 * k + __ffsll((long long)m) - 1 - SH_HALO_C;
                    last = 64 * k + 63 - __clzll((long long)m) - SH_HALO_C;
                }
                rowL[r - r0] = (short)first;
                rowR[r - r0] = (short)last;
            }
        }
        const int total = rows * (w + 1);               // the centres' columns are c0 - 1 .. c1
        for (int idx = tid; idx < total; idx += SH_THREADS) {
            const int i = idx / (w + 1), jx = idx - i * (w + 1);         // column c0 - 1 + jx: bits jx .. jx + 4 are its five
            unsigned int n5[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) n5[k] = sh_bits5(bm + (size_t)(i + k) * wpr, jx);
            const unsigned int code = ((n5[2] >> 2) & 1u) | (((n5[3] >> 2) & 1u) << 1) | (((n5[2] >> 3) & 1u) << 2) | (((n5[3] >> 3) & 1u) << 3);
            if (code == 0u && ((n5[2] >> 2) & 1u) == 0u) continue;
#pragma unroll
            for (int k = 1; k < 16; ++k) cnt[k - 1] += code == (unsigned int)k ? 1u : 0u;
            if ((n5[2] >> 2) & 1u) {
                // bits 1..3 of br[k]: whether the pixels of row k - 2, columns -1..1, are border pixels of the object
                unsigned int br[3];
#pragma unroll
                for (int k = 1; k <= 3; ++k) br[k - 1] = n5[k] & ~(n5[k - 1] & n5[k + 1] & (n5[k] << 1) & (n5[k] >> 1));
                if ((br[1] >> 2) & 1u) {
                    const unsigned int a = ((br[0] >> 2) & 1u) + ((br[2] >> 2) & 1u) + ((br[1] >> 1) & 1u) + ((br[1] >> 3) & 1u);
                    const unsigned int d = ((br[0] >> 1) & 1u) + ((br[0] >> 3) & 1u) + ((br[2] >> 1) & 1u) + ((br[2] >> 3) & 1u);
                    // 1 + 2 a + 10 d in {5, 7, 15, 17, 25, 27}, {21, 33}, {13, 23}
                    cnt[15] += (a == 2u || a == 3u) && d <= 2u ? 1u : 0u;
                    cnt[16] += (a == 0u && d == 2u) || (a == 1u && d == 3u) ? 1u : 0u;
                    cnt[17] += a == 1u && (d == 1u || d == 2u) ? 1u : 0u;
                }
            }
        }
        __syncthreads();                                // before the next strip's bitmap
    }
#pragma unroll
    for (int k = 0; k < SH_COUNTS; ++k) {
        const unsigned int t = wave_sum(cnt[k]);
        if (lane == 0) red[wave][k] = t;
    }
    __syncthreads();
    if (tid < SH_COUNTS) {
        unsigned int t = 0u;
        for (int q = 0; q < LT_WAVES; ++q) t += red[q][tid];
        if (tid < 15) quads[row * 16 + 1 + tid] = (int)t;
        else perim[row * 3 + (tid - 15)] = (int)t;
    }
    if (!want_hull) return;

    // ---- the hull: chains, the pixel centres inside or on them (as ex_region_pass), the two Feret searches
    if (tid == 0) nch[0] = build_chain(rowL, h, false, chL);
    if (tid == 64) nch[1] = build_chain(rowR, h, true, chR);
    __syncthreads();
    const int nl = nch[0], nr = nch[1];
    long long inside = 0;
    for (int i = tid; i < h; i += SH_THREADS) {
        const int y = 2 * i;
        int k = chain_segment(chL, nl, y);
        long long y0 = pt_y(chL[k]), x0 = pt_x(chL[k]), dy = pt_y(chL[k + 1]) - y0, dx = pt_x(chL[k + 1]) - x0;
        const long long jl = ceil_div(x0 * dy + dx * (y - y0), 2 * dy);
        k = chain_segment(chR, nr, y);
        y0 = pt_y(chR[k]); x0 = pt_x(chR[k]); dy = pt_y(chR[k + 1]) - y0; dx = pt_x(chR[k + 1]) - x0;
        const long long jr = floor_div(x0 * dy + dx * (y - y0), 2 * dy);
        const long long a = max(jl, 0ll), e = min(jr, (long long)w - 1);
        if (e >= a) inside += e - a + 1;
    }
    inside = wave_sum(inside);
    if (lane == 0) redc[wave] = inside;

    // The vertices are the left chain's, then the right chain's; the edges are the chains' segments and the two that join their
    // ends, which are single points where a chain's end is the other's.
    const int nv = nl + nr;
    auto vertex = [&](int i) { return i < nl ? chL[i] : chR[i - nl]; };
    long long far2 = 0;
    for (int i = tid; i < nv; i += SH_THREADS) {
        const int p = vertex(i);
        for (int j = i + 1; j < nv; ++j) {
            const int q = vertex(j);
            const long long dy = pt_y(q) - pt_y(p), dx = pt_x(q) - pt_x(p);
            far2 = max(far2, dy * dy + dx * dx);
        }
    }
    unsigned long long bw = 0ull, bd = 0ull;            // bd 0: no edge yet
    for (int e = tid; e < nv; e += SH_THREADS) {
        int pa, pb;
        if (e < nl - 1) { pa = chL[e]; pb = chL[e + 1]; }
        else if (e < nv - 2) { pa = chR[e - (nl - 1)]; pb = chR[e - (nl - 1) + 1]; }
        else if (e == nv - 2) { pa = chL[0]; pb = chR[0]; }
        else { pa = chL[nl - 1]; pb = chR[nr - 1]; }
        const long long ey = pt_y(pb) - pt_y(pa), ex = pt_x(pb) - pt_x(pa);
        const unsigned long long den = (unsigned long long)(ey * ey + ex * ex);
        if (den == 0ull) continue;
        long long wmax = 0;
        for (int j = 0; j < nv; ++j) {
            const int q = vertex(j);
            const long long cr = ey * (pt_x(q) - pt_x(pa)) - ex * (pt_y(q) - pt_y(pa));
            wmax = max(wmax, cr < 0 ? -cr : cr);
        }
        if (bd == 0ull || sh_narrower((unsigned long long)wmax, den, bw, bd)) { bw = (unsigned long long)wmax; bd = den; }
    }
    __syncthreads();                                    // the strips are done with the bitmap: it carries the threads' results now
    bm[tid] = (unsigned long long)far2;
    bm[SH_THREADS + tid] = bw;
    bm[2 * SH_THREADS + tid] = bd;
    __syncthreads();
    if (tid != 0) return;
    for (int q = 1; q < SH_THREADS; ++q) {
        far2 = max(far2, (long long)bm[q]);
        const unsigned long long w2 = bm[SH_THREADS + q], d2 = bm[2 * SH_THREADS + q];
        if (d2 != 0ull && (bd == 0ull || sh_narrower(w2, d2, bw, bd))) { bw = w2; bd = d2; }
    }
    long long* o = hull + row * 4;
    o[0] = redc[0] + redc[1] + redc[2] + redc[3];
    o[1] = far2;
    o[2] = (long long)bw;
    o[3] = (long long)bd;
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_shape(cs_preproc* p, const int32_t* labels, const int32_t* exclude, int32_t batch, int32_t height, int32_t width, int in_kind,
                   int32_t max_label, int want_hull, int64_t* moments, int32_t* box, int32_t* quads, int32_t* perim, int64_t* hull, int out_kind)
{
    if (!labels || !moments || !box || !quads || !perim) return fail(CS_ERR_INVALID, "NULL argument");
    if ((want_hull != 0) != (hull != nullptr)) return fail(CS_ERR_INVALID, "hull is required with want_hull and must be NULL without it");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if ((rc = label_cap("max_label", max_label, batch, 0, kShMaxRows, "the tables", "rows")) || (rc = image_limits(batch, height, width)) ||
        (rc = handle_check(p)) || (rc = state_begin(p)))
        return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width;
    const size_t npx = (size_t)batch * H * W;
    const int64_t rows = (int64_t)batch * max_label;
    const size_t mbytes = (size_t)rows * LB_MOMENTS * sizeof(int64_t), hbytes = want_hull ? (size_t)rows * 4 * sizeof(int64_t) : 0,
                 bbytes = (size_t)rows * 4 * sizeof(int), qbytes = (size_t)rows * 16 * sizeof(int), pbytes = (size_t)rows * 3 * sizeof(int);
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rc = S.tx_box.ensure((size_t)rows * 4 * sizeof(int)))) return rc;
    const int *d_lab = labels, *d_ex = exclude;
    if (in_host) {                                      // the upload of the labels in lab, of exclude in parent
        if ((rc = S.lab.ensure(npx * sizeof(int))) || (exclude && (rc = S.parent.ensure(npx * sizeof(int))))) return rc;
        HIPCHK(hipMemcpyAsync(S.lab.p, labels, npx * sizeof(int), hipMemcpyHostToDevice, st));
        d_lab = S.lab.as<int>();
        if (exclude) {
            HIPCHK(hipMemcpyAsync(S.parent.p, exclude, npx * sizeof(int), hipMemcpyHostToDevice, st));
            d_ex = S.parent.as<int>();
        }
    }
    // the records on their way to the host, the 8-byte ones first: moments, hull, box, quads, perim
    if (out_host && (rc = S.stage.ensure(mbytes + hbytes + bbytes + qbytes + pbytes))) return rc;
    char* base = S.stage.as<char>();
    unsigned long long* d_mom = out_host ? (unsigned long long*)base : (unsigned long long*)moments;
    long long* d_hull = !want_hull ? nullptr : out_host ? (long long*)(base + mbytes) : (long long*)hull;
    int* d_box = out_host ? (int*)(base + mbytes + hbytes) : box;
    int* d_quads = out_host ? (int*)(base + mbytes + hbytes + bbytes) : quads;
    int* d_perim = out_host ? (int*)(base + mbytes + hbytes + bbytes + qbytes) : perim;
    const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0;       // sh_outline loads pixel by pixel
    int* d_ebox = S.tx_box.as<int>();
    unsigned int* d_ctrl = S.ctrl.as<unsigned int>();

    if ((rc = S.clk_sh.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(d_ctrl, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_ebox, 0, (size_t)rows * 4 * sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_mom, 0, mbytes, st));
    if (d_hull) HIPCHK(hipMemsetAsync(d_hull, 0, hbytes, st));
    HIPCHK(hipMemsetAsync(d_box, 0, bbytes, st));
    HIPCHK(hipMemsetAsync(d_quads, 0, qbytes, st));
    HIPCHK(hipMemsetAsync(d_perim, 0, pbytes, st));
    hipLaunchKernelGGL(sh_moments, label_tile_grid(batch, H, W), dim3(LB_THREADS), 0, st, d_lab, d_ex, H, W, vec, (int)max_label, (int*)nullptr, d_ebox,
                       d_mom, d_ctrl);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_sh.record(1, st))) return rc;
    const int small = std::min(H, SH_SMALL_ROWS);
    hipLaunchKernelGGL(sh_outline, dim3((unsigned)rows), dim3(SH_THREADS), want_hull ? sh_hull_lds(small) : 0, st, d_lab, d_ex, H, W, (int)max_label,
                       (const unsigned long long*)d_mom, (const int*)d_ebox, 0, small, want_hull, d_box, d_quads, d_perim, d_hull);
    HIPCHK(hipGetLastError());
    if (H > small) {                                    // the boxes taller than the first launch's
        const size_t lds = want_hull ? sh_hull_lds(H) : 0;
        if (lds) HIPCHK(hipFuncSetAttribute((const void*)sh_outline, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(sh_outline, dim3((unsigned)rows), dim3(SH_THREADS), lds, st, d_lab, d_ex, H, W, (int)max_label,
                           (const unsigned long long*)d_mom, (const int*)d_ebox, small, H, want_hull, d_box, d_quads, d_perim, d_hull);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_sh.record(2, st))) return rc;
    unsigned int bad = 0u;
    HIPCHK(hipMemcpyAsync(&bad, d_ctrl, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(moments, d_mom, mbytes, hipMemcpyDeviceToHost, st));
        if (d_hull) HIPCHK(hipMemcpyAsync(hull, d_hull, hbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(box, d_box, bbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(quads, d_quads, qbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(perim, d_perim, pbytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host records
    if ((rc = S.clk_sh.finish())) return rc;
    if (bad) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    return CS_OK;
}

int cs_label_shape_last_timing(const cs_preproc* p, double* moments_ms, double* outline_ms)
{
    return clock_read(p, &SegmentState::clk_sh, {moments_ms, outline_ms});
}
