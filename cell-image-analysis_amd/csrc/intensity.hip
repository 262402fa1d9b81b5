// intensity.hip -- per-object intensity measurement of a label image on gfx950 (include/cellscreen.h, cs_label_intensity; the
// rule and the sizing: DESIGN 3u, restated in tests/intensity_reference.py).
//
// Per object (a label > 0 of an image, less the pixels where `exclude` is non-zero) and channel: area, sum r, sum c, and
// sum v, sum v^2, sum v*r, sum v*c, min v, max v.  All integers; mean, standard deviation, centroid and intensity-weighted
// centroid follow from them on the host.  Scattered global atomics are slow (the guides put single-lane ones at about 1/17 of
// the shaped rate), so, as lm_count (match.hip), the design makes them rare instead of fast:
//   li_pass      ONE read of every plane, 16-byte label loads where width and pointers allow, on the tile of label_tile.hpp.
//                A lane keeps one open run of its label with the sums of the run, coordinates relative to the tile so that
//                all but sum v^2 stay in 32 bits; the tile's origin is added once, when the run is flushed.  Flushes go into
//                a table in LDS that the workgroup owns, keyed by the label (64-bit integer adds, 32-bit min / max); the
//                lanes' last runs are first merged per distinct label.  Only the distinct labels of the
//                tile go on to the dense tables in global memory, as 64-bit integer atomics: 3 + 6 C per label and tile, not
//                per run.  A record is 3 + 4 C sums of 8 bytes and 2 C words, 28 + 40 C bytes with its key, so the table has
//                LI_SLOTS<C> slots: 512 at C = 1, 256 above (DESIGN 3u has the occupancy).  A label that finds no room in LDS
//                goes to the global tables directly.
//   li_close     the minimum travels as 65536 - v under an atomic maximum, so that cleared tables need no second initial
//                value; this pass turns it back, and an absent object keeps its zeros.
// No floating point; every result is a sum, a minimum or a maximum of integers, so it does not depend on the order of
// arrival or on slot placement, and is bit-identical run to run.  A label is range-checked before it is a key or an index.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int LI_THREADS = LT_THREADS;           // of li_close too
static constexpr int LI_LDS_PROBES = 16;
static constexpr int kLiMaxChannels = 4;
static constexpr int64_t kLiMaxCells = 1 << 22;         // batch * max_label * channels
static constexpr unsigned int LI_MIN_BIAS = 65536u;     // a minimum v travels as LI_MIN_BIAS - v >= 1

template <int C> struct LiSlots { static constexpr int log2 = C == 1 ? 9 : 8; };

// the sums of a run or of a merged set of runs, image coordinates: area, sum r, sum c, then per channel sum v, v^2, v*r, v*c
template <int C> struct LiRec {
    unsigned long long s[3 + 4 * C];
    unsigned int mn[C], mx[C];
};

// a lane's open run, tile coordinates (r in 0..63, c in 0..255, at most 64 pixels): everything but v^2 fits 32 bits
template <int C> struct LiRun {
    unsigned int n, sr, sc;
    unsigned int sv[C], svr[C], svc[C], mn[C], mx[C];
    unsigned long long sv2[C];
};

template <int C> __device__ inline void li_reset(LiRun<C>& a)
{
    a.n = a.sr = a.sc = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        a.sv[ch] = a.svr[ch] = a.svc[ch] = 0u;
        a.sv2[ch] = 0ull;
        a.mn[ch] = 0xFFFFFFFFu;
        a.mx[ch] = 0u;
    }
}

template <int C> __device__ inline LiRec<C> li_rec(const LiRun<C>& a, unsigned int r0, unsigned int c0)
{
    LiRec<C> o;
    o.s[0] = a.n;
    o.s[1] = a.sr + (unsigned long long)a.n * r0;
    o.s[2] = a.sc + (unsigned long long)a.n * c0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        o.s[3 + 4 * ch] = a.sv[ch];
        o.s[4 + 4 * ch] = a.sv2[ch];
        o.s[5 + 4 * ch] = a.svr[ch] + (unsigned long long)a.sv[ch] * r0;
        o.s[6 + 4 * ch] = a.svc[ch] + (unsigned long long)a.sv[ch] * c0;
        o.mn[ch] = a.mn[ch];
        o.mx[ch] = a.mx[ch];
    }
    return o;
}

struct LiTables {
    unsigned long long* geom;                           // [B][max_label][3]
    unsigned long long* stats;                          // [B][max_label][C][6]
    int max_label;
};

// label is in 1..max_label
template <int C> __device__ inline void li_global(const LiTables& T, int b, int label, const LiRec<C>& o)
{
    const size_t row = (size_t)b * T.max_label + (label - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicAdd(&T.geom[row * 3 + j], o.s[j]);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        unsigned long long* st = T.stats + (row * C + ch) * 6;
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&st[j], o.s[3 + 4 * ch + j]);
        atomicMax(&st[4], (unsigned long long)(LI_MIN_BIAS - o.mn[ch]));
        atomicMax(&st[5], (unsigned long long)o.mx[ch]);
    }
}

template <int C> struct LiLds {
    static constexpr int SLOTS = 1 << LiSlots<C>::log2;
    int key[SLOTS];                                     // 0: empty
    unsigned long long s[3 + 4 * C][SLOTS];
    unsigned int mn[C][SLOTS], mx[C][SLOTS];
};

template <int C> __device__ inline void li_insert(LiLds<C>& L, const LiTables& T, int b, int label, const LiRec<C>& o)
{
    constexpr int SLOTS = LiLds<C>::SLOTS;
    unsigned int h = ((unsigned int)label * 0x9E3779B1u) >> (32 - LiSlots<C>::log2);
    for (int i = 0; i < LI_LDS_PROBES; ++i) {
        const int old = atomicCAS(&L.key[h], 0, label);
        if (old == 0 || old == label) {
#pragma unroll
            for (int j = 0; j < 3 + 4 * C; ++j) atomicAdd(&L.s[j][h], o.s[j]);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                atomicMin(&L.mn[ch][h], o.mn[ch]);
                atomicMax(&L.mx[ch][h], o.mx[ch]);
            }
            return;
        }
        h = (h + 1) & (SLOTS - 1);
    }
    li_global<C>(T, b, label, o);                       // no room: straight to the global tables
}

// li_pass keeps its own load of a row, its own closing merge and its own claim of an LDS slot (li_insert) instead of
// label_load4, merge_open_runs and table_claim of label_tile.hpp: with them it takes up to 31 fewer VGPRs, and its pass at one
// channel without `exclude` measured 3 % slower than this form on an MI355X (profiles/label_tools_refactor.json).
// grid (ceil(W/256), ceil(H/64), B).  image: [B][H][W][C] PIX; labels, exclude (or null): [B][H][W] int.  vec: the width is a
// multiple of 4 and every plane's pointer allows the wide loads (decided on the host).
template <typename PIX, int C>
__global__ __launch_bounds__(LI_THREADS) void li_pass(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                      const int* __restrict__ exclude, int H, int W, int vec, LiTables T,
                                                      unsigned int* __restrict__ ctrl)
{
    constexpr int SLOTS = LiLds<C>::SLOTS;
    __shared__ LiLds<C> L;
    for (int s = threadIdx.x; s < SLOTS; s += LI_THREADS) {
        L.key[s] = 0;
#pragma unroll
        for (int j = 0; j < 3 + 4 * C; ++j) L.s[j][s] = 0ull;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            L.mn[ch][s] = 0xFFFFFFFFu;
            L.mx[ch][s] = 0u;
        }
    }
    __syncthreads();

    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const unsigned int r0 = tile.r0, c0 = tile.c0;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const PIX* im = image + plane * C;
    const bool wide = vec && c_base + 3 < W;
    // the widest load the image rows allow: 4 pixels are 4 C sizeof(PIX) bytes, aligned to their largest power of two
    constexpr int PXB = 4 * C * (int)sizeof(PIX);
    constexpr int PXA = (PXB & -PXB) < 16 ? (PXB & -PXB) : 16;

    unsigned int bad = 0u;
    int cur = 0;                                        // the open run's label; run.n == 0: none
    LiRun<C> run;
    li_reset<C>(run);
#pragma unroll 2
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        PIX px[4 * C];
        const size_t at = (size_t)r * W + c_base;
        if (wide) {
            const int4 q = *(const int4*)(ll + at);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            if (ee) {
                const int4 u = *(const int4*)(ee + at);
                e[0] = u.x; e[1] = u.y; e[2] = u.z; e[3] = u.w;
            }
            __builtin_memcpy(px, __builtin_assume_aligned(im + at * C, PXA), PXB);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = c_base + k < W;
                x[k] = in ? ll[at + k] : 0;
                if (ee) e[k] = in ? ee[at + k] : 0;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) px[k * C + ch] = in ? im[(at + k) * C + ch] : (PIX)0;
            }
        }
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab == 0) continue;
            if (lab < 0 || lab > T.max_label) { bad = 1u; continue; }
            if (e[k] != 0) continue;
            if (run.n != 0u && lab != cur) {
                li_insert<C>(L, T, b, cur, li_rec<C>(run, r0, c0));
                run.n = 0u;
            }
            const unsigned int cc = (unsigned int)(4 * lane + k);
            if (run.n == 0u) {
                cur = lab;
                li_reset<C>(run);
            }
            ++run.n;
            run.sr += rr;
            run.sc += cc;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const unsigned int v = px[k * C + ch];
                run.sv[ch] += v;
                run.sv2[ch] += (unsigned long long)(v * v);       // 65535^2 < 2^32
                run.svr[ch] += v * rr;
                run.svc[ch] += v * cc;
                run.mn[ch] = min(run.mn[ch], v);
                run.mx[ch] = max(run.mx[ch], v);
            }
        }
    }
    // the open run of every lane: one insertion per distinct label of the wave
    LiRec<C> mine_rec = li_rec<C>(run, r0, c0);
    bool open = run.n != 0u;
    for (;;) {
        const unsigned long long m = __ballot(open);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const int lw = __shfl(cur, leader);
        const bool mine = open && cur == lw;
        LiRec<C> o;
#pragma unroll
        for (int j = 0; j < 3 + 4 * C; ++j) o.s[j] = wave_sum(mine ? mine_rec.s[j] : 0ull);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            unsigned int lo = mine ? mine_rec.mn[ch] : 0xFFFFFFFFu, hi = mine ? mine_rec.mx[ch] : 0u;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                lo = min(lo, (unsigned int)__shfl_xor(lo, s));
                hi = max(hi, (unsigned int)__shfl_xor(hi, s));
            }
            o.mn[ch] = lo;
            o.mx[ch] = hi;
        }
        if (lane == leader) li_insert<C>(L, T, b, lw, o);
        if (mine) open = false;
    }
    __syncthreads();
    // the distinct labels of the tile
    for (int s = threadIdx.x; s < SLOTS; s += LI_THREADS) {
        const int label = L.key[s];
        if (label == 0) continue;
        LiRec<C> o;
#pragma unroll
        for (int j = 0; j < 3 + 4 * C; ++j) o.s[j] = L.s[j][s];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            o.mn[ch] = L.mn[ch][s];
            o.mx[ch] = L.mx[ch][s];
        }
        li_global<C>(T, b, label, o);
    }
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

// stats: cells = rows * C records of 6; the minimum back from its travelling form
__global__ __launch_bounds__(LI_THREADS) void li_close(unsigned long long* __restrict__ stats, int64_t cells)
{
    const int64_t stride = (int64_t)gridDim.x * LI_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * LI_THREADS + threadIdx.x; s < cells; s += stride) {
        const unsigned long long enc = stats[s * 6 + 4];
        if (enc != 0ull) stats[s * 6 + 4] = (unsigned long long)LI_MIN_BIAS - enc;
    }
}

template <typename PIX, int C>
static void li_launch(const void* image, const int* labels, const int* exclude, int batch, int H, int W, int vec, const LiTables& T,
                      unsigned int* ctrl, hipStream_t st)
{
    hipLaunchKernelGGL((li_pass<PIX, C>), label_tile_grid(batch, H, W), dim3(LI_THREADS), 0, st, (const PIX*)image, labels, exclude, H, W, vec, T, ctrl);
}

template <typename PIX>
static void li_launch_c(int C, const void* image, const int* labels, const int* exclude, int batch, int H, int W, int vec, const LiTables& T,
                        unsigned int* ctrl, hipStream_t st)
{
    switch (C) {
    case 1: li_launch<PIX, 1>(image, labels, exclude, batch, H, W, vec, T, ctrl, st); break;
    case 2: li_launch<PIX, 2>(image, labels, exclude, batch, H, W, vec, T, ctrl, st); break;
    case 3: li_launch<PIX, 3>(image, labels, exclude, batch, H, W, vec, T, ctrl, st); break;
    default: li_launch<PIX, 4>(image, labels, exclude, batch, H, W, vec, T, ctrl, st); break;
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_intensity(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                       int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, int64_t* geom, int64_t* stats,
                       int out_kind)
{
    if (!image || !labels || !geom || !stats) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kLiMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kLiMaxChannels);
    if ((rc = label_cap("max_label", max_label, batch, channels, kLiMaxCells, "the tables", "cells")) || (rc = image_limits(batch, height, width)) || (rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width, C = channels;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const int64_t rows = (int64_t)batch * max_label, cells = rows * C;
    const size_t gbytes = (size_t)rows * 3 * sizeof(int64_t), sbytes = (size_t)cells * 6 * sizeof(int64_t);
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    if ((rc = S.ctrl.ensure(8 * sizeof(int)))) return rc;
    const void* d_img = image;
    const int *d_lab = labels, *d_ex = exclude;
    if (in_host) {                                      // the upload of the image in img, of the labels in lab, of exclude in parent
        if ((rc = S.img.ensure(npx * C * esz)) || (rc = S.lab.ensure(npx * sizeof(int))) ||
            (exclude && (rc = S.parent.ensure(npx * sizeof(int)))))
            return rc;
        HIPCHK(hipMemcpyAsync(S.img.p, image, npx * C * esz, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(S.lab.p, labels, npx * sizeof(int), hipMemcpyHostToDevice, st));
        d_img = S.img.p;
        d_lab = S.lab.as<int>();
        if (exclude) {
            HIPCHK(hipMemcpyAsync(S.parent.p, exclude, npx * sizeof(int), hipMemcpyHostToDevice, st));
            d_ex = S.parent.as<int>();
        }
    }
    if (out_host && (rc = S.stage.ensure(gbytes + sbytes))) return rc;      // both tables on their way to the host: geom, then stats
    unsigned long long* d_geom = out_host ? S.stage.as<unsigned long long>() : (unsigned long long*)geom;
    unsigned long long* d_stats = out_host ? (unsigned long long*)(S.stage.as<char>() + gbytes) : (unsigned long long*)stats;
    constexpr int PA[2][4] = {{4, 8, 4, 16}, {8, 16, 8, 16}};              // what li_pass assumes of 4 pixels: PXA
    const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0 &&
                    ((uintptr_t)d_img & (uintptr_t)(PA[esz - 1][C - 1] - 1)) == 0;
    const LiTables T{d_geom, d_stats, (int)max_label};

    if ((rc = S.clk_in.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(S.ctrl.p, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
    HIPCHK(hipMemsetAsync(d_stats, 0, sbytes, st));
    if ((rc = S.clk_in.record(1, st))) return rc;
    if (pixel_type == CS_PIX_U8) li_launch_c<unsigned char>(C, d_img, d_lab, d_ex, batch, H, W, vec, T, S.ctrl.as<unsigned int>(), st);
    else li_launch_c<unsigned short>(C, d_img, d_lab, d_ex, batch, H, W, vec, T, S.ctrl.as<unsigned int>(), st);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(li_close, dim3((unsigned)std::min<int64_t>((cells + LI_THREADS - 1) / LI_THREADS, 4096)), dim3(LI_THREADS), 0, st, d_stats,
                       cells);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_in.record(2, st))) return rc;
    unsigned int bad = 0u;
    HIPCHK(hipMemcpyAsync(&bad, S.ctrl.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stats, d_stats, sbytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host tables
    if ((rc = S.clk_in.finish())) return rc;
    if (bad) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    return CS_OK;
}

int cs_label_intensity_last_timing(const cs_preproc* p, double* clear_ms, double* pass_ms)
{
    return clock_read(p, &SegmentState::clk_in, {clear_ms, pass_ms});
}
