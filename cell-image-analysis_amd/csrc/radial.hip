// radial.hip -- per-object radial intensity distribution and edge intensities of a label image on gfx950 (include/cellscreen.h,
// cs_label_radial; the rule and the sizing: DESIGN 3za, restated in tests/radial_reference.py).
//
// Per object (a label > 0 of an image, less the pixels where `exclude` is non-zero; a pixel's effective label is 0 where it is
// excluded): E2, the exact squared Euclidean distance of every object pixel to the nearest position that is not the object's
// (another label, background, an excluded pixel, anything outside the image); the centre, the deepest pixel with the smallest
// raster index, or the caller's; per (object, ring, wedge) the pixel count and per channel sum v, the ring decided in integers
// from E2 and the squared straight-line distance to the centre; over the pixels with E2 == 1 the count and per channel sum v,
// sum v^2, min, max.  All integers; FracAtD, MeanFrac, RadialCV and the edge measures follow on the host.
//   lr_columns   as ex_columns (expand.hip): one thread per column, two sweeps, 16 rows per step in registers.  Per pixel the
//                distance g within its column to the nearest pixel with another effective label or to the image's edge (the
//                first position outside is at distance 1), capped at 128.  A label outside 0..max_label sets the status word.
//   lr_rows      one row strip of 256 pixels with a halo of 127 on both sides, column distances and effective labels, in LDS.
//                An object pixel starts from g^2 and looks outwards to both sides while dx^2 < best: a pixel of its own label
//                gives dx^2 + g^2, the first foreign pixel of a side gives dx^2 and ends that side (everything behind it is
//                farther).  Within a column of the object's own label only the column's nearest foreign position can be nearest
//                overall, so the two passes are exact together.  A best above 127^2 is not exact (capped g, halo): it sets the
//                second status word.  E2 goes out as uint16; the centre by a 64-bit atomicMax of (E2 << 32) | ~raster per
//                distinct label of a wave (merge_open_runs).  A maximum does not depend on the order of arrival.
//   lr_centers   per table row: the key back into row, column, E2; the caller's centre over the first two where given.
//   lr_bins      on the tile of label_tile.hpp.  A lane keeps two open runs: one under its label (area, sum r, sum c, the edge
//                records) and one under (label, ring, wedge) (n, sum v per channel).  Runs go into two tables in LDS, the
//                lanes' last runs merged per distinct key of the wave first; only the distinct keys of a tile reach the dense
//                tables, as 64-bit integer atomics (the edge count as a 32-bit one).  A key that finds no room in LDS goes to
//                the global tables directly.  A tile holds 16384 pixels, so the ring table in LDS sums in 32 bits.
//                LDS: 1024 ring slots of 8 + 4 C bytes and 256 / 256 / 128 / 128 label slots of 36 + 24 C bytes at
//                C = 1 / 2 / 3 / 4: 28 / 38 / 34 / 41 KB, 3 to 5 workgroups per CU by LDS.
//   lr_close     the edge minimum travels as 65536 - v under an atomic maximum (li_close of intensity.hip); this turns it back.
// No floating point; every result is a sum, a minimum or a maximum of integers: bit-identical run to run, and every pixel is a
// function of its own image.  A label is range-checked before it is a key or an index.  Products: (B - k)^2 C2 <= 225 * 2 *
// 4095^2 and k^2 E2 <= 225 * 127^2 are taken in 64 bits; v^2 <= 65535^2 stays unsigned below 2^32.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int LR_THREADS = LT_THREADS;
static constexpr int LR_CAP = 128;                      // column distances are capped here: only E2 <= 127^2 is exact
static constexpr int LR_HALO = LR_CAP - 1;
static constexpr int LR_ROW = LR_THREADS;               // pixels of one row per workgroup in the row pass
static constexpr int LR_STEP = 16;                      // rows a thread of the column pass loads before it uses the first
static constexpr int LR_LDS_PROBES = 16;
static constexpr int LR_RING_LOG2 = 10;
static constexpr int kLrMaxChannels = 4;
static constexpr int kLrMaxBins = CS_RADIAL_MAX_BINS;
static constexpr int64_t kLrMaxCells = 1 << 22;         // batch * max_label * channels
static constexpr size_t kLrMaxRing = (size_t)1 << 30;   // bytes of the ring table
static constexpr unsigned int LR_MIN_BIAS = 65536u;     // a minimum v travels as LR_MIN_BIAS - v >= 1
static_assert(LR_HALO * LR_HALO == CS_RADIAL_MAX_D2, "the header states the depth limit");

template <int C> struct LrLabelSlots { static constexpr int log2 = C <= 2 ? 8 : 7; };

// the effective label: 0 for background, an excluded pixel and a label out of range (the column pass reports that one)
__device__ inline int lr_eff(int lab, int ex, int max_label) { return lab <= 0 || lab > max_label || ex != 0 ? 0 : lab; }

// ---- lr_columns ---------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 256), B).  status[0]: a label out of range.
__global__ __launch_bounds__(LR_THREADS) void lr_columns(const int* __restrict__ labels, const int* __restrict__ exclude, int H, int W,
                                                         int max_label, unsigned char* __restrict__ g, unsigned int* __restrict__ status)
{
    const int x = blockIdx.x * LR_THREADS + threadIdx.x;
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.y * H * W + x;
    int d = 0, prev = -1;                               // above the image there is no label
    bool bad = false;
    for (int y0 = 0; y0 < H; y0 += LR_STEP) {
        int v[LR_STEP], e[LR_STEP];
#pragma unroll
        for (int k = 0; k < LR_STEP; ++k) {
            v[k] = y0 + k < H ? labels[base + (size_t)(y0 + k) * W] : 0;
            e[k] = exclude && y0 + k < H ? exclude[base + (size_t)(y0 + k) * W] : 0;
        }
#pragma unroll
        for (int k = 0; k < LR_STEP; ++k) {
            if (y0 + k >= H) continue;
            bad |= v[k] < 0 || v[k] > max_label;
            const int lab = lr_eff(v[k], e[k], max_label);
            d = lab == prev ? min(d + 1, LR_CAP) : 1;
            prev = lab;
            g[base + (size_t)(y0 + k) * W] = (unsigned char)d;
        }
    }
    if (bad) *status = 1u;                              // a plain store of a constant
    d = 0;
    prev = -1;
    for (int y1 = H - 1; y1 >= 0; y1 -= LR_STEP) {
        int v[LR_STEP], e[LR_STEP];
        unsigned char m[LR_STEP];
#pragma unroll
        for (int k = 0; k < LR_STEP; ++k) {
            v[k] = y1 - k >= 0 ? labels[base + (size_t)(y1 - k) * W] : 0;
            e[k] = exclude && y1 - k >= 0 ? exclude[base + (size_t)(y1 - k) * W] : 0;
            m[k] = y1 - k >= 0 ? g[base + (size_t)(y1 - k) * W] : 0;
        }
#pragma unroll
        for (int k = 0; k < LR_STEP; ++k) {
            if (y1 - k < 0) continue;
            const int lab = lr_eff(v[k], e[k], max_label);
            d = lab == prev ? min(d + 1, LR_CAP) : 1;
            prev = lab;
            if (d < (int)m[k]) g[base + (size_t)(y1 - k) * W] = (unsigned char)d;
        }
    }
}

// ---- lr_rows ------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 256), H, B).  e2: [B][H][W] uint16, 0 off the objects.  deepest: [B][max_label], cleared.  status[1]: a depth
// above the limit.
__global__ __launch_bounds__(LR_THREADS) void lr_rows(const int* __restrict__ labels, const int* __restrict__ exclude,
                                                      const unsigned char* __restrict__ g, int H, int W, int max_label,
                                                      unsigned short* __restrict__ e2, unsigned long long* __restrict__ deepest,
                                                      unsigned int* __restrict__ status)
{
    __shared__ unsigned char sg[LR_ROW + 2 * LR_HALO];
    __shared__ int sl[LR_ROW + 2 * LR_HALO];
    const int t = threadIdx.x, x0 = blockIdx.x * LR_ROW, b = blockIdx.z;
    const size_t row = ((size_t)b * H + blockIdx.y) * W;
    int any = 0;
    for (int i = t; i < LR_ROW + 2 * LR_HALO; i += LR_THREADS) {
        const int xx = x0 - LR_HALO + i;
        const bool in = xx >= 0 && xx < W;
        const int lab = in ? lr_eff(labels[row + xx], exclude ? exclude[row + xx] : 0, max_label) : 0;     // outside: background
        sl[i] = lab;
        sg[i] = lab > 0 ? g[row + xx] : (unsigned char)0;   // read under the object's own label only
        any |= lab > 0 && i >= LR_HALO && i < LR_HALO + LR_ROW;
    }
    if (!__syncthreads_or(any)) {                       // a strip without objects; also the barrier behind the loads
        if (x0 + t < W) e2[row + x0 + t] = (unsigned short)0;
        return;
    }
    const int x = x0 + t, c = t + LR_HALO;
    const int lab = x < W ? sl[c] : 0;
    int best = 0;
    if (lab > 0) {
        const int g0 = sg[c];
        best = g0 * g0;
        bool left = true, right = true;
        for (int dx = 1; dx <= LR_HALO && dx * dx < best && (left || right); ++dx) {
            if (left) {
                const bool own = sl[c - dx] == lab;
                const int gl = sg[c - dx];
                best = min(best, dx * dx + (own ? gl * gl : 0));
                left = own;
            }
            if (right) {
                const bool own = sl[c + dx] == lab;
                const int gr = sg[c + dx];
                best = min(best, dx * dx + (own ? gr * gr : 0));
                right = own;
            }
        }
        if (best > LR_HALO * LR_HALO) *status = 1u;     // a plain store of a constant
    }
    if (x < W) e2[row + x] = (unsigned short)best;      // <= 128^2
    const unsigned long long mine = ((unsigned long long)(unsigned int)best << 32) | (unsigned int)~(unsigned int)(blockIdx.y * W + x);
    merge_open_runs(lab > 0, lab, t & 63, [&](int lw, bool own, bool leader) {
        const unsigned long long top = wave_max(own ? mine : 0ull);
        if (leader) atomicMax(&deepest[(size_t)b * max_label + (lw - 1)], top);
    });
}

// ---- lr_centers ---------------------------------------------------------------------------------------------------------------
// center: [rows][4] int32: row, column, E2 of the deepest pixel, 0 (the edge count, added by lr_bins); given: [rows][2] or null
__global__ __launch_bounds__(LR_THREADS) void lr_centers(const unsigned long long* __restrict__ deepest, const int* __restrict__ given,
                                                         int W, int64_t rows, int* __restrict__ center)
{
    const int64_t stride = (int64_t)gridDim.x * LR_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x; s < rows; s += stride) {
        const unsigned long long k = deepest[s];
        int r = 0, c = 0;
        if (k != 0ull) {                                // an object pixel has E2 >= 1
            const unsigned int raster = ~(unsigned int)k;
            r = given ? given[2 * s] : (int)(raster / (unsigned int)W);
            c = given ? given[2 * s + 1] : (int)(raster % (unsigned int)W);
        }
        center[4 * s] = r;
        center[4 * s + 1] = c;
        center[4 * s + 2] = (int)(k >> 32);
        center[4 * s + 3] = 0;
    }
}

// ---- lr_bins ------------------------------------------------------------------------------------------------------------------
struct LrTables {
    unsigned long long* geom;                           // [B][max_label][3]
    int* center;                                        // [B][max_label][4]
    unsigned long long* ring;                           // [B][max_label][bins][8][1 + C]
    unsigned long long* edge;                           // [B][max_label][C][4]
    int max_label, bins;
};

// the run under a label, tile coordinates (at most 64 pixels: all but sum v^2 fit 32 bits); mn holds LR_MIN_BIAS - min, 0: none
template <int C> struct LrLabelRun {
    unsigned int n, sr, sc, en, sv[C], mn[C], mx[C];
    unsigned long long sv2[C];
};

template <int C> __device__ inline void lr_reset(LrLabelRun<C>& a)
{
    a.n = a.sr = a.sc = a.en = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        a.sv[ch] = a.mn[ch] = a.mx[ch] = 0u;
        a.sv2[ch] = 0ull;
    }
}

// image coordinates: area, sum r, sum c, the edge count, per channel the edge's sum v and sum v^2; 2 C maxima
template <int C> struct LrLabelRec {
    static constexpr int N = 4 + 2 * C;
    unsigned long long s[N];
    unsigned int mx[2 * C];
};

template <int C> __device__ inline LrLabelRec<C> lr_rec(const LrLabelRun<C>& a, unsigned int r0, unsigned int c0)
{
    LrLabelRec<C> o;
    o.s[0] = a.n;
    o.s[1] = a.sr + (unsigned long long)a.n * r0;
    o.s[2] = a.sc + (unsigned long long)a.n * c0;
    o.s[3] = a.en;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        o.s[4 + 2 * ch] = a.sv[ch];
        o.s[5 + 2 * ch] = a.sv2[ch];
        o.mx[2 * ch] = a.mn[ch];
        o.mx[2 * ch + 1] = a.mx[ch];
    }
    return o;
}

template <int C> struct LrLabelLds {
    static constexpr int LOG2 = LrLabelSlots<C>::log2, SLOTS = 1 << LOG2, N = 4 + 2 * C;
    int key[SLOTS];                                     // 0: empty
    unsigned long long s[N][SLOTS];
    unsigned int mx[2 * C][SLOTS];
};

template <int C> struct LrRingLds {
    static constexpr int SLOTS = 1 << LR_RING_LOG2;
    int key[SLOTS];                                     // 0: empty; else ((label - 1) << 7 | ring << 3 | wedge) + 1
    unsigned int s[1 + C][SLOTS];                       // n, sum v: a tile's 16384 pixels of 65535 stay below 2^30
};

// where sum j and maximum m of a label's record go in the global tables; label is in 1..max_label
template <int C> __device__ inline void lr_label_add(const LrTables& T, int b, int label, int j, unsigned long long v)
{
    const size_t row = (size_t)b * T.max_label + (label - 1);
    if (j < 3) atomicAdd(&T.geom[row * 3 + j], v);
    else if (j == 3) atomicAdd(&T.center[row * 4 + 3], (int)v);
    else atomicAdd(&T.edge[(row * C + (j - 4) / 2) * 4 + (j - 4) % 2], v);
}

template <int C> __device__ inline void lr_label_top(const LrTables& T, int b, int label, int m, unsigned int v)
{
    const size_t row = (size_t)b * T.max_label + (label - 1);
    atomicMax(&T.edge[(row * C + m / 2) * 4 + 2 + m % 2], (unsigned long long)v);
}

template <int C> __device__ inline void lr_label_flush(LrLabelLds<C>& L, const LrTables& T, int b, int label, const LrLabelRec<C>& o)
{
    constexpr int N = LrLabelRec<C>::N, LOG2 = LrLabelLds<C>::LOG2;
    const int s = table_claim(L.key, LOG2, ((unsigned int)label * 0x9E3779B1u) >> (32 - LOG2), label, LR_LDS_PROBES);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (o.s[j] == 0ull) continue;
        if (s >= 0) atomicAdd(&L.s[j][s], o.s[j]);
        else lr_label_add<C>(T, b, label, j, o.s[j]);   // no room: straight to the global tables
    }
#pragma unroll
    for (int m = 0; m < 2 * C; ++m) {
        if (o.mx[m] == 0u) continue;
        if (s >= 0) atomicMax(&L.mx[m][s], o.mx[m]);
        else lr_label_top<C>(T, b, label, m, o.mx[m]);
    }
}

// key - 1 = (label - 1) << 7 | ring << 3 | wedge
template <int C> __device__ inline unsigned long long* lr_ring_at(const LrTables& T, int b, int key)
{
    const unsigned int k = (unsigned int)(key - 1);
    const size_t row = (size_t)b * T.max_label + (k >> 7);
    return T.ring + ((row * T.bins + ((k >> 3) & 15u)) * 8 + (k & 7u)) * (1 + C);
}

template <int C> __device__ inline void lr_ring_flush(LrRingLds<C>& L, const LrTables& T, int b, int key, unsigned int n, const unsigned int (&sv)[C])
{
    const int s = table_claim(L.key, LR_RING_LOG2, ((unsigned int)key * 0x9E3779B1u) >> (32 - LR_RING_LOG2), key, LR_LDS_PROBES);
    if (s >= 0) {
        atomicAdd(&L.s[0][s], n);
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
            if (sv[ch] != 0u) atomicAdd(&L.s[1 + ch][s], sv[ch]);
        return;
    }
    unsigned long long* at = lr_ring_at<C>(T, b, key);
    atomicAdd(&at[0], (unsigned long long)n);
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        if (sv[ch] != 0u) atomicAdd(&at[1 + ch], (unsigned long long)sv[ch]);
}

// the ring of a pixel: the number of k in 1..B-1 with (B - k)^2 C2 >= k^2 E2; the predicate falls with k
__device__ inline int lr_ring(int bins, unsigned int c2, unsigned int e2)
{
    int k = 1;
    for (; k < bins; ++k) {
        const unsigned int a = (unsigned int)((bins - k) * (bins - k)), q = (unsigned int)(k * k);
        if ((unsigned long long)a * c2 < (unsigned long long)q * e2) break;
    }
    return k - 1;
}

// grid (ceil(W/256), ceil(H/64), B).  image: [B][H][W][C] PIX; labels, exclude (or null): [B][H][W] int; e2: [B][H][W] uint16 of
// lr_rows (8-byte aligned).  vec: the width is a multiple of 4 and every plane's pointer allows the wide loads.
template <typename PIX, int C>
__global__ __launch_bounds__(LR_THREADS) void lr_bins(const PIX* __restrict__ image, const int* __restrict__ labels, const int* __restrict__ exclude,
                                                      const unsigned short* __restrict__ e2, int H, int W, int vec, LrTables T)
{
    __shared__ LrLabelLds<C> LL;
    __shared__ LrRingLds<C> LRG;
    constexpr int N = LrLabelRec<C>::N;
    for (int s = threadIdx.x; s < LrLabelLds<C>::SLOTS; s += LR_THREADS) {
        LL.key[s] = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) LL.s[j][s] = 0ull;
#pragma unroll
        for (int m = 0; m < 2 * C; ++m) LL.mx[m][s] = 0u;
    }
    for (int s = threadIdx.x; s < LrRingLds<C>::SLOTS; s += LR_THREADS) {
        LRG.key[s] = 0;
#pragma unroll
        for (int j = 0; j < 1 + C; ++j) LRG.s[j][s] = 0u;
    }
    __syncthreads();

    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const unsigned int r0 = tile.r0, c0 = tile.c0;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const unsigned short* dd = e2 + plane;
    const PIX* im = image + plane * C;
    const bool wide = vec && c_base + 3 < W;
    constexpr int PXB = 4 * C * (int)sizeof(PIX);
    constexpr int PXA = (PXB & -PXB) < 16 ? (PXB & -PXB) : 16;

    int cur = 0, rkey = 0;                              // the open runs' label and ring key; 0: none
    int cr = 0, cc = 0;                                 // the centre of `cur`
    LrLabelRun<C> run;
    lr_reset<C>(run);
    unsigned int rn = 0u, rsv[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) rsv[ch] = 0u;
#pragma unroll 2
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        unsigned short dv[4];
        PIX px[4 * C];
        const size_t at = (size_t)r * W + c_base;
        if (wide) {
            const int4 q = *(const int4*)(ll + at);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            if (ee) {
                const int4 u = *(const int4*)(ee + at);
                e[0] = u.x; e[1] = u.y; e[2] = u.z; e[3] = u.w;
            }
            __builtin_memcpy(dv, __builtin_assume_aligned(dd + at, 8), 8);
            __builtin_memcpy(px, __builtin_assume_aligned(im + at * C, PXA), PXB);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = c_base + k < W;
                x[k] = in ? ll[at + k] : 0;
                if (ee) e[k] = in ? ee[at + k] : 0;
                dv[k] = in ? dd[at + k] : (unsigned short)0;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) px[k * C + ch] = in ? im[(at + k) * C + ch] : (PIX)0;
            }
        }
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab <= 0 || lab > T.max_label || e[k] != 0) continue;      // a bad label: lr_columns has reported it
            const int col = c_base + k;
            if (lab != cur) {
                if (cur != 0) {
                    lr_label_flush<C>(LL, T, b, cur, lr_rec<C>(run, r0, c0));
                    lr_ring_flush<C>(LRG, T, b, rkey, rn, rsv);
                    rkey = 0;
                }
                cur = lab;
                lr_reset<C>(run);
                const int* ctr = T.center + ((size_t)b * T.max_label + (lab - 1)) * 4;
                cr = ctr[0];
                cc = ctr[1];
            }
            const unsigned int d2 = dv[k];
            const int dr = r - cr, dc = col - cc;
            const unsigned int adr = (unsigned int)(dr < 0 ? -dr : dr), adc = (unsigned int)(dc < 0 ? -dc : dc);
            const int ring = lr_ring(T.bins, adr * adr + adc * adc, d2);
            const int wedge = (dr > 0 ? 1 : 0) + (dc > 0 ? 2 : 0) + (adr > adc ? 4 : 0);
            const int key = (int)(((unsigned int)(lab - 1) << 7) | ((unsigned int)ring << 3) | (unsigned int)wedge) + 1;
            if (key != rkey) {
                if (rkey != 0) lr_ring_flush<C>(LRG, T, b, rkey, rn, rsv);
                rkey = key;
                rn = 0u;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) rsv[ch] = 0u;
            }
            ++rn;
            ++run.n;
            run.sr += rr;
            run.sc += (unsigned int)(4 * lane + k);
            const bool on_edge = d2 == 1u;
            run.en += on_edge ? 1u : 0u;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const unsigned int v = px[k * C + ch];
                rsv[ch] += v;
                if (on_edge) {
                    run.sv[ch] += v;
                    run.sv2[ch] += (unsigned long long)(v * v);             // 65535^2 < 2^32
                    run.mn[ch] = max(run.mn[ch], LR_MIN_BIAS - v);
                    run.mx[ch] = max(run.mx[ch], v);
                }
            }
        }
    }
    // the open runs of every lane: one insertion per distinct key of the wave
    {
        const LrLabelRec<C> mine_rec = lr_rec<C>(run, r0, c0);
        merge_open_runs(cur != 0, cur, lane, [&](int lw, bool mine, bool leader) {
            constexpr int LOG2 = LrLabelLds<C>::LOG2;
            int slot = -1;
            if (leader) slot = table_claim(LL.key, LOG2, ((unsigned int)lw * 0x9E3779B1u) >> (32 - LOG2), lw, LR_LDS_PROBES);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const unsigned long long t = wave_sum(mine ? mine_rec.s[j] : 0ull);
                if (!leader || t == 0ull) continue;
                if (slot >= 0) atomicAdd(&LL.s[j][slot], t);
                else lr_label_add<C>(T, b, lw, j, t);
            }
#pragma unroll
            for (int m = 0; m < 2 * C; ++m) {
                const unsigned int t = wave_max(mine ? mine_rec.mx[m] : 0u);
                if (!leader || t == 0u) continue;
                if (slot >= 0) atomicMax(&LL.mx[m][slot], t);
                else lr_label_top<C>(T, b, lw, m, t);
            }
        });
        merge_open_runs(rkey != 0, rkey, lane, [&](int kw, bool mine, bool leader) {
            const unsigned int n = wave_sum(mine ? rn : 0u);
            unsigned int sv[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) sv[ch] = wave_sum(mine ? rsv[ch] : 0u);     // a wave's 4096 pixels: below 2^28
            if (leader) lr_ring_flush<C>(LRG, T, b, kw, n, sv);
        });
    }
    __syncthreads();
    // the distinct keys of the tile
    for (int s = threadIdx.x; s < LrLabelLds<C>::SLOTS; s += LR_THREADS) {
        const int label = LL.key[s];
        if (label == 0) continue;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const unsigned long long t = LL.s[j][s];
            if (t != 0ull) lr_label_add<C>(T, b, label, j, t);
        }
#pragma unroll
        for (int m = 0; m < 2 * C; ++m) {
            const unsigned int t = LL.mx[m][s];
            if (t != 0u) lr_label_top<C>(T, b, label, m, t);
        }
    }
    for (int s = threadIdx.x; s < LrRingLds<C>::SLOTS; s += LR_THREADS) {
        const int key = LRG.key[s];
        if (key == 0) continue;
        unsigned long long* at = lr_ring_at<C>(T, b, key);
#pragma unroll
        for (int j = 0; j < 1 + C; ++j) {
            const unsigned int t = LRG.s[j][s];
            if (t != 0u) atomicAdd(&at[j], (unsigned long long)t);
        }
    }
}

// edge: cells = rows * C records of 4; the minimum back from its travelling form.  An object without edge pixels has none.
__global__ __launch_bounds__(LR_THREADS) void lr_close(unsigned long long* __restrict__ edge, int64_t cells)
{
    const int64_t stride = (int64_t)gridDim.x * LR_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x; s < cells; s += stride) {
        const unsigned long long enc = edge[s * 4 + 2];
        if (enc != 0ull) edge[s * 4 + 2] = (unsigned long long)LR_MIN_BIAS - enc;
    }
}

template <typename PIX, int C>
static void lr_launch(const void* image, const int* labels, const int* exclude, const unsigned short* e2, int batch, int H, int W, int vec,
                      const LrTables& T, hipStream_t st)
{
    hipLaunchKernelGGL((lr_bins<PIX, C>), label_tile_grid(batch, H, W), dim3(LR_THREADS), 0, st, (const PIX*)image, labels, exclude, e2, H, W, vec, T);
}

template <typename PIX>
static void lr_launch_c(int C, const void* image, const int* labels, const int* exclude, const unsigned short* e2, int batch, int H, int W, int vec,
                        const LrTables& T, hipStream_t st)
{
    switch (C) {
    case 1: lr_launch<PIX, 1>(image, labels, exclude, e2, batch, H, W, vec, T, st); break;
    case 2: lr_launch<PIX, 2>(image, labels, exclude, e2, batch, H, W, vec, T, st); break;
    case 3: lr_launch<PIX, 3>(image, labels, exclude, e2, batch, H, W, vec, T, st); break;
    default: lr_launch<PIX, 4>(image, labels, exclude, e2, batch, H, W, vec, T, st); break;
    }
}

static unsigned int lr_blocks(int64_t n) { return (unsigned int)std::max<int64_t>(1, std::min<int64_t>((n + LR_THREADS - 1) / LR_THREADS, 4096)); }

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_radial(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                    int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, const cs_radial_params* params,
                    const int32_t* centers, int64_t* geom, int32_t* center, int64_t* ring, int64_t* edge, uint16_t* d2, int out_kind)
{
    if (!image || !labels || !params || !geom || !center || !ring || !edge) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kLrMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kLrMaxChannels);
    if (params->bins < 1) return fail(CS_ERR_INVALID, "cs_radial_params.bins %d: must be >= 1", (int)params->bins);
    if (params->reserved != 0) return fail(CS_ERR_INVALID, "cs_radial_params.reserved must be 0");
    if (params->bins > kLrMaxBins) return fail(CS_ERR_UNSUPPORTED, "cs_radial_params.bins %d: at most %d rings", (int)params->bins, kLrMaxBins);
    if ((rc = label_cap("max_label", max_label, batch, channels, kLrMaxCells, "the tables", "cells")) || (rc = image_limits(batch, height, width)))
        return rc;
    const int H = height, W = width, C = channels, bins = params->bins;
    const int64_t rows = (int64_t)batch * max_label;
    const size_t rbytes = (size_t)rows * bins * 8 * (1 + C) * sizeof(int64_t);
    if (rbytes > kLrMaxRing)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x max_label %d x bins %d x channels %d: the ring table takes %zu bytes, above %zu (split the batch)",
                    (int)batch, (int)max_label, bins, C, rbytes, kLrMaxRing);
    if (centers)
        for (int64_t s = 0; s < rows; ++s)
            if (centers[2 * s] < 0 || centers[2 * s] >= H || centers[2 * s + 1] < 0 || centers[2 * s + 1] >= W)
                return fail(CS_ERR_INVALID, "centers: row %lld is (%d, %d), outside the image %dx%d", (long long)s, (int)centers[2 * s],
                            (int)centers[2 * s + 1], H, W);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const int64_t cells = rows * C;
    const size_t cbytes = (size_t)rows * 4 * sizeof(int32_t), gbytes = (size_t)rows * 3 * sizeof(int64_t),
                 ebytes = (size_t)cells * 4 * sizeof(int64_t), kbytes = (size_t)rows * sizeof(unsigned long long);
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    // column distances in mask, the E2 plane in dq, the deepest keys in key, the caller's centres in rec, the status words in ctrl
    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rc = S.mask.ensure(npx)) || (rc = S.dq.ensure(npx * sizeof(uint16_t))) ||
        (rc = S.key.ensure(kbytes)) || (centers && (rc = S.rec.ensure((size_t)rows * 2 * sizeof(int32_t)))))
        return rc;
    const void* d_img = image;
    const int *d_lab = labels, *d_ex = exclude;
    if (in_host) {                                      // as cs_label_intensity: the image in img, the labels in lab, exclude in parent
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
    const int* d_given = nullptr;
    if (centers) {
        HIPCHK(hipMemcpyAsync(S.rec.p, centers, (size_t)rows * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        d_given = S.rec.as<int>();
    }
    if (out_host && (rc = S.stage.ensure(cbytes + gbytes + rbytes + ebytes))) return rc;        // on their way to the host: center, geom, ring, edge
    char* sg = S.stage.as<char>();
    int* d_center = out_host ? (int*)sg : (int*)center;
    unsigned long long* d_geom = out_host ? (unsigned long long*)(sg + cbytes) : (unsigned long long*)geom;
    unsigned long long* d_ring = out_host ? (unsigned long long*)(sg + cbytes + gbytes) : (unsigned long long*)ring;
    unsigned long long* d_edge = out_host ? (unsigned long long*)(sg + cbytes + gbytes + rbytes) : (unsigned long long*)edge;
    unsigned short* d_e2 = S.dq.as<unsigned short>();
    unsigned long long* d_key = S.key.as<unsigned long long>();
    unsigned int* d_status = S.ctrl.as<unsigned int>();
    constexpr int PA[2][4] = {{4, 8, 4, 16}, {8, 16, 8, 16}};              // what lr_bins assumes of 4 pixels: PXA
    const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0 &&
                    ((uintptr_t)d_img & (uintptr_t)(PA[esz - 1][C - 1] - 1)) == 0;
    const LrTables T{d_geom, d_center, d_ring, d_edge, (int)max_label, bins};

    if ((rc = S.clk_ra.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(d_status, 0, 2 * sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_key, 0, kbytes, st));
    HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
    HIPCHK(hipMemsetAsync(d_ring, 0, rbytes, st));
    HIPCHK(hipMemsetAsync(d_edge, 0, ebytes, st));
    hipLaunchKernelGGL(lr_columns, dim3((unsigned)((W + LR_THREADS - 1) / LR_THREADS), (unsigned)batch), dim3(LR_THREADS), 0, st, d_lab, d_ex, H, W,
                       (int)max_label, S.mask.as<unsigned char>(), d_status);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ra.record(1, st))) return rc;
    hipLaunchKernelGGL(lr_rows, dim3((unsigned)((W + LR_ROW - 1) / LR_ROW), (unsigned)H, (unsigned)batch), dim3(LR_THREADS), 0, st, d_lab, d_ex,
                       S.mask.as<const unsigned char>(), H, W, (int)max_label, d_e2, d_key, d_status + 1);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(lr_centers, dim3(lr_blocks(rows)), dim3(LR_THREADS), 0, st, d_key, d_given, W, rows, d_center);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ra.record(2, st))) return rc;
    if (pixel_type == CS_PIX_U8) lr_launch_c<unsigned char>(C, d_img, d_lab, d_ex, d_e2, batch, H, W, vec, T, st);
    else lr_launch_c<unsigned short>(C, d_img, d_lab, d_ex, d_e2, batch, H, W, vec, T, st);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(lr_close, dim3(lr_blocks(cells)), dim3(LR_THREADS), 0, st, d_edge, cells);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ra.record(3, st))) return rc;
    unsigned int status[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(center, d_center, cbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ring, d_ring, rbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(edge, d_edge, ebytes, hipMemcpyDeviceToHost, st));
    }
    if (d2) HIPCHK(hipMemcpyAsync(d2, d_e2, npx * sizeof(uint16_t), out_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status words, the host tables
    if ((rc = S.clk_ra.finish())) return rc;
    if (status[0]) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    if (status[1])
        return fail(CS_ERR_UNSUPPORTED, "an object is deeper than %d px (E2 above %d): depths beyond are not exact", LR_HALO, (int)CS_RADIAL_MAX_D2);
    return CS_OK;
}

int cs_label_radial_last_timing(const cs_preproc* p, double* columns_ms, double* rows_ms, double* bins_ms)
{
    return clock_read(p, &SegmentState::clk_ra, {columns_ms, rows_ms, bins_ms});
}
