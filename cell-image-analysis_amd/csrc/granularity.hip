// granularity.hip -- per-object granularity spectrum of a label image on gfx950 (include/cellscreen.h, cs_label_granularity; the
// rule and the sizing: DESIGN 3zb, restated in tests/granularity_reference.py).
//
// Per channel a working plane P (the image, or its rounded s x s block means; with `masked` the pixels off the objects count as
// 0), and for k = 1..steps the erosion E_k of E_(k-1) by the 3 x 3 cross and the reconstruction by dilation R_k of E_k under P.
// Per object (a label > 0 of an image, less the pixels where `exclude` is non-zero), step and channel the sum of R_k over the
// object's pixels; per image, step and channel the sum of R_k over the working plane.  The spectrum follows on the host.
//   gp_prepare   ONE read of the interleaved image: planar P and E <- P, the block means, the mask rule, the range check of the
//                labels.  A thread takes max(4, s) columns of the s rows of a block row, 16-byte label loads where width and
//                pointers allow.
//   gr_erode     R <- the cross minimum of E, four pixels per thread; the host then copies E <- R, so that no tile reads what
//                another has already eroded.
//   gr_recon     one round of R <- min(dilate(R), P), sp_recon's scheme (segment.hip) on uint16: a 64 x 32 tile with a one-pixel
//                halo relaxes in LDS until it is quiet.  R only rises and never passes the fixed point, so a halo read while a
//                neighbour writes is only late, never wrong; a round in which no tile changed anything is the fixed point.  All
//                channels and images go in one launch.  After a step's first round only the tiles at a moving front run: those
//                that changed, or had a neighbour change, in the round before (a stamp per tile); the others leave at once.
//                Every step starts again from E_k: R_(k-1) lies above the fixed point, and the iteration cannot come down.
//   gr_start / gr_advance   one thread: the round's "something changed" flag decides whether the step goes on.  The host enqueues
//                rounds in groups (8, 16, 32, then 64 at a time) and reads one int per group; a step takes at most Hs * Ws rounds
//                that change something, one more sets the cap flag and ends it.
//   gs_sums      the walk of label_tile.hpp over the labels, reading R[r / s][c / s]: a lane keeps one open run of its label,
//                runs are merged per wave by ballot and per workgroup in a table in LDS keyed by the label, and only the distinct
//                labels of a tile go on to the dense table, as 64-bit integer atomics.  Once per step, and once for k = 0 (R_0 =
//                P) together with geom.  The pixels at the origin of their block are the working plane: their sum, reduced per
//                workgroup, is one atomic per channel into image_sums.
// No floating point; every result is a minimum, a maximum or a sum of integers, so it does not depend on the order of arrival,
// and is bit-identical run to run.  A label is range-checked before it is a key or an index.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int GR_THREADS = LT_THREADS;
static constexpr int GR_TW = 64, GR_TH = 32;            // the reconstruction's tile
static constexpr int GR_LW = GR_TW + 2, GR_LH = GR_TH + 2;      // with its halo
static constexpr int GR_PER = GR_TH / (GR_THREADS / GR_TW);     // pixels per thread: rows lw, lw + 4, ...
static constexpr int GR_GROUP = 8, GR_GROUP_MAX = 64;   // rounds between two reads of the control word: a step's first group, the largest
static constexpr int GS_LOG2 = 8, GS_SLOTS = 1 << GS_LOG2, GS_PROBES = 16;
static constexpr int kGrMaxChannels = 4;
static constexpr int64_t kGrMaxCells = 1 << 22;         // batch * max_label * channels
static constexpr size_t kGrMaxBytes = (size_t)1 << 30;  // of the sums table and of the planes stack
enum { GC_BAD = 0, GC_CHANGED, GC_ACTIVE, GC_ROUNDS, GC_TOTAL, GC_CAPPED, GC_N = 8 };

// ---- prepare ---------------------------------------------------------------------------------------------------------------------
// grid (ceil(Hs * spans / 256), B), spans = ceil(W / G) with G = max(4, S) columns per thread.  image: [B][H][W][C] PIX; labels,
// exclude (null unless masked): [B][H][W] int; P, E: [B][C][Hs][Ws].  vec: the width is a multiple of 4 and every plane's pointer
// allows the wide loads (decided on the host).
template <typename PIX, int C, int S>
__global__ __launch_bounds__(GR_THREADS) void gp_prepare(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                         const int* __restrict__ exclude, int H, int W, int Hs, int Ws, int vec, int masked,
                                                         int max_label, unsigned short* __restrict__ P, unsigned short* __restrict__ E,
                                                         unsigned int* __restrict__ ctrl)
{
    constexpr int G = S < 4 ? 4 : S, NO = G / S;
    constexpr int PXB = 4 * C * (int)sizeof(PIX);       // 4 pixels, aligned to their largest power of two
    constexpr int PXA = (PXB & -PXB) < 16 ? (PXB & -PXB) : 16;
    const int spans = (W + G - 1) / G;
    const int idx = blockIdx.x * GR_THREADS + threadIdx.x;
    if (idx >= Hs * spans) return;
    const int R = idx / spans, c0 = (idx % spans) * G, b = blockIdx.y;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const PIX* im = image + plane * C;
    const bool wide = vec && c0 + G <= W;
    unsigned int sum[NO][C], cnt[NO], bad = 0u;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        cnt[o] = 0u;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) sum[o][ch] = 0u;
    }
    for (int dr = 0; dr < S; ++dr) {
        const int r = R * S + dr;
        if (r >= H) break;
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
            const int cq = c0 + 4 * q;
            if (cq >= W) break;
            int x[4], e[4] = {0, 0, 0, 0};
            PIX px[4 * C];
            const size_t at = (size_t)r * W + cq;
            if (wide) {
                const int4 v = *(const int4*)(ll + at);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                if (ee) {
                    const int4 u = *(const int4*)(ee + at);
                    e[0] = u.x; e[1] = u.y; e[2] = u.z; e[3] = u.w;
                }
                __builtin_memcpy(px, __builtin_assume_aligned(im + at * C, PXA), PXB);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = cq + k < W;
                    x[k] = in ? ll[at + k] : 0;
                    if (ee) e[k] = in ? ee[at + k] : 0;
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) px[k * C + ch] = in ? im[(at + k) * C + ch] : (PIX)0;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (cq + k >= W) continue;
                const int lab = x[k];
                if (lab < 0 || lab > max_label) bad = 1u;
                const bool keep = !masked || (lab != 0 && e[k] == 0);
                const int o = (4 * q + k) / S;
                ++cnt[o];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) sum[o][ch] += keep ? (unsigned int)px[k * C + ch] : 0u;
            }
        }
    }
    const size_t HW = (size_t)Hs * Ws;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        const int cw = c0 / S + o;
        if (cw >= Ws || cnt[o] == 0u) continue;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const unsigned short v = (unsigned short)((2u * sum[o][ch] + cnt[o]) / (2u * cnt[o]));     // 2 * 64 * 65535 + 64 < 2^24
            const size_t i = ((size_t)b * C + ch) * HW + (size_t)R * Ws + cw;
            P[i] = v;
            E[i] = v;
        }
    }
    if (bad) ctrl[GC_BAD] = 1u;                         // a plain store of a constant
}

// ---- erode -----------------------------------------------------------------------------------------------------------------------
// grid (ceil(Hs * ceil(Ws / 4) / 256), B, C).  R <- min over the cross of E; neighbours outside the plane are ignored.  wide: Ws is
// a multiple of 4 (the planes are the handle's own, so their rows are then 8-byte aligned).
__global__ __launch_bounds__(GR_THREADS) void gr_erode(const unsigned short* __restrict__ E, unsigned short* __restrict__ R, int Hs, int Ws, int wide)
{
    const int quads = (Ws + 3) / 4;
    const int idx = blockIdx.x * GR_THREADS + threadIdx.x;
    if (idx >= Hs * quads) return;
    const int r = idx / quads, c0 = (idx % quads) * 4;
    const size_t base = ((size_t)blockIdx.y * gridDim.z + blockIdx.z) * Hs * Ws;
    const unsigned short* e = E + base;
    unsigned int mid[6], up[4], dn[4];
    auto row4 = [&](int rr, unsigned int(&o)[4]) {
        if (rr < 0 || rr >= Hs) {
            o[0] = o[1] = o[2] = o[3] = 0xFFFFu;
        } else if (wide) {
            const ushort4 v = *(const ushort4*)(e + (size_t)rr * Ws + c0);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = c0 + k < Ws ? (unsigned int)e[(size_t)rr * Ws + c0 + k] : 0xFFFFu;
        }
    };
    unsigned int m4[4];
    row4(r - 1, up);
    row4(r + 1, dn);
    row4(r, m4);
    mid[0] = c0 > 0 ? (unsigned int)e[(size_t)r * Ws + c0 - 1] : 0xFFFFu;
    mid[5] = c0 + 4 < Ws ? (unsigned int)e[(size_t)r * Ws + c0 + 4] : 0xFFFFu;
#pragma unroll
    for (int k = 0; k < 4; ++k) mid[k + 1] = m4[k];
    unsigned short out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (unsigned short)min(min(min(mid[k], mid[k + 1]), mid[k + 2]), min(up[k], dn[k]));
    unsigned short* o = R + base + (size_t)r * Ws + c0;
    if (wide) {
        *(ushort4*)o = make_ushort4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < Ws) o[k] = out[k];
    }
}

// ---- reconstruct -----------------------------------------------------------------------------------------------------------------
// one thread: the control words before the rounds of a step
__global__ void gr_start(int* __restrict__ ctrl)
{
    ctrl[GC_CHANGED] = 0;
    ctrl[GC_ROUNDS] = 0;
    ctrl[GC_ACTIVE] = 1;
}

// one thread, after every round.  A round that changed something is counted against the cap; a path through the plane has fewer
// than Hs * Ws pixels, so the cap never binds on a correct run.
__global__ void gr_advance(int* __restrict__ ctrl, int cap)
{
    if (ctrl[GC_ACTIVE] == 0) return;
    ++ctrl[GC_TOTAL];
    if (ctrl[GC_CHANGED] == 0) {
        ctrl[GC_ACTIVE] = 0;
    } else if (++ctrl[GC_ROUNDS] > cap) {
        ctrl[GC_ACTIVE] = 0;
        ctrl[GC_CAPPED] = 1;
    }
    ctrl[GC_CHANGED] = 0;
}

// grid (tx * C, ceil(Hs / 32), B) with tx = ceil(Ws / 64): the tiles of all channels and images in one launch.
__global__ __launch_bounds__(GR_THREADS) void gr_recon(const unsigned short* __restrict__ P, unsigned short* R, int Hs, int Ws, int tx, int* ctrl,
                                                       int* stamp)
{
    if (ctrl[GC_ACTIVE] == 0) return;
    // Only a tile at a moving front can change: after a step's first round a tile runs when it or one of its four neighbours
    // changed in the round before (the halo is one pixel of the cross, so corners do not matter).  stamp holds the round, counted
    // over the whole call, in which a tile last changed.  Neighbours store into these words while this kernel runs, so two waves
    // may read different values: every thread votes and the workgroup decides once, at a barrier all of its threads reach
    // (__syncthreads_or), so it leaves whole or stays whole.  A neighbour that overwrites its stamp in this very round is seen as
    // well (>=), and a change missed now is seen in the next round, which then follows because that neighbour raised the flag.  A
    // tile that is skipped was quiet on its halo when it last ran and no neighbour has changed since, so a round without a change
    // is still the fixed point.
    const int round = ctrl[GC_TOTAL];
    const int tile = ((int)(blockIdx.z * (gridDim.x / tx) + blockIdx.x / tx) * (int)gridDim.y + (int)blockIdx.y) * tx + (int)(blockIdx.x % tx);
    {
        const int bx = blockIdx.x % tx, by = blockIdx.y;
        int last = stamp[tile];
        if (bx > 0) last = max(last, stamp[tile - 1]);
        if (bx + 1 < tx) last = max(last, stamp[tile + 1]);
        if (by > 0) last = max(last, stamp[tile - tx]);
        if (by + 1 < (int)gridDim.y) last = max(last, stamp[tile + tx]);
        const int go = ctrl[GC_ROUNDS] == 0 || last >= round - 1;          // a step's first round: every tile
        if (!__syncthreads_or(go)) return;
    }
    __shared__ unsigned short sR[GR_LH * GR_LW];
    volatile unsigned short* v = sR;
    const int lx = threadIdx.x & 63, lw = threadIdx.x >> 6;
    const int ch = blockIdx.x / tx, C = gridDim.x / tx;
    const int x0 = (blockIdx.x % tx) * GR_TW, y0 = blockIdx.y * GR_TH;
    const size_t base = ((size_t)blockIdx.z * C + ch) * Hs * Ws;
    for (int i = threadIdx.x; i < GR_LH * GR_LW; i += GR_THREADS) {
        const int y = y0 + i / GR_LW - 1, x = x0 + i % GR_LW - 1;
        sR[i] = y >= 0 && y < Hs && x >= 0 && x < Ws ? R[base + (size_t)y * Ws + x] : (unsigned short)0;
    }
    const int x = x0 + lx;
    int d[GR_PER], cur[GR_PER], was[GR_PER];
#pragma unroll
    for (int k = 0; k < GR_PER; ++k) {
        const int y = y0 + lw + 4 * k;
        d[k] = x < Ws && y < Hs ? (int)P[base + (size_t)y * Ws + x] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GR_PER; ++k) was[k] = cur[k] = sR[(lw + 4 * k + 1) * GR_LW + lx + 1];
    for (int it = 0; it < GR_TW * GR_TH; ++it) {                            // a path inside the tile has at most that many pixels
        int chg = 0;
#pragma unroll
        for (int k = 0; k < GR_PER; ++k) {
            if (cur[k] >= d[k]) continue;
            const int c = (lw + 4 * k + 1) * GR_LW + lx + 1;
            int m = max(max((int)v[c - 1], (int)v[c + 1]), max((int)v[c - GR_LW], (int)v[c + GR_LW]));
            m = min(m, d[k]);
            if (m > cur[k]) { cur[k] = m; v[c] = (unsigned short)m; chg = 1; }
        }
        if (!__syncthreads_or(chg)) break;
    }
    int any = 0;
#pragma unroll
    for (int k = 0; k < GR_PER; ++k)
        if (cur[k] != was[k]) { R[base + (size_t)(y0 + lw + 4 * k) * Ws + x] = (unsigned short)cur[k]; any = 1; }     // in the plane: d > 0 there only
    any = __syncthreads_or(any);
    if (threadIdx.x == 0 && any) {
        atomicOr(&ctrl[GC_CHANGED], 1);
        stamp[tile] = round;
    }
}

// ---- sums ------------------------------------------------------------------------------------------------------------------------
struct GsTables {
    unsigned long long* geom;                           // [B][max_label][3]; null but at k = 0
    unsigned long long* sums;                           // [B][max_label][steps + 1][C]
    unsigned long long* image_sums;                     // [B][steps + 1][C]
    int max_label, steps1, k;
};

template <int C> struct GsLds {
    int key[GS_SLOTS];                                  // 0: empty
    unsigned long long s[3 + C][GS_SLOTS];              // n, sum r, sum c, then per channel sum R
};

// label is in 1..max_label; j: 0..2 geom, 3.. the channel's sum
template <int C> __device__ inline void gs_global(const GsTables& T, int b, int label, int j, unsigned long long t)
{
    const size_t row = (size_t)b * T.max_label + (label - 1);
    if (j < 3) {
        if (T.geom) atomicAdd(&T.geom[row * 3 + j], t);
    } else {
        atomicAdd(&T.sums[(row * T.steps1 + T.k) * C + (j - 3)], t);
    }
}

// a lane's closed run: tile coordinates (at most 64 pixels of at most 65535)
template <int C> __device__ inline void gs_flush(GsLds<C>& L, const GsTables& T, int b, int label, unsigned int r0, unsigned int c0, unsigned int n,
                                                 unsigned int sr, unsigned int sc, const unsigned int (&sv)[C])
{
    unsigned long long o[3 + C];
    o[0] = n;
    o[1] = sr + (unsigned long long)n * r0;
    o[2] = sc + (unsigned long long)n * c0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[3 + ch] = sv[ch];
    const int slot = table_claim(L.key, GS_LOG2, ((unsigned int)label * 0x9E3779B1u) >> (32 - GS_LOG2), label, GS_PROBES);
#pragma unroll
    for (int j = 0; j < 3 + C; ++j) {
        if (slot >= 0) atomicAdd(&L.s[j][slot], o[j]);
        else gs_global<C>(T, b, label, j, o[j]);        // no room: straight to the global tables
    }
}

// grid (ceil(W/256), ceil(H/64), B).  labels, exclude (or null): [B][H][W] int; R: [B][C][Hs][Ws], read at [r >> shift][c >> shift].
// vec: the width is a multiple of 4 and the label planes' pointers allow the wide loads.
template <int C>
__global__ __launch_bounds__(GR_THREADS) void gs_sums(const int* __restrict__ labels, const int* __restrict__ exclude,
                                                      const unsigned short* __restrict__ R, int H, int W, int Hs, int Ws, int shift, int vec,
                                                      GsTables T)
{
    __shared__ GsLds<C> L;
    __shared__ unsigned long long wsum[LT_WAVES][C];
    for (int s = threadIdx.x; s < GS_SLOTS; s += GR_THREADS) {
        L.key[s] = 0;
#pragma unroll
        for (int j = 0; j < 3 + C; ++j) L.s[j][s] = 0ull;
    }
    __syncthreads();

    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const unsigned int r0 = tile.r0, c0 = tile.c0;
    const size_t plane = (size_t)b * H * W, HW = (size_t)Hs * Ws;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const unsigned short* rp = R + (size_t)b * C * HW;
    const bool wide = vec && c_base + 3 < W;
    const bool wide_r = shift == 0 && (W & 3) == 0 && c_base + 3 < W;      // the planes are the handle's own: rows 8-byte aligned
    const int smask = (1 << shift) - 1;

    int cur = 0;                                        // the open run's label; 0: none
    unsigned int n = 0u, sr = 0u, sc = 0u, sv[C], isum[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) sv[ch] = isum[ch] = 0u;
#pragma unroll 2
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        unsigned int val[4][C];
        const size_t at = (size_t)r * W + c_base;
        label_load4(ll + at, W - c_base, wide, x);
        if (ee) label_load4(ee + at, W - c_base, wide, e);
        const size_t rrow = (size_t)(r >> shift) * Ws;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if (wide_r) {
                const ushort4 q = *(const ushort4*)(rp + ch * HW + rrow + c_base);
                val[0][ch] = q.x; val[1][ch] = q.y; val[2][ch] = q.z; val[3][ch] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) val[k][ch] = c_base + k < W ? (unsigned int)rp[ch * HW + rrow + ((c_base + k) >> shift)] : 0u;
            }
        }
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
        const bool row_origin = (r & smask) == 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c_base + k >= W) continue;
            if (row_origin && ((c_base + k) & smask) == 0) {                // the block's origin stands for its pixel of the working plane
#pragma unroll
                for (int ch = 0; ch < C; ++ch) isum[ch] += val[k][ch];
            }
            const int lab = x[k];
            if (lab <= 0 || lab > T.max_label || e[k] != 0) continue;       // a bad label: gp_prepare has reported it
            if (lab != cur) {
                if (cur != 0) gs_flush<C>(L, T, b, cur, r0, c0, n, sr, sc, sv);
                cur = lab;
                n = sr = sc = 0u;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) sv[ch] = 0u;
            }
            ++n;
            sr += rr;
            sc += (unsigned int)(4 * lane + k);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) sv[ch] += val[k][ch];
        }
    }
    // the open run of every lane: one insertion per distinct label of the wave
    {
        unsigned long long mine_rec[3 + C];
        mine_rec[0] = n;
        mine_rec[1] = sr + (unsigned long long)n * r0;
        mine_rec[2] = sc + (unsigned long long)n * c0;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) mine_rec[3 + ch] = sv[ch];
        merge_open_runs(cur != 0, cur, lane, [&](int lw, bool mine, bool leader) {
            int slot = -1;
            if (leader) slot = table_claim(L.key, GS_LOG2, ((unsigned int)lw * 0x9E3779B1u) >> (32 - GS_LOG2), lw, GS_PROBES);
#pragma unroll
            for (int j = 0; j < 3 + C; ++j) {
                const unsigned long long t = wave_sum(mine ? mine_rec[j] : 0ull);
                if (!leader || t == 0ull) continue;
                if (slot >= 0) atomicAdd(&L.s[j][slot], t);
                else gs_global<C>(T, b, lw, j, t);
            }
        });
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const unsigned long long t = wave_sum((unsigned long long)isum[ch]);
        if (lane == 0) wsum[tile.wave][ch] = t;
    }
    __syncthreads();
    // the distinct labels of the tile
    for (int s = threadIdx.x; s < GS_SLOTS; s += GR_THREADS) {
        const int label = L.key[s];
        if (label == 0) continue;
#pragma unroll
        for (int j = 0; j < 3 + C; ++j) {
            const unsigned long long t = L.s[j][s];
            if (t != 0ull) gs_global<C>(T, b, label, j, t);
        }
    }
    if (threadIdx.x < C) {
        unsigned long long t = 0ull;
#pragma unroll
        for (int w = 0; w < LT_WAVES; ++w) t += wsum[w][threadIdx.x];
        if (t != 0ull) atomicAdd(&T.image_sums[((size_t)b * T.steps1 + T.k) * C + threadIdx.x], t);
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------------
struct GpArgs {
    const void* image;
    const int *labels, *exclude;
    int batch, H, W, Hs, Ws, vec, masked, max_label;
    unsigned short *P, *E;
    unsigned int* ctrl;
};

template <typename PIX, int C, int S> static void gp_launch(const GpArgs& a, hipStream_t st)
{
    constexpr int G = S < 4 ? 4 : S;
    const int64_t items = (int64_t)a.Hs * ((a.W + G - 1) / G);
    hipLaunchKernelGGL((gp_prepare<PIX, C, S>), dim3((unsigned)((items + GR_THREADS - 1) / GR_THREADS), (unsigned)a.batch), dim3(GR_THREADS), 0, st,
                       (const PIX*)a.image, a.labels, a.exclude, a.H, a.W, a.Hs, a.Ws, a.vec, a.masked, a.max_label, a.P, a.E, a.ctrl);
}

template <typename PIX, int C> static void gp_launch_s(int s, const GpArgs& a, hipStream_t st)
{
    switch (s) {
    case 1: gp_launch<PIX, C, 1>(a, st); break;
    case 2: gp_launch<PIX, C, 2>(a, st); break;
    case 4: gp_launch<PIX, C, 4>(a, st); break;
    default: gp_launch<PIX, C, 8>(a, st); break;
    }
}

template <typename PIX> static void gp_launch_c(int C, int s, const GpArgs& a, hipStream_t st)
{
    switch (C) {
    case 1: gp_launch_s<PIX, 1>(s, a, st); break;
    case 2: gp_launch_s<PIX, 2>(s, a, st); break;
    case 3: gp_launch_s<PIX, 3>(s, a, st); break;
    default: gp_launch_s<PIX, 4>(s, a, st); break;
    }
}

static void gs_launch_c(int C, const int* labels, const int* exclude, const unsigned short* R, int batch, int H, int W, int Hs, int Ws, int shift,
                        int vec, const GsTables& T, hipStream_t st)
{
    const dim3 grid = label_tile_grid(batch, H, W), block(GR_THREADS);
    switch (C) {
    case 1: hipLaunchKernelGGL(gs_sums<1>, grid, block, 0, st, labels, exclude, R, H, W, Hs, Ws, shift, vec, T); break;
    case 2: hipLaunchKernelGGL(gs_sums<2>, grid, block, 0, st, labels, exclude, R, H, W, Hs, Ws, shift, vec, T); break;
    case 3: hipLaunchKernelGGL(gs_sums<3>, grid, block, 0, st, labels, exclude, R, H, W, Hs, Ws, shift, vec, T); break;
    default: hipLaunchKernelGGL(gs_sums<4>, grid, block, 0, st, labels, exclude, R, H, W, Hs, Ws, shift, vec, T); break;
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_granularity(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                         int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, const cs_granularity_params* params,
                         int64_t* geom, int64_t* sums, int64_t* image_sums, uint16_t* planes, int out_kind)
{
    if (!image || !labels || !params || !geom || !sums || !image_sums) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kGrMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kGrMaxChannels);
    if (params->steps < 1) return fail(CS_ERR_INVALID, "cs_granularity_params.steps %d: must be >= 1", (int)params->steps);
    const int s = params->subsample;
    if (s != 1 && s != 2 && s != 4 && s != 8) return fail(CS_ERR_INVALID, "cs_granularity_params.subsample %d: must be 1, 2, 4 or 8", s);
    if (params->masked != 0 && params->masked != 1) return fail(CS_ERR_INVALID, "cs_granularity_params.masked %d: must be 0 or 1", (int)params->masked);
    if (params->reserved != 0) return fail(CS_ERR_INVALID, "cs_granularity_params.reserved must be 0");
    if (params->steps > CS_GRANULARITY_MAX_STEPS)
        return fail(CS_ERR_UNSUPPORTED, "cs_granularity_params.steps %d: at most %d steps", (int)params->steps, CS_GRANULARITY_MAX_STEPS);
    if ((rc = label_cap("max_label", max_label, batch, channels, kGrMaxCells, "the tables", "cells")) || (rc = image_limits(batch, height, width)))
        return rc;
    const int H = height, W = width, C = channels, steps = params->steps, steps1 = steps + 1;
    const int Hs = (H + s - 1) / s, Ws = (W + s - 1) / s, shift = s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : 3;
    const int64_t rows = (int64_t)batch * max_label;
    const size_t HW = (size_t)Hs * Ws, sbytes = (size_t)rows * steps1 * C * sizeof(int64_t),
                 pbytes = (size_t)batch * C * HW * sizeof(uint16_t);    // one working plane per channel and image
    if (sbytes > kGrMaxBytes)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x max_label %d x steps %d x channels %d: the sums table takes %zu bytes, above %zu (split the batch)",
                    (int)batch, (int)max_label, steps, C, sbytes, kGrMaxBytes);
    if (planes && pbytes * steps1 > kGrMaxBytes)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x steps %d x channels %d x %d x %d: the planes stack takes %zu bytes, above %zu (split the batch)",
                    (int)batch, steps, C, Hs, Ws, pbytes * steps1, kGrMaxBytes);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const size_t gbytes = (size_t)rows * 3 * sizeof(int64_t), ibytes = (size_t)batch * steps1 * C * sizeof(int64_t);
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    // P in dq, E in rec, R in key, the tiles' stamps in ttop, the control words in ctrl
    const int tx = (Ws + GR_TW - 1) / GR_TW, ty = (Hs + GR_TH - 1) / GR_TH;
    const size_t tbytes = (size_t)batch * C * tx * ty * sizeof(int);    // the round in which a tile last changed
    if ((rc = S.ctrl.ensure(GC_N * sizeof(int))) || (rc = S.dq.ensure(pbytes)) || (rc = S.rec.ensure(pbytes)) || (rc = S.key.ensure(pbytes)) ||
        (rc = S.ttop.ensure(tbytes)))
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
    if (out_host && (rc = S.stage.ensure(gbytes + sbytes + ibytes))) return rc;      // on their way to the host: geom, sums, image_sums
    char* sg = S.stage.as<char>();
    unsigned long long* d_geom = out_host ? (unsigned long long*)sg : (unsigned long long*)geom;
    unsigned long long* d_sums = out_host ? (unsigned long long*)(sg + gbytes) : (unsigned long long*)sums;
    unsigned long long* d_isums = out_host ? (unsigned long long*)(sg + gbytes + sbytes) : (unsigned long long*)image_sums;
    unsigned short *d_P = S.dq.as<unsigned short>(), *d_E = S.rec.as<unsigned short>(), *d_R = S.key.as<unsigned short>();
    int* d_ctrl = S.ctrl.as<int>();
    constexpr int PA[2][4] = {{4, 8, 4, 16}, {8, 16, 8, 16}};              // what gp_prepare assumes of 4 pixels: PXA
    const int vec_lab = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0;
    const int vec = vec_lab && ((uintptr_t)d_img & (uintptr_t)(PA[esz - 1][C - 1] - 1)) == 0;
    const GpArgs ga{d_img, d_lab, params->masked ? d_ex : nullptr, (int)batch, H, W, Hs, Ws, vec, (int)params->masked, (int)max_label, d_P, d_E,
                    (unsigned int*)d_ctrl};
    const hipMemcpyKind out_copy = out_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const dim3 one(1);
    const dim3 rgrid((unsigned)(tx * C), (unsigned)ty, (unsigned)batch);
    const dim3 egrid((unsigned)(((int64_t)Hs * ((Ws + 3) / 4) + GR_THREADS - 1) / GR_THREADS), (unsigned)batch, (unsigned)C);
    const int cap = (int)std::min<int64_t>((int64_t)HW, 1 << 30);
    bool sums_open = false;                             // a sums pass whose two events have not been read yet
    double sums_ms = 0.0;
    // the sums of step k from plane `src`, with the planes' copy
    auto sums_of = [&](int k, const unsigned short* src) -> int {
        int r;
        if ((r = S.clk_gs.record(0, st))) return r;
        gs_launch_c(C, d_lab, d_ex, src, batch, H, W, Hs, Ws, shift, vec_lab, GsTables{k == 0 ? d_geom : nullptr, d_sums, d_isums, (int)max_label, steps1, k},
                    st);
        HIPCHK(hipGetLastError());
        if ((r = S.clk_gs.record(1, st))) return r;
        sums_open = true;
        if (planes)
            for (int b = 0; b < batch; ++b)
                HIPCHK(hipMemcpyAsync(planes + ((size_t)b * steps1 + k) * C * HW, src + (size_t)b * C * HW, C * HW * sizeof(uint16_t), out_copy, st));
        return CS_OK;
    };
    // after a synchronisation of the stream: the open sums pass has run
    auto sums_read = [&]() -> int {
        if (!sums_open) return CS_OK;
        sums_open = false;
        if (const int r = S.clk_gs.finish()) return r;
        sums_ms += S.clk_gs.ms[0];
        return CS_OK;
    };

    S.gr_rounds = S.gr_reads = 0;
    if ((rc = S.clk_gr.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(d_ctrl, 0, GC_N * sizeof(int), st));
    HIPCHK(hipMemsetAsync(S.ttop.p, 0xff, tbytes, st));  // -1: never
    HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
    HIPCHK(hipMemsetAsync(d_sums, 0, sbytes, st));
    HIPCHK(hipMemsetAsync(d_isums, 0, ibytes, st));
    if (pixel_type == CS_PIX_U8) gp_launch_c<unsigned char>(C, s, ga, st);
    else gp_launch_c<unsigned short>(C, s, ga, st);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_gr.record(1, st))) return rc;
    if ((rc = sums_of(0, d_P))) return rc;              // R_0 = P
    for (int k = 1; k <= steps; ++k) {
        hipLaunchKernelGGL(gr_erode, egrid, dim3(GR_THREADS), 0, st, d_E, d_R, Hs, Ws, (int)((Ws & 3) == 0));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(d_E, d_R, pbytes, hipMemcpyDeviceToDevice, st));      // E_k; R starts from it
        hipLaunchKernelGGL(gr_start, one, one, 0, st, d_ctrl);
        // the rounds, read back once per group, every group twice as long as the one before: most steps settle within the first,
        // and one that has to carry a level across the plane is not read hundreds of times.  The cap ends a step on the device, so
        // this loop ends.
        int group = GR_GROUP;
        for (int active = 1; active; ++S.gr_reads, group = std::min(2 * group, GR_GROUP_MAX)) {
            for (int r = 0; r < group; ++r) {
                hipLaunchKernelGGL(gr_recon, rgrid, dim3(GR_THREADS), 0, st, d_P, d_R, Hs, Ws, tx, d_ctrl, S.ttop.as<int>());
                hipLaunchKernelGGL(gr_advance, one, one, 0, st, d_ctrl, cap);
            }
            HIPCHK(hipGetLastError());
            int w[GC_ACTIVE + 1] = {0};                   // one read: the label check's word rides along with `active`
            HIPCHK(hipMemcpyAsync(w, d_ctrl, sizeof w, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            active = w[GC_ACTIVE];
            if ((rc = sums_read())) return rc;
            if (w[GC_BAD]) {                             // known since gp_prepare: the call ends at its first read, the tables stay unwritten
                S.gr_ms[0] = S.gr_ms[1] = S.gr_ms[2] = 0.0;
                return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
            }
        }
        if ((rc = sums_of(k, d_R))) return rc;
    }
    if ((rc = S.clk_gr.record(2, st))) return rc;
    int words[GC_N] = {0};
    HIPCHK(hipMemcpyAsync(words, d_ctrl, sizeof words, hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(sums, d_sums, sbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(image_sums, d_isums, ibytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the last host synchronisation: the status words, the host tables
    if ((rc = sums_read()) || (rc = S.clk_gr.finish())) return rc;
    S.gr_ms[0] = S.clk_gr.ms[0];
    S.gr_ms[1] = std::max(0.0, S.clk_gr.ms[1] - sums_ms);
    S.gr_ms[2] = sums_ms;
    S.gr_rounds = words[GC_TOTAL];
    if (words[GC_CAPPED])
        return fail(CS_ERR_UNSUPPORTED, "a reconstruction did not settle within %d rounds (the plane is %d x %d)", cap, Hs, Ws);
    return CS_OK;
}

int cs_label_granularity_last_timing(const cs_preproc* p, double* prepare_ms, double* steps_ms, double* sums_ms)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    const SegmentState* S = p->seg;
    if (prepare_ms) *prepare_ms = S ? S->gr_ms[0] : 0.0;
    if (steps_ms) *steps_ms = S ? S->gr_ms[1] : 0.0;
    if (sums_ms) *sums_ms = S ? S->gr_ms[2] : 0.0;
    return CS_OK;
}

int cs_label_granularity_last_rounds(const cs_preproc* p, int32_t* rounds, int32_t* reads)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    const SegmentState* S = p->seg;
    if (rounds) *rounds = S ? S->gr_rounds : 0;
    if (reads) *reads = S ? S->gr_reads : 0;
    return CS_OK;
}
