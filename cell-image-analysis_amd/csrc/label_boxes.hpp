// label_boxes.hpp -- the first pass of the per-object tools that walk an object's bounding box afterwards: tx_boxes of
// cs_label_texture (texture.hip) and sh_moments of cs_label_shape (shape.hip) are the two instances of lb_pass.
//
// The walk of label_tile.hpp over labels and exclude alone: one open run per lane with its count and its extent, merged per wave,
// then per workgroup in a table in LDS keyed by the label; only the distinct labels of a tile reach the global tables, as integer
// atomics.  With MOMENTS the run also carries the nine power sums of its pixels' coordinates up to order 3, relative to the
// tile's origin (r in 0..63, c in 0..255), so that a lane's 64 pixels keep every one of them in 32 bits (64 * 255^3 < 2^31) and
// a tile's 16384 keep the five up to order 2 in 32 bits too (16384 * 255^2 < 2^31); the origin is added once per label and tile,
// by the binomial expansion, when the label leaves for the global table.  A record in LDS is 24 bytes without and 76 with the
// moments, so the table has 1024 or 256 slots: 24 and 19 KB, eight workgroups a CU either way.  A label that finds no room goes
// to the global tables directly.  No floating point; sums and maxima of integers do not depend on the order of arrival.
#pragma once
#include "label_tile.hpp"
#include "stage_host.hpp"

namespace cs {

static constexpr int LB_THREADS = LT_THREADS;
static constexpr int LB_PROBES = 16;
static constexpr int LB_MOMENTS = 10;                   // n, r, c, r^2, rc, c^2, r^3, r^2 c, r c^2, c^3

template <bool MOMENTS> struct LbTable {
    static constexpr int log2 = MOMENTS ? 8 : 10;
    static constexpr int slots = 1 << log2;
};

// An extent travels as four numbers that only grow, so that a cleared table is the empty extent and one maximum merges two:
// kMaxSide - first row, last row + 1, kMaxSide - first column, last column + 1.
struct LbExtent {
    int e[4];
};

// the power sums of a set of pixels without the count, tile coordinates: r, c, r^2, rc, c^2 and r^3, r^2 c, r c^2, c^3
struct LbSums {
    unsigned int s[5];
    unsigned long long t[4];
};

// the ten moments of n pixels in image coordinates from their sums relative to (r0, c0); every term below 2^59
__device__ inline void lb_translate(unsigned long long n, const LbSums& a, unsigned long long r0, unsigned long long c0,
                                    unsigned long long (&m)[LB_MOMENTS])
{
    const unsigned long long sr = a.s[0], sc = a.s[1], srr = a.s[2], src = a.s[3], scc = a.s[4];
    m[0] = n;
    m[1] = sr + n * r0;
    m[2] = sc + n * c0;
    m[3] = srr + 2 * r0 * sr + n * r0 * r0;
    m[4] = src + r0 * sc + c0 * sr + n * r0 * c0;
    m[5] = scc + 2 * c0 * sc + n * c0 * c0;
    m[6] = a.t[0] + 3 * r0 * srr + 3 * r0 * r0 * sr + n * r0 * r0 * r0;
    m[7] = a.t[1] + c0 * srr + 2 * r0 * src + 2 * r0 * c0 * sr + r0 * r0 * sc + n * r0 * r0 * c0;
    m[8] = a.t[2] + r0 * scc + 2 * c0 * src + 2 * r0 * c0 * sc + c0 * c0 * sr + n * r0 * c0 * c0;
    m[9] = a.t[3] + 3 * c0 * scc + 3 * c0 * c0 * sc + n * c0 * c0 * c0;
}

// grid (ceil(W/256), ceil(H/64), B).  labels, exclude (or null): [B][H][W] int.  box: [B][max_label][4], encoded as LbExtent.
// Without MOMENTS count: [B][max_label] and mom is not used; with them mom: [B][max_label][10] and count is not used.  All cleared.
template <bool MOMENTS>
__global__ __launch_bounds__(LB_THREADS) void lb_pass(const int* __restrict__ labels, const int* __restrict__ exclude, int H, int W, int vec,
                                                      int max_label, int* __restrict__ count, int* __restrict__ box,
                                                      unsigned long long* __restrict__ mom, unsigned int* __restrict__ ctrl)
{
    constexpr int LOG2 = LbTable<MOMENTS>::log2, SLOTS = LbTable<MOMENTS>::slots, MS = MOMENTS ? SLOTS : 1;
    __shared__ int key[SLOTS];                          // 0: empty
    __shared__ unsigned int cnt[SLOTS];
    __shared__ int ext[4][SLOTS];
    __shared__ unsigned int low[5][MS];
    __shared__ unsigned long long cub[4][MS];
    for (int s = threadIdx.x; s < SLOTS; s += LB_THREADS) {
        key[s] = 0;
        cnt[s] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ext[j][s] = 0;
        if constexpr (MOMENTS) {
#pragma unroll
            for (int j = 0; j < 5; ++j) low[j][s] = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) cub[j][s] = 0ull;
        }
    }
    __syncthreads();
    const LabelTile tile = label_tile();
    const size_t plane = (size_t)tile.b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    int* crow = MOMENTS ? nullptr : count + (size_t)tile.b * max_label;
    int* brow = box + (size_t)tile.b * max_label * 4;
    unsigned long long* mrow = MOMENTS ? mom + (size_t)tile.b * max_label * LB_MOMENTS : nullptr;
    const bool wide = vec && tile.c_base + 3 < W;
    // label is in 1..max_label; the sums are the tile's
    auto to_global = [&](int label, unsigned int n, const LbExtent& x, const LbSums& a) {
        if constexpr (MOMENTS) {
            unsigned long long m[LB_MOMENTS];
            lb_translate(n, a, (unsigned long long)tile.r0, (unsigned long long)tile.c0, m);
#pragma unroll
            for (int j = 0; j < LB_MOMENTS; ++j) atomicAdd(&mrow[(size_t)(label - 1) * LB_MOMENTS + j], m[j]);
        } else {
            atomicAdd(&crow[label - 1], (int)n);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicMax(&brow[(size_t)(label - 1) * 4 + j], x.e[j]);
    };
    auto flush = [&](int label, unsigned int n, const LbExtent& x, const LbSums& a) {
        const int s = table_claim(key, LOG2, ((unsigned int)label * 0x9E3779B1u) >> (32 - LOG2), label, LB_PROBES);
        if (s >= 0) {
            atomicAdd(&cnt[s], n);
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicMax(&ext[j][s], x.e[j]);
            if constexpr (MOMENTS) {
#pragma unroll
                for (int j = 0; j < 5; ++j) atomicAdd(&low[j][s], a.s[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) atomicAdd(&cub[j][s], a.t[j]);
            }
        } else {                                        // no room: straight to the global tables
            to_global(label, n, x, a);
        }
    };

    unsigned int bad = 0u, n = 0u;
    int cur = 0;
    LbExtent x = {{0, 0, 0, 0}};
    unsigned int q[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};     // the open run's sums; a lane's 64 pixels keep them in 32 bits
    auto sums_of_run = [&]() {
        LbSums a;
#pragma unroll
        for (int j = 0; j < 5; ++j) a.s[j] = q[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) a.t[j] = q[5 + j];
        return a;
    };
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int v[4], e[4] = {0, 0, 0, 0};
        const size_t at = (size_t)r * W + tile.c_base;
        label_load4(ll + at, W - tile.c_base, wide, v);
        if (ee) label_load4(ee + at, W - tile.c_base, wide, e);
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = v[k];
            if (lab == 0) continue;
            if (lab < 0 || lab > max_label) { bad = 1u; continue; }
            if (e[k] != 0) continue;
            if (n != 0u && lab != cur) {
                flush(cur, n, x, sums_of_run());
                n = 0u;
            }
            const int c = tile.c_base + k;
            if (n == 0u) {
                cur = lab;
                x.e[0] = kMaxSide - r;
                x.e[2] = kMaxSide - c;
                x.e[3] = c + 1;
                if constexpr (MOMENTS) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) q[j] = 0u;
                }
            }
            ++n;
            x.e[1] = r + 1;                             // the rows only grow
            x.e[2] = max(x.e[2], kMaxSide - c);
            x.e[3] = max(x.e[3], c + 1);
            if constexpr (MOMENTS) {
                const unsigned int cc = (unsigned int)(4 * tile.lane + k);
                q[0] += rr;
                q[1] += cc;
                q[2] += rr * rr;
                q[3] += rr * cc;
                q[4] += cc * cc;
                q[5] += rr * rr * rr;
                q[6] += rr * rr * cc;
                q[7] += rr * cc * cc;
                q[8] += cc * cc * cc;
            }
        }
    }
    merge_open_runs(n != 0u, cur, tile.lane, [&](int lw, bool mine, bool leader) {
        const unsigned int t = wave_sum(mine ? n : 0u);
        LbExtent m;
#pragma unroll
        for (int j = 0; j < 4; ++j) m.e[j] = wave_max(mine ? x.e[j] : 0);
        LbSums a = {};
        if constexpr (MOMENTS) {                        // a wave's 4096 pixels: the cubes need 64 bits from here on
#pragma unroll
            for (int j = 0; j < 5; ++j) a.s[j] = wave_sum(mine ? q[j] : 0u);
#pragma unroll
            for (int j = 0; j < 4; ++j) a.t[j] = wave_sum(mine ? (unsigned long long)q[5 + j] : 0ull);
        }
        if (leader) flush(lw, t, m, a);
    });
    __syncthreads();
    for (int s = threadIdx.x; s < SLOTS; s += LB_THREADS) {
        const int label = key[s];
        if (label == 0) continue;
        LbExtent m;
#pragma unroll
        for (int j = 0; j < 4; ++j) m.e[j] = ext[j][s];
        LbSums a = {};
        if constexpr (MOMENTS) {
#pragma unroll
            for (int j = 0; j < 5; ++j) a.s[j] = low[j][s];
#pragma unroll
            for (int j = 0; j < 4; ++j) a.t[j] = cub[j][s];
        }
        to_global(label, cnt[s], m, a);
    }
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

}  // namespace cs
