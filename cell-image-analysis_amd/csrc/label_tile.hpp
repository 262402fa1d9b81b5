// label_tile.hpp -- the walk over an int32 label stack [B][H][W] that ex_label_pass (extract.hip), lm_count (match.hip),
// li_pass (intensity.hip), lq_count / lq_scatter (quantile.hip), lb_pass (label_boxes.hpp: texture.hip, shape.hip) , lc_moments / lc_thresholded (colocalize.hip), lr_bins (radial.hip) and gs_sums (granularity.hip) share: the tile, the load
// of a lane's four labels, the wave reductions, the closing merge of the lanes' open runs and the claim of a slot in an
// open-addressing table.  nb_scan (neighbors.hip) has a tile of its own, with a halo, and takes the claim and the reductions; lr_rows (radial.hip) works on row strips and takes the closing merge and the reductions.  Each kernel keeps its own row loop, its unroll and its run bookkeeping: what they do per pixel
// differs, and so does what they hold in registers.
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

// The tile: 256 threads; a lane owns 4 columns x 16 rows, a wave 256 columns x 16 rows, a workgroup 256 columns x 64 rows.
// Label rows are long runs of one value, so a lane that walks its 4 x 16 pixels row by row changes its run rarely.
static constexpr int LT_THREADS = 256;
static constexpr int LT_WAVES = LT_THREADS / 64;
static constexpr int LT_ROWS = 16;                      // rows per wave
static constexpr int LT_COLS = 4 * 64;                  // columns per wave (4 per lane)
static constexpr int LT_TILE_ROWS = LT_WAVES * LT_ROWS; // rows per workgroup

// grid (ceil(W/256), ceil(H/64), B)
inline dim3 label_tile_grid(int batch, int H, int W)
{
    return dim3((unsigned)((W + LT_COLS - 1) / LT_COLS), (unsigned)((H + LT_TILE_ROWS - 1) / LT_TILE_ROWS), (unsigned)batch);
}

struct LabelTile {
    int lane, wave, b;                                  // b: the image
    int r0, c0;                                         // the tile's origin
    int r_base, c_base;                                 // the first of the thread's LT_ROWS rows and of its 4 columns
};

__device__ inline LabelTile label_tile()
{
    LabelTile t;
    t.lane = threadIdx.x & 63;
    t.wave = threadIdx.x >> 6;
    t.b = blockIdx.z;
    t.r0 = blockIdx.y * LT_TILE_ROWS;
    t.c0 = blockIdx.x * LT_COLS;
    t.r_base = t.r0 + t.wave * LT_ROWS;
    t.c_base = t.c0 + 4 * t.lane;
    return t;
}

// A lane's four labels of one row, `at` pointing at the first: one 16-byte load where `wide` holds (the caller knows that the
// width is a multiple of 4, the plane 16-byte aligned and all four columns inside), else the first n of them, 0 for the rest.
__device__ inline void label_load4(const int* at, int n, bool wide, int (&x)[4])
{
    if (wide) {
        const int4 q = *(const int4*)at;
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < n ? at[k] : 0;
    }
}

// ---- wave reductions: every lane gets the result ------------------------------------------------------------------------------
template <typename T, typename Op> __device__ inline T wave_reduce(T v, Op op)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = op(v, (T)__shfl_xor(v, m));
    return v;
}
template <typename T> __device__ inline T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <typename T> __device__ inline T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return min(a, b); }); }
template <typename T> __device__ inline T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return max(a, b); }); }

// The closing merge of a wave: every lane may hold one open run under a key.  Until no run is open, the first lane that has one
// leads; body(key, mine, leader) runs on every lane with the leader's key, whether this lane's open run has that key, and
// whether this lane is the leader, so that the body can reduce over the wave and let the leader write once per distinct key;
// then those runs are closed.  Called by whole waves.
template <typename K, typename F> __device__ inline void merge_open_runs(bool open, K key, int lane, F body)
{
    for (;;) {
        const unsigned long long m = __ballot(open);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const K kw = __shfl(key, leader);
        const bool mine = open && key == kw;
        body(kw, mine, lane == leader);
        if (mine) open = false;
    }
}

// The slot of `key` in an open-addressing table of 2^log2 keys (0: an empty slot), claimed by atomicCAS if the key is new:
// linear probing from the caller's hash h, at most `probes` slots.  -1: no room within them.
template <typename K> __device__ inline int table_claim(K* keys, int log2, unsigned int h, K key, int probes)
{
    const unsigned int mask = (1u << log2) - 1u;
    for (int i = 0; i < probes; ++i) {
        const K old = atomicCAS(&keys[h], (K)0, key);
        if (old == (K)0 || old == key) return (int)h;
        h = (h + 1) & mask;
    }
    return -1;
}

}  // namespace cs
