// spots.hip -- local maxima of a difference-of-Gaussians response in one channel of an image stack, as a sorted list and as
// per-object records, on gfx950 (include/cellscreen.h, cs_spot_detect and cs_spot_fill; the rule: DESIGN 3zi, restated in
// tests/spots_reference.py).
//
// R = (A_a - A_b + 2^23) >> 24 with A_t(i, j) = sum_k w_t[|k|] sum_l w_t[|l|] x(fold(i + k, H), fold(j + l, W)), the separable
// 48-bit sums of cs_segment_smooth under two tables (w_a of radius 0: the identity, A_a = x * 2^32).  A pixel is a spot iff
// R >= T_b and its key (R, -raster index) is the greatest of the (2m + 1)^2 window clipped to the image; keys are distinct, so
// "the greatest" needs no tie rule beyond the key itself.
//   sd_rows    sm_rows' staging (segment.hip): a row segment with the halo of the wider table goes into LDS once as 16-bit
//              values and yields both tables' row sums from the same two sliding register windows, so the image is read once for
//              both sigmas.  Both sums are uint32 and exact (65535 * 65536 < 2^32).  Lanes are 3 words apart: an odd stride.
//   sd_cols    sm_cols' walk: [rows + 2 r][64 columns] of each table's row sums in LDS (dynamic, at most 100,352 bytes at both
//              radii 64), lanes across the columns, a thread produces 4 adjacent rows; the 48-bit sum as two 32-bit halves that
//              meet once.  Writes R, int32; the difference is shifted as a signed 64-bit value, which floors.
//   sd_peaks   a 64 x 32 tile of 64-bit keys with a halo of m in LDS.  Only a pixel at or above the threshold is a candidate, and a
//              candidate walks its window row by row until it meets a greater key: in noise that is after a few reads, and a
//              wave-row without a candidate left (most of them, at a threshold of a few sigmas) leaves the walk at once.  A
//              separable running maximum would cost every pixel 2 (2m + 1) reads, a second plane in LDS and a barrier; the walk
//              costs (2m + 1)^2 reads only where a lane of the wave is a spot, or sits on a plateau.  A wave owns a row segment of
//              64 columns, so one ballot is the segment's spots: one 64-bit word per row and tile column.
//   sd_count, sd_scan, sd_place    the list's order without a sort and without an arrival order: the spots of every image row
//              are counted from the ballot words (a thread per row), scanned over the rows of the batch (a workgroup per 256
//              rows, their sums scanned by one workgroup), and placed by the row's thread in column order from the row's offset.
//              The same thread adds the spot to its object's record, through a table in LDS keyed by the object before 64-bit
//              integer atomics reach the dense table, and counts the image's spots and those on label 0.
//   sd_geom    area, sum r, sum c per object on the tile of label_tile.hpp: cs_label_intensity's geom.  li_pass itself computes
//              the channel sums in the same registers and lives in intensity.hip's translation unit; this is its walk without
//              the pixels.  It also range-checks every label of the stack.
// No floating point and no float atomics: every output is a function of the inputs alone, bit-identical run to run.  A label is
// range-checked before it is a key or an index, and a list position before it is written.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int SD_THREADS = 256;
static constexpr int SD_MAX_R = 64;                     // radius of a table
static constexpr int SD_MAX_M = 8;                      // half-width of the peak window
static constexpr int SD_ROW_E = 6;
static constexpr int SD_ROW_SEG = 768;                  // pixels of a row segment: 2 * 64 * SD_ROW_E
static constexpr int SD_ROW_LINES = SD_THREADS / 64;
static constexpr int SD_ROW_LEN = SD_ROW_SEG + 2 * SD_MAX_R + SD_ROW_E;
static constexpr int SD_COL_W = 64, SD_COL_WAVES = SD_THREADS / 64, SD_COL_E = 4;
static constexpr int SD_COL_TR = 64;                    // rows of a column tile
static constexpr int SD_PK_W = 64;                      // the peak pass's tile
static constexpr int SD_PK_H = 32;
static constexpr int SD_PK_LW = SD_PK_W + 2 * SD_MAX_M, SD_PK_LH = SD_PK_H + 2 * SD_MAX_M;
static constexpr int SD_CHUNK = SD_THREADS;             // image rows per workgroup of sd_count / sd_place
static constexpr int SD_SLOTS_LOG2 = 9, SD_LDS_PROBES = 16;
static constexpr int SD_REC = 6, SD_SPOT = 8;
static constexpr int64_t kSdMaxRows = 1 << 22;          // batch * max_label
static constexpr int64_t kSdMaxSpots = 1 << 22;         // per call
static constexpr size_t kSdMaxScratch = (size_t)1 << 30;   // the row sums and the response: 12 bytes per pixel
static_assert(SD_ROW_SEG == 2 * 64 * SD_ROW_E, "a lane makes two groups of SD_ROW_E outputs");
static_assert(SD_PK_W == 64, "a wave's ballot is a row segment");

struct SdWeights {
    int ra, rb;
    unsigned int wa[SD_MAX_R + 1], wb[SD_MAX_R + 1];
};

// index i of a line of n reflected about the edges: ... 2 1 0 | 0 1 2 ... n-1 | n-1 n-2 ..., period 2n; any i
__device__ inline int sd_fold(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// ---- the response --------------------------------------------------------------------------------------------------------------
// grid (ceil(W / SD_ROW_SEG), ceil(H / SD_ROW_LINES), B).  in: pixel (b, y, x) at in[b * in_img + (y * W + x) * in_pix].
// Ta, Tb: [B][H][W] uint32.
template <typename PIX>
__global__ __launch_bounds__(SD_THREADS) void sd_rows(const PIX* __restrict__ in, size_t in_img, int in_pix, int H, int W, const SdWeights wt,
                                                      unsigned int* __restrict__ Ta, unsigned int* __restrict__ Tb)
{
    __shared__ unsigned short sm[SD_ROW_LINES * SD_ROW_LEN];
    constexpr int E = SD_ROW_E;
    const int tp = threadIdx.x & 63, line = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SD_ROW_SEG, y = blockIdx.y * SD_ROW_LINES + line, b = blockIdx.z;
    const int r = max(wt.ra, wt.rb), r_both = min(wt.ra, wt.rb), seg = min(SD_ROW_SEG, W - x0), len = seg + 2 * r;
    unsigned short* s = sm + line * SD_ROW_LEN;
    const PIX* src = in + (size_t)b * in_img + (size_t)(y < H ? y : 0) * W * in_pix;
    for (int pos = tp; pos < len + E; pos += 64)
        s[pos] = y < H && pos < len ? (unsigned short)src[(size_t)sd_fold(x0 - r + pos, W) * in_pix] : (unsigned short)0;
    __syncthreads();
    if (y >= H) return;
    const size_t row = ((size_t)b * H + y) * W + x0;
    const bool a_wider = wt.ra > wt.rb;
    for (int j = tp * E; j < seg; j += 64 * E) {
        const unsigned short* c = s + r + j;            // c[d]: the pixel x0 + j + d
        unsigned int lo[E], hi[E], aa[E], ab[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            lo[e] = hi[e] = c[e];
            aa[e] = wt.wa[0] * lo[e];
            ab[e] = wt.wb[0] * lo[e];
        }
        for (int k = 1; k <= r; ++k) {                  // lo[e] = c[e - k], hi[e] = c[e + k]
#pragma unroll
            for (int e = E - 1; e > 0; --e) lo[e] = lo[e - 1];
#pragma unroll
            for (int e = 0; e < E - 1; ++e) hi[e] = hi[e + 1];
            lo[0] = c[-k];
            hi[E - 1] = c[E - 1 + k];
            if (k <= r_both) {                          // uniform
                const unsigned int wa = wt.wa[k], wb = wt.wb[k];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    aa[e] += wa * (lo[e] + hi[e]);
                    ab[e] += wb * (lo[e] + hi[e]);
                }
            } else if (a_wider) {
                const unsigned int wa = wt.wa[k];
#pragma unroll
                for (int e = 0; e < E; ++e) aa[e] += wa * (lo[e] + hi[e]);
            } else {
                const unsigned int wb = wt.wb[k];
#pragma unroll
                for (int e = 0; e < E; ++e) ab[e] += wb * (lo[e] + hi[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (j + e < seg) {
                Ta[row + j + e] = aa[e];
                Tb[row + j + e] = ab[e];
            }
    }
}

// the 48-bit column sums of E adjacent rows under one table; c[d * 64]: the row sum of row y0 + j + d of the thread's column
template <bool COARSE> __device__ inline void sd_col_sum(const unsigned int* c, const SdWeights& wt, unsigned long long (&A)[SD_COL_E])
{
    constexpr int E = SD_COL_E;
    const int r = COARSE ? wt.rb : wt.ra;
    const unsigned int w0 = COARSE ? wt.wb[0] : wt.wa[0];
    unsigned int lh[E], ll[E], hh[E], hl[E], ah[E], al[E];      // the two windows and the sums, high and low halves
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned int t = c[e * SD_COL_W];
        lh[e] = hh[e] = t >> 16;
        ll[e] = hl[e] = t & 0xffffu;
        ah[e] = w0 * lh[e];
        al[e] = w0 * ll[e];
    }
    for (int k = 1; k <= r; ++k) {
        const unsigned int w = COARSE ? wt.wb[k] : wt.wa[k];
        const unsigned int a = c[-k * SD_COL_W], z = c[(E - 1 + k) * SD_COL_W];
#pragma unroll
        for (int e = E - 1; e > 0; --e) {
            lh[e] = lh[e - 1];
            ll[e] = ll[e - 1];
        }
#pragma unroll
        for (int e = 0; e < E - 1; ++e) {
            hh[e] = hh[e + 1];
            hl[e] = hl[e + 1];
        }
        lh[0] = a >> 16;
        ll[0] = a & 0xffffu;
        hh[E - 1] = z >> 16;
        hl[E - 1] = z & 0xffffu;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            ah[e] += w * (lh[e] + hh[e]);
            al[e] += w * (ll[e] + hl[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) A[e] = ((unsigned long long)ah[e] << 16) + al[e];
}

// grid (ceil(W / SD_COL_W), ceil(H / SD_COL_TR), B); dynamic LDS sd_cols_lds(H, ra, rb) bytes.  R: [B][H][W] int32.
__global__ __launch_bounds__(SD_THREADS) void sd_cols(const unsigned int* __restrict__ Ta, const unsigned int* __restrict__ Tb, int H, int W,
                                                      const SdWeights wt, int* __restrict__ R)
{
    extern __shared__ unsigned int sd_tile[];
    constexpr int E = SD_COL_E;
    const int col = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * SD_COL_W + col, y0 = blockIdx.y * SD_COL_TR;
    const int ra = wt.ra, rb = wt.rb, rows = min(SD_COL_TR, H - y0), lena = rows + 2 * ra, lenb = rows + 2 * rb;
    const size_t base = (size_t)blockIdx.z * H * W;
    unsigned int* ta = sd_tile;
    unsigned int* tb = sd_tile + (size_t)(lena + E) * SD_COL_W;
    for (int pos = wv; pos < lena + E; pos += SD_COL_WAVES)
        ta[pos * SD_COL_W + col] = x < W && pos < lena ? Ta[base + (size_t)sd_fold(y0 - ra + pos, H) * W + x] : 0u;
    for (int pos = wv; pos < lenb + E; pos += SD_COL_WAVES)
        tb[pos * SD_COL_W + col] = x < W && pos < lenb ? Tb[base + (size_t)sd_fold(y0 - rb + pos, H) * W + x] : 0u;
    __syncthreads();
    if (x >= W) return;
    for (int j = wv * E; j < rows; j += SD_COL_WAVES * E) {
        unsigned long long Aa[E], Ab[E];
        sd_col_sum<false>(ta + (ra + j) * SD_COL_W + col, wt, Aa);
        sd_col_sum<true>(tb + (rb + j) * SD_COL_W + col, wt, Ab);
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (j + e < rows)                           // |A_a - A_b| < 2^48: the signed shift floors
                R[base + (size_t)(y0 + j + e) * W + x] = (int)(((long long)Aa[e] - (long long)Ab[e] + (1ll << 23)) >> 24);
    }
}

static size_t sd_cols_lds(int H, int ra, int rb)
{
    const int rows = std::min(SD_COL_TR, H);
    return (size_t)(2 * rows + 2 * ra + 2 * rb + 2 * SD_COL_E) * SD_COL_W * sizeof(unsigned int);
}

// ---- the peaks -----------------------------------------------------------------------------------------------------------------
// the key of pixel idx with response v, |v| < 2^24: greater response first, then the smaller raster index; never 0
__device__ inline unsigned long long sd_key(int v, unsigned int idx)
{
    return ((unsigned long long)(unsigned int)(v + (1 << 24)) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

// grid (ceil(W / SD_PK_W), ceil(H / SD_PK_H), B).  R: [B][H][W]; thr: [B]; masks: [B][H][gridDim.x] 64-bit words, bit k of word
// (b, y, i): pixel (y, 64 i + k) of image b is a spot.
__global__ __launch_bounds__(SD_THREADS) void sd_peaks(const int* __restrict__ R, int H, int W, int m, const int* __restrict__ thr,
                                                       unsigned long long* __restrict__ masks)
{
    __shared__ unsigned long long K[SD_PK_LH * SD_PK_LW];       // the keys of the tile and its halo; 0 outside the image
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.z;
    const int x0 = blockIdx.x * SD_PK_W, y0 = blockIdx.y * SD_PK_H;
    const int tw = SD_PK_W + 2 * m, th = SD_PK_H + 2 * m, side = 2 * m + 1;
    const int* Rb = R + (size_t)b * H * W;
    for (int ly = wv; ly < th; ly += SD_THREADS / 64) {
        const int gy = y0 - m + ly;
        for (int lx = lane; lx < tw; lx += 64) {
            const int gx = x0 - m + lx;
            unsigned long long key = 0ull;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const unsigned int idx = (unsigned int)gy * (unsigned int)W + (unsigned int)gx;
                key = sd_key(Rb[idx], idx);
            }
            K[ly * SD_PK_LW + lx] = key;
        }
    }
    __syncthreads();
    const int t = thr[b];
    for (int ry = wv; ry < SD_PK_H; ry += SD_THREADS / 64) {    // uniform over the wave
        const int gy = y0 + ry, gx = x0 + lane;
        if (gy >= H) break;
        const unsigned long long* k = K + ry * SD_PK_LW + lane;  // the corner of the pixel's window
        const unsigned long long own = k[m * SD_PK_LW + m];
        const int resp = (int)(unsigned int)(own >> 32) - (1 << 24);
        bool alive = gx < W && resp >= t;               // a candidate until a greater key shows up in its window
        for (int dy = 0; dy < side && __ballot(alive) != 0ull; ++dy)
            for (int dx = 0; dx < side; ++dx)
                if (alive && k[dy * SD_PK_LW + dx] > own) alive = false;
        const unsigned long long word = __ballot(alive);
        if (lane == 0) masks[((size_t)b * H + gy) * gridDim.x + blockIdx.x] = word;
    }
}

// ---- the list ------------------------------------------------------------------------------------------------------------------
// the exclusive prefix of v over the workgroup's threads and, in total, the workgroup's sum; scratch: SD_THREADS / 64 + 1 words
__device__ inline unsigned int sd_block_scan(unsigned int v, unsigned int* scratch, unsigned int& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned int inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned int u = __shfl_up(inc, s);
        if (lane >= s) inc += u;
    }
    __syncthreads();                                    // scratch may still be read from an earlier call
    if (lane == 63) scratch[wv] = inc;
    __syncthreads();
    unsigned int before = 0u, all = 0u;
    for (int w = 0; w < SD_THREADS / 64; ++w) {
        const unsigned int s = scratch[w];
        if (w < wv) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}

// grid ceil(rows / SD_CHUNK).  masks: [rows][nwx]; row_n: [rows]; chunk_n: [gridDim.x]
__global__ __launch_bounds__(SD_THREADS) void sd_count(const unsigned long long* __restrict__ masks, int64_t rows, int nwx,
                                                       unsigned int* __restrict__ row_n, unsigned int* __restrict__ chunk_n)
{
    __shared__ unsigned int scratch[SD_THREADS / 64 + 1];
    const int64_t row = (int64_t)blockIdx.x * SD_CHUNK + threadIdx.x;
    unsigned int n = 0u;
    if (row < rows) {
        const unsigned long long* w = masks + (size_t)row * nwx;
        for (int i = 0; i < nwx; ++i) n += (unsigned int)__popcll(w[i]);
        row_n[row] = n;
    }
    unsigned int total;
    (void)sd_block_scan(n, scratch, total);
    if (threadIdx.x == 0) chunk_n[blockIdx.x] = total;
}

// one workgroup: chunk_n[n] becomes its exclusive prefix, *total the sum
__global__ __launch_bounds__(SD_THREADS) void sd_scan(unsigned int* __restrict__ chunk_n, int64_t n, unsigned int* __restrict__ total)
{
    __shared__ unsigned int scratch[SD_THREADS / 64 + 1];
    unsigned int carry = 0u;
    for (int64_t base = 0; base < n; base += SD_THREADS) {
        const int64_t i = base + threadIdx.x;
        const unsigned int v = i < n ? chunk_n[i] : 0u;
        unsigned int all;
        const unsigned int before = sd_block_scan(v, scratch, all);
        if (i < n) chunk_n[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

struct SdLds {
    int key[1 << SD_SLOTS_LOG2];                        // row of the dense table + 1; 0: empty
    unsigned long long s[SD_REC][1 << SD_SLOTS_LOG2];
};

// row: b * max_label + label - 1; o: n, sum R, sum R^2, max R, sum r, sum c
__device__ inline void sd_global(unsigned long long* __restrict__ table, int row, const unsigned long long (&o)[SD_REC])
{
    unsigned long long* t = table + (size_t)row * SD_REC;
#pragma unroll
    for (int j = 0; j < SD_REC; ++j) {
        if (j == 3) atomicMax(&t[j], o[j]);
        else atomicAdd(&t[j], o[j]);
    }
}

struct SdPlace {
    const unsigned long long* masks;                    // [rows][nwx]
    const unsigned int* row_n;                          // [rows]
    const unsigned int* chunk_off;                      // [chunks]
    const int* R;                                       // [B][H][W]
    const int* labels;                                  // [B][H][W] or null
    const int* exclude;                                 // [B][H][W] or null
    int* list;                                          // [capacity][SD_SPOT]
    long long* offsets;                                 // [B + 1]
    unsigned long long* counts;                         // [B][2]
    unsigned long long* table;                          // [B][max_label][SD_REC] or null
    int64_t rows, capacity;
    int H, W, nwx, max_label;
};

// grid ceil(rows / SD_CHUNK): sd_count's.  A thread places the spots of its image row in column order.
__global__ __launch_bounds__(SD_THREADS) void sd_place(const SdPlace P)
{
    __shared__ unsigned int scratch[SD_THREADS / 64 + 1];
    __shared__ SdLds L;
    for (int s = threadIdx.x; s < (1 << SD_SLOTS_LOG2); s += SD_THREADS) {
        L.key[s] = 0;
#pragma unroll
        for (int j = 0; j < SD_REC; ++j) L.s[j][s] = 0ull;
    }
    const int64_t row = (int64_t)blockIdx.x * SD_CHUNK + threadIdx.x;
    const bool live = row < P.rows;
    const unsigned int n = live ? P.row_n[row] : 0u;
    unsigned int all;
    int64_t pos = (int64_t)P.chunk_off[blockIdx.x] + sd_block_scan(n, scratch, all);       // its barriers order the clearing too
    if (live) {
        const int H = P.H, W = P.W;
        const int b = (int)(row / H), r = (int)(row - (int64_t)b * H);
        if (r == 0) P.offsets[b] = pos;
        if (row == P.rows - 1) P.offsets[b + 1] = pos + n;
        const size_t plane = (size_t)b * H * W;
        const int* Rb = P.R + plane;
        const unsigned long long* words = P.masks + (size_t)row * P.nwx;
        unsigned int n0 = 0u;
        for (int i = 0; i < P.nwx && n != 0u; ++i) {
            unsigned long long word = words[i];
            while (word != 0ull) {
                const int c = 64 * i + __ffsll((long long)word) - 1;
                word &= word - 1ull;
                const size_t at = (size_t)r * W + c;
                int label = 0;
                if (P.labels) {
                    label = P.labels[plane + at];
                    if (label < 0 || label > P.max_label) label = 0;           // sd_geom reports it; never an index here
                    else if (P.exclude && P.exclude[plane + at] != 0) label = 0;
                }
                const int v = Rb[at];
                if (pos < P.capacity) {
                    int4 head, tail;
                    head.x = r; head.y = c; head.z = label; head.w = v;
                    tail.x = r > 0 ? Rb[at - W] : INT32_MIN;
                    tail.y = r < H - 1 ? Rb[at + W] : INT32_MIN;
                    tail.z = c > 0 ? Rb[at - 1] : INT32_MIN;
                    tail.w = c < W - 1 ? Rb[at + 1] : INT32_MIN;
                    int4* o = (int4*)(P.list + (size_t)pos * SD_SPOT);
                    o[0] = head;
                    o[1] = tail;
                }
                ++pos;
                if (label == 0) {
                    ++n0;
                } else {                                // v >= T_b >= 1
                    const int trow = b * P.max_label + (label - 1);
                    const unsigned long long o[SD_REC] = {1ull, (unsigned long long)v, (unsigned long long)v * (unsigned long long)v,
                                                          (unsigned long long)v, (unsigned long long)r, (unsigned long long)c};
                    const int h = table_claim(L.key, SD_SLOTS_LOG2, ((unsigned int)(trow + 1) * 0x9E3779B1u) >> (32 - SD_SLOTS_LOG2),
                                              trow + 1, SD_LDS_PROBES);
                    if (h < 0) {
                        sd_global(P.table, trow, o);    // no room: straight to the dense table
                    } else {
#pragma unroll
                        for (int j = 0; j < SD_REC; ++j) {
                            if (j == 3) atomicMax(&L.s[j][h], o[j]);
                            else atomicAdd(&L.s[j][h], o[j]);
                        }
                    }
                }
            }
        }
        if (n != 0u) {
            atomicAdd(&P.counts[2 * b], (unsigned long long)n);
            if (n0 != 0u) atomicAdd(&P.counts[2 * b + 1], (unsigned long long)n0);
        }
    }
    if (!P.table) return;                               // uniform
    __syncthreads();
    for (int s = threadIdx.x; s < (1 << SD_SLOTS_LOG2); s += SD_THREADS) {
        const int key = L.key[s];
        if (key == 0) continue;
        unsigned long long o[SD_REC];
#pragma unroll
        for (int j = 0; j < SD_REC; ++j) o[j] = L.s[j][s];
        sd_global(P.table, key - 1, o);
    }
}

// ---- the objects' geometry -----------------------------------------------------------------------------------------------------
struct SgLds {
    int key[1 << SD_SLOTS_LOG2];                        // the label; 0: empty
    unsigned long long s[3][1 << SD_SLOTS_LOG2];
};

__device__ inline void sg_insert(SgLds& L, unsigned long long* __restrict__ geom, int max_label, int b, int label, const unsigned long long (&o)[3])
{
    const int h = table_claim(L.key, SD_SLOTS_LOG2, ((unsigned int)label * 0x9E3779B1u) >> (32 - SD_SLOTS_LOG2), label, SD_LDS_PROBES);
    if (h < 0) {
        unsigned long long* g = geom + ((size_t)b * max_label + (label - 1)) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicAdd(&g[j], o[j]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicAdd(&L.s[j][h], o[j]);
}

// grid label_tile_grid.  labels, exclude (or null): [B][H][W] int; geom: [B][max_label][3]: area, sum r, sum c.  vec: the width
// is a multiple of 4 and both planes are 16-byte aligned.  *ctrl = 1 where a label is negative or above max_label.
__global__ __launch_bounds__(LT_THREADS) void sd_geom(const int* __restrict__ labels, const int* __restrict__ exclude, int H, int W, int vec,
                                                      unsigned long long* __restrict__ geom, int max_label, unsigned int* __restrict__ ctrl)
{
    __shared__ SgLds L;
    for (int s = threadIdx.x; s < (1 << SD_SLOTS_LOG2); s += LT_THREADS) {
        L.key[s] = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) L.s[j][s] = 0ull;
    }
    __syncthreads();
    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const bool wide = vec && c_base + 3 < W;
    unsigned int bad = 0u;
    int cur = 0;                                        // the open run's label; n == 0: none
    unsigned int n = 0u, sr = 0u, sc = 0u;              // tile coordinates, at most 64 pixels
    auto rec = [&](unsigned long long (&o)[3]) {
        o[0] = n;
        o[1] = sr + (unsigned long long)n * (unsigned int)tile.r0;
        o[2] = sc + (unsigned long long)n * (unsigned int)tile.c0;
    };
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        const size_t at = (size_t)r * W + c_base;
        const int n_in = min(4, W - c_base);            // <= 0: the lane is off the image
        label_load4(ll + at, n_in, wide, x);
        if (ee) label_load4(ee + at, n_in, wide, e);
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab == 0) continue;
            if (lab < 0 || lab > max_label) { bad = 1u; continue; }
            if (e[k] != 0) continue;
            if (n != 0u && lab != cur) {
                unsigned long long o[3];
                rec(o);
                sg_insert(L, geom, max_label, b, cur, o);
                n = sr = sc = 0u;
            }
            cur = lab;
            ++n;
            sr += rr;
            sc += (unsigned int)(4 * lane + k);
        }
    }
    unsigned long long mine[3];
    rec(mine);
    merge_open_runs(n != 0u, cur, lane, [&](int label, bool is_mine, bool leader) {
        unsigned long long o[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = wave_sum(is_mine ? mine[j] : 0ull);
        if (leader) sg_insert(L, geom, max_label, b, label, o);
    });
    __syncthreads();
    for (int s = threadIdx.x; s < (1 << SD_SLOTS_LOG2); s += LT_THREADS) {
        const int label = L.key[s];
        if (label == 0) continue;
        unsigned long long* g = geom + ((size_t)b * max_label + (label - 1)) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicAdd(&g[j], L.s[j][s]);
    }
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

// the table rules of cs_spot_params; wt receives the tables in force
static int spot_check(const cs_spot_params& sp, int32_t channels, SdWeights& wt)
{
    if (sp.channel < 0 || sp.channel >= channels) return fail(CS_ERR_INVALID, "channel %d outside 0..%d", (int)sp.channel, (int)channels - 1);
    if (sp.reserved != 0) return fail(CS_ERR_INVALID, "cs_spot_params.reserved must be 0");
    if (sp.radius_a < 0 || sp.radius_a > SD_MAX_R) return fail(CS_ERR_INVALID, "radius_a %d outside 0..%d", (int)sp.radius_a, SD_MAX_R);
    if (sp.radius_b < 1 || sp.radius_b > SD_MAX_R) return fail(CS_ERR_INVALID, "radius_b %d outside 1..%d", (int)sp.radius_b, SD_MAX_R);
    for (int t = 0; t < 2; ++t) {
        const int32_t* w = t ? sp.weights_b : sp.weights_a;
        const int radius = t ? sp.radius_b : sp.radius_a;
        const char* name = t ? "weights_b" : "weights_a";
        long long sum = 0;
        for (int k = 0; k <= SD_MAX_R; ++k) {
            if (w[k] < 0) return fail(CS_ERR_INVALID, "%s[%d] = %d: negative", name, k, (int)w[k]);
            if (k > radius && w[k] != 0) return fail(CS_ERR_INVALID, "%s[%d] = %d beyond its radius %d", name, k, (int)w[k], radius);
            sum += k ? 2ll * w[k] : (long long)w[k];
            (t ? wt.wb : wt.wa)[k] = (unsigned int)w[k];
        }
        if (w[0] < 1) return fail(CS_ERR_INVALID, "%s[0] = %d: the centre tap must be at least 1", name, (int)w[0]);
        if (sum != 65536) return fail(CS_ERR_INVALID, "%s[0] + 2 * sum(%s[1..%d]) = %lld, not 65536", name, name, radius, sum);
    }
    if (sp.radius_a == sp.radius_b && memcmp(sp.weights_a, sp.weights_b, sizeof sp.weights_a) == 0)
        return fail(CS_ERR_INVALID, "weights_a and weights_b are equal: the response would be 0 everywhere");
    if (sp.min_distance < 1 || sp.min_distance > SD_MAX_M)
        return fail(CS_ERR_INVALID, "min_distance %d outside 1..%d", (int)sp.min_distance, SD_MAX_M);
    wt.ra = sp.radius_a;
    wt.rb = sp.radius_b;
    return CS_OK;
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_spot_detect(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                   int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, const cs_spot_params* params,
                   const int32_t* thresholds, int64_t* counts, int64_t* geom, int64_t* spots, int32_t* response, int out_kind, int64_t* n_spots)
{
    if (!image || !params || !thresholds || !counts || !n_spots) return fail(CS_ERR_INVALID, "NULL argument");
    if (labels && (!geom || !spots)) return fail(CS_ERR_INVALID, "geom or spots is NULL with labels");
    if (!labels && exclude) return fail(CS_ERR_INVALID, "exclude without labels");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (labels && max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    SdWeights wt;
    if ((rc = spot_check(*params, channels, wt))) return rc;
    for (int b = 0; b < batch; ++b)
        if (thresholds[b] < 1) return fail(CS_ERR_INVALID, "thresholds[%d] = %d: must be >= 1 (1/256 counts)", b, (int)thresholds[b]);
    if ((labels && (rc = label_cap("max_label", max_label, batch, 0, kSdMaxRows, "the tables", "rows"))) || (rc = image_limits(batch, height, width)))
        return rc;
    const int H = height, W = width, C = channels, m = params->min_distance;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    if (npx * 12 >= kSdMaxScratch)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x %d x %d: the response scratch (12 bytes per pixel) is capped below %zu bytes per call",
                    (int)batch, H, W, kSdMaxScratch);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    S.sp_n = -1;                                        // until this call has succeeded
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;
    const int nwx = (W + SD_PK_W - 1) / SD_PK_W;
    const int64_t rows = (int64_t)batch * H, chunks = (rows + SD_CHUNK - 1) / SD_CHUNK;
    // no two spots lie within m of each other: a bound on the list
    const int64_t capacity = std::min<int64_t>(kSdMaxSpots, (int64_t)batch * ((H + m) / (m + 1)) * ((W + m) / (m + 1)));
    const int64_t trows = labels ? (int64_t)batch * max_label : 0;
    const size_t cbytes = (size_t)batch * 2 * sizeof(int64_t), gbytes = (size_t)trows * 3 * sizeof(int64_t),
                 sbytes = (size_t)trows * SD_REC * sizeof(int64_t), rbytes = npx * sizeof(int);

    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rc = S.thr.ensure((size_t)batch * sizeof(int))) || (rc = S.sm_t.ensure(npx * 2 * sizeof(unsigned int))) ||
        (rc = S.mask.ensure((size_t)rows * nwx * sizeof(unsigned long long))) || (rc = S.counts.ensure((size_t)rows * sizeof(unsigned int))) ||
        (rc = S.chunks.ensure((size_t)chunks * sizeof(unsigned int))) || (rc = S.sp_list.ensure((size_t)capacity * SD_SPOT * sizeof(int))) ||
        (rc = S.sp_off.ensure((size_t)(batch + 1) * sizeof(int64_t))))
        return rc;
    const bool r_direct = response && !out_host;        // the response straight into the caller's plane
    if (!r_direct && (rc = S.dq.ensure(rbytes))) return rc;
    const void* d_img = image;
    const int *d_lab = labels, *d_ex = exclude;
    if (in_host) {                                      // the upload of the image in img, of the labels in lab, of exclude in parent
        if ((rc = S.img.ensure(npx * C * esz)) || (labels && (rc = S.lab.ensure(npx * sizeof(int)))) ||
            (exclude && (rc = S.parent.ensure(npx * sizeof(int)))))
            return rc;
        HIPCHK(hipMemcpyAsync(S.img.p, image, npx * C * esz, hipMemcpyHostToDevice, st));
        d_img = S.img.p;
        if (labels) {
            HIPCHK(hipMemcpyAsync(S.lab.p, labels, npx * sizeof(int), hipMemcpyHostToDevice, st));
            d_lab = S.lab.as<int>();
        }
        if (exclude) {
            HIPCHK(hipMemcpyAsync(S.parent.p, exclude, npx * sizeof(int), hipMemcpyHostToDevice, st));
            d_ex = S.parent.as<int>();
        }
    }
    if (out_host && (rc = S.stage.ensure(cbytes + gbytes + sbytes))) return rc;         // counts, geom, spots on their way to the host
    unsigned long long* d_counts = out_host ? S.stage.as<unsigned long long>() : (unsigned long long*)counts;
    unsigned long long* d_geom = !labels ? nullptr : out_host ? (unsigned long long*)(S.stage.as<char>() + cbytes) : (unsigned long long*)geom;
    unsigned long long* d_spots = !labels ? nullptr : out_host ? (unsigned long long*)(S.stage.as<char>() + cbytes + gbytes) : (unsigned long long*)spots;
    int* d_R = r_direct ? response : S.dq.as<int>();
    unsigned int* d_ctrl = S.ctrl.as<unsigned int>();   // [0]: a bad label; [1]: the number of spots
    unsigned int* Ta = S.sm_t.as<unsigned int>();
    unsigned int* Tb = Ta + npx;

    if ((rc = S.clk_sd.record(0, st))) return rc;
    HIPCHK(hipMemcpyAsync(S.thr.p, thresholds, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_ctrl, 0, 2 * sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_counts, 0, cbytes, st));
    if (labels) {
        HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
        HIPCHK(hipMemsetAsync(d_spots, 0, sbytes, st));
    }
    {
        const dim3 rgrid((unsigned)((W + SD_ROW_SEG - 1) / SD_ROW_SEG), (unsigned)((H + SD_ROW_LINES - 1) / SD_ROW_LINES), (unsigned)batch);
        const dim3 cgrid((unsigned)((W + SD_COL_W - 1) / SD_COL_W), (unsigned)((H + SD_COL_TR - 1) / SD_COL_TR), (unsigned)batch);
        const size_t lds = sd_cols_lds(H, wt.ra, wt.rb);
        HIPCHK(hipFuncSetAttribute((const void*)sd_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (pixel_type == CS_PIX_U8)
            hipLaunchKernelGGL(sd_rows<unsigned char>, rgrid, dim3(SD_THREADS), 0, st, (const unsigned char*)d_img + params->channel, (size_t)H * W * C, C, H,
                               W, wt, Ta, Tb);
        else
            hipLaunchKernelGGL(sd_rows<unsigned short>, rgrid, dim3(SD_THREADS), 0, st, (const unsigned short*)d_img + params->channel, (size_t)H * W * C, C,
                               H, W, wt, Ta, Tb);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sd_cols, cgrid, dim3(SD_THREADS), lds, st, (const unsigned int*)Ta, (const unsigned int*)Tb, H, W, wt, d_R);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_sd.record(1, st))) return rc;
    {
        const dim3 pgrid((unsigned)nwx, (unsigned)((H + SD_PK_H - 1) / SD_PK_H), (unsigned)batch);
        hipLaunchKernelGGL(sd_peaks, pgrid, dim3(SD_THREADS), 0, st, (const int*)d_R, H, W, m, (const int*)S.thr.as<int>(), S.mask.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sd_count, dim3((unsigned)chunks), dim3(SD_THREADS), 0, st, (const unsigned long long*)S.mask.as<unsigned long long>(), rows, nwx,
                           S.counts.as<unsigned int>(), S.chunks.as<unsigned int>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sd_scan, dim3(1), dim3(SD_THREADS), 0, st, S.chunks.as<unsigned int>(), chunks, d_ctrl + 1);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_sd.record(2, st))) return rc;
    {
        if (labels) {
            const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0;
            hipLaunchKernelGGL(sd_geom, label_tile_grid(batch, H, W), dim3(LT_THREADS), 0, st, d_lab, d_ex, H, W, vec, d_geom, (int)max_label, d_ctrl);
            HIPCHK(hipGetLastError());
        }
        const SdPlace P{S.mask.as<unsigned long long>(), S.counts.as<unsigned int>(), S.chunks.as<unsigned int>(), d_R, d_lab, d_ex,
                        S.sp_list.as<int>(), S.sp_off.as<long long>(), d_counts, d_spots, rows, capacity, H, W, nwx, labels ? (int)max_label : 0};
        hipLaunchKernelGGL(sd_place, dim3((unsigned)chunks), dim3(SD_THREADS), 0, st, P);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_sd.record(3, st))) return rc;
    unsigned int flags[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(flags, d_ctrl, sizeof flags, hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(counts, d_counts, cbytes, hipMemcpyDeviceToHost, st));
        if (labels) {
            HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(spots, d_spots, sbytes, hipMemcpyDeviceToHost, st));
        }
        if (response) {
            HIPCHK(hipMemcpyAsync(response, d_R, rbytes, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the count, the host tables
    if ((rc = S.clk_sd.finish())) return rc;
    if (flags[0]) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    if ((int64_t)flags[1] > kSdMaxSpots)
        return fail(CS_ERR_UNSUPPORTED, "%lld spots: the list is capped at %lld spots per call (raise the thresholds or detect fewer images per call)",
                    (long long)flags[1], (long long)kSdMaxSpots);
    S.sp_n = flags[1];
    S.sp_batch = batch;
    *n_spots = flags[1];
    return CS_OK;
}

int cs_spot_fill(cs_preproc* p, int32_t* list, int64_t capacity, int64_t* offsets, int out_kind)
{
    if (!offsets) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(out_kind)) return fail(CS_ERR_INVALID, "out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (capacity < 0) return fail(CS_ERR_INVALID, "capacity %lld: must be >= 0", (long long)capacity);
    if (capacity > 0 && !list) return fail(CS_ERR_INVALID, "list is NULL with capacity %lld", (long long)capacity);
    if (const int rc = handle_check(p)) return rc;
    const SegmentState* S = p->seg;
    if (!S || S->sp_n < 0) return fail(CS_ERR_INVALID, "no spot list on the handle: cs_spot_detect has not succeeded on it");
    if (capacity < S->sp_n) return fail(CS_ERR_INVALID, "capacity %lld: the list has %lld spots", (long long)capacity, (long long)S->sp_n);
    HIPCHK(hipSetDevice(p->device));
    const hipMemcpyKind kind = out_kind == CS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(hipMemcpyAsync(offsets, S->sp_off.p, (size_t)(S->sp_batch + 1) * sizeof(int64_t), kind, p->stream));
    if (S->sp_n > 0) {
        HIPCHK(hipMemcpyAsync(list, S->sp_list.p, (size_t)S->sp_n * SD_SPOT * sizeof(int32_t), kind, p->stream));
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    return CS_OK;
}

int cs_spot_last_timing(const cs_preproc* p, double* response_ms, double* peaks_ms, double* records_ms)
{
    return clock_read(p, &SegmentState::clk_sd, {response_ms, peaks_ms, records_ms});
}
