// segment.hip -- the project's own classical segmenter on gfx950: a global threshold (Otsu's, as scikit-image 0.18.3 computes
// it on an integer image, or a fixed one), optional hole filling, and connected-component labelling with scipy.ndimage.label's
// numbering.  It is NOT StarDist: by default touching cells come out as one region, which the extraction's area and
// eccentricity rules then judge; cs_segment_split (below, "split_touching") cuts such regions at their necks with an exact
// integer distance-transform watershed, cs_segment_split_intensity along the intensity valleys between their cores.  The
// labels feed cs_extract_measure on the same handle and stream without leaving the device.
//
// Kernels, per batch:
//   sg_hist      exact integer histogram of one channel.  A workgroup owns a contiguous part of one image and one window of
//                32,768 values (128 KB of 32-bit LDS bins: uint8 needs one window of 256, uint16 two), counts with LDS integer
//                atomics -- equal values of a wave are first merged into one add -- and writes its bins with plain stores to a
//                slab of its own.  No global atomics: a 65,536-bin table per image in global memory would take one
//                memory-side atomic per pixel of a noisy image.
//   sg_otsu      one workgroup per image: sums the slabs, finds [min, max], int64 prefix sums of counts and counts * value,
//                then the between-class variance of every cut in explicitly rounded fp64, first argmax.
//   sg_mask      foreground = pixel > threshold, one byte per pixel.
//   sg_tile      union-find of a 64 x 16 tile in LDS (atomicMin links, larger index to smaller), every pixel then points to
//                the tile-local component's minimum linear index.
//   sg_border    merges across tile borders with atomicMin on the global parents.
//   sg_flatten   path compression: every pixel points to its component's minimum linear index; counts roots per chunk.
//   sg_scan / sg_rank / sg_gather   exclusive scan of the root counts per image, label = rank of the root + 1 in raster order.
//   sg_edge / sg_fill   (fill_holes) the same labelling on the inverted mask, 4-connected; background components without a
//                pixel on the image border become foreground (scipy.ndimage.binary_fill_holes, default structure).
//   sp_*         cs_segment_split only: see "split_touching" further down.
//   si_*         cs_segment_split_intensity only: the same watershed on heights made from the image (each component's own
//                intensity range stretched to 254 levels) instead of from the mask; see "split_by intensity".
//   bg_*         cs_segment_background only: the optional correction of the channel BEFORE all of the above (3x3 median, white
//                top-hat); see "background correction" further down.  Its plane then stands in the channel's place.
//   lt_*         cs_segment_local only: the local mean threshold in the global one's place; see "local mean threshold".
//   cl_*         cs_segment_clean only: the optional cleanup of the mask BEFORE the labelling (binary opening on a bit-packed
//                tile in LDS, minimum area by pixel counts per union-find root); see "mask cleanup" further down.  Its plane
//                then stands in the channel's place, cut at the fixed threshold 0.
//   hy_*         cs_segment_hysteresis only: the hysteresis threshold in the plain cut's (or the local rule's) place, a level
//                plane (0 / weak / strong), its weak components, and a flag per root; see "hysteresis threshold" further down.
//   ns_*         cs_segment_noise only: the noise-adaptive threshold in the plain cut's place, background + k * noise from robust
//                statistics on a mesh of tiles; see "noise-adaptive threshold" further down.
//   sm_*         cs_segment_smooth only: the optional Gaussian smoothing of the channel BEFORE all of the above, the background
//                correction included (separable, 16-bit fixed-point weights, one rounding); see "Gaussian smoothing".
// The final parents are a function of the mask alone (the minimum index of a component), so the labels do not depend on
// execution order, on the run, or on the other images of the batch.
#include "segment_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace cs {

static constexpr int SG_THREADS = 256;
static constexpr int SG_TW = 64, SG_TH = 16;            // tile of the LDS union-find: a wave reads one 64-pixel row
static constexpr int SG_TILE = SG_TW * SG_TH;
static constexpr int SG_CHUNK = 4 * SG_THREADS;         // linear pixels per workgroup in the per-pixel passes
static constexpr int SG_WAVES = SG_THREADS / 64;
static constexpr int HIST_THREADS = 1024;
static constexpr int HIST_WINDOW = 32768;               // 32-bit LDS bins per workgroup
static constexpr int HIST_MAX_PARTS = 16;
static constexpr int HIST_PART_PX = 16384;              // no part smaller than this

// ---- histogram ---------------------------------------------------------------------------------------------------------------
// One LDS add per distinct value among the first rounds' leaders (background-heavy images put most of a wave on one or two
// values), single adds for what is left.  Called by whole waves.
__device__ inline void hist_add(unsigned int* bins, int v, bool valid)
{
    const int lane = threadIdx.x & 63;
    bool pend = valid;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const unsigned long long m = __ballot(pend);
        if (m == 0ull) return;
        const int leader = __ffsll((long long)m) - 1;
        const int vl = __shfl(v, leader);
        const bool mine = pend && v == vl;
        const unsigned long long mm = __ballot(mine);
        if (lane == leader) atomicAdd(&bins[vl], (unsigned int)__popcll(mm));
        if (mine) pend = false;
    }
    if (pend) atomicAdd(&bins[v], 1u);
}

// grid (parts, NB / LB, B); slab[((b * parts + part) * NB) + value]
template <typename PIX, int NB>
__global__ __launch_bounds__(HIST_THREADS) void sg_hist(const PIX* __restrict__ image, int C, int ch, int HW, int parts,
                                                        unsigned int* __restrict__ slab)
{
    constexpr int LB = NB < HIST_WINDOW ? NB : HIST_WINDOW;
    extern __shared__ unsigned int sg_bins[];
    const int t = threadIdx.x, part = blockIdx.x, win = blockIdx.y, b = blockIdx.z;
    for (int k = t; k < LB; k += HIST_THREADS) sg_bins[k] = 0u;
    __syncthreads();
    const int per = (HW + parts - 1) / parts;
    const int p0 = min(part * per, HW), p1 = min(p0 + per, HW);
    const PIX* img = image + (size_t)b * HW * C + ch;
    for (int i0 = p0; i0 < p1; i0 += HIST_THREADS) {
        const int i = i0 + t;
        const bool in = i < p1;
        const int v = in ? (int)img[(size_t)i * C] : 0;
        hist_add(sg_bins, v - win * LB, in && v / LB == win);
    }
    __syncthreads();
    unsigned int* out = slab + ((size_t)b * parts + part) * NB + (size_t)win * LB;
    for (int k = t; k < LB; k += HIST_THREADS) out[k] = sg_bins[k];
}

// ---- Otsu's threshold (skimage.filters.threshold_otsu of 0.18.3 on an integer image) ------------------------------------
//   counts over every integer of [min, max]; w1 = cumsum(counts), w2 = the same from the top; m1 = cumsum(counts * v) / w1,
//   m2 from the top; var = (w1[:-1] * w2[1:]) * (m1[:-1] - m2[1:]) ** 2; threshold = v[first argmax].
// Every cumulative sum is an integer below 2^53 (at most 2^24 pixels of at most 2^16), so the library's float64 sums are
// exact and equal to these int64 ones; each quotient, difference and product is then one correctly rounded fp64 operation
// in the library's order.  A constant image returns its value (n == 1: no cut to weigh).
__device__ inline void block_excl_scan2(long long& a, long long& b, long long* buf /* [2][HIST_THREADS] */, long long& ta, long long& tb)
{
    const int t = threadIdx.x;
    buf[t] = a; buf[HIST_THREADS + t] = b;
    __syncthreads();
    for (int d = 1; d < HIST_THREADS; d <<= 1) {
        const long long xa = t >= d ? buf[t - d] : 0, xb = t >= d ? buf[HIST_THREADS + t - d] : 0;
        __syncthreads();
        buf[t] += xa; buf[HIST_THREADS + t] += xb;
        __syncthreads();
    }
    ta = buf[HIST_THREADS - 1]; tb = buf[2 * HIST_THREADS - 1];
    a = buf[t] - a; b = buf[HIST_THREADS + t] - b;
}

template <int NB>
__global__ __launch_bounds__(HIST_THREADS) void sg_otsu(const unsigned int* __restrict__ slab, int parts, unsigned int* hist /* [B][NB] */,
                                                        int* __restrict__ thr)
{
    __shared__ long long buf[2 * HIST_THREADS];
    __shared__ int s_lo, s_hi;
    __shared__ double bvar[HIST_THREADS / 64];
    __shared__ int bidx[HIST_THREADS / 64];
    const int t = threadIdx.x, b = blockIdx.x;
    unsigned int* h = hist + (size_t)b * NB;
    if (t == 0) { s_lo = NB; s_hi = -1; }
    __syncthreads();
    int lo = NB, hi = -1;
    for (int k = t; k < NB; k += HIST_THREADS) {
        unsigned int c = 0u;
        for (int p = 0; p < parts; ++p) c += slab[((size_t)b * parts + p) * NB + k];
        h[k] = c;
        if (c) { lo = min(lo, k); hi = max(hi, k); }
    }
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __threadfence_block();
    __syncthreads();                                    // the summed histogram and its range are complete
    lo = s_lo; hi = s_hi;
    const int n = hi - lo + 1;
    const int per = (n + HIST_THREADS - 1) / HIST_THREADS;
    const int i0 = min(t * per, n), i1 = min(i0 + per, n);
    long long w = 0, s = 0;
    for (int i = i0; i < i1; ++i) {
        const long long c = h[lo + i];
        w += c; s += c * (lo + i);
    }
    long long Wt, St;
    block_excl_scan2(w, s, buf, Wt, St);
    double best = -1.0;
    int bi = 0x7fffffff;
    for (int i = i0; i < i1 && i < n - 1; ++i) {
        const long long c = h[lo + i];
        w += c; s += c * (lo + i);
        const double w1 = (double)w, w2 = (double)(Wt - w);
        const double m1 = __ddiv_rn((double)s, w1), m2 = __ddiv_rn((double)(St - s), w2);
        const double d = __dsub_rn(m1, m2);
        const double var = __dmul_rn(__dmul_rn(w1, w2), __dmul_rn(d, d));
        if (var > best) { best = var; bi = i; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(best, m);
        const int oi = __shfl_xor(bi, m);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((t & 63) == 0) { bvar[t >> 6] = best; bidx[t >> 6] = bi; }
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < HIST_THREADS / 64; ++q)
            if (bvar[q] > best || (bvar[q] == best && bidx[q] < bi)) { best = bvar[q]; bi = bidx[q]; }
        thr[b] = n <= 1 ? lo : lo + bi;
    }
}

__global__ __launch_bounds__(SG_THREADS) void sg_fixed(int* __restrict__ thr, int batch, int value)
{
    const int b = blockIdx.x * SG_THREADS + threadIdx.x;
    if (b < batch) thr[b] = value;
}

// grid (ceil(HW / SG_CHUNK), B)
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void sg_mask(const PIX* __restrict__ image, int C, int ch, int HW, const int* __restrict__ thr,
                                                      unsigned char* __restrict__ mask)
{
    const int b = blockIdx.y, th = thr[b];
    const PIX* img = image + (size_t)b * HW * C + ch;
    unsigned char* m = mask + (size_t)b * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i < HW) m[i] = (int)img[(size_t)i * C] > th ? 1 : 0;
    }
}

// ---- union-find: parents point to smaller indices, a root points to itself, background is -1 ------------------------------
// Links are made with atomicMin at a root, towards the smaller root, so the minimum index of a component is never linked
// and ends as the one root.  A find that reads a parent another lane is just lowering sees the old or the new one: both
// lead into the same component, and the atomicMin's return value tells a union whether it really linked a root.
template <int SCOPE>
__device__ inline int uf_load(const int* P, int x) { return __hip_atomic_load(P + x, __ATOMIC_RELAXED, SCOPE); }

template <int SCOPE>
__device__ inline int uf_find(const int* P, int x)
{
    int p;
    while ((p = uf_load<SCOPE>(P, x)) != x) x = p;
    return x;
}

template <int SCOPE>
__device__ inline void uf_union(int* P, int a, int b)
{
    for (;;) {
        a = uf_find<SCOPE>(P, a);
        b = uf_find<SCOPE>(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);            // a > b
        if (old == a) return;                           // a was a root: linked
        a = old;                                        // someone linked a first: carry on from where it points
    }
}

// grid (ceil(W/64), ceil(H/16), B).  Lane l of wave w owns column l of rows w, w+4, w+8, w+12: the first reads of the
// left and upper neighbours fall on consecutive LDS banks.
// EQ: two foreground neighbours are joined only where `val` is equal on them (the plateaus of cs_segment_split's seeds).
template <bool EQ>
__global__ __launch_bounds__(SG_THREADS) void sg_tile(const unsigned char* __restrict__ mask, int H, int W, int invert, int conn8,
                                                      int* __restrict__ P, const unsigned char* __restrict__ val)
{
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ int L[SG_TILE];
    __shared__ unsigned char V[EQ ? SG_TILE : 1];
    const int lx = threadIdx.x & 63, lw = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SG_TW, y0 = blockIdx.y * SG_TH, b = blockIdx.z;
    const unsigned char* m = mask + (size_t)b * H * W;
    int* Pb = P + (size_t)b * H * W;
    const int x = x0 + lx;
    bool fg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = lw + 4 * k, y = y0 + ly;
        fg[k] = x < W && y < H && ((m[(size_t)y * W + x] != 0) != (invert != 0));
        L[ly * SG_TW + lx] = fg[k] ? ly * SG_TW + lx : -1;
        if (EQ) V[ly * SG_TW + lx] = fg[k] ? val[(size_t)b * H * W + (size_t)y * W + x] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!fg[k]) continue;
        const int ly = lw + 4 * k, idx = ly * SG_TW + lx;
        auto joins = [&](int n) { return uf_load<WG>(L, n) >= 0 && (!EQ || V[n] == V[idx]); };
        if (lx > 0 && joins(idx - 1)) uf_union<WG>(L, idx, idx - 1);
        if (ly > 0) {
            if (joins(idx - SG_TW)) uf_union<WG>(L, idx, idx - SG_TW);
            else if (conn8) {                           // with the pixel above joined, both diagonals already hang on it
                if (lx > 0 && joins(idx - SG_TW - 1)) uf_union<WG>(L, idx, idx - SG_TW - 1);
                if (lx < SG_TW - 1 && joins(idx - SG_TW + 1)) uf_union<WG>(L, idx, idx - SG_TW + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = lw + 4 * k, y = y0 + ly;
        if (x >= W || y >= H) continue;
        int r = -1;
        if (fg[k]) {
            const int q = uf_find<WG>(L, ly * SG_TW + lx);
            r = (y0 + (q >> 6)) * W + x0 + (q & 63);
        }
        Pb[(size_t)y * W + x] = r;
    }
}

// Every pair of neighbours that a tile border separates: the pixels of the first row of a tile with the row above, the pixels
// of the first column of a tile with the column to the left.  grid (ceil(n / 256), B), n = nrb * W + ncb * H.
template <bool EQ>
__global__ __launch_bounds__(SG_THREADS) void sg_border(int H, int W, int conn8, int* __restrict__ P, const unsigned char* __restrict__ val)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int nrb = (H - 1) / SG_TH, ncb = (W - 1) / SG_TW;
    int id = blockIdx.x * SG_THREADS + threadIdx.x;
    int* Pb = P + (size_t)blockIdx.y * H * W;
    const unsigned char* vb = EQ ? val + (size_t)blockIdx.y * H * W : nullptr;
    int i = 0;
    auto joins = [&](int n) { return uf_load<AG>(Pb, n) >= 0 && (!EQ || vb[n] == vb[i]); };
    if (id < nrb * W) {
        const int y = (id / W + 1) * SG_TH, x = id % W;
        i = y * W + x;
        if (uf_load<AG>(Pb, i) < 0) return;
        if (joins(i - W)) uf_union<AG>(Pb, i, i - W);
        else if (conn8) {
            if (x > 0 && joins(i - W - 1)) uf_union<AG>(Pb, i, i - W - 1);
            if (x < W - 1 && joins(i - W + 1)) uf_union<AG>(Pb, i, i - W + 1);
        }
        return;
    }
    id -= nrb * W;
    if (id >= ncb * H) return;
    const int x = (id / H + 1) * SG_TW, y = id % H;
    i = y * W + x;
    if (uf_load<AG>(Pb, i) < 0) return;
    if (joins(i - 1)) uf_union<AG>(Pb, i, i - 1);
    else if (conn8) {                                   // with the left pixel joined, the two left diagonals already hang on it
        if (y > 0 && joins(i - W - 1)) uf_union<AG>(Pb, i, i - W - 1);
        if (y < H - 1 && joins(i + W - 1)) uf_union<AG>(Pb, i, i + W - 1);
    }
}

// grid (nchunks, B).  Other workgroups replace parents with roots while this one follows them, so the accesses are agent-scope
// atomics like sg_border's.  No ordering is needed beyond that: every value a location ever holds is an ancestor in the same
// component, roots do not change in this kernel and chains strictly descend, so a find ends at the root whichever value it reads.
__global__ __launch_bounds__(SG_THREADS) void sg_flatten(int HW, int* __restrict__ P, int* __restrict__ chunk_cnt, int nchunks)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    __shared__ int wc[SG_WAVES];
    int* Pb = P + (size_t)blockIdx.y * HW;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        int r = uf_load<AG>(Pb, i);
        if (r < 0) continue;
        r = uf_find<AG>(Pb, r);
        cnt += r == i;
        __hip_atomic_store(Pb + i, r, __ATOMIC_RELAXED, AG);
    }
    if (!chunk_cnt) return;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(size_t)blockIdx.y * nchunks + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// ---- fill_holes -------------------------------------------------------------------------------------------------------------
// grid (ceil((2W + 2H) / 256), B): the roots of the (inverted-mask) components with a pixel on the image border
__global__ __launch_bounds__(SG_THREADS) void sg_edge(int H, int W, const int* __restrict__ P, int* __restrict__ touches)
{
    int id = blockIdx.x * SG_THREADS + threadIdx.x;
    int y, x;
    if (id < W) { y = 0; x = id; }
    else if (id < 2 * W) { y = H - 1; x = id - W; }
    else if (id < 2 * W + H) { y = id - 2 * W; x = 0; }
    else if (id < 2 * W + 2 * H) { y = id - 2 * W - H; x = W - 1; }
    else return;
    const size_t base = (size_t)blockIdx.y * H * W;
    const int r = P[base + (size_t)y * W + x];
    if (r >= 0) touches[base + r] = 1;
}

__global__ __launch_bounds__(SG_THREADS) void sg_fill(int HW, const int* __restrict__ P, const int* __restrict__ touches,
                                                      unsigned char* __restrict__ mask)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int r = P[base + i];
        if (r >= 0 && touches[base + r] == 0) mask[base + i] = 1;
    }
}

// ---- renumbering: consecutive ids in raster order of each component's first pixel (its root) ---------------------------------
// grid (B): exclusive scan of the per-chunk root counts of one image, in place; the total is the image's component count
__global__ __launch_bounds__(HIST_THREADS) void sg_scan(int* __restrict__ chunk_cnt, int nchunks, int* __restrict__ n_labels)
{
    __shared__ int buf[HIST_THREADS];
    const int t = threadIdx.x;
    int* c = chunk_cnt + (size_t)blockIdx.x * nchunks;
    const int per = (nchunks + HIST_THREADS - 1) / HIST_THREADS;
    const int c0 = min(t * per, nchunks), c1 = min(c0 + per, nchunks);
    int s = 0;
    for (int k = c0; k < c1; ++k) s += c[k];
    buf[t] = s;
    __syncthreads();
    for (int d = 1; d < HIST_THREADS; d <<= 1) {
        const int x = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += x;
        __syncthreads();
    }
    int run = buf[t] - s;
    for (int k = c0; k < c1; ++k) {
        const int v = c[k];
        c[k] = run;
        run += v;
    }
    if (t == HIST_THREADS - 1) n_labels[blockIdx.x] = buf[t];
}

// grid (nchunks, B): roots get their label, background 0; the other foreground pixels are written by sg_gather.
// SEL: only the roots whose `drop` flag is 0 are numbered, the others get 0 (the seeds among the plateaus of cs_segment_split).
template <bool SEL>
__global__ __launch_bounds__(SG_THREADS) void sg_rank(int HW, const int* __restrict__ P, const int* __restrict__ chunk_off, int nchunks,
                                                      int* __restrict__ labels, const int* __restrict__ drop)
{
    __shared__ int wc[4][SG_WAVES];
    const size_t base = (size_t)blockIdx.y * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before[4], par[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        par[k] = i < HW ? P[base + i] : -1;
        bool root = i < HW && par[k] == i;
        if (SEL) {
            if (root && drop[base + i] != 0) { root = false; par[k] = -1; }
            else if (!root && par[k] >= 0) par[k] = -2;         // not a root: left to the gather
        }
        const unsigned long long m = __ballot(root);
        before[k] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wc[k][wave] = __popcll(m);
    }
    __syncthreads();
    int run = chunk_off[(size_t)blockIdx.y * nchunks + blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        int mine = run;
#pragma unroll
        for (int q = 0; q < SG_WAVES; ++q) {
            if (q < wave) mine += wc[k][q];
            run += wc[k][q];
        }
        if (i < HW) {
            if (par[k] == -1) labels[base + i] = 0;
            else if (par[k] == i) labels[base + i] = mine + before[k] + 1;
        }
    }
}

__global__ __launch_bounds__(SG_THREADS) void sg_gather(int HW, const int* __restrict__ P, int* labels)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int r = P[base + i];
        if (r >= 0 && r != i) labels[base + i] = labels[base + r];      // roots are not written here
    }
}

// ---- split_touching (cs_segment_split): an exact integer distance-transform watershed -------------------------------------
// A function of the mask alone (tests/split_reference.py restates it):
//   Dq   = min(isqrt(4 * D2), 255), D2 the exact squared Euclidean distance to the nearest background pixel of the image
//          (outside the image is not background): the distance in half pixels, one byte;
//   R    = reconstruction by dilation of max(Dq - h, 0) under Dq; seeds = the regional maxima of R inside the mask;
//   flood: for v = 255 .. 1 the unlabelled pixels of mask & Dq >= v take the label that reaches them with the smallest
//          (steps, label); regions are renumbered by their first pixel.
// Kernels:
//   sp_columns   distance to the nearest background pixel of the column, capped at 128 (one thread per column, two sweeps).
//   sp_rows      D2 = min over |dx| <= 127 of dx^2 + g^2 from a row strip in LDS (the window ends where dx^2 reaches the best
//                so far), the integer square root, Dq and the marker max(Dq - h, 0); the batch's largest Dq by atomicMax.
//                D2 >= 128^2 is not told apart: both 4 * 127.5^2 and everything above give Dq = 255.
//   sp_recon     one round of R <- min(dilate(R), Dq): a 64 x 16 tile with a one-pixel halo relaxes in LDS until it is
//                quiet.  R only grows and never passes the fixed point, so a halo read while a neighbour writes is only
//                late, never wrong; a round in which no tile changed anything is the fixed point.
//   sg_tile<true> / sg_border<true> / sg_flatten   plateaus: the union-find of the labelling, joining neighbours of equal R.
//   sp_higher    flags the roots of plateaus with a pixel that has a higher neighbour (plain stores of 1, as sg_edge).
//   sp_seedcount / sg_scan / sg_rank<true> / sp_seedkey   seed ids = ranks of the unflagged roots; every pixel of a seed
//                plateau gets the key (level 0, 0 steps, id), every other pixel SP_NONE.
//   sp_flood     one round of one level: key = [63:56] 255 - level at which the pixel was labelled, [55:32] steps, [31:0] label.
//                An open pixel (Dq >= v, unlabelled or labelled at this level) takes the minimum over its labelled neighbours
//                of (this level, steps + 1, label), where a neighbour of an earlier level counts 0 steps; pixels of earlier
//                levels are final.  Keys only fall towards the one fixed point of the level, whatever the order (min-min).
//                Tiles with no open pixel at or above the level leave at once (tile_top).
//   sp_advance_* one thread: the round's "something changed" flag decides whether the reconstruction goes on and whether
//                the flood stays at its level or goes one down.  The host enqueues rounds in groups and reads one int per group.
//   sp_first / sp_parent   each region's first pixel (atomicMin per seed id), then parents = that pixel, which is what
//                sg_scan / sg_rank / sg_gather number.
// Integer atomics only, no floating point at all.
static constexpr int SP_CAP = 128;                      // column distances are capped here: only D2 < 128^2 matters
static constexpr int SP_HALO = SP_CAP - 1;
static constexpr int SP_ROW = SG_THREADS;               // pixels of one row per workgroup in the row pass
static constexpr int SP_LW = SG_TW + 2, SP_LH = SG_TH + 2;      // a tile with its halo
static constexpr unsigned long long SP_NONE = ~0ull;
enum { CT_VMAX = 0, CT_CHANGED, CT_ACTIVE, CT_LEVEL, CT_ROUNDS, CT_N = 8 };
static constexpr int SP_RECON_GROUP = 16, SP_FLOOD_GROUP = 64;  // rounds enqueued between two reads of the control word

// grid (ceil(W / 256), B)
__global__ __launch_bounds__(SG_THREADS) void sp_columns(const unsigned char* __restrict__ mask, int H, int W, unsigned char* __restrict__ g)
{
    const int x = blockIdx.x * SG_THREADS + threadIdx.x;
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.y * H * W + x;
    int d = SP_CAP;                                     // nothing above the image: outside is not background
    for (int y0 = 0; y0 < H; y0 += 16) {
        unsigned char m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = y0 + k < H ? mask[base + (size_t)(y0 + k) * W] : 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (y0 + k >= H) continue;
            d = m[k] ? min(d + 1, SP_CAP) : 0;
            g[base + (size_t)(y0 + k) * W] = (unsigned char)d;
        }
    }
    d = SP_CAP;
    for (int y1 = H - 1; y1 >= 0; y1 -= 16) {
        unsigned char m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = y1 - k >= 0 ? g[base + (size_t)(y1 - k) * W] : 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (y1 - k < 0) continue;
            d = m[k] ? min(d + 1, SP_CAP) : 0;
            if (d < (int)m[k]) g[base + (size_t)(y1 - k) * W] = (unsigned char)d;
        }
    }
}

// grid (ceil(W / 256), H, B)
__global__ __launch_bounds__(SG_THREADS) void sp_rows(const unsigned char* __restrict__ g, int H, int W, int h, unsigned char* __restrict__ dq,
                                                      unsigned char* __restrict__ R, int* __restrict__ ctrl)
{
    __shared__ unsigned char s[SP_ROW + 2 * SP_HALO];
    const int t = threadIdx.x, x0 = blockIdx.x * SP_ROW;
    const size_t row = ((size_t)blockIdx.z * H + blockIdx.y) * W;
    for (int i = t; i < SP_ROW + 2 * SP_HALO; i += SG_THREADS) {
        const int xx = x0 - SP_HALO + i;
        s[i] = xx >= 0 && xx < W ? g[row + xx] : (unsigned char)SP_CAP;
    }
    __syncthreads();
    const int x = x0 + t;
    int q = 0;
    if (x < W) {
        const int c = t + SP_HALO, g0 = s[c];
        int best = g0 * g0;
        for (int dx = 1; dx <= SP_HALO && dx * dx < best; ++dx) {         // at most 127 steps; 0 on background
            const int a = min((int)s[c - dx], (int)s[c + dx]);
            best = min(best, dx * dx + a * a);
        }
        const int n = min(4 * best, 255 * 255);
#pragma unroll
        for (int bit = 128; bit >= 1; bit >>= 1) {                        // integer square root, 8 bits
            const int r = q | bit;
            if (r * r <= n) q = r;
        }
        dq[row + x] = (unsigned char)q;
        R[row + x] = (unsigned char)max(q - h, 0);
    }
    int m = q;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
    if ((t & 63) == 0 && m > 0) atomicMax(&ctrl[CT_VMAX], m);
}

// one thread: sets the control words before the reconstruction (mode 0) and before the flood (mode 1)
__global__ void sp_start(int* __restrict__ ctrl, int mode)
{
    ctrl[CT_CHANGED] = 0;
    ctrl[CT_ROUNDS] = 0;
    if (mode == 0) ctrl[CT_ACTIVE] = 1;
    else ctrl[CT_LEVEL] = ctrl[CT_VMAX];
}

__global__ void sp_advance_recon(int* __restrict__ ctrl, int cap)
{
    if (ctrl[CT_ACTIVE] == 0) return;
    if (ctrl[CT_CHANGED] == 0 || ++ctrl[CT_ROUNDS] >= cap) ctrl[CT_ACTIVE] = 0;
    ctrl[CT_CHANGED] = 0;
}

__global__ void sp_advance_flood(int* __restrict__ ctrl, int cap)
{
    const int v = ctrl[CT_LEVEL];
    if (v < 1) return;
    if (ctrl[CT_CHANGED] == 0 || ++ctrl[CT_ROUNDS] >= cap) {
        ctrl[CT_LEVEL] = v - 1;
        ctrl[CT_ROUNDS] = 0;
    }
    ctrl[CT_CHANGED] = 0;
}

// grid (ceil(W/64), ceil(H/16), B), the thread-to-pixel map of sg_tile
__global__ __launch_bounds__(SG_THREADS) void sp_recon(const unsigned char* __restrict__ dq, int H, int W, int conn8, unsigned char* R,
                                                       int* ctrl)
{
    if (ctrl[CT_ACTIVE] == 0) return;
    __shared__ unsigned char sR[SP_LH * SP_LW];
    volatile unsigned char* v = sR;
    const int lx = threadIdx.x & 63, lw = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SG_TW, y0 = blockIdx.y * SG_TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    for (int i = threadIdx.x; i < SP_LH * SP_LW; i += SG_THREADS) {
        const int y = y0 + i / SP_LW - 1, x = x0 + i % SP_LW - 1;
        sR[i] = y >= 0 && y < H && x >= 0 && x < W ? R[base + (size_t)y * W + x] : 0;
    }
    const int x = x0 + lx;
    int d[4], cur[4], was[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + lw + 4 * k;
        d[k] = x < W && y < H ? (int)dq[base + (size_t)y * W + x] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) was[k] = cur[k] = sR[(lw + 4 * k + 1) * SP_LW + lx + 1];
    for (int it = 0; it < SG_TILE; ++it) {                                  // a path inside the tile has at most SG_TILE pixels
        int ch = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (cur[k] >= d[k]) continue;
            const int c = (lw + 4 * k + 1) * SP_LW + lx + 1;
            int m = max(max((int)v[c - 1], (int)v[c + 1]), max((int)v[c - SP_LW], (int)v[c + SP_LW]));
            if (conn8) m = max(m, max(max((int)v[c - SP_LW - 1], (int)v[c - SP_LW + 1]), max((int)v[c + SP_LW - 1], (int)v[c + SP_LW + 1])));
            m = min(m, d[k]);
            if (m > cur[k]) { cur[k] = m; v[c] = (unsigned char)m; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
    }
    int any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cur[k] != was[k]) { R[base + (size_t)(y0 + lw + 4 * k) * W + x] = (unsigned char)cur[k]; any = 1; }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0 && any) atomicOr(&ctrl[CT_CHANGED], 1);
}

// grid (nchunks, B): a pixel with a higher neighbour disqualifies its plateau
__global__ __launch_bounds__(SG_THREADS) void sp_higher(int H, int W, int conn8, const unsigned char* __restrict__ R, const int* __restrict__ P,
                                                        int* __restrict__ drop)
{
    const size_t base = (size_t)blockIdx.y * H * W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= H * W) continue;
        const int r = P[base + i];
        if (r < 0) continue;
        const int y = i / W, x = i % W, me = R[base + i];
        bool hi = false;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0)) continue;
                const int yy = y + dy, xx = x + dx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W && (int)R[base + (size_t)yy * W + xx] > me) hi = true;
            }
        if (hi) drop[base + r] = 1;
    }
}

// grid (nchunks, B): seeds (roots that are not flagged) per chunk
__global__ __launch_bounds__(SG_THREADS) void sp_seedcount(int HW, const int* __restrict__ P, const int* __restrict__ drop,
                                                           int* __restrict__ chunk_cnt, int nchunks)
{
    __shared__ int wc[SG_WAVES];
    const size_t base = (size_t)blockIdx.y * HW;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i < HW && P[base + i] == i && drop[base + i] == 0) ++cnt;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(size_t)blockIdx.y * nchunks + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// grid (nchunks, B): seed_id holds the id at seed roots and 0 at the other roots
__global__ __launch_bounds__(SG_THREADS) void sp_seedkey(int HW, const int* __restrict__ P, const int* __restrict__ seed_id,
                                                         unsigned long long* __restrict__ key)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int r = P[base + i];
        const int id = r >= 0 ? seed_id[base + r] : 0;
        key[base + i] = id > 0 ? (unsigned long long)id : SP_NONE;
    }
}

// grid (ceil(W/64), ceil(H/16), B), the thread-to-pixel map of sg_tile
__global__ __launch_bounds__(SG_THREADS) void sp_flood(const unsigned char* __restrict__ dq, int H, int W, int conn8, unsigned long long* key,
                                                       unsigned char* tile_top, int* ctrl)
{
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP, AG = __HIP_MEMORY_SCOPE_AGENT;
    const int v = ctrl[CT_LEVEL];
    if (v < 1) return;
    const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if ((int)tile_top[tile] < v) return;
    __shared__ unsigned long long sK[SP_LH * SP_LW];
    __shared__ int s_top;
    const unsigned long long code = (unsigned long long)(255 - v);
    const int lx = threadIdx.x & 63, lw = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SG_TW, y0 = blockIdx.y * SG_TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    if (threadIdx.x == 0) s_top = 0;
    for (int i = threadIdx.x; i < SP_LH * SP_LW; i += SG_THREADS) {
        const int y = y0 + i / SP_LW - 1, x = x0 + i % SP_LW - 1;
        sK[i] = y >= 0 && y < H && x >= 0 && x < W ? __hip_atomic_load(key + base + (size_t)y * W + x, __ATOMIC_RELAXED, AG) : SP_NONE;
    }
    const int x = x0 + lx;
    int d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + lw + 4 * k;
        d[k] = x < W && y < H ? (int)dq[base + (size_t)y * W + x] : 0;
    }
    __syncthreads();
    unsigned long long cur[4], was[4];
    bool open[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        was[k] = cur[k] = sK[(lw + 4 * k + 1) * SP_LW + lx + 1];
        open[k] = d[k] >= v && (cur[k] == SP_NONE || (cur[k] >> 56) == code);
    }
    for (int it = 0; it < SG_TILE; ++it) {
        int ch = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!open[k]) continue;
            const int c = (lw + 4 * k + 1) * SP_LW + lx + 1;
            unsigned long long best = cur[k];
            auto look = [&](int n) {
                const unsigned long long kn = __hip_atomic_load(&sK[n], __ATOMIC_RELAXED, WG);
                if (kn == SP_NONE) return;
                const unsigned long long steps = (kn >> 56) == code ? ((kn >> 32) & 0xffffffull) : 0ull;
                const unsigned long long cand = (code << 56) | ((steps + 1ull) << 32) | (kn & 0xffffffffull);
                if (cand < best) best = cand;
            };
            look(c - 1); look(c + 1); look(c - SP_LW); look(c + SP_LW);
            if (conn8) { look(c - SP_LW - 1); look(c - SP_LW + 1); look(c + SP_LW - 1); look(c + SP_LW + 1); }
            if (best < cur[k]) {
                cur[k] = best;
                __hip_atomic_store(&sK[c], best, __ATOMIC_RELAXED, WG);
                ch = 1;
            }
        }
        if (!__syncthreads_or(ch)) break;
    }
    int any = 0, top = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (cur[k] != was[k]) {
            __hip_atomic_store(key + base + (size_t)(y0 + lw + 4 * k) * W + x, cur[k], __ATOMIC_RELAXED, AG);
            any = 1;
        }
        if (d[k] > 0 && (cur[k] == SP_NONE || (cur[k] >> 56) == code)) top = max(top, d[k]);     // still open at this level or below
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) top = max(top, __shfl_xor(top, m));
    if ((threadIdx.x & 63) == 0 && top > 0) atomicMax(&s_top, top);
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        tile_top[tile] = (unsigned char)s_top;
        if (any) atomicOr(&ctrl[CT_CHANGED], 1);
    }
}

// grid (nchunks, B): first[id - 1] = the smallest linear index with that seed id (first was filled with 0x7f7f7f7f)
__global__ __launch_bounds__(SG_THREADS) void sp_first(int HW, const unsigned long long* __restrict__ key, int* first)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const unsigned long long kk = key[base + i];
        if (kk == SP_NONE) continue;
        int* f = first + base + ((int)(kk & 0xffffffffull) - 1);
        if (i < __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(f, i);
    }
}

// grid (nchunks, B): parents = the region's first pixel, and the root counts per chunk as sg_flatten leaves them
__global__ __launch_bounds__(SG_THREADS) void sp_parent(int HW, const unsigned long long* __restrict__ key, const int* __restrict__ first,
                                                        int* __restrict__ P, int* __restrict__ chunk_cnt, int nchunks)
{
    __shared__ int wc[SG_WAVES];
    const size_t base = (size_t)blockIdx.y * HW;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const unsigned long long kk = key[base + i];
        const int r = kk == SP_NONE ? -1 : first[base + ((int)(kk & 0xffffffffull) - 1)];
        P[base + i] = r;
        cnt += r == i;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(size_t)blockIdx.y * nchunks + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// ---- split_by intensity (cs_segment_split_intensity): the same watershed on a height plane made from the image ---------------------
// A function of the mask and the guide plane G alone (tests/split_intensity_reference.py restates it):
//   lo_c, hi_c  the smallest and largest G over the pixels of component c of the mask (filled holes included);
//   Hq   = 1 + ((G - lo_c) * 254) / max(hi_c - lo_c, min_contrast, 1) on the mask, a byte in 1..255 (65535 * 254 fits 32 bits),
//          0 on background: every component has its own 254 levels, and one flatter than min_contrast is not stretched;
//   then R, the seeds, the flood and the numbering of the distance split, with Hq in Dq's place and depth in h's.
// Kernels:
//   si_range     lo / hi per component at the root's slot of two per-pixel int planes (they live in the key buffer, which the
//                flood fills only later): atomicMin / atomicMax per run of equal roots among the first rounds' leaders of a wave,
//                as cl_count -- the lanes that share the leader's root reduce their minimum and maximum across the wave first.
//                A minimum does not depend on the order it is taken in.
//   si_height    Hq and the marker max(Hq - depth, 0); the batch's largest Hq by one atomicMax per wave, as sp_rows.
// Components come from label_mask, so one spread over many tiles has one root.  Integer atomics only, no floating point.
static constexpr int SI_NONE = 0x7f7f7f7f;              // lo before the first pixel: what a memset of 0x7f leaves

template <typename PIX>
__device__ inline int si_pixel(const PIX* __restrict__ guide, int C, int ch, size_t px) { return (int)guide[px * C + ch]; }

// grid (nchunks, B); lo: [B][HW] filled with SI_NONE, hi: [B][HW] zero before
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void si_range(int HW, const int* __restrict__ P, const PIX* __restrict__ guide, int C, int ch,
                                                       int* __restrict__ lo, int* __restrict__ hi)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const size_t base = (size_t)blockIdx.y * HW;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        const int root = i < HW ? P[base + i] : -1;
        const int g = root >= 0 ? si_pixel(guide, C, ch, base + i) : 0;
        bool pend = root >= 0;
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            const unsigned long long m = __ballot(pend);
            if (m == 0ull) break;
            const int leader = __ffsll((long long)m) - 1;
            const int rl = __shfl(root, leader);
            const bool mine = pend && root == rl;
            int mn = mine ? g : SI_NONE, mx = mine ? g : 0;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                mn = min(mn, __shfl_xor(mn, d));
                mx = max(mx, __shfl_xor(mx, d));
            }
            if (lane == leader) {
                if (mn < __hip_atomic_load(lo + base + rl, __ATOMIC_RELAXED, AG)) atomicMin(&lo[base + rl], mn);
                if (mx > __hip_atomic_load(hi + base + rl, __ATOMIC_RELAXED, AG)) atomicMax(&hi[base + rl], mx);
            }
            if (mine) pend = false;
        }
        if (pend) {
            if (g < __hip_atomic_load(lo + base + root, __ATOMIC_RELAXED, AG)) atomicMin(&lo[base + root], g);
            if (g > __hip_atomic_load(hi + base + root, __ATOMIC_RELAXED, AG)) atomicMax(&hi[base + root], g);
        }
    }
}

// grid (nchunks, B)
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void si_height(int HW, const int* __restrict__ P, const PIX* __restrict__ guide, int C, int ch,
                                                        const int* __restrict__ lo, const int* __restrict__ hi, int depth, int min_contrast,
                                                        unsigned char* __restrict__ hq, unsigned char* __restrict__ R, int* __restrict__ ctrl)
{
    const size_t base = (size_t)blockIdx.y * HW;
    int top = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int root = P[base + i];
        int q = 0;
        if (root >= 0) {
            const int l = lo[base + root];
            const unsigned int span = (unsigned int)max(max(hi[base + root] - l, min_contrast), 1);
            q = 1 + (int)((unsigned int)(si_pixel(guide, C, ch, base + i) - l) * 254u / span);
        }
        hq[base + i] = (unsigned char)q;
        R[base + i] = (unsigned char)max(q - depth, 0);
        top = max(top, q);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) top = max(top, __shfl_xor(top, d));
    if ((threadIdx.x & 63) == 0 && top > 0) atomicMax(&ctrl[CT_VMAX], top);
}

// ---- background correction (cs_segment_background): 3x3 median, white top-hat by a flat square ------------------------------
// out = x - dilate(erode(x)) with the square of side w = 2r + 1, windows clipped to the image (DESIGN 3l;
// tests/background_reference.py restates it).  The square is separable and min / max passes commute across axes:
//   bg_rows<min>  ->  bg_cols<min>  ->  bg_cols<max>  ->  bg_rows<max, fused>: out = x - opening, in the pixel type.
// A pass puts its lines with a halo of r on either side into LDS as 16-bit values (outside the image: the operation's
// identity, which is what clipping the window means), then doubles in place: after step j an element holds the min / max over
// the 2^j elements from itself on, and with 2^K <= w < 2^(K+1) a window is two overlapping spans of 2^K: K = floor(log2 w)
// <= 8 steps whatever r, no per-r template.  Doubling in place: a chunk of BG_E elements per thread is read (with its partners
// further on), a barrier, then written; chunks ascend, so a later chunk never reads what an earlier one wrote.
//   bg_rows   256 threads, 4 rows x up to 1024 pixels; wave k owns row k, lanes run along the row.
//   bg_cols   1024 threads, 64 columns x TR rows (TR = 2r rounded up to 64, within 128..512: the halo is never more than the
//             tile itself); LDS is [row][64 columns], lanes run across the columns, so a wave's 64 accesses are 64 consecutive
//             16-bit values of one row at every step: no bank is hit twice.  Dynamic LDS, (TR + 2r) * 128 bytes <= 130,816.
//   bg_median 3x3 median with the edge pixel repeated (scipy.ndimage.median_filter's default "reflect" at size 3), one thread
//             per pixel, reads the selected channel of the stack in place.
// min, max and subtract on integers only, no atomics: the plane is a function of its own image alone.
static constexpr int BG_E = 8;                          // elements a thread holds across the barrier of a doubling chunk
static constexpr int BG_MAX_R = 255;
static constexpr int BG_ROW_SEG = 1024, BG_ROW_LINES = SG_THREADS / 64;
static constexpr int BG_ROW_LEN = BG_ROW_SEG + 2 * BG_MAX_R;
static constexpr int BG_COL_THREADS = 1024, BG_COL_W = 64;
static constexpr int BG_COL_TR_MIN = 128, BG_COL_TR_MAX = 512;

static inline int bg_col_rows(int r) { return std::min(BG_COL_TR_MAX, std::max(BG_COL_TR_MIN, (2 * r + 63) / 64 * 64)); }
static inline int bg_levels(int r)
{
    int k = 0;
    while ((2 << k) <= 2 * r + 1) ++k;
    return k;                                           // 2^k <= 2r + 1 < 2^(k+1)
}

template <bool IS_MAX>
__device__ inline int bg_op(int a, int b) { return IS_MAX ? max(a, b) : min(a, b); }

// s: this thread's line (element `pos` at s[pos * es]); the thread owns positions tp, tp + pstep, ...  Called by the whole
// workgroup with the same len and levels.
template <bool IS_MAX>
__device__ inline void bg_double(unsigned short* s, int es, int len, int tp, int pstep, int levels)
{
    for (int j = 0; j < levels; ++j) {
        const int d = 1 << j;
        for (int p0 = 0; p0 < len; p0 += BG_E * pstep) {
            int v[BG_E];
#pragma unroll
            for (int e = 0; e < BG_E; ++e) {
                const int pos = p0 + e * pstep + tp;
                v[e] = 0;
                if (pos < len) {
                    v[e] = s[pos * es];
                    if (pos + d < len) v[e] = bg_op<IS_MAX>(v[e], (int)s[(pos + d) * es]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < BG_E; ++e) {
                const int pos = p0 + e * pstep + tp;
                if (pos < len) s[pos * es] = (unsigned short)v[e];
            }
        }
        __syncthreads();
    }
}

// grid (ceil(W / BG_ROW_SEG), ceil(H / BG_ROW_LINES), B).  in: pixel (b, y, x) at in[b * in_img + (y * W + x) * in_pix].
// FUSE: out = orig - result, orig addressed the same way.
template <typename PIX, bool IS_MAX, bool FUSE>
__global__ __launch_bounds__(SG_THREADS) void bg_rows(const PIX* __restrict__ in, size_t in_img, int in_pix, int H, int W, int r, int levels,
                                                      const PIX* __restrict__ orig, size_t orig_img, int orig_pix, PIX* __restrict__ out)
{
    __shared__ unsigned short sm[BG_ROW_LINES * BG_ROW_LEN];
    const int tp = threadIdx.x & 63, line = threadIdx.x >> 6;
    const int x0 = blockIdx.x * BG_ROW_SEG, y = blockIdx.y * BG_ROW_LINES + line, b = blockIdx.z;
    const int seg = min(BG_ROW_SEG, W - x0), len = seg + 2 * r;
    constexpr unsigned short ident = IS_MAX ? 0 : 0xffff;
    unsigned short* s = sm + line * BG_ROW_LEN;
    const PIX* src = in + (size_t)b * in_img + (size_t)(y < H ? y : 0) * W * in_pix;
    for (int pos = tp; pos < len; pos += 64) {
        const int x = x0 - r + pos;
        s[pos] = y < H && x >= 0 && x < W ? (unsigned short)src[(size_t)x * in_pix] : ident;
    }
    __syncthreads();
    bg_double<IS_MAX>(s, 1, len, tp, 64, levels);
    if (y >= H) return;
    const int off = 2 * r + 1 - (1 << levels);
    for (int pos = tp; pos < seg; pos += 64) {
        int v = bg_op<IS_MAX>((int)s[pos], (int)s[pos + off]);
        const size_t px = (size_t)y * W + x0 + pos;
        if (FUSE) v = (int)orig[(size_t)b * orig_img + px * orig_pix] - v;
        out[(size_t)b * H * W + px] = (PIX)v;
    }
}

// grid (ceil(W / 64), ceil(H / TR), B), planes in and out; dynamic LDS (min(TR, H) + 2r) * 64 * 2 bytes
template <typename PIX, bool IS_MAX>
__global__ __launch_bounds__(BG_COL_THREADS) void bg_cols(const PIX* __restrict__ in, int H, int W, int r, int levels, int TR,
                                                          PIX* __restrict__ out)
{
    extern __shared__ unsigned short bg_sm[];
    const int col = threadIdx.x & 63, tp = threadIdx.x >> 6;
    constexpr int PS = BG_COL_THREADS / BG_COL_W;
    const int x = blockIdx.x * BG_COL_W + col, y0 = blockIdx.y * TR;
    const int rows = min(TR, H - y0), len = rows + 2 * r;
    constexpr unsigned short ident = IS_MAX ? 0 : 0xffff;
    const size_t base = (size_t)blockIdx.z * H * W;
    unsigned short* s = bg_sm + col;
    for (int pos = tp; pos < len; pos += PS) {
        const int y = y0 - r + pos;
        s[pos * BG_COL_W] = x < W && y >= 0 && y < H ? (unsigned short)in[base + (size_t)y * W + x] : ident;
    }
    __syncthreads();
    bg_double<IS_MAX>(s, BG_COL_W, len, tp, PS, levels);
    if (x >= W) return;
    const int off = 2 * r + 1 - (1 << levels);
    for (int pos = tp; pos < rows; pos += PS)
        out[base + (size_t)(y0 + pos) * W + x] = (PIX)bg_op<IS_MAX>((int)s[pos * BG_COL_W], (int)s[(pos + off) * BG_COL_W]);
}

__device__ inline void bg_sort3(int& a, int& b, int& c)
{
    const int lo = min(a, b), hi = max(a, b);
    a = min(lo, c);
    const int m = max(lo, c);
    b = min(m, hi);
    c = max(m, hi);
}

// grid (ceil(HW / SG_CHUNK), B).  The median of nine from the three sorted columns: the largest of their minima, the median of
// their medians and the smallest of their maxima hold it between them.
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void bg_median(const PIX* __restrict__ image, int C, int ch, int H, int W, PIX* __restrict__ out)
{
    const int HW = H * W;
    const PIX* img = image + (size_t)blockIdx.y * HW * C + ch;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int y = i / W, x = i % W;
        const int ys[3] = {max(y - 1, 0), y, min(y + 1, H - 1)}, xs[3] = {max(x - 1, 0), x, min(x + 1, W - 1)};
        int lo[3], mid[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = img[((size_t)ys[0] * W + xs[c]) * C];
            mid[c] = img[((size_t)ys[1] * W + xs[c]) * C];
            hi[c] = img[((size_t)ys[2] * W + xs[c]) * C];
            bg_sort3(lo[c], mid[c], hi[c]);
        }
        int a = max(max(lo[0], lo[1]), lo[2]), c = min(min(hi[0], hi[1]), hi[2]);
        bg_sort3(mid[0], mid[1], mid[2]);
        int m = mid[1];
        bg_sort3(a, m, c);
        out[(size_t)blockIdx.y * HW + i] = (PIX)m;
    }
}

// ---- local mean threshold (cs_segment_local) -----------------------------------------------------------------------------------
// fg = n * x - S - n * delta > 0 and x > floor, with S the sum of x over the window [i - r, i + r] x [j - r, j + r] of side
// w = 2r + 1 (n = w * w), indices outside the image reflected about the edge (d c b a | a b c d, period 2 * side, so r may exceed
// a side): x > skimage.filters.threshold_local(x, w, 'mean', offset=-delta) decided in integers, an exact tie being background
// (tests/local_reference.py restates it).  The square is separable: row sums, then column sums of the row sums.
//   lt_rows   256 threads, 4 rows x up to 1024 pixels; wave k owns row k.  The row with a halo of r on either side goes into
//             LDS as 32-bit values; lane l sums its own run of CH consecutive values (CH odd, so the 64 lanes of an access are
//             on 64 different banks), the wave scans the 64 totals, and each lane turns its run into inclusive prefix sums in
//             place.  A window is the difference of two prefixes; lanes run along the row for the loads and the stores.  A
//             prefix is at most 1534 * 65535 and a row sum at most 511 * 65535: both fit 32 bits.
//   lt_cols   256 threads, 64 columns x 4 row tiles of TR rows (TR as bg_cols': 2r rounded up to 64, within 128..512, so the
//             2r halo rows are never more than the tile); lanes run across the columns, every access of a wave is 64 consecutive
//             values of one row.  A thread walks down its column with the window's sum in a 64-bit register (n * x and S reach
//             1.7e10): 2r + 1 row sums to start, then one in and one out per pixel, compared and written as 0 / 1.  No LDS:
//             the row that leaves was read 2r + 1 rows earlier by the same wave and comes from the cache.
// Integer sums do not depend on their order and there are no atomics: the plane is a function of its own image alone.
static constexpr int LT_MAX_R = 255;
static constexpr int LT_ROW_SEG = 1024, LT_ROW_LINES = SG_THREADS / 64;
static constexpr int LT_ROW_LEN = LT_ROW_SEG + 2 * LT_MAX_R;
static constexpr int LT_COL_W = 64, LT_COL_TILES = SG_THREADS / 64;
static constexpr int LT_COL_U = 8;                      // rows a thread of lt_cols loads before it uses the first

// index i of a line of n reflected about the edges: ... 2 1 0 | 0 1 2 ... n-1 | n-1 n-2 ..., period 2n; any i
__device__ inline int lt_fold(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// grid (ceil(W / LT_ROW_SEG), ceil(H / LT_ROW_LINES), B).  in: pixel (b, y, x) at in[b * in_img + (y * W + x) * in_pix].
// sums: [B][H][W] uint32, the sum over [x - r, x + r] of row y.
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void lt_rows(const PIX* __restrict__ in, size_t in_img, int in_pix, int H, int W, int r,
                                                      unsigned int* __restrict__ sums)
{
    __shared__ unsigned int sm[LT_ROW_LINES * LT_ROW_LEN];
    const int tp = threadIdx.x & 63, line = threadIdx.x >> 6;
    const int x0 = blockIdx.x * LT_ROW_SEG, y = blockIdx.y * LT_ROW_LINES + line, b = blockIdx.z;
    const int seg = min(LT_ROW_SEG, W - x0), len = seg + 2 * r;
    unsigned int* s = sm + line * LT_ROW_LEN;
    const PIX* src = in + (size_t)b * in_img + (size_t)(y < H ? y : 0) * W * in_pix;
    for (int pos = tp; pos < len; pos += 64) s[pos] = y < H ? (unsigned int)src[(size_t)lt_fold(x0 - r + pos, W) * in_pix] : 0u;
    __syncthreads();
    const int ch = ((len + 63) / 64) | 1;               // >= len / 64 and odd
    const int p0 = min(tp * ch, len), p1 = min(p0 + ch, len);
    unsigned int total = 0;
    for (int pos = p0; pos < p1; ++pos) total += s[pos];
    unsigned int before = total;                        // inclusive scan of the lanes' totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int up = __shfl_up(before, d, 64);
        if (tp >= d) before += up;
    }
    before -= total;
    for (int pos = p0; pos < p1; ++pos) {
        before += s[pos];
        s[pos] = before;
    }
    __syncthreads();
    if (y >= H) return;
    unsigned int* dst = sums + ((size_t)b * H + y) * W + x0;
    for (int pos = tp; pos < seg; pos += 64) dst[pos] = s[pos + 2 * r] - (pos ? s[pos - 1] : 0u);
}

// what lt_cols writes for one pixel: 0 / 1 of the one rule, or with LEVELS the level under two deltas (n_weak <= n_delta): 0, 1 where
// only the weak rule holds, 2 where the strong one does.  Both compare the one margin n * v - S; the floor is common to both.
template <bool LEVELS>
__device__ inline unsigned char lt_cut(long long n, int v, long long S, long long n_delta, long long n_weak, int floor)
{
    if (!LEVELS) return (n * v - S - n_delta > 0 && v > floor) ? 1 : 0;
    const long long m = n * v - S;
    return v > floor ? (m - n_delta > 0 ? 2 : (m - n_weak > 0 ? 1 : 0)) : 0;
}

// grid (ceil(W / LT_COL_W), ceil(H / (LT_COL_TILES * TR)), B).  x: the pixels, addressed as lt_rows' in; out: [B][H][W] 0 / 1,
// with LEVELS (cs_segment_hysteresis) 0 / 1 / 2.
template <typename PIX, bool LEVELS>
__global__ __launch_bounds__(SG_THREADS) void lt_cols(const unsigned int* __restrict__ sums, const PIX* __restrict__ x, size_t x_img,
                                                      int x_pix, int H, int W, int r, int TR, long long n, long long n_delta,
                                                      long long n_weak, int floor, unsigned char* __restrict__ out)
{
    const int col = blockIdx.x * LT_COL_W + (threadIdx.x & 63);
    const int y0 = (blockIdx.y * LT_COL_TILES + (threadIdx.x >> 6)) * TR, y1 = min(y0 + TR, H);
    if (col >= W || y0 >= H) return;
    const unsigned int* sc = sums + (size_t)blockIdx.z * H * W + col;
    const PIX* xc = x + (size_t)blockIdx.z * x_img + (size_t)col * x_pix;
    unsigned char* oc = out + (size_t)blockIdx.z * H * W + col;
    long long S = 0;
#pragma unroll 8
    for (int k = -r; k <= r; ++k) S += sc[(size_t)lt_fold(y0 + k, H) * W];
    int y = y0;
    for (; y + LT_COL_U <= y1; y += LT_COL_U) {         // the loads of LT_COL_U rows in flight before the first is used
        int v[LT_COL_U];
        unsigned int in[LT_COL_U], gone[LT_COL_U];
#pragma unroll
        for (int u = 0; u < LT_COL_U; ++u) {
            v[u] = xc[(size_t)(y + u) * W * x_pix];
            in[u] = sc[(size_t)lt_fold(y + u + r + 1, H) * W];
            gone[u] = sc[(size_t)lt_fold(y + u - r, H) * W];
        }
#pragma unroll
        for (int u = 0; u < LT_COL_U; ++u) {
            oc[(size_t)(y + u) * W] = lt_cut<LEVELS>(n, v[u], S, n_delta, n_weak, floor);
            S += (long long)in[u] - (long long)gone[u];
        }
    }
    for (; y < y1; ++y) {
        const int v = xc[(size_t)y * W * x_pix];
        oc[(size_t)y * W] = lt_cut<LEVELS>(n, v, S, n_delta, n_weak, floor);
        S += (long long)sc[(size_t)lt_fold(y + r + 1, H) * W] - (long long)sc[(size_t)lt_fold(y - r, H) * W];
    }
}

// ---- Gaussian smoothing (cs_segment_smooth) ------------------------------------------------------------------------------------
// y = (A + 2^31) >> 32 with T(i, j) = sum_k w[|k|] x(i, fold(j + k, W)) and A(i, j) = sum_k w[|k|] T(fold(i + k, H), j), k = -r..r,
// fold being lt_fold (scipy's mode='reflect'; r may exceed a side) and w[0] + 2 * sum_{k >= 1} w[k] = 2^16 (DESIGN 3o;
// tests/smooth_reference.py restates it).  The table comes with the call (cs_smooth_params): the kernels are exact for any table
// that passes smooth_check.  x <= 65535, so T <= 65535 * 2^16 fits 32 bits and A < 2^48; a constant image is a fixed point.
//   sm_rows   256 threads, 4 rows x up to 768 pixels; wave k owns row k.  The row with a halo of r on either side goes into LDS
//             as 16-bit values.  A lane produces SM_ROW_E = 6 adjacent outputs at a time from two sliding windows of registers,
//             x[j - k ..] and x[j + k ..]: one step of k costs it two LDS reads (the value that enters each window) and six
//             (left + right) * w[k], 17 bits times at most 17, accumulated in 32 bits.  Lanes are 6 halfwords = 3 words apart
//             in LDS: an odd stride, so the 32 lanes of an access are on 32 different banks.  Writes T, 4 bytes per pixel.
//   sm_cols   256 threads, 64 columns x 128 rows; LDS is [rows + 2r][64 columns] of T (dynamic, at most 66,560 bytes), lanes run
//             across the columns, so every access of a wave is 64 consecutive words of one row.  A thread produces SM_COL_E = 4
//             adjacent rows of its column, again from two sliding windows.  The 48-bit sum without a 64-bit multiply: T is split
//             into its high and low 16 bits, each half has a 32-bit accumulator (at most 65535 * 2^16 < 2^32, as the weights
//             sum to 2^16), and the two meet once: A = (hi << 16) + lo, plus 2^31, shifted by 32.
// The weights are a kernel argument by value, indexed by the uniform k: scalar loads, no vector register holds them.  Integer
// multiplies and adds only, no atomics: the plane is a function of its own image and the table alone.
static constexpr int SM_MAX_R = 64;
static constexpr int SM_ROW_E = 6, SM_ROW_SEG = 2 * 64 * SM_ROW_E, SM_ROW_LINES = SG_THREADS / 64;
static constexpr int SM_ROW_LEN = SM_ROW_SEG + 2 * SM_MAX_R + SM_ROW_E;          // a last lane's windows run up to E - 2 past the halo
static constexpr int SM_COL_W = 64, SM_COL_WAVES = SG_THREADS / 64, SM_COL_E = 4, SM_COL_TR = 128;

struct SmWeights {
    int r;
    unsigned int w[SM_MAX_R + 1];
};

// grid (ceil(W / SM_ROW_SEG), ceil(H / SM_ROW_LINES), B).  in: pixel (b, y, x) at in[b * in_img + (y * W + x) * in_pix].
// T: [B][H][W] uint32.
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void sm_rows(const PIX* __restrict__ in, size_t in_img, int in_pix, int H, int W, const SmWeights wt,
                                                      unsigned int* __restrict__ T)
{
    __shared__ unsigned short sm[SM_ROW_LINES * SM_ROW_LEN];
    constexpr int E = SM_ROW_E;
    const int tp = threadIdx.x & 63, line = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SM_ROW_SEG, y = blockIdx.y * SM_ROW_LINES + line, b = blockIdx.z;
    const int r = wt.r, seg = min(SM_ROW_SEG, W - x0), len = seg + 2 * r;
    unsigned short* s = sm + line * SM_ROW_LEN;
    const PIX* src = in + (size_t)b * in_img + (size_t)(y < H ? y : 0) * W * in_pix;
    for (int pos = tp; pos < len + E; pos += 64)
        s[pos] = y < H && pos < len ? (unsigned short)src[(size_t)lt_fold(x0 - r + pos, W) * in_pix] : (unsigned short)0;
    __syncthreads();
    if (y >= H) return;
    unsigned int* dst = T + ((size_t)b * H + y) * W + x0;
    const unsigned int w0 = wt.w[0];
    for (int j = tp * E; j < seg; j += 64 * E) {
        const unsigned short* c = s + r + j;            // c[d]: the pixel x0 + j + d
        unsigned int lo[E], hi[E], acc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            lo[e] = hi[e] = c[e];
            acc[e] = w0 * lo[e];
        }
        for (int k = 1; k <= r; ++k) {                  // lo[e] = c[e - k], hi[e] = c[e + k]
            const unsigned int w = wt.w[k];
#pragma unroll
            for (int e = E - 1; e > 0; --e) lo[e] = lo[e - 1];
#pragma unroll
            for (int e = 0; e < E - 1; ++e) hi[e] = hi[e + 1];
            lo[0] = c[-k];
            hi[E - 1] = c[E - 1 + k];
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += w * (lo[e] + hi[e]);
        }
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (j + e < seg) dst[j + e] = acc[e];
    }
}

// grid (ceil(W / SM_COL_W), ceil(H / SM_COL_TR), B); dynamic LDS (min(SM_COL_TR, H) + 2r + SM_COL_E) * 64 * 4 bytes.
// out: [B][H][W] of the pixel type.
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void sm_cols(const unsigned int* __restrict__ T, int H, int W, const SmWeights wt, PIX* __restrict__ out)
{
    extern __shared__ unsigned int sm_tile[];
    constexpr int E = SM_COL_E;
    const int col = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * SM_COL_W + col, y0 = blockIdx.y * SM_COL_TR;
    const int r = wt.r, rows = min(SM_COL_TR, H - y0), len = rows + 2 * r;
    const size_t base = (size_t)blockIdx.z * H * W;
    for (int pos = wv; pos < len + E; pos += SM_COL_WAVES)
        sm_tile[pos * SM_COL_W + col] = x < W && pos < len ? T[base + (size_t)lt_fold(y0 - r + pos, H) * W + x] : 0u;
    __syncthreads();
    if (x >= W) return;
    const unsigned int w0 = wt.w[0];
    for (int j = wv * E; j < rows; j += SM_COL_WAVES * E) {
        const unsigned int* c = sm_tile + (r + j) * SM_COL_W + col;      // c[d * 64]: T of row y0 + j + d
        unsigned int lh[E], ll[E], hh[E], hl[E], ah[E], al[E];  // the two windows and the sums, high and low halves
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const unsigned int t = c[e * SM_COL_W];
            lh[e] = hh[e] = t >> 16;
            ll[e] = hl[e] = t & 0xffffu;
            ah[e] = w0 * lh[e];
            al[e] = w0 * ll[e];
        }
        for (int k = 1; k <= r; ++k) {
            const unsigned int w = wt.w[k];
            const unsigned int a = c[-k * SM_COL_W], z = c[(E - 1 + k) * SM_COL_W];
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
        for (int e = 0; e < E; ++e)
            if (j + e < rows) {
                const unsigned long long A = ((unsigned long long)ah[e] << 16) + al[e] + (1ull << 31);
                out[base + (size_t)(y0 + j + e) * W + x] = (PIX)(A >> 32);
            }
    }
}

// ---- mask cleanup (cs_segment_clean): binary opening, minimum area -------------------------------------------------------------
// Between the hole filling and the labelling, on the 0 / 1 mask alone (tests/clean_reference.py restates it):
//   opening   r erosions then r dilations by the 3 x 3 cross (connectivity 1) or square (2), outside the image background for
//             the erosion: scipy.ndimage.binary_opening(mask, generate_binary_structure(2, k), iterations=r).
//   min area  components (under the segmenter's connectivity) of fewer than `a` pixels become background.
//   cl_open   one workgroup opens a tile of 256 x 32 pixels.  The mask is packed one pixel per bit: a wave reads 64 consecutive
//             bytes of a row and its ballot is the 64-bit word of that row segment (bit i = pixel x + i).  The tile sits in LDS
//             with a halo of one word (64 >= 2r pixels) left and right and 2r rows above and below: r pixels for the erosion,
//             r more for the dilation of what it leaves.  Pixels outside the image are loaded as 0, which is all the erosion's
//             border rule needs; the dilation may grow into them, and nothing there finds a way back in that a path inside the
//             image would not have (the structures are convex).  An elementary step is shifts, ANDs and ORs of a word, its two
//             row neighbours and the carried-in bits of the words left and right, from one LDS buffer to the other; a frame of
//             zero words around the two buffers stands for what is beyond them, and whatever creeps in from there moves one
//             pixel per step and has 2r pixels to go.  The mask crosses HBM once each way however large r is.
//   cl_count  pixels per component at the root's slot of a per-pixel int table: one atomicAdd per run of equal roots among the
//             first rounds' leaders of a wave (a row segment inside one component is one add), as hist_add.  Integer sums do
//             not depend on their order.
//   cl_drop   out = 1 where the pixel's root counts at least `a`.
// Components come from label_mask (tile union-find, border merge, flatten), so a component spread over many tiles is counted
// as one.  Shifts, ANDs, ORs and integer adds only: the plane is a function of the mask alone.
static constexpr int CL_MAX_R = 15;
static constexpr int CL_MAX_AREA = 1 << 24;             // kMaxSide^2: no component is larger
static constexpr int CL_TWW = 4, CL_TW = 64 * CL_TWW;   // words and pixels of a tile's row
static constexpr int CL_TH = 32;                        // rows of a tile
static constexpr int CL_LW = CL_TWW + 2;                // words of a row in LDS: the tile and one halo word on either side
static constexpr int CL_SW = CL_LW + 2;                 // with the frame of zero words
static constexpr int CL_ROWS = CL_TH + 4 * CL_MAX_R;    // rows in LDS at the largest radius
static constexpr int CL_LOAD_U = 4;                     // row segments a wave loads before its first ballot

// grid (ceil(W / CL_TW), ceil(H / CL_TH), B)
__global__ __launch_bounds__(SG_THREADS) void cl_open(const unsigned char* __restrict__ mask, int H, int W, int r, int square,
                                                      unsigned char* __restrict__ out)
{
    __shared__ unsigned long long buf[2][(CL_ROWS + 2) * CL_SW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * CL_TW, y0 = blockIdx.y * CL_TH;
    const int rows = CL_TH + 4 * r, nseg = rows * CL_LW;
    const unsigned char* m = mask + (size_t)blockIdx.z * H * W;
    for (int i = threadIdx.x; i < (rows + 2) * CL_SW; i += SG_THREADS) buf[0][i] = buf[1][i] = 0ull;        // the frame stays
    __syncthreads();
    for (int s0 = wave; s0 < nseg; s0 += SG_WAVES * CL_LOAD_U) {
        unsigned char v[CL_LOAD_U];
#pragma unroll
        for (int u = 0; u < CL_LOAD_U; ++u) {
            const int s = s0 + u * SG_WAVES;
            const int y = y0 - 2 * r + s / CL_LW, x = x0 + (s % CL_LW - 1) * 64 + lane;
            v[u] = s < nseg && y >= 0 && y < H && x >= 0 && x < W ? m[(size_t)y * W + x] : 0;
        }
#pragma unroll
        for (int u = 0; u < CL_LOAD_U; ++u) {
            const int s = s0 + u * SG_WAVES;
            const unsigned long long bits = __ballot(v[u] != 0);
            if (lane == 0 && s < nseg) buf[0][(s / CL_LW + 1) * CL_SW + s % CL_LW + 1] = bits;
        }
    }
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < 2 * r; ++step, cur ^= 1) {
        const unsigned long long* a = buf[cur];
        unsigned long long* b = buf[cur ^ 1];
        const bool erode = step < r;
        for (int s = threadIdx.x; s < nseg; s += SG_THREADS) {
            const int c = (s / CL_LW + 1) * CL_SW + s % CL_LW + 1;
            unsigned long long res;
            if (square) {                               // the row's own 1 x 3 step on the three rows, then across them
                unsigned long long h[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int q = c + (k - 1) * CL_SW;
                    const unsigned long long w = a[q], lt = (w << 1) | (a[q - 1] >> 63), rt = (w >> 1) | (a[q + 1] << 63);
                    h[k] = erode ? (w & lt & rt) : (w | lt | rt);
                }
                res = erode ? (h[0] & h[1] & h[2]) : (h[0] | h[1] | h[2]);
            } else {
                const unsigned long long w = a[c], lt = (w << 1) | (a[c - 1] >> 63), rt = (w >> 1) | (a[c + 1] << 63);
                const unsigned long long up = a[c - CL_SW], dn = a[c + CL_SW];
                res = erode ? (w & lt & rt & up & dn) : (w | lt | rt | up | dn);
            }
            b[c] = res;
        }
        __syncthreads();
    }
    unsigned char* o = out + (size_t)blockIdx.z * H * W;
    for (int s = wave; s < CL_TH * CL_TWW; s += SG_WAVES) {
        const int ly = s / CL_TWW, lw = s % CL_TWW;
        const int y = y0 + ly, x = x0 + lw * 64 + lane;
        if (y >= H || x >= W) continue;
        const unsigned long long w = buf[cur][(2 * r + ly + 1) * CL_SW + lw + 2];
        o[(size_t)y * W + x] = (unsigned char)((w >> lane) & 1ull);
    }
}

// grid (nchunks, B); cnt: [B][HW], zero before
__global__ __launch_bounds__(SG_THREADS) void cl_count(int HW, const int* __restrict__ P, int* __restrict__ cnt)
{
    const size_t base = (size_t)blockIdx.y * HW;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        const int root = i < HW ? P[base + i] : -1;
        bool pend = root >= 0;
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            const unsigned long long m = __ballot(pend);
            if (m == 0ull) break;
            const int leader = __ffsll((long long)m) - 1;
            const int rl = __shfl(root, leader);
            const bool mine = pend && root == rl;
            const unsigned long long mm = __ballot(mine);
            if (lane == leader) atomicAdd(&cnt[base + rl], __popcll(mm));
            if (mine) pend = false;
        }
        if (pend) atomicAdd(&cnt[base + root], 1);
    }
}

// grid (nchunks, B); out may be the mask that P was made from
__global__ __launch_bounds__(SG_THREADS) void cl_drop(int HW, const int* __restrict__ P, const int* __restrict__ cnt, int min_area,
                                                      unsigned char* __restrict__ out)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int root = P[base + i];
        out[base + i] = root >= 0 && cnt[base + root] >= min_area ? 1 : 0;
    }
}

// ---- hysteresis threshold (cs_segment_hysteresis) -----------------------------------------------------------------------------
// Two rules of one form, the weak one with the lower number, so that strong pixels are weak pixels too.  The result keeps the
// pixels of those components of the weak mask (under the segmenter's connectivity) that hold at least one strong pixel:
// skimage.filters.apply_hysteresis_threshold with integer rules (tests/hysteresis_reference.py restates it).
//   hy_levels   global rule: level = 2 where x > thr[b], 1 where x > low_b only, else 0; low_b = min(weak, thr[b]) in counts or
//               (thr[b] * q) >> 16 as a fraction, derived from the image's own threshold on the device.
//   lt_cols<PIX, true>   local rule: the level under local_delta and the weak delta from the one margin (lt_rows as it is).
//   label_mask  components of "level != 0": sg_tile takes any non-zero byte for foreground.
//   hy_mark     flag[root] = 1 for every pixel of level 2, in a zeroed int plane with one slot per pixel of each image (the
//               area step's counts plane).  Every writer stores the same constant: plain stores, no atomics, and the outcome
//               does not depend on their order.  A wave without a strong pixel (most of a field) skips the parent loads.
//   hy_keep     out = 1 where the pixel's root is flagged.
// Roots are indices inside their own image and the flags are addressed image by image, so nothing crosses between the images
// of a batch.  Comparisons and stores of constants only: the plane is a function of its own image alone.
// grid (nchunks, B)
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void hy_levels(const PIX* __restrict__ image, int C, int ch, int HW, const int* __restrict__ thr,
                                                        int fraction, int weak, unsigned char* __restrict__ level)
{
    const int b = blockIdx.y, th = thr[b];
    const int low = fraction ? (int)(((unsigned long long)(unsigned int)max(th, 0) * (unsigned int)weak) >> 16) : min(weak, th);
    const PIX* img = image + (size_t)b * HW * C + ch;
    unsigned char* m = level + (size_t)b * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int v = (int)img[(size_t)i * C];
        m[i] = v > th ? 2 : (v > low ? 1 : 0);
    }
}

// grid (nchunks, B); flag: [B][HW], zero before; P after sg_flatten: every pixel of level > 0 holds its root
__global__ __launch_bounds__(SG_THREADS) void hy_mark(int HW, const unsigned char* __restrict__ level, const int* __restrict__ P,
                                                      int* __restrict__ flag)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        const bool strong = i < HW && level[base + i] == 2;
        if (__ballot(strong) == 0ull) continue;         // the whole wave decides alike
        if (!strong) continue;
        const int root = P[base + i];
        if (root >= 0) flag[base + root] = 1;
    }
}

// grid (nchunks, B)
__global__ __launch_bounds__(SG_THREADS) void hy_keep(int HW, const int* __restrict__ P, const int* __restrict__ flag,
                                                      unsigned char* __restrict__ out)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int root = P[base + i];
        out[base + i] = root >= 0 && flag[base + root] != 0 ? 1 : 0;
    }
}

// ---- noise-adaptive threshold (cs_segment_noise) ------------------------------------------------------------------------------
// The cut is background + k * noise, both estimated from the image on a mesh of tiles (tests/noise_reference.py
// restates it).  Along an axis of n pixels there are m = max(1, n >> shift) tiles of side T = 1 << shift; the last one runs to
// n and is at most 2T - 1 wide.
//   ns_stats    one workgroup per tile and image: an exact selection of the lower median (rank (N - 1) / 2) and then of the same
//               rank among |x - med|, each by radix: a 256-bin LDS histogram of the high byte (hist_add's wave aggregation),
//               a scan to the bucket that holds the rank, then the low byte among that bucket's values (uint8: the one pass).
//               A tile of at most 4096 pixels (every regular tile up to T = 64) is read once and stays in 16 registers; the
//               others (up to 511 x 511) are read again in each pass, row by row.  Counts are integers: the atomics' order
//               cannot change them.  Writes B8 = 256 med and S8 = max((dev * 97164) >> 8, floor8).
//   ns_filter   the median of the 3 x 3 mesh neighbourhood (mesh replicated at its edges) of both maps, one thread per node.
//   ns_cut      per pixel the two nodes and weights of each axis (bilinear between tile centres at doubled coordinates
//               C2_i = start_i + end_i - 1, constant outside the outer centres), N_B, N_S and D in 64-bit integers, and
//               256 (256 v D - N_B) > k8 N_S; with a weak rule the 0 / 1 / 2 level plane of the hysteresis stage, whose
//               label_mask, hy_mark and hy_keep then run as they are.
// The mesh is addressed image by image; nothing crosses between the images of a batch.  No floating point anywhere.
static constexpr int NS_REG = 16;                       // pixels a thread of ns_stats keeps in registers
static constexpr int NS_MAD_Q16 = 97164;                // 1.4826 * 65536

// The bucket of a 256-bin histogram that holds `rank`, and the rank inside it: sel[0], sel[1].  All 256 threads call it; the
// bins are complete before and may be cleared after.
__device__ inline void ns_find(const unsigned int* bins, int rank, int* sel, unsigned int* wsum)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned int c = bins[t];
    unsigned int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    for (int q = 0; q < wave; ++q) incl += wsum[q];
    const unsigned int excl = incl - c;
    if (excl <= (unsigned int)rank && (unsigned int)rank < incl) { sel[0] = t; sel[1] = rank - (int)excl; }
    __syncthreads();
}

// grid (mx, my, B); mesh: [B][2][my][mx], B8 then S8
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void ns_stats(const PIX* __restrict__ image, int C, int ch, int H, int W, int shift, int floor8,
                                                       int* __restrict__ mesh)
{
    __shared__ unsigned int bins[256];
    __shared__ unsigned int wsum[SG_WAVES];
    __shared__ int sel[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int mx = gridDim.x, my = gridDim.y, b = blockIdx.z;
    const int x0 = blockIdx.x << shift, y0 = blockIdx.y << shift;
    const int tw = ((int)blockIdx.x == mx - 1 ? W : x0 + (1 << shift)) - x0, th = ((int)blockIdx.y == my - 1 ? H : y0 + (1 << shift)) - y0;
    const int N = tw * th, rank = (N - 1) >> 1;
    const PIX* img = image + ((size_t)b * H * W + (size_t)y0 * W + x0) * C + ch;
    const bool in_regs = N <= NS_REG * SG_THREADS;      // the whole workgroup decides alike
    int reg[NS_REG];
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < NS_REG; ++k) {
            const int i = k * SG_THREADS + t;
            reg[k] = i < N ? (int)img[((size_t)(i / tw) * W + i % tw) * C] : 0;
        }
    }
    // f(value, valid) on every pixel of the tile, called by whole waves
    auto each = [&](auto&& f) {
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < NS_REG; ++k) {
                if (k * SG_THREADS >= N) break;
                f(reg[k], k * SG_THREADS + t < N);
            }
        } else {
            for (int y = wave; y < th; y += SG_WAVES)
                for (int xb = 0; xb < tw; xb += 64) {
                    const bool in = xb + lane < tw;
                    f(in ? (int)img[((size_t)y * W + xb + lane) * C] : 0, in);
                }
        }
    };
    // the value of `rank` among |x - centre| (centre < 0: among x itself)
    auto select = [&](int centre) {
        auto key = [&](int v) { return centre < 0 ? v : abs(v - centre); };
        int hi = 0, r = rank;
        if (sizeof(PIX) > 1) {
            bins[t] = 0u;
            __syncthreads();
            each([&](int v, bool ok) { hist_add(bins, key(v) >> 8, ok); });
            __syncthreads();
            ns_find(bins, r, sel, wsum);
            hi = sel[0]; r = sel[1];
            __syncthreads();                            // sel is read before the next ns_find writes it
        }
        bins[t] = 0u;
        __syncthreads();
        each([&](int v, bool ok) {
            const int q = key(v);
            hist_add(bins, q & 255, ok && (q >> 8) == hi);
        });
        __syncthreads();
        ns_find(bins, r, sel, wsum);
        const int lo = sel[0];
        __syncthreads();
        return (hi << 8) | lo;
    };
    const int med = select(-1);
    const int dev = select(med);
    if (t == 0) {
        const size_t node = ((size_t)b * 2 * my + blockIdx.y) * mx + blockIdx.x;
        mesh[node] = 256 * med;
        mesh[node + (size_t)my * mx] = max((int)(((long long)dev * NS_MAD_Q16) >> 8), floor8);
    }
}

// grid (ceil(my * mx / 256), 2, B): raw and out are [B][2][my][mx]
__global__ __launch_bounds__(SG_THREADS) void ns_filter(const int* __restrict__ raw, int my, int mx, int* __restrict__ out)
{
    const int n = blockIdx.x * SG_THREADS + threadIdx.x;
    if (n >= my * mx) return;
    const int j = n / mx, i = n % mx;
    const size_t base = ((size_t)blockIdx.z * 2 + blockIdx.y) * my * mx;
    int v[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            v[(dy + 1) * 3 + dx + 1] = raw[base + (size_t)min(max(j + dy, 0), my - 1) * mx + min(max(i + dx, 0), mx - 1)];
    // the fifth of nine: Paeth's network of 19 exchanges
#define NS_SORT2(a, b) { const int lo_ = min(v[a], v[b]), hi_ = max(v[a], v[b]); v[a] = lo_; v[b] = hi_; }
    NS_SORT2(1, 2) NS_SORT2(4, 5) NS_SORT2(7, 8) NS_SORT2(0, 1) NS_SORT2(3, 4) NS_SORT2(6, 7) NS_SORT2(1, 2) NS_SORT2(4, 5)
    NS_SORT2(7, 8) NS_SORT2(0, 3) NS_SORT2(5, 8) NS_SORT2(4, 7) NS_SORT2(3, 6) NS_SORT2(1, 4) NS_SORT2(2, 5) NS_SORT2(4, 7)
    NS_SORT2(4, 2) NS_SORT2(6, 4) NS_SORT2(4, 2)
#undef NS_SORT2
    out[base + n] = v[4];
}

// One axis of the interpolation at pixel p: the first of the two nodes, the second's offset (0 with a single node), w0, w1.
struct NsAxis {
    int i0, step, w0, w1;
};
__device__ inline NsAxis ns_axis(int p, int n, int m, int shift)
{
    if (m == 1) return NsAxis{0, 0, 1, 0};
    const int T = 1 << shift;
    const int i0 = min(max((2 * p - T + 1) >> (shift + 1), 0), m - 2);      // arithmetic shift: -1 left of the first centre
    const int c0 = 2 * i0 * T + T - 1;
    const int c1 = i0 + 1 == m - 1 ? (m - 1) * T + n - 1 : c0 + 2 * T;       // the last tile runs to n
    const int D = c1 - c0, w1 = min(max(2 * p - c0, 0), D);
    return NsAxis{i0, 1, D - w1, w1};
}

// grid (nchunks, B); mesh: the filtered [B][2][my][mx]; weak8 < 0: a 0 / 1 plane, else levels 0 / 1 / 2
template <typename PIX>
__global__ __launch_bounds__(SG_THREADS) void ns_cut(const PIX* __restrict__ image, int C, int ch, int H, int W, int shift, int my, int mx,
                                                     const int* __restrict__ mesh, int k8, int weak8, unsigned char* __restrict__ out)
{
    const int b = blockIdx.y, HW = H * W;
    const PIX* img = image + (size_t)b * HW * C + ch;
    const int* mB = mesh + (size_t)b * 2 * my * mx;
    const int* mS = mB + (size_t)my * mx;
    unsigned char* o = out + (size_t)b * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const NsAxis ay = ns_axis(i / W, H, my, shift), ax = ns_axis(i % W, W, mx, shift);
        const int n00 = ay.i0 * mx + ax.i0, n01 = n00 + ax.step, n10 = n00 + ay.step * mx, n11 = n10 + ax.step;
        const long long w00 = ay.w0 * ax.w0, w01 = ay.w0 * ax.w1, w10 = ay.w1 * ax.w0, w11 = ay.w1 * ax.w1;     // each below 2^20
        const long long NB = w00 * mB[n00] + w01 * mB[n01] + w10 * mB[n10] + w11 * mB[n11];
        const long long NS = w00 * mS[n00] + w01 * mS[n01] + w10 * mS[n10] + w11 * mS[n11];
        const long long D = (long long)(ay.w0 + ay.w1) * (ax.w0 + ax.w1);
        const long long lhs = 256 * (256 * (long long)img[(size_t)i * C] * D - NB);
        const int strong = lhs > k8 * NS ? 1 : 0;
        o[i] = (unsigned char)(weak8 < 0 ? strong : strong + (lhs > weak8 * NS ? 1 : 0));
    }
}

// ---- host state (segment_internal.hpp) --------------------------------------------------------------------------------------
void segment_state_free(SegmentState* s) { delete s; }

// f(PIX()) with the pixel type of the call; f is a generic lambda
template <typename F>
static auto by_pixel(int pixel_type, F&& f)
{
    if (pixel_type == CS_PIX_U8) return f((unsigned char)0);
    return f((unsigned short)0);
}

// tile union-find, border merge, path compression (with the root counts when chunk_cnt is given); with `val` only neighbours
// of equal val are joined
static hipError_t label_mask(const unsigned char* mask, int batch, int H, int W, int invert, int conn8, int* parent, int* chunk_cnt,
                             int nchunks, hipStream_t st, const unsigned char* val = nullptr)
{
    const dim3 tgrid((unsigned)((W + SG_TW - 1) / SG_TW), (unsigned)((H + SG_TH - 1) / SG_TH), (unsigned)batch);
    if (val) hipLaunchKernelGGL(sg_tile<true>, tgrid, dim3(SG_THREADS), 0, st, mask, H, W, invert, conn8, parent, val);
    else hipLaunchKernelGGL(sg_tile<false>, tgrid, dim3(SG_THREADS), 0, st, mask, H, W, invert, conn8, parent, val);
    const int nb = ((H - 1) / SG_TH) * W + ((W - 1) / SG_TW) * H;
    if (nb > 0) {
        const dim3 bgrid((unsigned)((nb + SG_THREADS - 1) / SG_THREADS), (unsigned)batch);
        if (val) hipLaunchKernelGGL(sg_border<true>, bgrid, dim3(SG_THREADS), 0, st, H, W, conn8, parent, val);
        else hipLaunchKernelGGL(sg_border<false>, bgrid, dim3(SG_THREADS), 0, st, H, W, conn8, parent, val);
    }
    hipLaunchKernelGGL(sg_flatten, dim3((unsigned)nchunks, (unsigned)batch), dim3(SG_THREADS), 0, st, H * W, parent, chunk_cnt, nchunks);
    return hipGetLastError();
}

// returns a cs status: the histogram tables may not fit (CS_ERR_NOMEM)
template <typename PIX, int NB>
static int otsu_thresholds(const PIX* img, int C, int ch, int batch, int HW, SegmentState& S, hipStream_t st)
{
    constexpr int LB = NB < HIST_WINDOW ? NB : HIST_WINDOW;
    int parts = std::max(1, std::min(HIST_MAX_PARTS, 256 / batch));
    parts = std::max(1, std::min(parts, (HW + HIST_PART_PX - 1) / HIST_PART_PX));
    int rc;
    if ((rc = S.slab.ensure((size_t)batch * parts * NB * sizeof(unsigned int))) || (rc = S.hist.ensure((size_t)batch * NB * sizeof(unsigned int))))
        return rc;
    const size_t lds = (size_t)LB * sizeof(unsigned int);
    HIPCHK(hipFuncSetAttribute((const void*)sg_hist<PIX, NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((sg_hist<PIX, NB>), dim3((unsigned)parts, (unsigned)(NB / LB), (unsigned)batch), dim3(HIST_THREADS), lds, st, img, C, ch,
                       HW, parts, S.slab.as<unsigned int>());
    hipLaunchKernelGGL((sg_otsu<NB>), dim3((unsigned)batch), dim3(HIST_THREADS), 0, st, S.slab.as<unsigned int>(), parts,
                       S.hist.as<unsigned int>(), S.thr.as<int>());
    HIPCHK(hipGetLastError());
    return CS_OK;
}

// The argument rules of the image and of where the result goes that every entry point shares, up to the sizes; out_name is what
// the entry point calls the kind of its output.  image_limits has the rest: some entry points have rules of their own between.
static int image_check(const void* image, const void* out, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                       int32_t width, int in_kind, int out_kind, const char* out_name)
{
    if (!image || !out) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / %s must be CS_MEM_HOST or CS_MEM_DEVICE", out_name);
    if (channels < 1 || channel < 0 || channel >= channels)
        return fail(CS_ERR_INVALID, "channel %d of %d: need 0 <= channel < channels", (int)channel, (int)channels);
    return stack_dims(batch, height, width);
}

// The rules of cs_segment_params; sp receives the parameters in force.
static int segment_check(const cs_segment_params* params, cs_segment_params& sp)
{
    sp = cs_segment_params{CS_THRESH_OTSU, 0, 1, 0};
    if (params) {
        sp = *params;
        if (sp.threshold_mode != CS_THRESH_OTSU && sp.threshold_mode != CS_THRESH_FIXED)
            return fail(CS_ERR_INVALID, "threshold_mode %d: CS_THRESH_OTSU or CS_THRESH_FIXED", (int)sp.threshold_mode);
        if (sp.threshold_mode == CS_THRESH_FIXED && (sp.threshold < 0 || sp.threshold > 65535))
            return fail(CS_ERR_INVALID, "threshold %d outside 0..65535", (int)sp.threshold);
        if (sp.connectivity != 1 && sp.connectivity != 2) return fail(CS_ERR_INVALID, "connectivity %d: 1 or 2", (int)sp.connectivity);
        if (sp.fill_holes != 0 && sp.fill_holes != 1) return fail(CS_ERR_INVALID, "fill_holes %d: 0 or 1", (int)sp.fill_holes);
    }
    return CS_OK;
}

int state_begin(cs_preproc* p)
{
    HIPCHK(hipSetDevice(p->device));
    if (!p->seg) p->seg = new SegmentState();
    return CS_OK;
}

// d_img: where the image is on the device, the upload buffer for a host image
static int upload_image(SegmentState& S, const void* image, size_t bytes, int in_kind, hipStream_t st, const void*& d_img)
{
    d_img = image;
    if (in_kind == CS_MEM_HOST) {
        if (const int rc = S.img.ensure(bytes)) return rc;
        HIPCHK(hipMemcpyAsync(S.img.p, image, bytes, hipMemcpyHostToDevice, st));
        d_img = S.img.p;
    }
    return CS_OK;
}

// A call that produces a plane (background, local, clean, smooth, hysteresis): where its image and its plane are.
struct PlaneCall {
    SegmentState* S;
    hipStream_t st;
    bool on_device;                                     // image and plane are both the caller's device memory
    const void* d_img;                                  // the image on the device (null: segment_begin uploads it later)
    void* host;                                         // the caller's host plane, or null
    void* d_out;                                        // the plane on the device: the caller's pointer, or the staging plane
    size_t out_bytes;
};

// the state, the upload (image_bytes 0: none here) and the device destination of the plane
static int plane_begin(cs_preproc* p, const void* image, size_t image_bytes, int in_kind, void* out, size_t out_bytes, int out_kind,
                       PlaneCall& c)
{
    int rc;
    if ((rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    c = PlaneCall{&S, p->stream, in_kind == CS_MEM_DEVICE && out_kind == CS_MEM_DEVICE, nullptr, nullptr, out, out_bytes};
    if (image_bytes && (rc = upload_image(S, image, image_bytes, in_kind, c.st, c.d_img))) return rc;
    if (out_kind == CS_MEM_HOST) {
        if ((rc = S.stage.ensure(out_bytes))) return rc;
        c.host = out;
        c.d_out = S.stage.p;
    }
    return CS_OK;
}

// The end of such a call, its launches and the clock's last record on the stream.  thresholds: where S.thr goes, or null.
static int plane_end(const PlaneCall& c, StageClock& clk, int32_t* thresholds, int batch)
{
    if (c.on_device && !thresholds) {
        clk.pending = true;                             // no host synchronisation: the times are read when they are asked for
        return CS_OK;
    }
    if (thresholds) HIPCHK(hipMemcpyAsync(thresholds, c.S->thr.p, batch * sizeof(int), hipMemcpyDeviceToHost, c.st));
    if (c.host) HIPCHK(hipMemcpyAsync(c.host, c.d_out, c.out_bytes, hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipStreamSynchronize(c.st));                   // the one host synchronisation: the caller's host buffers are free / filled
    return clk.finish();
}

// What the labelling entry points do up to the mask: the state, the uploads, the common workspace, the thresholds, the mask
// (between the clock's events 0 and 1) and the hole filling.  d_img / d_lab are where the image and the labels are on the device.
struct SegmentCall {
    int batch, H, W, HW, nchunks;
    size_t npx;
    int* d_lab;
    dim3 pgrid;
    const void* d_img;
};

// the state, the uploads and the common workspace
static int segment_begin(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t batch, int32_t height, int32_t width,
                         int in_kind, int32_t* labels, int labels_kind, SegmentCall& c)
{
    int rc;
    if ((rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    const int H = height, W = width, HW = H * W;
    const size_t npx = (size_t)batch * HW;
    const int nchunks = (HW + SG_CHUNK - 1) / SG_CHUNK;
    const void* d_img;
    if ((rc = upload_image(S, image, npx * channels * (pixel_type == CS_PIX_U8 ? 1 : 2), in_kind, p->stream, d_img))) return rc;
    int* d_lab = labels;
    if (labels_kind == CS_MEM_HOST) {
        if ((rc = S.lab.ensure(npx * sizeof(int)))) return rc;
        d_lab = S.lab.as<int>();
    }
    if ((rc = S.mask.ensure(npx)) || (rc = S.parent.ensure(npx * sizeof(int))) || (rc = S.thr.ensure(batch * sizeof(int))) ||
        (rc = S.chunks.ensure((size_t)batch * nchunks * sizeof(int))) || (rc = S.counts.ensure(batch * sizeof(int))))
        return rc;
    c = SegmentCall{(int)batch, H, W, HW, nchunks, npx, d_lab, dim3((unsigned)nchunks, (unsigned)batch), d_img};
    return CS_OK;
}

// thr[b]: the fixed threshold, or Otsu's of image b
static int segment_thresholds(SegmentState& S, const SegmentCall& c, int pixel_type, int C, int channel, const cs_segment_params& sp,
                              hipStream_t st)
{
    if (sp.threshold_mode == CS_THRESH_FIXED) {
        hipLaunchKernelGGL(sg_fixed, dim3((unsigned)((c.batch + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, st, S.thr.as<int>(),
                           c.batch, (int)sp.threshold);
        HIPCHK(hipGetLastError());
        return CS_OK;
    }
    return by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        return otsu_thresholds<PIX, (sizeof(PIX) == 1 ? 256 : 65536)>((const PIX*)c.d_img, C, channel, c.batch, c.HW, S, st);
    });
}

// clk: the clock whose events 0 and 1 frame the thresholds and the mask (the state may not exist before this call), or null
static int segment_mask(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                        int32_t width, int in_kind, const cs_segment_params& sp, int32_t* labels, int labels_kind, SegmentCall& c,
                        StageClock SegmentState::*which)
{
    int rc;
    if ((rc = segment_begin(p, image, pixel_type, channels, batch, height, width, in_kind, labels, labels_kind, c))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = c.H, W = c.W, HW = c.HW, C = channels, nchunks = c.nchunks;
    const size_t npx = c.npx;
    int* d_lab = c.d_lab;
    const dim3 pgrid = c.pgrid;
    StageClock* clk = which ? &(S.*which) : nullptr;

    if (clk && (rc = clk->record(0, st))) return rc;
    if ((rc = segment_thresholds(S, c, pixel_type, C, channel, sp, st))) return rc;
    by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        hipLaunchKernelGGL(sg_mask<PIX>, pgrid, dim3(SG_THREADS), 0, st, (const PIX*)c.d_img, C, (int)channel, HW, S.thr.as<int>(),
                           S.mask.as<unsigned char>());
    });
    HIPCHK(hipGetLastError());
    if (clk && (rc = clk->record(1, st))) return rc;

    if (sp.fill_holes) {
        // background components, 4-connected; the label buffer holds the "touches the image border" flags meanwhile
        HIPCHK(hipMemsetAsync(d_lab, 0, npx * sizeof(int), st));
        HIPCHK(label_mask(S.mask.as<unsigned char>(), batch, H, W, 1, 0, S.parent.as<int>(), nullptr, nchunks, st));
        hipLaunchKernelGGL(sg_edge, dim3((unsigned)((2 * W + 2 * H + SG_THREADS - 1) / SG_THREADS), (unsigned)batch), dim3(SG_THREADS), 0, st, H,
                           W, S.parent.as<int>(), d_lab);
        hipLaunchKernelGGL(sg_fill, pgrid, dim3(SG_THREADS), 0, st, HW, S.parent.as<int>(), d_lab, S.mask.as<unsigned char>());
        HIPCHK(hipGetLastError());
    }
    return CS_OK;
}

// scan of the root counts, labels of the roots, labels of the rest: from parents that point to each region's first pixel
static hipError_t number_regions(SegmentState& S, const SegmentCall& c, hipStream_t st)
{
    hipLaunchKernelGGL(sg_scan, dim3((unsigned)c.batch), dim3(HIST_THREADS), 0, st, S.chunks.as<int>(), c.nchunks, S.counts.as<int>());
    hipLaunchKernelGGL(sg_rank<false>, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, S.parent.as<int>(), S.chunks.as<int>(), c.nchunks, c.d_lab,
                       (const int*)nullptr);
    hipLaunchKernelGGL(sg_gather, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, S.parent.as<int>(), c.d_lab);
    return hipGetLastError();
}

// The channel as a stage's passes read it: pointer, image stride and pixel stride in elements.
template <typename PIX>
struct ChannelView {
    const PIX* p;
    size_t img;
    int pix;
};

// The optional 3 x 3 median of a stage, between its clock's events 0 and 1: x views the median's plane, else the channel in place.
template <typename PIX>
static int median_step(SegmentState& S, StageClock& clk, const PIX* d_img, int C, int ch, int batch, int H, int W, bool median,
                       hipStream_t st, ChannelView<PIX>& x)
{
    const int HW = H * W;
    int rc;
    x = ChannelView<PIX>{d_img + ch, (size_t)HW * C, C};
    if ((rc = clk.record(0, st))) return rc;
    if (median) {
        if ((rc = S.med.ensure((size_t)batch * HW * sizeof(PIX)))) return rc;
        hipLaunchKernelGGL(bg_median<PIX>, dim3((unsigned)((HW + SG_CHUNK - 1) / SG_CHUNK), (unsigned)batch), dim3(SG_THREADS), 0, st, d_img, C,
                           ch, H, W, S.med.as<PIX>());
        HIPCHK(hipGetLastError());
        x = ChannelView<PIX>{S.med.as<PIX>(), (size_t)HW, 1};
    }
    return clk.record(1, st, median);
}

// median (optional) and the four passes of the top-hat on the stream; d_out is a [B][H][W] plane on the device
template <typename PIX>
static int background_launch(SegmentState& S, const PIX* d_img, int C, int ch, int batch, int H, int W, int r, bool median, PIX* d_out,
                             hipStream_t st)
{
    const int HW = H * W, levels = bg_levels(r), TR = bg_col_rows(r);
    const size_t plane = (size_t)batch * HW * sizeof(PIX);
    int rc;
    if ((rc = S.bg_a.ensure(plane)) || (rc = S.bg_b.ensure(plane))) return rc;
    ChannelView<PIX> x;                                 // what the opening is subtracted from
    if ((rc = median_step(S, S.clk_bg, d_img, C, ch, batch, H, W, median, st, x))) return rc;
    PIX *A = S.bg_a.as<PIX>(), *B = S.bg_b.as<PIX>();
    const dim3 rgrid((unsigned)((W + BG_ROW_SEG - 1) / BG_ROW_SEG), (unsigned)((H + BG_ROW_LINES - 1) / BG_ROW_LINES), (unsigned)batch);
    const dim3 cgrid((unsigned)((W + BG_COL_W - 1) / BG_COL_W), (unsigned)((H + TR - 1) / TR), (unsigned)batch);
    const size_t lds = (size_t)(std::min(TR, H) + 2 * r) * BG_COL_W * sizeof(unsigned short);
    HIPCHK(hipFuncSetAttribute((const void*)bg_cols<PIX, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipFuncSetAttribute((const void*)bg_cols<PIX, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((bg_rows<PIX, false, false>), rgrid, dim3(SG_THREADS), 0, st, x.p, x.img, x.pix, H, W, r, levels, (const PIX*)nullptr,
                       (size_t)0, 0, A);
    hipLaunchKernelGGL((bg_cols<PIX, false>), cgrid, dim3(BG_COL_THREADS), lds, st, (const PIX*)A, H, W, r, levels, TR, B);
    hipLaunchKernelGGL((bg_cols<PIX, true>), cgrid, dim3(BG_COL_THREADS), lds, st, (const PIX*)B, H, W, r, levels, TR, A);
    hipLaunchKernelGGL((bg_rows<PIX, true, true>), rgrid, dim3(SG_THREADS), 0, st, (const PIX*)A, (size_t)HW, 1, H, W, r, levels, x.p, x.img,
                       x.pix, d_out);
    HIPCHK(hipGetLastError());
    return S.clk_bg.record(2, st);
}

// median (optional), row sums, column sums + compare on the stream; d_out is a [B][H][W] uint8 plane on the device: 0 / 1, or
// with weak_delta (cs_segment_hysteresis) the levels 0 / 1 / 2 under that delta and lp.delta
template <typename PIX>
static int local_launch(SegmentState& S, const PIX* d_img, int C, int ch, int batch, int H, int W, const cs_local_params& lp,
                        unsigned char* d_out, hipStream_t st, const int32_t* weak_delta = nullptr)
{
    const int HW = H * W, r = lp.radius, TR = bg_col_rows(r);
    int rc;
    if ((rc = S.lt_sum.ensure((size_t)batch * HW * sizeof(unsigned int)))) return rc;
    ChannelView<PIX> x;                                 // both sides of the comparison read this
    if ((rc = median_step(S, S.clk_lt, d_img, C, ch, batch, H, W, lp.median != 0, st, x))) return rc;
    const dim3 rgrid((unsigned)((W + LT_ROW_SEG - 1) / LT_ROW_SEG), (unsigned)((H + LT_ROW_LINES - 1) / LT_ROW_LINES), (unsigned)batch);
    const dim3 cgrid((unsigned)((W + LT_COL_W - 1) / LT_COL_W), (unsigned)((H + LT_COL_TILES * TR - 1) / (LT_COL_TILES * TR)), (unsigned)batch);
    const long long n = (long long)(2 * r + 1) * (2 * r + 1);
    hipLaunchKernelGGL(lt_rows<PIX>, rgrid, dim3(SG_THREADS), 0, st, x.p, x.img, x.pix, H, W, r, S.lt_sum.as<unsigned int>());
    if (weak_delta)
        hipLaunchKernelGGL((lt_cols<PIX, true>), cgrid, dim3(SG_THREADS), 0, st, (const unsigned int*)S.lt_sum.as<unsigned int>(), x.p, x.img,
                           x.pix, H, W, r, TR, n, n * lp.delta, n * *weak_delta, (int)lp.floor, d_out);
    else
        hipLaunchKernelGGL((lt_cols<PIX, false>), cgrid, dim3(SG_THREADS), 0, st, (const unsigned int*)S.lt_sum.as<unsigned int>(), x.p, x.img,
                           x.pix, H, W, r, TR, n, n * lp.delta, 0ll, (int)lp.floor, d_out);
    HIPCHK(hipGetLastError());
    return S.clk_lt.record(2, st);
}

static int local_check(const cs_local_params& lp)
{
    if (lp.radius < 1 || lp.radius > LT_MAX_R) return fail(CS_ERR_INVALID, "local radius %d outside 1..%d", (int)lp.radius, LT_MAX_R);
    if (lp.delta < -65535 || lp.delta > 65535) return fail(CS_ERR_INVALID, "local delta %d outside -65535..65535", (int)lp.delta);
    if (lp.floor < -1 || lp.floor > 65535) return fail(CS_ERR_INVALID, "local floor %d outside -1..65535", (int)lp.floor);
    if (lp.median != 0 && lp.median != 1) return fail(CS_ERR_INVALID, "median %d: 0 or 1", (int)lp.median);
    return CS_OK;
}

// median (optional), row pass, column pass on the stream; d_out is a [B][H][W] plane on the device
template <typename PIX>
static int smooth_launch(SegmentState& S, const PIX* d_img, int C, int ch, int batch, int H, int W, const SmWeights& wt, bool median,
                         PIX* d_out, hipStream_t st)
{
    const int HW = H * W, r = wt.r;
    int rc;
    if ((rc = S.sm_t.ensure((size_t)batch * HW * sizeof(unsigned int)))) return rc;
    ChannelView<PIX> x;
    if ((rc = median_step(S, S.clk_sm, d_img, C, ch, batch, H, W, median, st, x))) return rc;
    const dim3 rgrid((unsigned)((W + SM_ROW_SEG - 1) / SM_ROW_SEG), (unsigned)((H + SM_ROW_LINES - 1) / SM_ROW_LINES), (unsigned)batch);
    const dim3 cgrid((unsigned)((W + SM_COL_W - 1) / SM_COL_W), (unsigned)((H + SM_COL_TR - 1) / SM_COL_TR), (unsigned)batch);
    const size_t lds = (size_t)(std::min(SM_COL_TR, H) + 2 * r + SM_COL_E) * SM_COL_W * sizeof(unsigned int);
    HIPCHK(hipFuncSetAttribute((const void*)sm_cols<PIX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(sm_rows<PIX>, rgrid, dim3(SG_THREADS), 0, st, x.p, x.img, x.pix, H, W, wt, S.sm_t.as<unsigned int>());
    hipLaunchKernelGGL(sm_cols<PIX>, cgrid, dim3(SG_THREADS), lds, st, (const unsigned int*)S.sm_t.as<unsigned int>(), H, W, wt, d_out);
    HIPCHK(hipGetLastError());
    return S.clk_sm.record(2, st);
}

// the table rules of cs_smooth_params; wt receives the table in force
static int smooth_check(const cs_smooth_params& sp, SmWeights& wt)
{
    if (sp.radius < 1 || sp.radius > SM_MAX_R) return fail(CS_ERR_INVALID, "smooth radius %d outside 1..%d", (int)sp.radius, SM_MAX_R);
    if (sp.median != 0 && sp.median != 1) return fail(CS_ERR_INVALID, "median %d: 0 or 1", (int)sp.median);
    if (sp.reserved != 0) return fail(CS_ERR_INVALID, "cs_smooth_params.reserved must be 0");
    long long sum = 0;
    for (int k = 0; k <= SM_MAX_R; ++k) {
        const int32_t w = sp.weights[k];
        if (w < 0) return fail(CS_ERR_INVALID, "weights[%d] = %d: negative", k, (int)w);
        if (k > sp.radius && w != 0) return fail(CS_ERR_INVALID, "weights[%d] = %d beyond radius %d", k, (int)w, (int)sp.radius);
        sum += k ? 2ll * w : (long long)w;
        wt.w[k] = (unsigned int)w;
    }
    if (sp.weights[0] < 1) return fail(CS_ERR_INVALID, "weights[0] = %d: the centre tap must be at least 1", (int)sp.weights[0]);
    if (sum != 65536) return fail(CS_ERR_INVALID, "weights[0] + 2 * sum(weights[1..radius]) = %lld, not 65536", sum);
    wt.r = sp.radius;
    return CS_OK;
}

// The workspace of the two splits beyond segment_mask's: heights, reconstruction, keys, tile tops, control words.
struct SplitCall {
    dim3 tgrid;
    size_t ntiles;
};

static int split_workspace(SegmentState& S, const SegmentCall& c, SplitCall& w)
{
    w.tgrid = dim3((unsigned)((c.W + SG_TW - 1) / SG_TW), (unsigned)((c.H + SG_TH - 1) / SG_TH), (unsigned)c.batch);
    w.ntiles = (size_t)w.tgrid.x * w.tgrid.y * w.tgrid.z;
    int rc;
    if ((rc = S.dq.ensure(c.npx)) || (rc = S.rec.ensure(c.npx)) || (rc = S.key.ensure(c.npx * sizeof(unsigned long long))) ||
        (rc = S.ttop.ensure(w.ntiles)) || (rc = S.ctrl.ensure(CT_N * sizeof(int))))
        return rc;
    return CS_OK;
}

// What cs_segment_split and cs_segment_split_intensity share once the height plane (S.dq), the marker (S.rec) and the batch's
// largest height (ctrl[CT_VMAX]) are on the stream: the clock's event 2, the reconstruction, the seeds, the flood, the numbering,
// the copies out, the one final synchronisation and the clock's four spans.  dist: the optional copy of S.dq.
static int split_watershed(SegmentState& S, const SegmentCall& c, const SplitCall& w, int conn8, hipStream_t st, int32_t* labels,
                           int labels_kind, int32_t* n_labels, int32_t* thresholds, uint8_t* dist, StageClock& clk)
{
    const int H = c.H, W = c.W, HW = c.HW;
    const dim3 tgrid = w.tgrid;
    const size_t ntiles = w.ntiles;
    unsigned char *mask = S.mask.as<unsigned char>(), *dq = S.dq.as<unsigned char>(), *rec = S.rec.as<unsigned char>();
    unsigned long long* key = S.key.as<unsigned long long>();
    int *ctrl = S.ctrl.as<int>(), *parent = S.parent.as<int>();
    const dim3 one(1);
    int rc;
    if ((rc = clk.record(2, st))) return rc;

    // h-maxima: reconstruction in rounds, read back once per group of rounds; the bound of HW rounds never binds in practice
    hipLaunchKernelGGL(sp_start, one, one, 0, st, ctrl, 0);
    S.sp_recon_reads = S.sp_flood_reads = 0;
    for (int active = 1; active; ++S.sp_recon_reads) {
        for (int r = 0; r < SP_RECON_GROUP; ++r) {
            hipLaunchKernelGGL(sp_recon, tgrid, dim3(SG_THREADS), 0, st, dq, H, W, conn8, rec, ctrl);
            hipLaunchKernelGGL(sp_advance_recon, one, one, 0, st, ctrl, HW);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&active, ctrl + CT_ACTIVE, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // seeds: plateaus of equal R, those without a higher neighbour, ranked; the flags live in the key buffer, the ids in the labels
    int* drop = (int*)key;
    HIPCHK(hipMemsetAsync(drop, 0, c.npx * sizeof(int), st));
    HIPCHK(label_mask(mask, c.batch, H, W, 0, conn8, parent, nullptr, c.nchunks, st, rec));
    hipLaunchKernelGGL(sp_higher, c.pgrid, dim3(SG_THREADS), 0, st, H, W, conn8, rec, parent, drop);
    hipLaunchKernelGGL(sp_seedcount, c.pgrid, dim3(SG_THREADS), 0, st, HW, parent, drop, S.chunks.as<int>(), c.nchunks);
    hipLaunchKernelGGL(sg_scan, dim3((unsigned)c.batch), dim3(HIST_THREADS), 0, st, S.chunks.as<int>(), c.nchunks, S.counts.as<int>());
    hipLaunchKernelGGL(sg_rank<true>, c.pgrid, dim3(SG_THREADS), 0, st, HW, parent, S.chunks.as<int>(), c.nchunks, c.d_lab, (const int*)drop);
    hipLaunchKernelGGL(sp_seedkey, c.pgrid, dim3(SG_THREADS), 0, st, HW, parent, c.d_lab, key);
    HIPCHK(hipGetLastError());
    if ((rc = clk.record(3, st))) return rc;

    // flood, level by level from the batch's largest Dq; then each region's first pixel and the numbering
    HIPCHK(hipMemsetAsync(S.ttop.p, 0xff, ntiles, st));
    hipLaunchKernelGGL(sp_start, one, one, 0, st, ctrl, 1);
    for (int level = 1; level >= 1; ++S.sp_flood_reads) {
        for (int r = 0; r < SP_FLOOD_GROUP; ++r) {
            hipLaunchKernelGGL(sp_flood, tgrid, dim3(SG_THREADS), 0, st, dq, H, W, conn8, key, S.ttop.as<unsigned char>(), ctrl);
            hipLaunchKernelGGL(sp_advance_flood, one, one, 0, st, ctrl, HW);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&level, ctrl + CT_LEVEL, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipMemsetAsync(c.d_lab, 0x7f, c.npx * sizeof(int), st));
    hipLaunchKernelGGL(sp_first, c.pgrid, dim3(SG_THREADS), 0, st, HW, key, c.d_lab);
    hipLaunchKernelGGL(sp_parent, c.pgrid, dim3(SG_THREADS), 0, st, HW, key, c.d_lab, parent, S.chunks.as<int>(), c.nchunks);
    HIPCHK(hipGetLastError());
    HIPCHK(number_regions(S, c, st));
    if ((rc = clk.record(4, st))) return rc;
    HIPCHK(hipMemcpyAsync(n_labels, S.counts.p, c.batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (thresholds) HIPCHK(hipMemcpyAsync(thresholds, S.thr.p, c.batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (labels_kind == CS_MEM_HOST) HIPCHK(hipMemcpyAsync(labels, c.d_lab, c.npx * sizeof(int), hipMemcpyDeviceToHost, st));
    if (dist) HIPCHK(hipMemcpyAsync(dist, dq, c.npx, labels_kind == CS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return clk.finish();
}

// component ranges and heights of the mask in S.mask under the guide, on the stream: S.dq, S.rec and ctrl[CT_VMAX] as sp_rows
// leaves them.  The two range planes are the halves of the key buffer.
template <typename PIX>
static hipError_t heights_launch(SegmentState& S, const SegmentCall& c, const PIX* d_guide, int C, int ch, int depth, int min_contrast,
                                 hipStream_t st)
{
    int *lo = S.key.as<int>(), *hi = lo + c.npx;
    hipLaunchKernelGGL(si_range<PIX>, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, S.parent.as<const int>(), d_guide, C, ch, lo, hi);
    hipLaunchKernelGGL(si_height<PIX>, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, S.parent.as<const int>(), d_guide, C, ch, (const int*)lo,
                       (const int*)hi, depth, min_contrast, S.dq.as<unsigned char>(), S.rec.as<unsigned char>(), S.ctrl.as<int>());
    return hipGetLastError();
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_segment_threshold(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                         int32_t width, int in_kind, const cs_segment_params* params, int32_t* labels, int labels_kind, int32_t* n_labels,
                         int32_t* thresholds)
{
    if (!n_labels) return fail(CS_ERR_INVALID, "NULL argument");
    cs_segment_params sp;
    int rc;
    if ((rc = image_check(image, labels, pixel_type, channels, channel, batch, height, width, in_kind, labels_kind, "labels_kind")) ||
        (rc = image_limits(batch, height, width)) || (rc = segment_check(params, sp)) || (rc = handle_check(p)))
        return rc;
    SegmentCall c;
    if ((rc = segment_mask(p, image, pixel_type, channels, channel, batch, height, width, in_kind, sp, labels, labels_kind, c,
                           &SegmentState::clk_thr)))
        return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    HIPCHK(label_mask(S.mask.as<unsigned char>(), batch, c.H, c.W, 0, sp.connectivity == 2, S.parent.as<int>(), S.chunks.as<int>(), c.nchunks, st));
    HIPCHK(number_regions(S, c, st));
    if ((rc = S.clk_thr.record(2, st))) return rc;
    HIPCHK(hipMemcpyAsync(n_labels, S.counts.p, batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (thresholds) HIPCHK(hipMemcpyAsync(thresholds, S.thr.p, batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (labels_kind == CS_MEM_HOST) HIPCHK(hipMemcpyAsync(labels, c.d_lab, c.npx * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the counts
    return S.clk_thr.finish();
}

int cs_segment_last_timing(const cs_preproc* p, double* threshold_ms, double* label_ms)
{
    return clock_read(p, &SegmentState::clk_thr, {threshold_ms, label_ms});
}

int cs_segment_split(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                     int32_t width, int in_kind, const cs_segment_params* params, const cs_split_params* split, int32_t* labels,
                     int labels_kind, int32_t* n_labels, int32_t* thresholds, uint8_t* dist)
{
    if (!n_labels) return fail(CS_ERR_INVALID, "NULL argument");
    cs_segment_params sp;
    int rc;
    if ((rc = image_check(image, labels, pixel_type, channels, channel, batch, height, width, in_kind, labels_kind, "labels_kind")) ||
        (rc = image_limits(batch, height, width)) || (rc = segment_check(params, sp)))
        return rc;
    const int h = split ? (int)split->h : 3;
    if (h < 1 || h > 255) return fail(CS_ERR_INVALID, "split h %d outside 1..255 (half pixels)", h);
    if ((rc = handle_check(p))) return rc;
    SegmentCall c;
    if ((rc = segment_mask(p, image, pixel_type, channels, channel, batch, height, width, in_kind, sp, labels, labels_kind, c,
                           &SegmentState::clk_sp)))
        return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = c.H, W = c.W;
    SplitCall w;
    if ((rc = split_workspace(S, c, w))) return rc;

    // distances: the column distances live in the key buffer, which the flood fills only later
    HIPCHK(hipMemsetAsync(S.ctrl.p, 0, CT_N * sizeof(int), st));
    hipLaunchKernelGGL(sp_columns, dim3((unsigned)((W + SG_THREADS - 1) / SG_THREADS), (unsigned)batch), dim3(SG_THREADS), 0, st,
                       S.mask.as<unsigned char>(), H, W, S.key.as<unsigned char>());
    hipLaunchKernelGGL(sp_rows, dim3((unsigned)((W + SP_ROW - 1) / SP_ROW), (unsigned)H, (unsigned)batch), dim3(SG_THREADS), 0, st,
                       S.key.as<const unsigned char>(), H, W, h, S.dq.as<unsigned char>(), S.rec.as<unsigned char>(), S.ctrl.as<int>());
    HIPCHK(hipGetLastError());
    return split_watershed(S, c, w, sp.connectivity == 2, st, labels, labels_kind, n_labels, thresholds, dist, S.clk_sp);
}

int cs_segment_split_last_timing(const cs_preproc* p, double* threshold_ms, double* distance_ms, double* seed_ms, double* flood_ms)
{
    return clock_read(p, &SegmentState::clk_sp, {threshold_ms, distance_ms, seed_ms, flood_ms});
}

int cs_segment_split_intensity(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch,
                               int32_t height_px, int32_t width, int in_kind, const cs_segment_params* params,
                               const cs_split_intensity_params* split, const void* guide, int guide_pixel_type, int32_t guide_channels,
                               int32_t guide_channel, int32_t* labels, int labels_kind, int32_t* n_labels, int32_t* thresholds,
                               uint8_t* height)
{
    if (!n_labels) return fail(CS_ERR_INVALID, "NULL argument");
    cs_segment_params sp;
    int rc;
    if ((rc = image_check(image, labels, pixel_type, channels, channel, batch, height_px, width, in_kind, labels_kind, "labels_kind")) ||
        (rc = image_limits(batch, height_px, width)) || (rc = segment_check(params, sp)))
        return rc;
    if (!split || !guide) return fail(CS_ERR_INVALID, "NULL argument");
    if (split->depth < 1 || split->depth > 254) return fail(CS_ERR_INVALID, "split depth %d outside 1..254 (levels)", (int)split->depth);
    if (split->min_contrast < 0 || split->min_contrast > 65535)
        return fail(CS_ERR_INVALID, "split min_contrast %d outside 0..65535 (counts)", (int)split->min_contrast);
    if (split->reserved[0] != 0 || split->reserved[1] != 0) return fail(CS_ERR_INVALID, "reserved must be 0");
    if (guide_pixel_type != CS_PIX_U8 && guide_pixel_type != CS_PIX_U16)
        return fail(CS_ERR_INVALID, "guide_pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (guide_channels < 1 || guide_channel < 0 || guide_channel >= guide_channels)
        return fail(CS_ERR_INVALID, "guide channel %d of %d: need 0 <= channel < channels", (int)guide_channel, (int)guide_channels);
    if ((rc = handle_check(p))) return rc;
    SegmentCall c;
    if ((rc = segment_mask(p, image, pixel_type, channels, channel, batch, height_px, width, in_kind, sp, labels, labels_kind, c,
                           &SegmentState::clk_si)))
        return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    SplitCall w;
    if ((rc = split_workspace(S, c, w))) return rc;
    const void* d_guide = guide;
    if (in_kind == CS_MEM_HOST) {
        if (guide == image && guide_pixel_type == pixel_type && guide_channels == channels) d_guide = S.img.p;     // uploaded already
        else {
            const size_t bytes = c.npx * guide_channels * (guide_pixel_type == CS_PIX_U8 ? 1 : 2);
            if ((rc = S.si_guide.ensure(bytes))) return rc;
            HIPCHK(hipMemcpyAsync(S.si_guide.p, guide, bytes, hipMemcpyHostToDevice, st));
            d_guide = S.si_guide.p;
        }
    }
    // components of the mask (no numbering yet: the parents are free again before the plateaus need them), their ranges, heights
    const int conn8 = sp.connectivity == 2;
    HIPCHK(hipMemsetAsync(S.ctrl.p, 0, CT_N * sizeof(int), st));
    HIPCHK(hipMemsetAsync(S.key.p, 0x7f, c.npx * sizeof(int), st));
    HIPCHK(hipMemsetAsync(S.key.as<int>() + c.npx, 0, c.npx * sizeof(int), st));
    HIPCHK(label_mask(S.mask.as<unsigned char>(), batch, c.H, c.W, 0, conn8, S.parent.as<int>(), nullptr, c.nchunks, st));
    HIPCHK(by_pixel(guide_pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        return heights_launch(S, c, (const PIX*)d_guide, (int)guide_channels, (int)guide_channel, (int)split->depth, (int)split->min_contrast, st);
    }));
    return split_watershed(S, c, w, conn8, st, labels, labels_kind, n_labels, thresholds, height, S.clk_si);
}

int cs_segment_split_intensity_last_timing(const cs_preproc* p, double* threshold_ms, double* height_ms, double* seed_ms, double* flood_ms)
{
    return clock_read(p, &SegmentState::clk_si, {threshold_ms, height_ms, seed_ms, flood_ms});
}

int cs_segment_split_last_syncs(const cs_preproc* p, int32_t* reconstruction, int32_t* flood)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    const SegmentState* S = p->seg;
    if (reconstruction) *reconstruction = S ? S->sp_recon_reads : 0;
    if (flood) *flood = S ? S->sp_flood_reads : 0;
    return CS_OK;
}

int cs_segment_background(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                          int32_t width, int in_kind, const cs_background_params* params, void* out, int out_kind)
{
    if (!params) return fail(CS_ERR_INVALID, "NULL argument");
    int rc;
    if ((rc = image_check(image, out, pixel_type, channels, channel, batch, height, width, in_kind, out_kind, "out_kind"))) return rc;
    if (params->radius < 1 || params->radius > BG_MAX_R) return fail(CS_ERR_INVALID, "background radius %d outside 1..%d", (int)params->radius, BG_MAX_R);
    if (params->median != 0 && params->median != 1) return fail(CS_ERR_INVALID, "median %d: 0 or 1", (int)params->median);
    if ((rc = image_limits(batch, height, width)) || (rc = handle_check(p))) return rc;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2, npx = (size_t)batch * height * width;
    PlaneCall c;
    if ((rc = plane_begin(p, image, npx * channels * esz, in_kind, out, npx * esz, out_kind, c))) return rc;
    rc = by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        return background_launch(*c.S, (const PIX*)c.d_img, channels, channel, batch, height, width, params->radius, params->median != 0,
                                 (PIX*)c.d_out, c.st);
    });
    return rc ? rc : plane_end(c, c.S->clk_bg, nullptr, batch);
}

int cs_segment_background_last_timing(const cs_preproc* p, double* median_ms, double* tophat_ms)
{
    return clock_read(p, &SegmentState::clk_bg, {median_ms, tophat_ms});
}

int cs_segment_local(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                     int32_t width, int in_kind, const cs_local_params* params, uint8_t* out, int out_kind)
{
    if (!params) return fail(CS_ERR_INVALID, "NULL argument");
    int rc;
    if ((rc = image_check(image, out, pixel_type, channels, channel, batch, height, width, in_kind, out_kind, "out_kind")) ||
        (rc = local_check(*params)) || (rc = image_limits(batch, height, width)) || (rc = handle_check(p)))
        return rc;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2, npx = (size_t)batch * height * width;
    PlaneCall c;
    if ((rc = plane_begin(p, image, npx * channels * esz, in_kind, out, npx, out_kind, c))) return rc;
    rc = by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        return local_launch(*c.S, (const PIX*)c.d_img, channels, channel, batch, height, width, *params, (unsigned char*)c.d_out, c.st);
    });
    return rc ? rc : plane_end(c, c.S->clk_lt, nullptr, batch);
}

int cs_segment_local_last_timing(const cs_preproc* p, double* median_ms, double* sum_ms)
{
    return clock_read(p, &SegmentState::clk_lt, {median_ms, sum_ms});
}

int cs_segment_clean(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                     int32_t width, int in_kind, const cs_segment_params* params, const cs_clean_params* clean, uint8_t* out, int out_kind,
                     int32_t* thresholds)
{
    if (!clean) return fail(CS_ERR_INVALID, "NULL argument");
    cs_segment_params sp;
    int rc;
    if ((rc = image_check(image, out, pixel_type, channels, channel, batch, height, width, in_kind, out_kind, "labels_kind")) ||
        (rc = image_limits(batch, height, width)) || (rc = segment_check(params, sp)))
        return rc;
    const int r = clean->open_radius, k = clean->open_connectivity, a = clean->min_area;
    if (r < 0 || r > CL_MAX_R) return fail(CS_ERR_INVALID, "open_radius %d outside 0..%d (0: no opening)", r, CL_MAX_R);
    if (k != 1 && k != 2) return fail(CS_ERR_INVALID, "open_connectivity %d: 1 (cross) or 2 (square)", k);
    if (a < 0 || a > CL_MAX_AREA) return fail(CS_ERR_INVALID, "min_area %d outside 0..%d (0: no area step)", a, CL_MAX_AREA);
    if (r == 0 && a == 0) return fail(CS_ERR_INVALID, "open_radius and min_area are both 0: nothing to clean");
    if ((rc = handle_check(p))) return rc;
    // segment_mask uploads a host image, after the clock's first event: the upload counts as the mask's time
    PlaneCall pc;
    if ((rc = plane_begin(p, nullptr, 0, in_kind, out, (size_t)batch * height * width, out_kind, pc))) return rc;
    SegmentState& S = *pc.S;
    hipStream_t st = pc.st;
    unsigned char* d_out = (unsigned char*)pc.d_out;
    if ((rc = S.clk_cl.record(0, st))) return rc;
    // the mask as the segmenter makes it; its workspace for labels that go to the host (4 bytes per pixel) holds the hole
    // filling's flags and then the pixel counts
    SegmentCall c;
    if ((rc = segment_mask(p, image, pixel_type, channels, channel, batch, height, width, in_kind, sp, nullptr, CS_MEM_HOST, c, nullptr)))
        return rc;
    if ((rc = S.clk_cl.record(1, st))) return rc;
    const unsigned char* cur = S.mask.as<unsigned char>();
    if (r > 0) {
        const dim3 ogrid((unsigned)((c.W + CL_TW - 1) / CL_TW), (unsigned)((c.H + CL_TH - 1) / CL_TH), (unsigned)batch);
        hipLaunchKernelGGL(cl_open, ogrid, dim3(SG_THREADS), 0, st, cur, c.H, c.W, r, (int)(k == 2), d_out);
        HIPCHK(hipGetLastError());
        cur = d_out;
    }
    if ((rc = S.clk_cl.record(2, st, r > 0))) return rc;
    if (a > 0) {
        HIPCHK(hipMemsetAsync(c.d_lab, 0, c.npx * sizeof(int), st));
        HIPCHK(label_mask(cur, batch, c.H, c.W, 0, sp.connectivity == 2, S.parent.as<int>(), nullptr, c.nchunks, st));
        hipLaunchKernelGGL(cl_count, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, (const int*)S.parent.as<int>(), c.d_lab);
        hipLaunchKernelGGL(cl_drop, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, (const int*)S.parent.as<int>(), (const int*)c.d_lab, a, d_out);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_cl.record(3, st, a > 0))) return rc;
    return plane_end(pc, S.clk_cl, thresholds, batch);
}

int cs_segment_clean_last_timing(const cs_preproc* p, double* mask_ms, double* open_ms, double* area_ms)
{
    return clock_read(p, &SegmentState::clk_cl, {mask_ms, open_ms, area_ms});
}

int cs_segment_hysteresis(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch,
                          int32_t height, int32_t width, int in_kind, const cs_segment_params* params, const cs_local_params* local,
                          const cs_hysteresis_params* hysteresis, uint8_t* out, int out_kind, int32_t* thresholds)
{
    if (!hysteresis) return fail(CS_ERR_INVALID, "NULL argument");
    cs_segment_params sp;
    int rc;
    if ((rc = image_check(image, out, pixel_type, channels, channel, batch, height, width, in_kind, out_kind, "labels_kind")) ||
        (rc = image_limits(batch, height, width)) || (rc = segment_check(params, sp)))
        return rc;
    const int mode = hysteresis->mode, weak = hysteresis->weak;
    if (mode != CS_WEAK_ABSOLUTE && mode != CS_WEAK_FRACTION && mode != CS_WEAK_LOCAL)
        return fail(CS_ERR_INVALID, "hysteresis mode %d: CS_WEAK_ABSOLUTE, CS_WEAK_FRACTION or CS_WEAK_LOCAL", mode);
    if (hysteresis->reserved[0] != 0 || hysteresis->reserved[1] != 0) return fail(CS_ERR_INVALID, "cs_hysteresis_params.reserved must be 0");
    if (mode == CS_WEAK_LOCAL) {
        if (!local) return fail(CS_ERR_INVALID, "CS_WEAK_LOCAL needs cs_local_params");
        if ((rc = local_check(*local))) return rc;
        if (weak < -65535 || weak > 65535) return fail(CS_ERR_INVALID, "weak delta %d outside -65535..65535", weak);
        if (weak > local->delta) return fail(CS_ERR_INVALID, "weak delta %d above the local delta %d", weak, (int)local->delta);
    } else {
        if (local) return fail(CS_ERR_INVALID, "cs_local_params belong to CS_WEAK_LOCAL: pass NULL");
        if (mode == CS_WEAK_ABSOLUTE) {
            if (weak < 0 || weak > 65535) return fail(CS_ERR_INVALID, "weak threshold %d outside 0..65535", weak);
            if (sp.threshold_mode == CS_THRESH_FIXED && weak > sp.threshold)
                return fail(CS_ERR_INVALID, "weak threshold %d above the threshold %d", weak, (int)sp.threshold);
        } else if (weak < 1 || weak > 65535)
            return fail(CS_ERR_INVALID, "weak fraction %d / 65536 outside 1..65535", weak);
    }
    if ((rc = handle_check(p))) return rc;
    // the workspace of a call whose labels go to the host: its 4 bytes per pixel hold the flags; segment_begin uploads a host image
    SegmentCall c;
    if ((rc = segment_begin(p, image, pixel_type, channels, batch, height, width, in_kind, nullptr, CS_MEM_HOST, c))) return rc;
    PlaneCall pc;
    if ((rc = plane_begin(p, nullptr, 0, in_kind, out, c.npx, out_kind, pc))) return rc;
    SegmentState& S = *pc.S;
    hipStream_t st = pc.st;
    unsigned char *level = S.mask.as<unsigned char>(), *d_out = (unsigned char*)pc.d_out;
    if ((rc = S.clk_hy.record(0, st))) return rc;
    if (mode == CS_WEAK_LOCAL) {
        rc = by_pixel(pixel_type, [&](auto pix) {
            using PIX = decltype(pix);
            return local_launch(S, (const PIX*)c.d_img, channels, channel, batch, c.H, c.W, *local, level, st, &weak);
        });
        if (rc) return rc;
    } else {
        if ((rc = segment_thresholds(S, c, pixel_type, channels, channel, sp, st))) return rc;
        by_pixel(pixel_type, [&](auto pix) {
            using PIX = decltype(pix);
            hipLaunchKernelGGL(hy_levels<PIX>, c.pgrid, dim3(SG_THREADS), 0, st, (const PIX*)c.d_img, (int)channels, (int)channel, c.HW,
                               (const int*)S.thr.as<int>(), (int)(mode == CS_WEAK_FRACTION), weak, level);
        });
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_hy.record(1, st))) return rc;
    HIPCHK(hipMemsetAsync(c.d_lab, 0, c.npx * sizeof(int), st));
    HIPCHK(label_mask(level, batch, c.H, c.W, 0, sp.connectivity == 2, S.parent.as<int>(), nullptr, c.nchunks, st));
    hipLaunchKernelGGL(hy_mark, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, (const unsigned char*)level, (const int*)S.parent.as<int>(), c.d_lab);
    hipLaunchKernelGGL(hy_keep, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, (const int*)S.parent.as<int>(), (const int*)c.d_lab, d_out);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_hy.record(2, st))) return rc;
    if (thresholds && mode == CS_WEAK_LOCAL)
        for (int b = 0; b < batch; ++b) thresholds[b] = -1;                 // no single number
    return plane_end(pc, S.clk_hy, mode == CS_WEAK_LOCAL ? nullptr : thresholds, batch);
}

int cs_segment_hysteresis_last_timing(const cs_preproc* p, double* level_ms, double* link_ms)
{
    return clock_read(p, &SegmentState::clk_hy, {level_ms, link_ms});
}

int cs_segment_smooth(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                      int32_t width, int in_kind, const cs_smooth_params* params, void* plane, int plane_kind)
{
    if (!params) return fail(CS_ERR_INVALID, "NULL argument");
    SmWeights wt;
    int rc;
    if ((rc = image_check(image, plane, pixel_type, channels, channel, batch, height, width, in_kind, plane_kind, "plane_kind")) ||
        (rc = smooth_check(*params, wt)) || (rc = image_limits(batch, height, width)) || (rc = handle_check(p)))
        return rc;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2, npx = (size_t)batch * height * width;
    PlaneCall c;
    if ((rc = plane_begin(p, image, npx * channels * esz, in_kind, plane, npx * esz, plane_kind, c))) return rc;
    rc = by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        return smooth_launch(*c.S, (const PIX*)c.d_img, channels, channel, batch, height, width, wt, params->median != 0, (PIX*)c.d_out, c.st);
    });
    return rc ? rc : plane_end(c, c.S->clk_sm, nullptr, batch);
}

int cs_segment_smooth_last_timing(const cs_preproc* p, double* median_ms, double* smooth_ms)
{
    return clock_read(p, &SegmentState::clk_sm, {median_ms, smooth_ms});
}

int cs_segment_noise(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                     int32_t width, int in_kind, const cs_noise_params* noise, uint8_t* out, int out_kind, int32_t* mesh)
{
    if (!noise) return fail(CS_ERR_INVALID, "NULL argument");
    int rc;
    if ((rc = image_check(image, out, pixel_type, channels, channel, batch, height, width, in_kind, out_kind, "out_kind"))) return rc;
    const int T = noise->tile, k8 = noise->k8, weak8 = noise->weak_k8, floor8 = noise->floor8;
    if (T < 16 || T > 256 || (T & (T - 1)) != 0) return fail(CS_ERR_INVALID, "noise tile %d: a power of two in 16..256", T);
    if (k8 < 1 || k8 > 16383) return fail(CS_ERR_INVALID, "noise k8 %d outside 1..16383", k8);
    if (weak8 != -1 && (weak8 < 1 || weak8 > k8)) return fail(CS_ERR_INVALID, "weak k8 %d: -1 (no weak rule) or 1..k8 = %d", weak8, k8);
    if (floor8 < 0 || floor8 > 4095 * 256) return fail(CS_ERR_INVALID, "noise floor8 %d outside 0..%d", floor8, 4095 * 256);
    if (weak8 != -1 && noise->connectivity != 1 && noise->connectivity != 2)
        return fail(CS_ERR_INVALID, "connectivity %d: 1 or 2", (int)noise->connectivity);
    if (noise->reserved[0] != 0 || noise->reserved[1] != 0 || noise->reserved[2] != 0)
        return fail(CS_ERR_INVALID, "cs_noise_params.reserved must be 0");
    if ((rc = image_limits(batch, height, width)) || (rc = handle_check(p))) return rc;
    const bool link = weak8 != -1;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2, npx = (size_t)batch * height * width;
    // with a weak rule the workspace of a labelling call whose labels go to the host: its 4 bytes per pixel hold the flags
    SegmentCall c;
    PlaneCall pc;
    if (link) {
        if ((rc = segment_begin(p, image, pixel_type, channels, batch, height, width, in_kind, nullptr, CS_MEM_HOST, c)) ||
            (rc = plane_begin(p, nullptr, 0, in_kind, out, npx, out_kind, pc)))
            return rc;
        pc.d_img = c.d_img;
    } else if ((rc = plane_begin(p, image, npx * channels * esz, in_kind, out, npx, out_kind, pc)))
        return rc;
    SegmentState& S = *pc.S;
    hipStream_t st = pc.st;
    const int H = height, W = width;
    int shift = 4;
    while ((1 << shift) < T) ++shift;
    const int my = std::max(1, H >> shift), mx = std::max(1, W >> shift);
    const size_t nodes = (size_t)batch * 2 * my * mx;
    if ((rc = S.ns_mesh.ensure(2 * nodes * sizeof(int)))) return rc;
    int *raw = S.ns_mesh.as<int>(), *filt = raw + nodes;
    unsigned char* level = link ? S.mask.as<unsigned char>() : (unsigned char*)pc.d_out;
    const dim3 pgrid((unsigned)((H * W + SG_CHUNK - 1) / SG_CHUNK), (unsigned)batch);
    if ((rc = S.clk_ns.record(0, st))) return rc;
    by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        hipLaunchKernelGGL(ns_stats<PIX>, dim3((unsigned)mx, (unsigned)my, (unsigned)batch), dim3(SG_THREADS), 0, st, (const PIX*)pc.d_img,
                           (int)channels, (int)channel, H, W, shift, floor8, raw);
    });
    hipLaunchKernelGGL(ns_filter, dim3((unsigned)((my * mx + SG_THREADS - 1) / SG_THREADS), 2u, (unsigned)batch), dim3(SG_THREADS), 0, st,
                       (const int*)raw, my, mx, filt);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ns.record(1, st))) return rc;
    by_pixel(pixel_type, [&](auto pix) {
        using PIX = decltype(pix);
        hipLaunchKernelGGL(ns_cut<PIX>, pgrid, dim3(SG_THREADS), 0, st, (const PIX*)pc.d_img, (int)channels, (int)channel, H, W, shift, my, mx,
                           (const int*)filt, k8, weak8, level);
    });
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ns.record(2, st))) return rc;
    if (link) {
        HIPCHK(hipMemsetAsync(c.d_lab, 0, c.npx * sizeof(int), st));
        HIPCHK(label_mask(level, batch, H, W, 0, noise->connectivity == 2, S.parent.as<int>(), nullptr, c.nchunks, st));
        hipLaunchKernelGGL(hy_mark, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, (const unsigned char*)level, (const int*)S.parent.as<int>(), c.d_lab);
        hipLaunchKernelGGL(hy_keep, c.pgrid, dim3(SG_THREADS), 0, st, c.HW, (const int*)S.parent.as<int>(), (const int*)c.d_lab,
                           (unsigned char*)pc.d_out);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_ns.record(3, st, link))) return rc;
    if (mesh) HIPCHK(hipMemcpyAsync(mesh, filt, nodes * sizeof(int), hipMemcpyDeviceToHost, st));
    if (mesh && pc.on_device) {
        HIPCHK(hipStreamSynchronize(st));                 // the one host synchronisation: the mesh is filled
        return S.clk_ns.finish();
    }
    return plane_end(pc, S.clk_ns, nullptr, batch);
}

int cs_segment_noise_last_timing(const cs_preproc* p, double* mesh_ms, double* cut_ms, double* link_ms)
{
    return clock_read(p, &SegmentState::clk_ns, {mesh_ms, cut_ms, link_ms});
}
