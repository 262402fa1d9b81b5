// segment.hip -- the project's own classical segmenter on gfx950: a global threshold (Otsu's, as scikit-image 0.18.3 computes
// it on an integer image, or a fixed one), optional hole filling, and connected-component labelling with scipy.ndimage.label's
// numbering.  It is NOT StarDist: touching cells come out as one region, which the extraction's area and eccentricity rules
// then judge.  The labels feed cs_extract_measure on the same handle and stream without leaving the device.
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
// The final parents are a function of the mask alone (the minimum index of a component), so the labels do not depend on
// execution order, on the run, or on the other images of the batch.
#include "api_internal.hpp"

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
static constexpr int kSegMaxSide = 4096;
static constexpr int kSegMaxBatch = 65535;              // grid.y / grid.z

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
__global__ __launch_bounds__(SG_THREADS) void sg_tile(const unsigned char* __restrict__ mask, int H, int W, int invert, int conn8,
                                                      int* __restrict__ P)
{
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ int L[SG_TILE];
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
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!fg[k]) continue;
        const int ly = lw + 4 * k, idx = ly * SG_TW + lx;
        if (lx > 0 && uf_load<WG>(L, idx - 1) >= 0) uf_union<WG>(L, idx, idx - 1);
        if (ly > 0) {
            if (uf_load<WG>(L, idx - SG_TW) >= 0) uf_union<WG>(L, idx, idx - SG_TW);
            else if (conn8) {                           // with the pixel above set, both diagonals already hang on it
                if (lx > 0 && uf_load<WG>(L, idx - SG_TW - 1) >= 0) uf_union<WG>(L, idx, idx - SG_TW - 1);
                if (lx < SG_TW - 1 && uf_load<WG>(L, idx - SG_TW + 1) >= 0) uf_union<WG>(L, idx, idx - SG_TW + 1);
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
__global__ __launch_bounds__(SG_THREADS) void sg_border(int H, int W, int conn8, int* __restrict__ P)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int nrb = (H - 1) / SG_TH, ncb = (W - 1) / SG_TW;
    int id = blockIdx.x * SG_THREADS + threadIdx.x;
    int* Pb = P + (size_t)blockIdx.y * H * W;
    if (id < nrb * W) {
        const int y = (id / W + 1) * SG_TH, x = id % W, i = y * W + x;
        if (uf_load<AG>(Pb, i) < 0) return;
        if (uf_load<AG>(Pb, i - W) >= 0) uf_union<AG>(Pb, i, i - W);
        else if (conn8) {
            if (x > 0 && uf_load<AG>(Pb, i - W - 1) >= 0) uf_union<AG>(Pb, i, i - W - 1);
            if (x < W - 1 && uf_load<AG>(Pb, i - W + 1) >= 0) uf_union<AG>(Pb, i, i - W + 1);
        }
        return;
    }
    id -= nrb * W;
    if (id >= ncb * H) return;
    const int x = (id / H + 1) * SG_TW, y = id % H, i = y * W + x;
    if (uf_load<AG>(Pb, i) < 0) return;
    if (uf_load<AG>(Pb, i - 1) >= 0) uf_union<AG>(Pb, i, i - 1);
    else if (conn8) {                                   // with the left pixel set, the two left diagonals already hang on it
        if (y > 0 && uf_load<AG>(Pb, i - W - 1) >= 0) uf_union<AG>(Pb, i, i - W - 1);
        if (y < H - 1 && uf_load<AG>(Pb, i + W - 1) >= 0) uf_union<AG>(Pb, i, i + W - 1);
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

// grid (nchunks, B): roots get their label, background 0; the other foreground pixels are written by sg_gather
__global__ __launch_bounds__(SG_THREADS) void sg_rank(int HW, const int* __restrict__ P, const int* __restrict__ chunk_off, int nchunks,
                                                      int* __restrict__ labels)
{
    __shared__ int wc[4][SG_WAVES];
    const size_t base = (size_t)blockIdx.y * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before[4], par[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * SG_CHUNK + k * SG_THREADS + threadIdx.x;
        par[k] = i < HW ? P[base + i] : -1;
        const unsigned long long m = __ballot(i < HW && par[k] == i);
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
            if (par[k] < 0) labels[base + i] = 0;
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

// ---- host state ---------------------------------------------------------------------------------------------------------------
struct SegmentState {
    DevBuf img, lab, mask, parent, slab, hist, thr, chunks, counts;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double threshold_ms = 0.0, label_ms = 0.0;
    ~SegmentState()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

void segment_state_free(SegmentState* s) { delete s; }

// tile union-find, border merge, path compression (with the root counts when chunk_cnt is given)
static hipError_t label_mask(const unsigned char* mask, int batch, int H, int W, int invert, int conn8, int* parent, int* chunk_cnt,
                             int nchunks, hipStream_t st)
{
    const dim3 tgrid((unsigned)((W + SG_TW - 1) / SG_TW), (unsigned)((H + SG_TH - 1) / SG_TH), (unsigned)batch);
    hipLaunchKernelGGL(sg_tile, tgrid, dim3(SG_THREADS), 0, st, mask, H, W, invert, conn8, parent);
    const int nb = ((H - 1) / SG_TH) * W + ((W - 1) / SG_TW) * H;
    if (nb > 0)
        hipLaunchKernelGGL(sg_border, dim3((unsigned)((nb + SG_THREADS - 1) / SG_THREADS), (unsigned)batch), dim3(SG_THREADS), 0, st, H, W,
                           conn8, parent);
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

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_segment_threshold(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t channel, int32_t batch, int32_t height,
                         int32_t width, int in_kind, const cs_segment_params* params, int32_t* labels, int labels_kind, int32_t* n_labels,
                         int32_t* thresholds)
{
    if (!image || !labels || !n_labels) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if ((in_kind != CS_MEM_HOST && in_kind != CS_MEM_DEVICE) || (labels_kind != CS_MEM_HOST && labels_kind != CS_MEM_DEVICE))
        return fail(CS_ERR_INVALID, "in_kind / labels_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1 || channel < 0 || channel >= channels)
        return fail(CS_ERR_INVALID, "channel %d of %d: need 0 <= channel < channels", (int)channel, (int)channels);
    if (batch < 1 || height < 1 || width < 1) return fail(CS_ERR_INVALID, "batch %d, height %d, width %d: all must be >= 1", (int)batch,
                                                          (int)height, (int)width);
    if (height > kSegMaxSide || width > kSegMaxSide)
        return fail(CS_ERR_UNSUPPORTED, "image %dx%d: sides above %d are not supported", (int)height, (int)width, kSegMaxSide);
    if (batch > kSegMaxBatch) return fail(CS_ERR_UNSUPPORTED, "batch %d: at most %d images per call", (int)batch, kSegMaxBatch);
    cs_segment_params sp{CS_THRESH_OTSU, 0, 1, 0};
    if (params) {
        sp = *params;
        if (sp.threshold_mode != CS_THRESH_OTSU && sp.threshold_mode != CS_THRESH_FIXED)
            return fail(CS_ERR_INVALID, "threshold_mode %d: CS_THRESH_OTSU or CS_THRESH_FIXED", (int)sp.threshold_mode);
        if (sp.threshold_mode == CS_THRESH_FIXED && (sp.threshold < 0 || sp.threshold > 65535))
            return fail(CS_ERR_INVALID, "threshold %d outside 0..65535", (int)sp.threshold);
        if (sp.connectivity != 1 && sp.connectivity != 2) return fail(CS_ERR_INVALID, "connectivity %d: 1 or 2", (int)sp.connectivity);
        if (sp.fill_holes != 0 && sp.fill_holes != 1) return fail(CS_ERR_INVALID, "fill_holes %d: 0 or 1", (int)sp.fill_holes);
    }
    if (!p) {
        const int rc = require_gfx950(0);
        return rc ? rc : fail(CS_ERR_INVALID, "handle is NULL");
    }
    HIPCHK(hipSetDevice(p->device));
    if (!p->seg) p->seg = new SegmentState();
    SegmentState& S = *p->seg;
    for (hipEvent_t& e : S.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    hipStream_t st = p->stream;
    const int H = height, W = width, HW = H * W, C = channels;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const size_t npx = (size_t)batch * HW;
    const int nchunks = (HW + SG_CHUNK - 1) / SG_CHUNK;
    int rc;
    const void* d_img = image;
    if (in_kind == CS_MEM_HOST) {
        if ((rc = S.img.ensure(npx * C * esz))) return rc;
        HIPCHK(hipMemcpyAsync(S.img.p, image, npx * C * esz, hipMemcpyHostToDevice, st));
        d_img = S.img.p;
    }
    int* d_lab = labels;
    if (labels_kind == CS_MEM_HOST) {
        if ((rc = S.lab.ensure(npx * sizeof(int)))) return rc;
        d_lab = S.lab.as<int>();
    }
    if ((rc = S.mask.ensure(npx)) || (rc = S.parent.ensure(npx * sizeof(int))) || (rc = S.thr.ensure(batch * sizeof(int))) ||
        (rc = S.chunks.ensure((size_t)batch * nchunks * sizeof(int))) || (rc = S.counts.ensure(batch * sizeof(int))))
        return rc;

    HIPCHK(hipEventRecord(S.ev[0], st));
    if (sp.threshold_mode == CS_THRESH_FIXED) {
        hipLaunchKernelGGL(sg_fixed, dim3((unsigned)((batch + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, st, S.thr.as<int>(), (int)batch,
                           (int)sp.threshold);
        HIPCHK(hipGetLastError());
    } else if (pixel_type == CS_PIX_U8) {
        if ((rc = otsu_thresholds<unsigned char, 256>((const unsigned char*)d_img, C, channel, batch, HW, S, st))) return rc;
    } else {
        if ((rc = otsu_thresholds<unsigned short, 65536>((const unsigned short*)d_img, C, channel, batch, HW, S, st))) return rc;
    }
    const dim3 pgrid((unsigned)nchunks, (unsigned)batch);
    if (pixel_type == CS_PIX_U8)
        hipLaunchKernelGGL(sg_mask<unsigned char>, pgrid, dim3(SG_THREADS), 0, st, (const unsigned char*)d_img, C, (int)channel, HW,
                           S.thr.as<int>(), S.mask.as<unsigned char>());
    else
        hipLaunchKernelGGL(sg_mask<unsigned short>, pgrid, dim3(SG_THREADS), 0, st, (const unsigned short*)d_img, C, (int)channel, HW,
                           S.thr.as<int>(), S.mask.as<unsigned char>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[1], st));

    if (sp.fill_holes) {
        // background components, 4-connected; the label buffer holds the "touches the image border" flags meanwhile
        HIPCHK(hipMemsetAsync(d_lab, 0, npx * sizeof(int), st));
        HIPCHK(label_mask(S.mask.as<unsigned char>(), batch, H, W, 1, 0, S.parent.as<int>(), nullptr, nchunks, st));
        hipLaunchKernelGGL(sg_edge, dim3((unsigned)((2 * W + 2 * H + SG_THREADS - 1) / SG_THREADS), (unsigned)batch), dim3(SG_THREADS), 0, st, H,
                           W, S.parent.as<int>(), d_lab);
        hipLaunchKernelGGL(sg_fill, pgrid, dim3(SG_THREADS), 0, st, HW, S.parent.as<int>(), d_lab, S.mask.as<unsigned char>());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(label_mask(S.mask.as<unsigned char>(), batch, H, W, 0, sp.connectivity == 2, S.parent.as<int>(), S.chunks.as<int>(), nchunks, st));
    hipLaunchKernelGGL(sg_scan, dim3((unsigned)batch), dim3(HIST_THREADS), 0, st, S.chunks.as<int>(), nchunks, S.counts.as<int>());
    hipLaunchKernelGGL(sg_rank, pgrid, dim3(SG_THREADS), 0, st, HW, S.parent.as<int>(), S.chunks.as<int>(), nchunks, d_lab);
    hipLaunchKernelGGL(sg_gather, pgrid, dim3(SG_THREADS), 0, st, HW, S.parent.as<int>(), d_lab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[2], st));
    HIPCHK(hipMemcpyAsync(n_labels, S.counts.p, batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (thresholds) HIPCHK(hipMemcpyAsync(thresholds, S.thr.p, batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (labels_kind == CS_MEM_HOST) HIPCHK(hipMemcpyAsync(labels, d_lab, npx * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the counts
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    S.threshold_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, S.ev[1], S.ev[2]));
    S.label_ms = ms;
    return CS_OK;
}

int cs_segment_last_timing(const cs_preproc* p, double* threshold_ms, double* label_ms)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    const SegmentState* S = p->seg;
    if (threshold_ms) *threshold_ms = S ? S->threshold_ms : 0.0;
    if (label_ms) *label_ms = S ? S->label_ms : 0.0;
    return CS_OK;
}
