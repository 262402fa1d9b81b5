// quantile.hip -- per-object order statistics of a label image on gfx950: median, quantiles and MAD (include/cellscreen.h,
// cs_label_quantiles; the rule and the sizing: DESIGN 3v, restated in tests/quantile_reference.py).
//
// Per object (cs_label_intensity's: a label > 0 of an image, less the pixels where `exclude` is non-zero) and channel the
// sorted values s[0..n-1] are never formed: the values of an object are gathered into one contiguous segment and the wanted
// ranks are selected from it by radix.  Four steps, and kernel boundaries are the only ordering between workgroups:
//   lq_count     the walk of label_tile.hpp over labels and exclude alone: one open run per lane, merged per wave, counted
//                in a table in LDS keyed by the label; only the distinct labels of a tile reach `count`, as integer atomics.
//   lq_offsets   an exclusive scan of `count` per image, one workgroup per image: where an object's segment starts inside its
//                image's H * W slots.  Image b's slots start at b * H * W, so no image depends on another.
//   lq_scatter   the walk a second time: the counts per distinct label in LDS again, ONE returning add per distinct label and
//                tile on the object's cursor reserves a block of the segment, and every pixel takes its place in the block by
//                an add in LDS.  The values go into [C][B * H * W] uint16 (uint8 images widen here).  A label without a slot
//                in LDS reserves per pixel on the cursor.  The order inside a segment depends on arrival; no result does.
//   lq_select    one workgroup per (object, channel), absent ones leave before they touch LDS.  All ranks in two reads of
//                the segment: a 256-bin histogram of the high byte, its prefix, the bin of every rank, then one 256-bin
//                histogram of the low byte per distinct selected bin, filled through a bin-to-slot table.  A uint8 image
//                needs the second read alone.  With MAD two more reads on d = |2 v - (m_lo + m_hi)| (17 bits): 512 bins of
//                d >> 8, then 256.  An object of any size is the same workgroup looping.
// No floating point; a selected value does not depend on the order of arrival, so the tables are bit-identical run to run.
// A label is range-checked before it is a key or an index, and a slot of a segment before it is written.
#include "label_tile.hpp"
#include "segment_internal.hpp"

namespace cs {

static constexpr int LQ_THREADS = LT_THREADS;
static constexpr int LQ_LOG2 = 10;                      // the table of a tile in LDS: 1024 labels
static constexpr int LQ_SLOTS = 1 << LQ_LOG2;
static constexpr int LQ_PROBES = 16;
static constexpr int kLqMaxChannels = 4;
static constexpr int kLqMaxQ = 8;
static constexpr int kLqMaxDen = 65536;
static constexpr int64_t kLqMaxCells = 1 << 22;         // batch * max_label * channels * n_q
static constexpr int LQ_RANKS = 2 * kLqMaxQ + 2;        // lo and hi of every quantile, and of the median with MAD

__device__ inline unsigned int lq_hash(int label) { return ((unsigned int)label * 0x9E3779B1u) >> (32 - LQ_LOG2); }

// The walk that lq_count and lq_scatter share: the runs of one label in a lane's 4 x 16 pixels, flush(label, n) per closed
// run, and per distinct label of the wave for the runs still open at the end.  ll, ee (or null): the image's planes.  Returns
// whether the lane saw a label outside 1..max_label (such a pixel belongs to no run).  Called by whole waves.
template <typename F>
__device__ inline unsigned int lq_runs(const int* ll, const int* ee, const LabelTile& tile, int H, int W, bool wide, int max_label, F flush)
{
    unsigned int bad = 0u, n = 0u;
    int cur = 0;
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        const size_t at = (size_t)r * W + tile.c_base;
        label_load4(ll + at, W - tile.c_base, wide, x);
        if (ee) label_load4(ee + at, W - tile.c_base, wide, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab == 0) continue;
            if (lab < 0 || lab > max_label) { bad = 1u; continue; }
            if (e[k] != 0) continue;
            if (n != 0u && lab != cur) {
                flush(cur, n);
                n = 0u;
            }
            cur = lab;
            ++n;
        }
    }
    merge_open_runs(n != 0u, cur, tile.lane, [&](int lw, bool mine, bool leader) {
        const unsigned int t = wave_sum(mine ? n : 0u);
        if (leader) flush(lw, t);
    });
    return bad;
}

// grid (ceil(W/256), ceil(H/64), B).  labels, exclude (or null): [B][H][W] int.  count: [B][max_label], cleared.
__global__ __launch_bounds__(LQ_THREADS) void lq_count(const int* __restrict__ labels, const int* __restrict__ exclude, int H, int W, int vec,
                                                       int max_label, int* __restrict__ count, unsigned int* __restrict__ ctrl)
{
    __shared__ int key[LQ_SLOTS];                       // 0: empty
    __shared__ unsigned int cnt[LQ_SLOTS];
    for (int s = threadIdx.x; s < LQ_SLOTS; s += LQ_THREADS) {
        key[s] = 0;
        cnt[s] = 0u;
    }
    __syncthreads();
    const LabelTile tile = label_tile();
    const size_t plane = (size_t)tile.b * H * W;
    int* crow = count + (size_t)tile.b * max_label;
    const bool wide = vec && tile.c_base + 3 < W;
    const unsigned int bad = lq_runs(labels + plane, exclude ? exclude + plane : nullptr, tile, H, W, wide, max_label, [&](int label, unsigned int n) {
        const int s = table_claim(key, LQ_LOG2, lq_hash(label), label, LQ_PROBES);
        if (s >= 0) atomicAdd(&cnt[s], n);
        else atomicAdd(&crow[label - 1], (int)n);       // no room: straight to the global table
    });
    __syncthreads();
    for (int s = threadIdx.x; s < LQ_SLOTS; s += LQ_THREADS)
        if (key[s] != 0) atomicAdd(&crow[key[s] - 1], (int)cnt[s]);
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

// every lane gets the sum of v over the lanes up to and including its own
__device__ inline unsigned int lq_wave_scan(unsigned int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int t = (unsigned int)__shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// grid (B).  start, cursor: [B][max_label], the first slot of an object's segment inside its image, twice: lq_scatter moves
// the cursor.  A thread takes 4 neighbouring rows, the workgroup 1024 per step.
__global__ __launch_bounds__(LQ_THREADS) void lq_offsets(const int* __restrict__ count, int max_label, unsigned int* __restrict__ start,
                                                         unsigned int* __restrict__ cursor)
{
    __shared__ unsigned int wsum[LT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row0 = (size_t)blockIdx.x * max_label;
    unsigned int carry = 0u;
    for (int base = 0; base < max_label; base += 4 * LQ_THREADS) {
        const int i0 = base + 4 * (int)threadIdx.x;
        unsigned int c[4], mine = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = i0 + k < max_label ? (unsigned int)count[row0 + i0 + k] : 0u;
            mine += c[k];
        }
        const unsigned int incl = lq_wave_scan(mine, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned int off = carry + incl - mine, total = 0u;
#pragma unroll
        for (int w = 0; w < LT_WAVES; ++w) {
            if (w < wave) off += wsum[w];
            total += wsum[w];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < max_label) {
                start[row0 + i0 + k] = off;
                cursor[row0 + i0 + k] = off;
            }
            off += c[k];
        }
        carry += total;
        __syncthreads();                                // wsum is written again
    }
}

// the slot of a label that lq_runs' flushes claimed, -1: it found no room then and finds none now (slots are never given up)
__device__ inline int lq_find(const int* key, int label)
{
    unsigned int h = lq_hash(label);
    for (int i = 0; i < LQ_PROBES; ++i) {
        const int k = key[h];
        if (k == label) return (int)h;
        if (k == 0) return -1;
        h = (h + 1) & (LQ_SLOTS - 1);
    }
    return -1;
}

// grid (ceil(W/256), ceil(H/64), B).  image: [B][H][W][C] PIX.  cursor: [B][max_label] from lq_offsets.  val: [C][npx] uint16,
// npx = B * H * W.  vec: as li_pass (intensity.hip), decided on the host.
template <typename PIX, int C>
__global__ __launch_bounds__(LQ_THREADS) void lq_scatter(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                         const int* __restrict__ exclude, int H, int W, int vec, int max_label,
                                                         unsigned int* __restrict__ cursor, unsigned short* __restrict__ val, size_t npx)
{
    __shared__ int key[LQ_SLOTS];
    __shared__ unsigned int cnt[LQ_SLOTS], first[LQ_SLOTS];
    for (int s = threadIdx.x; s < LQ_SLOTS; s += LQ_THREADS) {
        key[s] = 0;
        cnt[s] = 0u;
    }
    __syncthreads();
    const LabelTile tile = label_tile();
    const size_t plane = (size_t)tile.b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const PIX* im = image + plane * C;
    unsigned int* crow = cursor + (size_t)tile.b * max_label;
    const bool wide = vec && tile.c_base + 3 < W;
    constexpr int PXB = 4 * C * (int)sizeof(PIX);
    constexpr int PXA = (PXB & -PXB) < 16 ? (PXB & -PXB) : 16;

    (void)lq_runs(ll, ee, tile, H, W, wide, max_label, [&](int label, unsigned int n) {
        const int s = table_claim(key, LQ_LOG2, lq_hash(label), label, LQ_PROBES);
        if (s >= 0) atomicAdd(&cnt[s], n);              // without a slot its pixels reserve one by one below
    });
    __syncthreads();
    for (int s = threadIdx.x; s < LQ_SLOTS; s += LQ_THREADS) {
        if (key[s] == 0) continue;
        first[s] = atomicAdd(&crow[key[s] - 1], cnt[s]);    // the block of this tile in the object's segment
        cnt[s] = 0u;
    }
    __syncthreads();

    const unsigned int slots = (unsigned int)H * (unsigned int)W;
    int last = 0, slot = -1;
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;
        int x[4], e[4] = {0, 0, 0, 0};
        PIX px[4 * C];
        const size_t at = (size_t)r * W + tile.c_base;
        label_load4(ll + at, W - tile.c_base, wide, x);
        if (ee) label_load4(ee + at, W - tile.c_base, wide, e);
        if (wide) {
            __builtin_memcpy(px, __builtin_assume_aligned(im + at * C, PXA), PXB);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = tile.c_base + k < W;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) px[k * C + ch] = in ? im[(at + k) * C + ch] : (PIX)0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab <= 0 || lab > max_label || e[k] != 0) continue;
            if (lab != last) {
                slot = lq_find(key, lab);
                last = lab;
            }
            const unsigned int pos = slot >= 0 ? first[slot] + atomicAdd(&cnt[slot], 1u) : atomicAdd(&crow[lab - 1], 1u);
            if (pos >= slots) continue;                 // cannot be, with the counts of the same planes: never past the image's slots
#pragma unroll
            for (int ch = 0; ch < C; ++ch) val[(size_t)ch * npx + plane + pos] = (unsigned short)px[k * C + ch];
        }
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------
struct LqQuantiles {
    int n_q;
    int num[kLqMaxQ], den[kLqMaxQ];
};

// f(v) on every value of a segment, by the whole workgroup: 16-byte loads between the segment's unaligned ends
template <typename F> __device__ inline void lq_each(const unsigned short* seg, unsigned int n, F f)
{
    const unsigned int head = min(n, (unsigned int)(((16u - (unsigned int)((uintptr_t)seg & 15u)) & 15u) >> 1));
    if (threadIdx.x < head) f((unsigned int)seg[threadIdx.x]);
    const uint4* q = (const uint4*)(seg + head);
    const unsigned int nv = (n - head) >> 3;
    for (unsigned int i = threadIdx.x; i < nv; i += LQ_THREADS) {
        const uint4 u = q[i];
        f(u.x & 0xFFFFu); f(u.x >> 16); f(u.y & 0xFFFFu); f(u.y >> 16);
        f(u.z & 0xFFFFu); f(u.z >> 16); f(u.w & 0xFFFFu); f(u.w >> 16);
    }
    const unsigned int done = head + 8u * nv;
    if (done + threadIdx.x < n) f((unsigned int)seg[done + threadIdx.x]);
}

// h[0 .. 64 * PER) in LDS becomes its exclusive prefix; called by one whole wave
template <int PER> __device__ inline void lq_prefix(unsigned int* h, int lane)
{
    unsigned int c[PER], mine = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        c[k] = h[lane * PER + k];
        mine += c[k];
    }
    unsigned int off = lq_wave_scan(mine, lane) - mine;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        h[lane * PER + k] = off;
        off += c[k];
    }
}

// the bin of rank r in an exclusive prefix: the largest b with excl[b] <= r; that bin is not empty when r is below the total
__device__ inline unsigned int lq_locate(const unsigned int* excl, int bins, unsigned int r)
{
    int lo = 0, hi = bins - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (excl[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return (unsigned int)lo;
}

struct LqSelect {
    unsigned int h1[512];                               // the high bins: 256 of v >> 8, 512 of d >> 8
    unsigned int h2[LQ_RANKS][256];                     // the low byte, per distinct selected high bin
    unsigned int rank[LQ_RANKS], bin[LQ_RANKS], below[LQ_RANKS], res[LQ_RANKS];
    unsigned int used;                                  // slots of h2
    unsigned char slot_of[512];                         // high bin -> slot of h2, 255: not selected
};

// The values at L.rank[0 .. n_r) of key(v) over the segment into L.res: key(v) < 256 * HB, and the high bin is known to be 0
// where `one_read`.  Called by the whole workgroup, L.rank written and a barrier passed.
template <int HB, typename K>
__device__ inline void lq_pick(LqSelect& L, const unsigned short* seg, unsigned int n, int n_r, bool one_read, K key)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = tid; s < 512; s += LQ_THREADS) {
        L.h1[s] = 0u;
        L.slot_of[s] = 255;
    }
    for (int s = tid; s < n_r * 256; s += LQ_THREADS) (&L.h2[0][0])[s] = 0u;   // at most n_r slots are used
    __syncthreads();
    if (!one_read) {
        lq_each(seg, n, [&](unsigned int v) { atomicAdd(&L.h1[key(v) >> 8], 1u); });
        __syncthreads();
        if (wave == 0) lq_prefix<HB * 4>(L.h1, lane);
        __syncthreads();
    }
    if (tid < n_r) {
        const unsigned int b = one_read ? 0u : lq_locate(L.h1, HB * 256, L.rank[tid]);
        L.bin[tid] = b;
        L.below[tid] = one_read ? 0u : L.h1[b];
    }
    __syncthreads();
    if (tid == 0) {
        unsigned int used = 0u;
        for (int j = 0; j < n_r; ++j)
            if (L.slot_of[L.bin[j]] == 255) L.slot_of[L.bin[j]] = (unsigned char)used++;
        L.used = used;
    }
    __syncthreads();
    lq_each(seg, n, [&](unsigned int v) {
        const unsigned int k = key(v), s = L.slot_of[k >> 8];
        if (s != 255u) atomicAdd(&L.h2[s][k & 255u], 1u);
    });
    __syncthreads();
    for (unsigned int s = wave; s < L.used; s += LT_WAVES) lq_prefix<4>(L.h2[s], lane);
    __syncthreads();
    if (tid < n_r) L.res[tid] = (L.bin[tid] << 8) | lq_locate(L.h2[L.slot_of[L.bin[tid]]], 256, L.rank[tid] - L.below[tid]);
    __syncthreads();
}

// grid (B * max_label * C): cell = row * C + channel.  count, start: [B][max_label]; val: [C][npx]; order: [cells][n_q][2],
// mad (or null): [cells][4], both cleared.  u16: the values exceed a byte.
__global__ __launch_bounds__(LQ_THREADS) void lq_select(const int* __restrict__ count, const unsigned int* __restrict__ start,
                                                        const unsigned short* __restrict__ val, size_t npx, int hw, int max_label, int C,
                                                        int u16, LqQuantiles Q, int* __restrict__ order, int* __restrict__ mad)
{
    const size_t cell = blockIdx.x, row = cell / (size_t)C;
    const int ch = (int)(cell - row * C);
    const unsigned int n = (unsigned int)count[row];
    if (n == 0u) return;                                // an absent object keeps its zeros
    __shared__ LqSelect L;
    const int tid = threadIdx.x, n_q = Q.n_q, n_r = 2 * n_q + (mad ? 2 : 0);
    const unsigned short* seg = val + (size_t)ch * npx + (row / (size_t)max_label) * (size_t)hw + start[row];
    if (tid < n_r) {
        const int q = tid >> 1;
        const long long num = q < n_q ? Q.num[q] : 1, den = q < n_q ? Q.den[q] : 2;     // behind the quantiles: the median's ranks
        const long long t = num * (long long)(n - 1u);  // below 2^40
        const long long lo = t / den;
        L.rank[tid] = (unsigned int)(lo + ((tid & 1) && t % den > 0 ? 1 : 0));
    }
    __syncthreads();
    lq_pick<1>(L, seg, n, n_r, !u16, [](unsigned int v) { return v; });
    if (tid < 2 * n_q) order[cell * (size_t)(2 * n_q) + tid] = (int)L.res[tid];
    if (!mad) return;
    const unsigned int m_lo = L.res[2 * n_q], m_hi = L.res[2 * n_q + 1], m2 = m_lo + m_hi;
    __syncthreads();                                    // res and rank are read before they are written again
    if (tid < 2) L.rank[tid] = L.rank[2 * n_q + tid];
    __syncthreads();
    lq_pick<2>(L, seg, n, 2, false, [m2](unsigned int v) { return 2u * v > m2 ? 2u * v - m2 : m2 - 2u * v; });
    if (tid == 0) {
        int* o = mad + cell * 4;
        o[0] = (int)m_lo; o[1] = (int)m_hi; o[2] = (int)L.res[0]; o[3] = (int)L.res[1];
    }
}

template <typename PIX>
static void lq_scatter_c(int C, const void* image, const int* labels, const int* exclude, int batch, int H, int W, int vec, int max_label,
                         unsigned int* cursor, unsigned short* val, size_t npx, hipStream_t st)
{
    const dim3 grid = label_tile_grid(batch, H, W), block(LQ_THREADS);
    const PIX* im = (const PIX*)image;
    switch (C) {
    case 1: hipLaunchKernelGGL((lq_scatter<PIX, 1>), grid, block, 0, st, im, labels, exclude, H, W, vec, max_label, cursor, val, npx); break;
    case 2: hipLaunchKernelGGL((lq_scatter<PIX, 2>), grid, block, 0, st, im, labels, exclude, H, W, vec, max_label, cursor, val, npx); break;
    case 3: hipLaunchKernelGGL((lq_scatter<PIX, 3>), grid, block, 0, st, im, labels, exclude, H, W, vec, max_label, cursor, val, npx); break;
    default: hipLaunchKernelGGL((lq_scatter<PIX, 4>), grid, block, 0, st, im, labels, exclude, H, W, vec, max_label, cursor, val, npx); break;
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_quantiles(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                       int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, const int32_t* q_num,
                       const int32_t* q_den, int32_t n_q, int want_mad, int32_t* count, int32_t* order, int32_t* mad, int out_kind)
{
    if (!image || !labels || !q_num || !q_den || !count || !order || (want_mad && !mad)) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    if (n_q < 1) return fail(CS_ERR_INVALID, "n_q %d: must be >= 1", (int)n_q);
    for (int32_t i = 0; i < n_q; ++i)
        if (q_den[i] < 1 || q_den[i] > kLqMaxDen || q_num[i] < 0 || q_num[i] > q_den[i])
            return fail(CS_ERR_INVALID, "quantile %d is %d/%d: 0 <= num <= den and 1 <= den <= %d are required", (int)i, (int)q_num[i], (int)q_den[i], kLqMaxDen);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kLqMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kLqMaxChannels);
    if (n_q > kLqMaxQ) return fail(CS_ERR_UNSUPPORTED, "n_q %d: at most %d quantiles per call", (int)n_q, kLqMaxQ);
    if (max_label > kMaxLabel || (int64_t)batch * max_label * channels * n_q > kLqMaxCells)
        return fail(CS_ERR_UNSUPPORTED, "max_label %d x batch %d x channels %d x n_q %d: the tables are capped at %d labels per image and %lld cells",
                    (int)max_label, (int)batch, (int)channels, (int)n_q, kMaxLabel, (long long)kLqMaxCells);
    if ((rc = image_limits(batch, height, width)) || (rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width, C = channels;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const int64_t rows = (int64_t)batch * max_label, cells = rows * C;
    const size_t cbytes = (size_t)rows * sizeof(int), obytes = (size_t)cells * n_q * 2 * sizeof(int),
                 mbytes = want_mad ? (size_t)cells * 4 * sizeof(int) : 0;
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rc = S.lq_val.ensure(npx * C * sizeof(unsigned short))) ||
        (rc = S.lq_off.ensure((size_t)rows * 2 * sizeof(unsigned int))))
        return rc;
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
    if (out_host && (rc = S.stage.ensure(cbytes + obytes + mbytes))) return rc;     // the tables on their way to the host: count, order, mad
    int* d_count = out_host ? S.stage.as<int>() : count;
    int* d_order = out_host ? (int*)(S.stage.as<char>() + cbytes) : order;
    int* d_mad = !want_mad ? nullptr : out_host ? (int*)(S.stage.as<char>() + cbytes + obytes) : mad;
    constexpr int PA[2][4] = {{4, 8, 4, 16}, {8, 16, 8, 16}};              // what lq_scatter assumes of 4 pixels: PXA
    const int vec_lab = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0;
    const int vec = vec_lab && ((uintptr_t)d_img & (uintptr_t)(PA[esz - 1][C - 1] - 1)) == 0;
    unsigned int* d_start = S.lq_off.as<unsigned int>();
    unsigned int* d_cursor = d_start + rows;
    unsigned short* d_val = S.lq_val.as<unsigned short>();
    unsigned int* d_ctrl = S.ctrl.as<unsigned int>();
    LqQuantiles Q{};
    Q.n_q = n_q;
    for (int i = 0; i < n_q; ++i) {
        Q.num[i] = q_num[i];
        Q.den[i] = q_den[i];
    }

    if ((rc = S.clk_lq.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(d_ctrl, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_count, 0, cbytes, st));
    HIPCHK(hipMemsetAsync(d_order, 0, obytes, st));
    if (want_mad) HIPCHK(hipMemsetAsync(d_mad, 0, mbytes, st));
    hipLaunchKernelGGL(lq_count, label_tile_grid(batch, H, W), dim3(LQ_THREADS), 0, st, d_lab, d_ex, H, W, vec_lab, (int)max_label, d_count, d_ctrl);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(lq_offsets, dim3((unsigned)batch), dim3(LQ_THREADS), 0, st, (const int*)d_count, (int)max_label, d_start, d_cursor);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_lq.record(1, st))) return rc;
    if (pixel_type == CS_PIX_U8) lq_scatter_c<unsigned char>(C, d_img, d_lab, d_ex, batch, H, W, vec, max_label, d_cursor, d_val, npx, st);
    else lq_scatter_c<unsigned short>(C, d_img, d_lab, d_ex, batch, H, W, vec, max_label, d_cursor, d_val, npx, st);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_lq.record(2, st))) return rc;
    hipLaunchKernelGGL(lq_select, dim3((unsigned)cells), dim3(LQ_THREADS), 0, st, (const int*)d_count, (const unsigned int*)d_start,
                       (const unsigned short*)d_val, npx, H * W, (int)max_label, C, pixel_type == CS_PIX_U16 ? 1 : 0, Q, d_order, d_mad);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_lq.record(3, st))) return rc;
    unsigned int bad = 0u;
    HIPCHK(hipMemcpyAsync(&bad, d_ctrl, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(count, d_count, cbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(order, d_order, obytes, hipMemcpyDeviceToHost, st));
        if (want_mad) HIPCHK(hipMemcpyAsync(mad, d_mad, mbytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host tables
    if ((rc = S.clk_lq.finish())) return rc;
    if (bad) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    return CS_OK;
}

int cs_label_quantiles_last_timing(const cs_preproc* p, double* count_ms, double* scatter_ms, double* select_ms)
{
    return clock_read(p, &SegmentState::clk_lq, {count_ms, scatter_ms, select_ms});
}
