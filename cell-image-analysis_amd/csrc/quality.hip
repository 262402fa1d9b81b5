// quality.hip -- focus and saturation records of an image, of the tiles of a mesh over it and of the objects of a label image on
// gfx950 (include/cellscreen.h, cs_image_quality and cs_object_focus; the rule: DESIGN 3zh, restated in tests/quality_reference.py).
//
// Per channel x and interior pixel (one with a full 3 x 3 neighbourhood inside the image): the 4-neighbour Laplacian L, the
// Tenengrad G = gx^2 + gy^2 of the 3 x 3 Sobel responses and Brenner's centred gradient Br; per image, mesh tile or object the
// sums n_int, L, L^2, G, Br, and per image and tile n, v, v^2.  All integers.
//
// The stencil lives in registers with row reuse, not in LDS: on the tile of label_tile.hpp a lane owns 4 columns and walks 16
// rows, so it keeps three rows of its 4 pixels and their two side neighbours (6 C words a row), loads every row once (16-byte
// loads where width and pointer allow) and takes the side neighbours from the next lanes by a wave shuffle; only lanes 0 and 63
// load their outer neighbour themselves.  A wave re-reads the row above and the row below its 16 (2 / 16 more loads, out of
// L2), and nothing waits on a barrier before the walk.  A tile in LDS would save those two rows and cost a barrier, a second
// copy of every pixel and the LDS the merge tables want.  The loads of row r + 2 are issued (q_issue) before the sums of row r
// and awaited (q_finish, with the shuffles) after them, so a row is in flight under the arithmetic of the row before.
//   iq_pass      ONE read of the interleaved planes.  A lane keeps the sums of one open run of a mesh tile (tile == 0: one tile
//                per image); a run is at most 64 pixels, so sum v and sum L stay in 32 bits.  When the lane's pixel moves to
//                another mesh tile the run is flushed into a table in LDS that the workgroup owns, indexed by the mesh tile's
//                place among those the workgroup tile meets (IQ_SLOTS of them; a tile beyond goes to the global table
//                directly).  The lanes' last runs are first merged per distinct mesh tile of the wave (merge_open_runs).  Only the
//                touched slots go on to the mesh table in global memory, as 64-bit integer atomics: 8 C per mesh tile and
//                workgroup.  Without a mesh every workgroup would add to the same 8 C words, so there it stores its sums into a
//                tile of its own instead (plain stores) and iq_close sums the workgroups' tiles.  The extremes with their counts
//                and the saturated pixels are reduced per wave, then per workgroup, and leave as one (min, n_at_min, max,
//                n_at_max, n_sat) partial per workgroup and channel: plain stores.
//   iq_close     one workgroup per image and channel: the mesh tiles summed into the image's record, the workgroups' partials
//                reduced to the extremes and their counts (equal extremes add their counts, a smaller one replaces).
//   lf_pass      li_pass's walk (intensity.hip): a run per lane keyed by the label, runs merged per wave, an LDS table per
//                workgroup keyed by the label, only the distinct labels of a tile reaching the dense tables; the stencil values
//                in the place of v * r, v * c.
// Bounds, sides <= 4096, v <= 65535 (T = 65535, n <= 2^24 pixels):
//   |L| <= 4 T = 262140 (four neighbours at T, the centre at 0, or the reverse), so L^2 <= 6.872e10 < 2^37 and
//       sum L^2 <= (4 T)^2 * 2^24 = 1.1529e18 < 2^63 = 9.2234e18; a run's |sum L| <= 64 * 4 T < 2^25.
//   |gx|, |gy| <= 4 T (weights 1 + 2 + 1 on one side at T, the other at 0), so G <= 2 (4 T)^2 and
//       sum G <= 2 (4 T)^2 * 2^24 = 2.3058e18 < 2^63.
//   Br <= 2 T^2 < 2^33, sum Br <= 2 T^2 * 2^24 = 1.4411e17; sum v^2 <= T^2 * 2^24 = 7.2055e16; sum v <= T * 2^24 < 2^40.
//   sum L is signed; it travels as a two's complement 64-bit word, for which the unsigned atomic add is the signed one.
// No floating point; every result is a sum, a count, a minimum or a maximum of integers, so it does not depend on the order of
// arrival, and is bit-identical run to run.  A label is range-checked before it is a key or an index.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int IQ_THREADS = LT_THREADS;
static constexpr int IQ_SLOTS = 96;                     // mesh tiles of a workgroup tile in LDS: 17 x 5 at tile = 16 off the grid
static constexpr int IQ_REC = 13, IQ_TILE = 8, IQ_FOCUS = 5, IQ_PART = 5;
static constexpr int kIqMaxChannels = 4;
static constexpr int64_t kIqMaxTiles = 1 << 20;         // batch * channels * m_r * m_c
static constexpr int64_t kLfMaxCells = 1 << 22;         // batch * max_label * channels
static constexpr int LF_LDS_PROBES = 16;

// ---- the rows in registers ---------------------------------------------------------------------------------------------------
// A row on its way into registers: a lane's 4 pixels as loaded, and for lanes 0 and 63 the pixel beyond the wave's 256 columns.
template <typename PIX, int C> struct QRaw {
    PIX px[4 * C];
    PIX left[C], right[C];
};

// The loads of row r, nothing waits on them here: 0 outside the image.  Called by whole waves.
template <typename PIX, int C>
__device__ inline void q_issue(const PIX* __restrict__ im, int r, int H, int W, int c_base, int lane, bool wide, QRaw<PIX, C>& w)
{
    constexpr int PXB = 4 * C * (int)sizeof(PIX);
    constexpr int PXA = (PXB & -PXB) < 16 ? (PXB & -PXB) : 16;
    const bool row_in = r >= 0 && r < H;                // uniform over the wave
    const size_t at = (size_t)(row_in ? r : 0) * W + c_base;
    if (row_in && wide) {
        __builtin_memcpy(w.px, __builtin_assume_aligned(im + at * C, PXA), PXB);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int ch = 0; ch < C; ++ch) w.px[k * C + ch] = row_in && c_base + k < W ? im[(at + k) * C + ch] : (PIX)0;
    }
    const bool l_in = row_in && lane == 0 && c_base >= 1 && c_base - 1 < W, r_in = row_in && lane == 63 && c_base + 4 < W;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        w.left[ch] = l_in ? im[(at - 1) * C + ch] : (PIX)0;
        w.right[ch] = r_in ? im[(at + 4) * C + ch] : (PIX)0;
    }
}

// q[j * C + ch], j = 0..5: the pixels at columns c_base - 1 .. c_base + 4 of the row in w; the side neighbours come from the next
// lanes.  Called by whole waves.
template <typename PIX, int C> __device__ inline void q_finish(const QRaw<PIX, C>& w, int lane, unsigned int (&q)[6 * C])
{
#pragma unroll
    for (int j = 0; j < 4 * C; ++j) q[C + j] = w.px[j];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const unsigned int left = __shfl_up(q[4 * C + ch], 1), right = __shfl_down(q[C + ch], 1);
        q[ch] = lane == 0 ? (unsigned int)w.left[ch] : left;
        q[5 * C + ch] = lane == 63 ? (unsigned int)w.right[ch] : right;
    }
}

struct QFocus {
    int l;
    unsigned long long l2, g, br;
};

// the focus values of the pixel at place k (0..3) of the middle row m, a above it, n below
template <int C> __device__ inline QFocus q_focus(const unsigned int (&a)[6 * C], const unsigned int (&m)[6 * C], const unsigned int (&n)[6 * C], int k, int ch)
{
    const int a0 = (int)a[k * C + ch], a1 = (int)a[(k + 1) * C + ch], a2 = (int)a[(k + 2) * C + ch];
    const int m0 = (int)m[k * C + ch], m1 = (int)m[(k + 1) * C + ch], m2 = (int)m[(k + 2) * C + ch];
    const int n0 = (int)n[k * C + ch], n1 = (int)n[(k + 1) * C + ch], n2 = (int)n[(k + 2) * C + ch];
    QFocus f;
    f.l = a1 + n1 + m0 + m2 - 4 * m1;
    const int gx = (a2 + 2 * m2 + n2) - (a0 + 2 * m0 + n0), gy = (n0 + 2 * n1 + n2) - (a0 + 2 * a1 + a2);
    const unsigned int bx = (unsigned int)abs(m2 - m0), by = (unsigned int)abs(n1 - a1);
    f.l2 = (unsigned long long)((long long)f.l * f.l);
    f.g = (unsigned long long)((long long)gx * gx) + (unsigned long long)((long long)gy * gy);
    f.br = (unsigned long long)(bx * bx) + (unsigned long long)(by * by);                 // T^2 < 2^32
    return f;
}

// ---- the image pass ----------------------------------------------------------------------------------------------------------
// a lane's open run: at most 64 pixels
template <int C> struct IqRun {
    unsigned int n, n_int;
    unsigned int sv[C];
    int sl[C];
    unsigned long long sv2[C], sl2[C], sg[C], sbr[C];
};

template <int C> __device__ inline void iq_reset(IqRun<C>& a)
{
    a.n = a.n_int = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        a.sv[ch] = 0u;
        a.sl[ch] = 0;
        a.sv2[ch] = a.sl2[ch] = a.sg[ch] = a.sbr[ch] = 0ull;
    }
}

// the record of a run, the order of a mesh record: n, sum v, sum v^2, n_int, sum L, sum L^2, sum G, sum Br
template <int C> struct IqRec { unsigned long long s[C][IQ_TILE]; };

template <int C> __device__ inline IqRec<C> iq_rec(const IqRun<C>& a)
{
    IqRec<C> o;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        o.s[ch][0] = a.n;
        o.s[ch][1] = a.sv[ch];
        o.s[ch][2] = a.sv2[ch];
        o.s[ch][3] = a.n_int;
        o.s[ch][4] = (unsigned long long)(long long)a.sl[ch];
        o.s[ch][5] = a.sl2[ch];
        o.s[ch][6] = a.sg[ch];
        o.s[ch][7] = a.sbr[ch];
    }
    return o;
}

struct IqMesh {
    unsigned long long* tiles;                          // [B][C][m_r][m_c][8]; per_wg: [B][C][workgroups of an image][8]
    int m_r, m_c;
    int per_wg;                                         // no mesh (m_r = m_c = 1): every workgroup stores its own sums
};

template <int C> struct IqLds {
    unsigned long long s[C][IQ_TILE][IQ_SLOTS];
    unsigned int part[LT_WAVES][C][IQ_PART];
};

// tr, tc: the mesh tile; tr0, tc0: the first the workgroup tile meets, lc of them across
template <int C>
__device__ inline void iq_insert(IqLds<C>& L, const IqMesh& M, int b, int tr, int tc, int tr0, int tc0, int lc, const IqRec<C>& o)
{
    const int slot = (tr - tr0) * lc + (tc - tc0);
    if (slot < IQ_SLOTS) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
#pragma unroll
            for (int j = 0; j < IQ_TILE; ++j) atomicAdd(&L.s[ch][j][slot], o.s[ch][j]);
        return;
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {                    // no room: straight to the global table
        unsigned long long* g = M.tiles + ((((size_t)b * C + ch) * M.m_r + tr) * M.m_c + tc) * IQ_TILE;
#pragma unroll
        for (int j = 0; j < IQ_TILE; ++j) atomicAdd(&g[j], o.s[ch][j]);
    }
}

struct IqSat { unsigned int level[kIqMaxChannels]; };

// grid (ceil(W/256), ceil(H/64), B).  image: [B][H][W][C] PIX.  vec: the width is a multiple of 4 and the pointer allows the wide
// loads (decided on the host).  part: [B][workgroups of an image][C][IQ_PART].
// Registers: 81 / 144 / 205 / 256 VGPRs at C = 1 / 2 / 3 / 4 (three rows of 6 C words, the row in flight, the run's 6 C + 2 sums,
// 5 C extremes and counts).  At C = 4 that is the most a wave can have, one wave per SIMD and no spill: anything added per channel
// to this kernel spills there, so split the channels into two launches first.
template <typename PIX, int C>
__global__ __launch_bounds__(IQ_THREADS) void iq_pass(const PIX* __restrict__ image, int H, int W, int vec, IqMesh M, IqSat sat,
                                                      unsigned int* __restrict__ part)
{
    __shared__ IqLds<C> L;
    for (int s = threadIdx.x; s < IQ_SLOTS; s += IQ_THREADS)
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
#pragma unroll
            for (int j = 0; j < IQ_TILE; ++j) L.s[ch][j][s] = 0ull;
    __syncthreads();

    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const PIX* im = image + (size_t)b * H * W * C;
    const bool wide = vec && c_base + 3 < W;
    // the mesh tiles the workgroup tile meets: rows tr0.., columns tc0..tc1
    const int tr0 = (int)(((long long)tile.r0 * M.m_r) / H), tc0 = (int)(((long long)tile.c0 * M.m_c) / W);
    const int tc1 = (int)(((long long)min(tile.c0 + LT_COLS - 1, W - 1) * M.m_c) / W), lc = tc1 - tc0 + 1;
    int tcol[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tcol[k] = (int)(((long long)min(c_base + k, W - 1) * M.m_c) / W);

    unsigned int mn[C], n_mn[C], mx[C], n_mx[C], n_sat[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        mn[ch] = 0xFFFFFFFFu;
        mx[ch] = 0u;
        n_mn[ch] = n_mx[ch] = n_sat[ch] = 0u;
    }
    int cur_r = 0, cur_c = 0;                           // the open run's mesh tile; run.n == 0: none
    IqRun<C> run;
    iq_reset<C>(run);
    unsigned int ra[6 * C], rm[6 * C], rn[6 * C];
    QRaw<PIX, C> raw;
    q_issue<PIX, C>(im, tile.r_base - 1, H, W, c_base, lane, wide, raw);
    q_finish<PIX, C>(raw, lane, ra);
    q_issue<PIX, C>(im, tile.r_base, H, W, c_base, lane, wide, raw);
    q_finish<PIX, C>(raw, lane, rm);
    q_issue<PIX, C>(im, tile.r_base + 1, H, W, c_base, lane, wide, raw);
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        q_finish<PIX, C>(raw, lane, rn);            // row r + 1, loaded under the sums of row r - 1
        q_issue<PIX, C>(im, r + 2, H, W, c_base, lane, wide, raw);
        const int tr = (int)(((long long)r * M.m_r) / H);
        const bool r_in = r >= 1 && r <= H - 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c_base + k;
            if (c >= W) continue;
            if (run.n != 0u && (tr != cur_r || tcol[k] != cur_c)) {
                iq_insert<C>(L, M, b, cur_r, cur_c, tr0, tc0, lc, iq_rec<C>(run));
                iq_reset<C>(run);
            }
            cur_r = tr;
            cur_c = tcol[k];
            const bool interior = r_in && c >= 1 && c <= W - 2;
            ++run.n;
            run.n_int += interior ? 1u : 0u;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const unsigned int v = rm[(k + 1) * C + ch];
                run.sv[ch] += v;
                run.sv2[ch] += (unsigned long long)(v * v);       // 65535^2 < 2^32
                if (v < mn[ch]) { mn[ch] = v; n_mn[ch] = 0u; }
                n_mn[ch] += v == mn[ch] ? 1u : 0u;
                if (v > mx[ch]) { mx[ch] = v; n_mx[ch] = 0u; }
                n_mx[ch] += v == mx[ch] ? 1u : 0u;
                n_sat[ch] += v >= sat.level[ch] ? 1u : 0u;
                if (interior) {
                    const QFocus f = q_focus<C>(ra, rm, rn, k, ch);
                    run.sl[ch] += f.l;
                    run.sl2[ch] += f.l2;
                    run.sg[ch] += f.g;
                    run.sbr[ch] += f.br;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 6 * C; ++j) {
            ra[j] = rm[j];
            rm[j] = rn[j];
        }
    }
    // the open run of every lane: one insertion per distinct mesh tile of the wave
    const IqRec<C> mine_rec = iq_rec<C>(run);
    merge_open_runs(run.n != 0u, cur_r * M.m_c + cur_c, lane, [&](int key, bool mine, bool leader) {
        IqRec<C> o;
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
#pragma unroll
            for (int j = 0; j < IQ_TILE; ++j) o.s[ch][j] = wave_sum(mine ? mine_rec.s[ch][j] : 0ull);
        if (leader) iq_insert<C>(L, M, b, key / M.m_c, key % M.m_c, tr0, tc0, lc, o);
    });
    // the extremes with their counts: per wave, then per workgroup.  A lane without pixels holds (2^32 - 1, 0) and (0, 0).
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const unsigned int lo = wave_min(mn[ch]), hi = wave_max(mx[ch]);
        const unsigned int n_lo = wave_sum(mn[ch] == lo ? n_mn[ch] : 0u), n_hi = wave_sum(mx[ch] == hi ? n_mx[ch] : 0u);
        const unsigned int ns = wave_sum(n_sat[ch]);
        if (lane == 0) {
            unsigned int* w = L.part[tile.wave][ch];
            w[0] = lo; w[1] = n_lo; w[2] = hi; w[3] = n_hi; w[4] = ns;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int ch = threadIdx.x;
        unsigned int lo = 0xFFFFFFFFu, n_lo = 0u, hi = 0u, n_hi = 0u, ns = 0u;
        for (int w = 0; w < LT_WAVES; ++w) {
            const unsigned int* q = L.part[w][ch];
            if (q[0] < lo) { lo = q[0]; n_lo = 0u; }
            if (q[0] == lo) n_lo += q[1];
            if (q[2] > hi) { hi = q[2]; n_hi = 0u; }
            if (q[2] == hi) n_hi += q[3];
            ns += q[4];
        }
        const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x, n_wg = (size_t)gridDim.x * gridDim.y;
        unsigned int* o = part + (((size_t)b * n_wg + wg) * C + ch) * IQ_PART;
        o[0] = lo; o[1] = n_lo; o[2] = hi; o[3] = n_hi; o[4] = ns;
    }
    // the mesh tiles the workgroup touched
    if (M.per_wg) {                                     // one slot, plain stores: 2048 atomics on 8 addresses would queue
        const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x, n_wg = (size_t)gridDim.x * gridDim.y;
        for (int s = threadIdx.x; s < C * IQ_TILE; s += IQ_THREADS)
            M.tiles[(((size_t)b * C + s / IQ_TILE) * n_wg + wg) * IQ_TILE + s % IQ_TILE] = L.s[s / IQ_TILE][s % IQ_TILE][0];
        return;
    }
    for (int s = threadIdx.x; s < IQ_SLOTS; s += IQ_THREADS) {
        if (L.s[0][0][s] == 0ull) continue;             // n == 0: untouched
        const int tr = tr0 + s / lc, tc = tc0 + s % lc;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            unsigned long long* g = M.tiles + ((((size_t)b * C + ch) * M.m_r + tr) * M.m_c + tc) * IQ_TILE;
#pragma unroll
            for (int j = 0; j < IQ_TILE; ++j) atomicAdd(&g[j], L.s[ch][j][s]);
        }
    }
}

// the sum of v over the workgroup, on thread 0 (others: undefined); scratch: LT_WAVES words, reusable after the call
__device__ inline unsigned long long iq_block_sum(unsigned long long v, unsigned long long* scratch)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0ull;
    for (int w = 0; w < LT_WAVES; ++w) t += scratch[w];
    return t;
}

// grid B * C.  tiles: [B][C][n_tiles][8]; part: [B][n_wg][C][IQ_PART]; records: [B][C][13]
__global__ __launch_bounds__(IQ_THREADS) void iq_close(const unsigned long long* __restrict__ tiles, int n_tiles,
                                                       const unsigned int* __restrict__ part, int n_wg, int C,
                                                       unsigned long long* __restrict__ records)
{
    __shared__ unsigned long long scratch[LT_WAVES];
    __shared__ unsigned int ext[2];
    const int b = blockIdx.x / C, ch = blockIdx.x % C;
    const unsigned long long* t = tiles + (size_t)blockIdx.x * n_tiles * IQ_TILE;
    unsigned long long s[IQ_TILE] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int i = threadIdx.x; i < n_tiles; i += IQ_THREADS)
#pragma unroll
        for (int j = 0; j < IQ_TILE; ++j) s[j] += t[(size_t)i * IQ_TILE + j];
    unsigned long long* o = records + (size_t)blockIdx.x * IQ_REC;
    constexpr int place[IQ_TILE] = {0, 1, 2, 8, 9, 10, 11, 12};
#pragma unroll
    for (int j = 0; j < IQ_TILE; ++j) {
        const unsigned long long v = iq_block_sum(s[j], scratch);
        if (threadIdx.x == 0) o[place[j]] = v;
    }
    // the extremes first, then the counts at them
    unsigned int lo = 0xFFFFFFFFu, hi = 0u;
    for (int i = threadIdx.x; i < n_wg; i += IQ_THREADS) {
        const unsigned int* q = part + (((size_t)b * n_wg + i) * C + ch) * IQ_PART;
        lo = min(lo, q[0]);
        hi = max(hi, q[2]);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (threadIdx.x == 0) { ext[0] = 0xFFFFFFFFu; ext[1] = 0u; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&ext[0], lo);
        atomicMax(&ext[1], hi);
    }
    __syncthreads();
    lo = ext[0];
    hi = ext[1];
    unsigned long long n_lo = 0ull, n_hi = 0ull, ns = 0ull;
    for (int i = threadIdx.x; i < n_wg; i += IQ_THREADS) {
        const unsigned int* q = part + (((size_t)b * n_wg + i) * C + ch) * IQ_PART;
        if (q[0] == lo) n_lo += q[1];
        if (q[2] == hi) n_hi += q[3];
        ns += q[4];
    }
    n_lo = iq_block_sum(n_lo, scratch);
    n_hi = iq_block_sum(n_hi, scratch);
    ns = iq_block_sum(ns, scratch);
    if (threadIdx.x == 0) {
        o[3] = lo; o[4] = hi; o[5] = n_lo; o[6] = n_hi; o[7] = ns;
    }
}

template <typename PIX>
static void iq_launch_c(int C, const void* image, int batch, int H, int W, int vec, const IqMesh& M, const IqSat& sat, unsigned int* part,
                        hipStream_t st)
{
    const dim3 grid = label_tile_grid(batch, H, W), block(IQ_THREADS);
    switch (C) {
    case 1: hipLaunchKernelGGL((iq_pass<PIX, 1>), grid, block, 0, st, (const PIX*)image, H, W, vec, M, sat, part); break;
    case 2: hipLaunchKernelGGL((iq_pass<PIX, 2>), grid, block, 0, st, (const PIX*)image, H, W, vec, M, sat, part); break;
    case 3: hipLaunchKernelGGL((iq_pass<PIX, 3>), grid, block, 0, st, (const PIX*)image, H, W, vec, M, sat, part); break;
    default: hipLaunchKernelGGL((iq_pass<PIX, 4>), grid, block, 0, st, (const PIX*)image, H, W, vec, M, sat, part); break;
    }
}

// ---- the object pass ---------------------------------------------------------------------------------------------------------
template <int C> struct LfSlots { static constexpr int log2 = C == 1 ? 9 : 8; };

// the sums of a run or of a merged set of runs, image coordinates: area, sum r, sum c, n_int, then per channel sum L, L^2, G, Br
template <int C> struct LfRec { unsigned long long s[4 + 4 * C]; };

// a lane's open run, tile coordinates (r in 0..63, c in 0..255, at most 64 pixels)
template <int C> struct LfRun {
    unsigned int n, sr, sc, n_int;
    int sl[C];
    unsigned long long sl2[C], sg[C], sbr[C];
};

template <int C> __device__ inline void lf_reset(LfRun<C>& a)
{
    a.n = a.sr = a.sc = a.n_int = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        a.sl[ch] = 0;
        a.sl2[ch] = a.sg[ch] = a.sbr[ch] = 0ull;
    }
}

template <int C> __device__ inline LfRec<C> lf_rec(const LfRun<C>& a, unsigned int r0, unsigned int c0)
{
    LfRec<C> o;
    o.s[0] = a.n;
    o.s[1] = a.sr + (unsigned long long)a.n * r0;
    o.s[2] = a.sc + (unsigned long long)a.n * c0;
    o.s[3] = a.n_int;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        o.s[4 + 4 * ch] = (unsigned long long)(long long)a.sl[ch];
        o.s[5 + 4 * ch] = a.sl2[ch];
        o.s[6 + 4 * ch] = a.sg[ch];
        o.s[7 + 4 * ch] = a.sbr[ch];
    }
    return o;
}

struct LfTables {
    unsigned long long* geom;                           // [B][max_label][3]
    unsigned long long* focus;                          // [B][max_label][C][5]
    int max_label;
};

// label is in 1..max_label
template <int C> __device__ inline void lf_global(const LfTables& T, int b, int label, const LfRec<C>& o)
{
    const size_t row = (size_t)b * T.max_label + (label - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicAdd(&T.geom[row * 3 + j], o.s[j]);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        unsigned long long* f = T.focus + (row * C + ch) * IQ_FOCUS;
        atomicAdd(&f[0], o.s[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&f[1 + j], o.s[4 + 4 * ch + j]);
    }
}

template <int C> struct LfLds {
    static constexpr int SLOTS = 1 << LfSlots<C>::log2;
    int key[SLOTS];                                     // 0: empty
    unsigned long long s[4 + 4 * C][SLOTS];
};

template <int C> __device__ inline void lf_insert(LfLds<C>& L, const LfTables& T, int b, int label, const LfRec<C>& o)
{
    const int h = table_claim(L.key, LfSlots<C>::log2, ((unsigned int)label * 0x9E3779B1u) >> (32 - LfSlots<C>::log2), label, LF_LDS_PROBES);
    if (h < 0) {
        lf_global<C>(T, b, label, o);                   // no room: straight to the global tables
        return;
    }
#pragma unroll
    for (int j = 0; j < 4 + 4 * C; ++j) atomicAdd(&L.s[j][h], o.s[j]);
}

// grid (ceil(W/256), ceil(H/64), B).  image: [B][H][W][C] PIX; labels, exclude (or null): [B][H][W] int.  vec: the width is a
// multiple of 4 and every plane's pointer allows the wide loads (decided on the host).
template <typename PIX, int C>
__global__ __launch_bounds__(IQ_THREADS) void lf_pass(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                      const int* __restrict__ exclude, int H, int W, int vec, LfTables T,
                                                      unsigned int* __restrict__ ctrl)
{
    constexpr int SLOTS = LfLds<C>::SLOTS;
    __shared__ LfLds<C> L;
    for (int s = threadIdx.x; s < SLOTS; s += IQ_THREADS) {
        L.key[s] = 0;
#pragma unroll
        for (int j = 0; j < 4 + 4 * C; ++j) L.s[j][s] = 0ull;
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

    unsigned int bad = 0u;
    int cur = 0;                                        // the open run's label; run.n == 0: none
    LfRun<C> run;
    lf_reset<C>(run);
    unsigned int ra[6 * C], rm[6 * C], rn[6 * C];
    QRaw<PIX, C> raw;
    q_issue<PIX, C>(im, tile.r_base - 1, H, W, c_base, lane, wide, raw);
    q_finish<PIX, C>(raw, lane, ra);
    q_issue<PIX, C>(im, tile.r_base, H, W, c_base, lane, wide, raw);
    q_finish<PIX, C>(raw, lane, rm);
    q_issue<PIX, C>(im, tile.r_base + 1, H, W, c_base, lane, wide, raw);
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        q_finish<PIX, C>(raw, lane, rn);            // row r + 1, loaded under the sums of row r - 1
        q_issue<PIX, C>(im, r + 2, H, W, c_base, lane, wide, raw);
        int x[4], e[4] = {0, 0, 0, 0};
        const size_t at = (size_t)r * W + c_base;
        const int n_in = min(4, W - c_base);            // <= 0: the lane is off the image
        label_load4(ll + at, n_in, wide, x);
        if (ee) label_load4(ee + at, n_in, wide, e);
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
        const bool r_in = r >= 1 && r <= H - 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab == 0) continue;
            if (lab < 0 || lab > T.max_label) { bad = 1u; continue; }
            if (e[k] != 0) continue;
            if (run.n != 0u && lab != cur) {
                lf_insert<C>(L, T, b, cur, lf_rec<C>(run, r0, c0));
                run.n = 0u;
            }
            const unsigned int cc = (unsigned int)(4 * lane + k);
            if (run.n == 0u) {
                cur = lab;
                lf_reset<C>(run);
            }
            ++run.n;
            run.sr += rr;
            run.sc += cc;
            const int c = c_base + k;
            if (r_in && c >= 1 && c <= W - 2) {
                ++run.n_int;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const QFocus f = q_focus<C>(ra, rm, rn, k, ch);
                    run.sl[ch] += f.l;
                    run.sl2[ch] += f.l2;
                    run.sg[ch] += f.g;
                    run.sbr[ch] += f.br;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 6 * C; ++j) {
            ra[j] = rm[j];
            rm[j] = rn[j];
        }
    }
    // the open run of every lane: one insertion per distinct label of the wave
    const LfRec<C> mine_rec = lf_rec<C>(run, r0, c0);
    merge_open_runs(run.n != 0u, cur, lane, [&](int label, bool mine, bool leader) {
        LfRec<C> o;
#pragma unroll
        for (int j = 0; j < 4 + 4 * C; ++j) o.s[j] = wave_sum(mine ? mine_rec.s[j] : 0ull);
        if (leader) lf_insert<C>(L, T, b, label, o);
    });
    __syncthreads();
    // the distinct labels of the tile
    for (int s = threadIdx.x; s < SLOTS; s += IQ_THREADS) {
        const int label = L.key[s];
        if (label == 0) continue;
        LfRec<C> o;
#pragma unroll
        for (int j = 0; j < 4 + 4 * C; ++j) o.s[j] = L.s[j][s];
        lf_global<C>(T, b, label, o);
    }
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

template <typename PIX>
static void lf_launch_c(int C, const void* image, const int* labels, const int* exclude, int batch, int H, int W, int vec, const LfTables& T,
                        unsigned int* ctrl, hipStream_t st)
{
    const dim3 grid = label_tile_grid(batch, H, W), block(IQ_THREADS);
    switch (C) {
    case 1: hipLaunchKernelGGL((lf_pass<PIX, 1>), grid, block, 0, st, (const PIX*)image, labels, exclude, H, W, vec, T, ctrl); break;
    case 2: hipLaunchKernelGGL((lf_pass<PIX, 2>), grid, block, 0, st, (const PIX*)image, labels, exclude, H, W, vec, T, ctrl); break;
    case 3: hipLaunchKernelGGL((lf_pass<PIX, 3>), grid, block, 0, st, (const PIX*)image, labels, exclude, H, W, vec, T, ctrl); break;
    default: hipLaunchKernelGGL((lf_pass<PIX, 4>), grid, block, 0, st, (const PIX*)image, labels, exclude, H, W, vec, T, ctrl); break;
    }
}

// what the passes assume of 4 pixels: PXA of q_issue
static int q_align(size_t esz, int C)
{
    constexpr int PA[2][4] = {{4, 8, 4, 16}, {8, 16, 8, 16}};
    return PA[esz - 1][C - 1];
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_image_quality(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t batch, int32_t height, int32_t width,
                     int in_kind, int32_t tile, const int32_t* sat_level, int64_t* records, int64_t* mesh, int out_kind)
{
    if (!image || !records) return fail(CS_ERR_INVALID, "NULL argument");
    if (tile != 0 && !mesh) return fail(CS_ERR_INVALID, "mesh is NULL with tile %d", (int)tile);
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (tile != 0 && (tile < 16 || tile > 1024)) return fail(CS_ERR_INVALID, "tile %d: must be 0 (no mesh) or 16..1024", (int)tile);
    if (channels > kIqMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kIqMaxChannels);
    IqSat sat;
    for (int ch = 0; ch < kIqMaxChannels; ++ch) {
        const int32_t level = sat_level && ch < channels ? sat_level[ch] : (pixel_type == CS_PIX_U8 ? 255 : 65535);
        if (level < 0 || level > 65536) return fail(CS_ERR_INVALID, "sat_level[%d] = %d: must be 0..65536", ch, (int)level);
        sat.level[ch] = (unsigned int)level;
    }
    if ((rc = image_limits(batch, height, width))) return rc;
    const int H = height, W = width, C = channels;
    const int m_r = tile ? (H + tile - 1) / tile : 1, m_c = tile ? (W + tile - 1) / tile : 1, n_tiles = m_r * m_c;
    if ((int64_t)batch * C * n_tiles > kIqMaxTiles)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x channels %d x mesh %d x %d: the mesh is capped at %lld tiles per call", (int)batch, C, m_r,
                    m_c, (long long)kIqMaxTiles);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const dim3 grid = label_tile_grid(batch, H, W);
    const int n_wg = (int)(grid.x * grid.y);
    const size_t rbytes = (size_t)batch * C * IQ_REC * sizeof(int64_t), mbytes = (size_t)batch * C * n_tiles * IQ_TILE * sizeof(int64_t);
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    const void* d_img = image;
    if (in_host) {
        if ((rc = S.img.ensure(npx * C * esz))) return rc;
        HIPCHK(hipMemcpyAsync(S.img.p, image, npx * C * esz, hipMemcpyHostToDevice, st));
        d_img = S.img.p;
    }
    if ((rc = S.slab.ensure((size_t)batch * n_wg * C * IQ_PART * sizeof(unsigned int)))) return rc;
    if (out_host && (rc = S.stage.ensure(rbytes + (tile ? mbytes : 0)))) return rc;    // the records, then the mesh
    const size_t wbytes = (size_t)batch * C * n_wg * IQ_TILE * sizeof(int64_t);        // without a mesh: a tile per workgroup
    if (!tile && (rc = S.hist.ensure(wbytes))) return rc;
    unsigned long long* d_rec = out_host ? S.stage.as<unsigned long long>() : (unsigned long long*)records;
    unsigned long long* d_mesh = !tile ? S.hist.as<unsigned long long>()
                                       : out_host ? (unsigned long long*)(S.stage.as<char>() + rbytes) : (unsigned long long*)mesh;
    const int vec = (W & 3) == 0 && ((uintptr_t)d_img & (uintptr_t)(q_align(esz, C) - 1)) == 0;
    const IqMesh M{d_mesh, m_r, m_c, tile ? 0 : 1};

    if ((rc = S.clk_iq.record(0, st))) return rc;
    if (tile) {                                         // without a mesh every word is stored
        HIPCHK(hipMemsetAsync(d_mesh, 0, mbytes, st));
    }
    if ((rc = S.clk_iq.record(1, st))) return rc;
    if (pixel_type == CS_PIX_U8) iq_launch_c<unsigned char>(C, d_img, batch, H, W, vec, M, sat, S.slab.as<unsigned int>(), st);
    else iq_launch_c<unsigned short>(C, d_img, batch, H, W, vec, M, sat, S.slab.as<unsigned int>(), st);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(iq_close, dim3((unsigned)(batch * C)), dim3(IQ_THREADS), 0, st, d_mesh, tile ? n_tiles : n_wg, S.slab.as<unsigned int>(), n_wg, C, d_rec);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_iq.record(2, st))) return rc;
    if (out_host) {
        HIPCHK(hipMemcpyAsync(records, d_rec, rbytes, hipMemcpyDeviceToHost, st));
        if (tile) {
            HIPCHK(hipMemcpyAsync(mesh, d_mesh, mbytes, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation
    return S.clk_iq.finish();
}

int cs_image_quality_last_timing(const cs_preproc* p, double* clear_ms, double* pass_ms)
{
    return clock_read(p, &SegmentState::clk_iq, {clear_ms, pass_ms});
}

int cs_object_focus(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                   int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, int64_t* geom, int64_t* focus, int out_kind)
{
    if (!image || !labels || !geom || !focus) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kIqMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kIqMaxChannels);
    if ((rc = label_cap("max_label", max_label, batch, channels, kLfMaxCells, "the tables", "cells")) || (rc = image_limits(batch, height, width)) ||
        (rc = handle_check(p)) || (rc = state_begin(p)))
        return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width, C = channels;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const int64_t rows = (int64_t)batch * max_label, cells = rows * C;
    const size_t gbytes = (size_t)rows * 3 * sizeof(int64_t), fbytes = (size_t)cells * IQ_FOCUS * sizeof(int64_t);
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
    if (out_host && (rc = S.stage.ensure(gbytes + fbytes))) return rc;      // both tables on their way to the host: geom, then focus
    unsigned long long* d_geom = out_host ? S.stage.as<unsigned long long>() : (unsigned long long*)geom;
    unsigned long long* d_focus = out_host ? (unsigned long long*)(S.stage.as<char>() + gbytes) : (unsigned long long*)focus;
    const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0 &&
                    ((uintptr_t)d_img & (uintptr_t)(q_align(esz, C) - 1)) == 0;
    const LfTables T{d_geom, d_focus, (int)max_label};

    if ((rc = S.clk_lf.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(S.ctrl.p, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
    HIPCHK(hipMemsetAsync(d_focus, 0, fbytes, st));
    if ((rc = S.clk_lf.record(1, st))) return rc;
    if (pixel_type == CS_PIX_U8) lf_launch_c<unsigned char>(C, d_img, d_lab, d_ex, batch, H, W, vec, T, S.ctrl.as<unsigned int>(), st);
    else lf_launch_c<unsigned short>(C, d_img, d_lab, d_ex, batch, H, W, vec, T, S.ctrl.as<unsigned int>(), st);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_lf.record(2, st))) return rc;
    unsigned int bad = 0u;
    HIPCHK(hipMemcpyAsync(&bad, S.ctrl.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(focus, d_focus, fbytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host tables
    if ((rc = S.clk_lf.finish())) return rc;
    if (bad) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    return CS_OK;
}

int cs_object_focus_last_timing(const cs_preproc* p, double* clear_ms, double* pass_ms)
{
    return clock_read(p, &SegmentState::clk_lf, {clear_ms, pass_ms});
}
