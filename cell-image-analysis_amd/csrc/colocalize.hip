// colocalize.hip -- per-object colocalization between the channels of an image on gfx950 (include/cellscreen.h,
// cs_label_colocalize; the rule and the sizing: DESIGN 3z, restated in tests/colocalize_reference.py).
//
// Per object (a label > 0 of an image, less the pixels where `exclude` is non-zero), channel c and pair of channels i < j: the
// sums Pearson's r, the regression slope, Manders' M1 / M2, the overlap coefficient, K1 / K2 and the rank-weighted coefficients
// follow from on the host.  All integers.  As li_pass (intensity.hip), the design makes scattered global atomics rare instead of
// fast: a lane keeps one open run of its label, runs go into a table in LDS keyed by the label, the lanes' last runs are first
// merged per distinct label of the wave, and only the distinct labels of a tile go on to the dense tables, as 64-bit atomics.
//   lc_moments      one read of every plane on the tile of label_tile.hpp: area, sum r, sum c (cs_label_intensity's geom bit for
//                   bit), per channel sum v, sum v^2, max v, per pair sum v_i v_j.  With rwc it marks every value an object pixel
//                   holds in a presence table [B][C][65536] bytes, by plain stores of the constant 1.
//                   A record is 3 + 2 C + P sums of 8 bytes, C words and its key: 76 / 112 / 156 bytes at C = 2 / 3 / 4, in
//                   512 / 256 / 256 slots: 38 / 28 / 39 KB of LDS, 4 / 5 / 4 workgroups per CU by LDS.
//   lc_ranks        one workgroup per (image, channel): the presence table into dense ranks (uint16) by an exclusive prefix
//                   count, a wave per 1/16 of the values, 64 values per step by ballot; the number of distinct values in levels.
//   lc_thresholded  the second walk.  When a lane's run changes label it reads the object's C maxima from the dense table of
//                   lc_moments (nothing in absolute mode), decides "above" per channel and sums per channel n_above, sum v[above]
//                   and per pair over the pixels above in both: n, sum v_i, v_j, v_i^2, v_j^2, v_i v_j and, with rwc, v_i w, v_j w
//                   with w = R - |rank_i - rank_j| from the rank tables (128 KB per image and channel: they stay in L2).
//                   A record is 2 C + 8 P (6 P without rwc) sums of 8 bytes: 12 / 30 / 56 at C = 2 / 3 / 4, in 512 / 256 / 128
//                   slots: 52 / 62 / 57 KB of LDS, 3 / 2 / 2 workgroups per CU by LDS.
// A label that finds no room in LDS goes to the global tables directly.  No floating point; every result is a sum or a maximum
// of integers, so it does not depend on the order of arrival or on slot placement, and is bit-identical run to run.  A label is
// range-checked before it is a key or an index.  Every product stays unsigned below 2^32: v_i v_j <= 65535^2, v den <= 65535 *
// 65536, num max <= 65536 * 65535, v w <= 65535 * 65536.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int LC_THREADS = LT_THREADS;
static constexpr int LC_RANK_THREADS = 1024;
static constexpr int LC_RANK_WAVES = LC_RANK_THREADS / 64;
static constexpr int LC_LDS_PROBES = 16;
static constexpr int LC_LEVELS = 65536;                 // the stride of a presence or rank table; uint8 uses its first 256
static constexpr int kLcMaxChannels = 4;
static constexpr int64_t kLcMaxCells = 1 << 22;         // batch * max_label * channels
static constexpr size_t kLcScratchPer = 3 * (size_t)LC_LEVELS;  // bytes per image and channel: presence + uint16 ranks
static constexpr size_t kLcMaxScratch = (size_t)1 << 30;

constexpr int lc_pairs(int C) { return C * (C - 1) / 2; }
template <int C> struct LcSlotsA { static constexpr int log2 = C == 2 ? 9 : 8; };
template <int C> struct LcSlotsB { static constexpr int log2 = C == 2 ? 9 : C == 3 ? 8 : 7; };

// merged sums under a label: N sums and M maxima
template <int N, int M> struct LcRec {
    unsigned long long s[N];
    unsigned int mx[M > 0 ? M : 1];
};

template <int N, int M, int LOG2> struct LcLds {
    static constexpr int SLOTS = 1 << LOG2;
    int key[SLOTS];                                     // 0: empty
    unsigned long long s[N][SLOTS];
    unsigned int mx[M > 0 ? M : 1][SLOTS];
};

template <int N, int M, int LOG2> __device__ inline void lc_lds_clear(LcLds<N, M, LOG2>& L)
{
    for (int s = threadIdx.x; s < (1 << LOG2); s += LC_THREADS) {
        L.key[s] = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) L.s[j][s] = 0ull;
#pragma unroll
        for (int m = 0; m < M; ++m) L.mx[m][s] = 0u;
    }
}

// false: no room within the probes, the caller goes to the global tables
template <int N, int M, int LOG2> __device__ inline bool lc_insert(LcLds<N, M, LOG2>& L, int label, const LcRec<N, M>& o)
{
    const unsigned int h = ((unsigned int)label * 0x9E3779B1u) >> (32 - LOG2);
    const int s = table_claim(L.key, LOG2, h, label, LC_LDS_PROBES);
    if (s < 0) return false;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (o.s[j] != 0ull) atomicAdd(&L.s[j][s], o.s[j]);
#pragma unroll
    for (int m = 0; m < M; ++m) atomicMax(&L.mx[m][s], o.mx[m]);
    return true;
}

// Where sum j and maximum m of a label's record go in the global tables is the kernel's: a sink has sum(label, j) and
// top(label, m).  label is in 1..max_label.
template <int N, int M, typename S> __device__ inline void lc_global(const S& sink, int label, const LcRec<N, M>& o)
{
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (o.s[j] != 0ull) atomicAdd(sink.sum(label, j), o.s[j]);
#pragma unroll
    for (int m = 0; m < M; ++m) atomicMax(sink.top(label, m), (unsigned long long)o.mx[m]);
}

// The open run of every lane: one insertion per distinct label of the wave.  The leader claims the slot, then every sum is
// reduced over the wave and added by the leader at once, so that no merged record is held in registers.  Called by whole waves.
template <int N, int M, int LOG2, typename S>
__device__ inline void lc_close(LcLds<N, M, LOG2>& L, bool open, int cur, int lane, const LcRec<N, M>& mine_rec, const S& sink)
{
    merge_open_runs(open, cur, lane, [&](int lw, bool mine, bool leader) {
        int slot = -1;
        if (leader) slot = table_claim(L.key, LOG2, ((unsigned int)lw * 0x9E3779B1u) >> (32 - LOG2), lw, LC_LDS_PROBES);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const unsigned long long t = wave_sum(mine ? mine_rec.s[j] : 0ull);
            if (!leader || t == 0ull) continue;
            if (slot >= 0) atomicAdd(&L.s[j][slot], t);
            else atomicAdd(sink.sum(lw, j), t);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const unsigned int t = wave_max(mine ? mine_rec.mx[m] : 0u);
            if (!leader) continue;
            if (slot >= 0) atomicMax(&L.mx[m][slot], t);
            else atomicMax(sink.top(lw, m), (unsigned long long)t);
        }
    });
}

// the distinct labels of the tile, after a barrier
template <int N, int M, int LOG2, typename S> __device__ inline void lc_drain(const LcLds<N, M, LOG2>& L, const S& sink)
{
    for (int s = threadIdx.x; s < (1 << LOG2); s += LC_THREADS) {
        const int label = L.key[s];
        if (label == 0) continue;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const unsigned long long t = L.s[j][s];
            if (t != 0ull) atomicAdd(sink.sum(label, j), t);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) atomicMax(sink.top(label, m), (unsigned long long)L.mx[m][s]);
    }
}

struct LcTables {
    unsigned long long* geom;                           // [B][max_label][3]
    unsigned long long* chan;                           // [B][max_label][C][5]
    unsigned long long* pair;                           // [B][max_label][P][9]
    int max_label;
};

struct LcThreshold {
    unsigned int num, den;                              // above iff v * den >= num * max_c; absolute: den = 1
    unsigned int abs_thr[4];                            // absolute: above iff v >= abs_thr[c]
    int absolute;
};

// A lane's four pixels of one row, as li_pass loads them.  labels x, exclude e (zeros without the plane), pixels px[k * C + ch].
template <typename PIX, int C>
__device__ inline void lc_load(const PIX* im, const int* ll, const int* ee, size_t at, int c_base, int W, bool wide, int (&x)[4], int (&e)[4],
                               PIX (&px)[4 * C])
{
    // the widest load the image rows allow: 4 pixels are 4 C sizeof(PIX) bytes, aligned to their largest power of two
    constexpr int PXB = 4 * C * (int)sizeof(PIX);
    constexpr int PXA = (PXB & -PXB) < 16 ? (PXB & -PXB) : 16;
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
}

// ---- lc_moments ---------------------------------------------------------------------------------------------------------------
// a lane's open run, tile coordinates (r in 0..63, c in 0..255, at most 64 pixels): everything but the products fits 32 bits
template <int C> struct LcRunA {
    unsigned int n, sr, sc, sv[C], mx[C];
    unsigned long long sv2[C], svv[lc_pairs(C)];
};

template <int C> __device__ inline void lc_reset(LcRunA<C>& a)
{
    a.n = a.sr = a.sc = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        a.sv[ch] = a.mx[ch] = 0u;
        a.sv2[ch] = 0ull;
    }
#pragma unroll
    for (int p = 0; p < lc_pairs(C); ++p) a.svv[p] = 0ull;
}

// image coordinates: area, sum r, sum c; per channel sum v, sum v^2; per pair sum v_i v_j; the maxima
template <int C> using LcRecA = LcRec<3 + 2 * C + lc_pairs(C), C>;

template <int C> __device__ inline LcRecA<C> lc_rec(const LcRunA<C>& a, unsigned int r0, unsigned int c0)
{
    LcRecA<C> o;
    o.s[0] = a.n;
    o.s[1] = a.sr + (unsigned long long)a.n * r0;
    o.s[2] = a.sc + (unsigned long long)a.n * c0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        o.s[3 + 2 * ch] = a.sv[ch];
        o.s[4 + 2 * ch] = a.sv2[ch];
        o.mx[ch] = a.mx[ch];
    }
#pragma unroll
    for (int p = 0; p < lc_pairs(C); ++p) o.s[3 + 2 * C + p] = a.svv[p];
    return o;
}

template <int C> struct LcSinkA {
    LcTables T;
    int b;
    __device__ unsigned long long* sum(int label, int j) const
    {
        const size_t row = (size_t)b * T.max_label + (label - 1);
        if (j < 3) return T.geom + row * 3 + j;
        if (j < 3 + 2 * C) return T.chan + (row * C + (j - 3) / 2) * 5 + (j - 3) % 2;
        return T.pair + (row * lc_pairs(C) + (j - 3 - 2 * C)) * 9;
    }
    __device__ unsigned long long* top(int label, int m) const { return T.chan + (((size_t)b * T.max_label + (label - 1)) * C + m) * 5 + 2; }
};

// grid (ceil(W/256), ceil(H/64), B).  image: [B][H][W][C] PIX; labels, exclude (or null): [B][H][W] int.  vec: the width is a
// multiple of 4 and every plane's pointer allows the wide loads (decided on the host).  presence: [B][C][LC_LEVELS] bytes, or null.
template <typename PIX, int C>
__global__ __launch_bounds__(LC_THREADS) void lc_moments(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                         const int* __restrict__ exclude, int H, int W, int vec, LcTables T,
                                                         unsigned char* __restrict__ presence, unsigned int* __restrict__ ctrl)
{
    constexpr int P = lc_pairs(C), N = 3 + 2 * C + P;
    __shared__ LcLds<N, C, LcSlotsA<C>::log2> L;
    lc_lds_clear(L);
    __syncthreads();

    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const unsigned int r0 = tile.r0, c0 = tile.c0;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const PIX* im = image + plane * C;
    unsigned char* pres = presence ? presence + (size_t)b * C * LC_LEVELS : nullptr;
    const bool wide = vec && c_base + 3 < W;
    const LcSinkA<C> sink{T, b};

    unsigned int bad = 0u;
    int cur = 0;                                        // the open run's label; run.n == 0: none
    LcRunA<C> run;
    lc_reset<C>(run);
#pragma unroll 2
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        PIX px[4 * C];
        lc_load<PIX, C>(im, ll, ee, (size_t)r * W + c_base, c_base, W, wide, x, e, px);
        const unsigned int rr = (unsigned int)(tile.wave * LT_ROWS + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab == 0) continue;
            if (lab < 0 || lab > T.max_label) { bad = 1u; continue; }
            if (e[k] != 0) continue;
            if (run.n != 0u && lab != cur) {
                const LcRecA<C> o = lc_rec<C>(run, r0, c0);
                if (!lc_insert(L, cur, o)) lc_global(sink, cur, o);
                run.n = 0u;
            }
            if (run.n == 0u) {
                cur = lab;
                lc_reset<C>(run);
            }
            ++run.n;
            run.sr += rr;
            run.sc += (unsigned int)(4 * lane + k);
            unsigned int v[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                v[ch] = px[k * C + ch];
                run.sv[ch] += v[ch];
                run.sv2[ch] += (unsigned long long)(v[ch] * v[ch]);     // 65535^2 < 2^32
                run.mx[ch] = max(run.mx[ch], v[ch]);
                if (pres) pres[(size_t)ch * LC_LEVELS + v[ch]] = (unsigned char)1;       // a plain store of a constant; v < 65536
            }
            int p = 0;
#pragma unroll
            for (int a = 0; a < C; ++a)
#pragma unroll
                for (int c = a + 1; c < C; ++c) run.svv[p++] += (unsigned long long)(v[a] * v[c]);
        }
    }
    lc_close(L, run.n != 0u, cur, lane, lc_rec<C>(run, r0, c0), sink);
    __syncthreads();
    lc_drain(L, sink);
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

// ---- lc_ranks -----------------------------------------------------------------------------------------------------------------
// grid (B * C).  presence, rank: [B][C][LC_LEVELS]; n: the values of the pixel type, 256 or 65536.  A wave owns n / 16
// consecutive values and walks them 64 at a time: first the counts, then, behind the waves before it, the ranks.
__global__ __launch_bounds__(LC_RANK_THREADS) void lc_ranks(const unsigned char* __restrict__ presence, unsigned short* __restrict__ rank,
                                                            int* __restrict__ levels, int n)
{
    __shared__ unsigned int part[LC_RANK_WAVES];
    const size_t base = (size_t)blockIdx.x * LC_LEVELS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, chunk = n / LC_RANK_WAVES, lo = wave * chunk;
    unsigned int cnt = 0u;
    for (int i = lane; i < chunk; i += 64) cnt += (unsigned int)__popcll(__ballot(presence[base + lo + i] != 0));
    if (lane == 0) part[wave] = cnt;                    // lane 0 took part in every step
    __syncthreads();
    unsigned int before = 0u, total = 0u;
    for (int w = 0; w < LC_RANK_WAVES; ++w) {
        if (w < wave) before += part[w];
        total += part[w];
    }
    for (int i = lane; i < chunk; i += 64) {
        const unsigned long long m = __ballot(presence[base + lo + i] != 0);
        rank[base + lo + i] = (unsigned short)(before + (unsigned int)__popcll(m & ((1ull << lane) - 1ull)));
        before += (unsigned int)__popcll(m);
    }
    if (threadIdx.x == 0) levels[blockIdx.x] = (int)total;
}

// ---- lc_thresholded -----------------------------------------------------------------------------------------------------------
template <int C, bool RWC> struct LcRunB {
    static constexpr int P = lc_pairs(C);
    unsigned int n;                                     // the pixels of the run: 0 is no open run
    unsigned int na[C], sa[C];                          // above in the channel: count, sum v (at most 64 pixels: 32 bits)
    unsigned int pn[P], pi[P], pj[P];                   // above in both: count, sum v_i, sum v_j
    unsigned long long pii[P], pjj[P], pij[P];
    unsigned long long piw[RWC ? P : 1], pjw[RWC ? P : 1];
};

template <int C, bool RWC> __device__ inline void lc_reset(LcRunB<C, RWC>& a)
{
    a.n = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) a.na[ch] = a.sa[ch] = 0u;
#pragma unroll
    for (int p = 0; p < lc_pairs(C); ++p) {
        a.pn[p] = a.pi[p] = a.pj[p] = 0u;
        a.pii[p] = a.pjj[p] = a.pij[p] = 0ull;
        if constexpr (RWC) a.piw[p] = a.pjw[p] = 0ull;
    }
}

template <int C, bool RWC> using LcRecB = LcRec<2 * C + (RWC ? 8 : 6) * lc_pairs(C), 0>;

template <int C, bool RWC> __device__ inline LcRecB<C, RWC> lc_rec(const LcRunB<C, RWC>& a)
{
    constexpr int K = RWC ? 8 : 6;
    LcRecB<C, RWC> o;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        o.s[2 * ch] = a.na[ch];
        o.s[2 * ch + 1] = a.sa[ch];
    }
#pragma unroll
    for (int p = 0; p < lc_pairs(C); ++p) {
        unsigned long long* q = o.s + 2 * C + K * p;
        q[0] = a.pn[p]; q[1] = a.pi[p]; q[2] = a.pj[p]; q[3] = a.pii[p]; q[4] = a.pjj[p]; q[5] = a.pij[p];
        if constexpr (RWC) { q[6] = a.piw[p]; q[7] = a.pjw[p]; }
    }
    return o;
}

template <int C, bool RWC> struct LcSinkB {
    static constexpr int K = RWC ? 8 : 6;
    LcTables T;
    int b;
    __device__ unsigned long long* sum(int label, int j) const
    {
        const size_t row = (size_t)b * T.max_label + (label - 1);
        if (j < 2 * C) return T.chan + (row * C + j / 2) * 5 + 3 + j % 2;
        return T.pair + (row * lc_pairs(C) + (j - 2 * C) / K) * 9 + 1 + (j - 2 * C) % K;
    }
    __device__ unsigned long long* top(int, int) const { return nullptr; }     // no maxima in this walk
};

// grid and planes as lc_moments, after it on the stream: T.chan holds every object's maxima.  rank: [B][C][LC_LEVELS] uint16 and
// levels: [B][C], both of lc_ranks, read only with RWC.
template <typename PIX, int C, bool RWC>
__global__ __launch_bounds__(LC_THREADS) void lc_thresholded(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                             const int* __restrict__ exclude, int H, int W, int vec, LcTables T, LcThreshold thr,
                                                             const unsigned short* __restrict__ rank, const int* __restrict__ levels)
{
    constexpr int P = lc_pairs(C), N = 2 * C + (RWC ? 8 : 6) * P;
    __shared__ LcLds<N, 0, LcSlotsB<C>::log2> L;
    lc_lds_clear(L);
    __syncthreads();

    const LabelTile tile = label_tile();
    const int lane = tile.lane, b = tile.b, c_base = tile.c_base;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const PIX* im = image + plane * C;
    const bool wide = vec && c_base + 3 < W;
    const LcSinkB<C, RWC> sink{T, b};

    unsigned int R[P];                                  // per pair: the larger number of distinct values
    const unsigned short* rk = nullptr;
    if constexpr (RWC) {
        rk = rank + (size_t)b * C * LC_LEVELS;
        int p = 0;
#pragma unroll
        for (int a = 0; a < C; ++a)
#pragma unroll
            for (int c = a + 1; c < C; ++c) R[p++] = (unsigned int)max(levels[b * C + a], levels[b * C + c]);
    }
    unsigned int rhs[C];                                // above iff v * den >= rhs
#pragma unroll
    for (int ch = 0; ch < C; ++ch) rhs[ch] = thr.abs_thr[ch];

    int cur = 0;
    LcRunB<C, RWC> run;
    lc_reset<C, RWC>(run);
#pragma unroll 2
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], e[4] = {0, 0, 0, 0};
        PIX px[4 * C];
        lc_load<PIX, C>(im, ll, ee, (size_t)r * W + c_base, c_base, W, wide, x, e, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lab = x[k];
            if (lab <= 0 || lab > T.max_label || e[k] != 0) continue;   // a bad label: lc_moments has reported it
            if (run.n != 0u && lab != cur) {
                const LcRecB<C, RWC> o = lc_rec<C, RWC>(run);
                if (!lc_insert(L, cur, o)) lc_global(sink, cur, o);
                run.n = 0u;
            }
            if (run.n == 0u) {
                cur = lab;
                lc_reset<C, RWC>(run);
                if (!thr.absolute) {
                    const unsigned long long* st = T.chan + ((size_t)b * T.max_label + (lab - 1)) * C * 5;
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) rhs[ch] = thr.num * (unsigned int)st[ch * 5 + 2];     // <= 65536 * 65535
                }
            }
            ++run.n;
            unsigned int v[C], rv[C];
            bool up[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                v[ch] = px[k * C + ch];
                up[ch] = v[ch] * thr.den >= rhs[ch];    // <= 65535 * 65536; a tie is above
                rv[ch] = 0u;
                if (up[ch]) {
                    ++run.na[ch];
                    run.sa[ch] += v[ch];
                    if constexpr (RWC) rv[ch] = rk[(size_t)ch * LC_LEVELS + v[ch]];
                }
            }
            int p = 0;
#pragma unroll
            for (int a = 0; a < C; ++a)
#pragma unroll
                for (int c = a + 1; c < C; ++c, ++p) {
                    if (!(up[a] && up[c])) continue;
                    ++run.pn[p];
                    run.pi[p] += v[a];
                    run.pj[p] += v[c];
                    run.pii[p] += (unsigned long long)(v[a] * v[a]);
                    run.pjj[p] += (unsigned long long)(v[c] * v[c]);
                    run.pij[p] += (unsigned long long)(v[a] * v[c]);
                    if constexpr (RWC) {
                        const unsigned int w = R[p] - (rv[a] > rv[c] ? rv[a] - rv[c] : rv[c] - rv[a]);   // 1..65536
                        run.piw[p] += (unsigned long long)(v[a] * w);                                  // <= 65535 * 65536
                        run.pjw[p] += (unsigned long long)(v[c] * w);
                    }
                }
        }
    }
    lc_close(L, run.n != 0u, cur, lane, lc_rec<C, RWC>(run), sink);
    __syncthreads();
    lc_drain(L, sink);
}

struct LcPlanes {
    const void* image;
    const int *labels, *exclude;
    int batch, H, W, vec;
};

template <typename PIX, int C>
static void lc_launch_a(const LcPlanes& p, const LcTables& T, unsigned char* presence, unsigned int* ctrl, hipStream_t st)
{
    hipLaunchKernelGGL((lc_moments<PIX, C>), label_tile_grid(p.batch, p.H, p.W), dim3(LC_THREADS), 0, st, (const PIX*)p.image, p.labels, p.exclude,
                       p.H, p.W, p.vec, T, presence, ctrl);
}

template <typename PIX, int C>
static void lc_launch_b(const LcPlanes& p, const LcTables& T, const LcThreshold& thr, const unsigned short* rank, const int* levels, hipStream_t st)
{
    if (rank)
        hipLaunchKernelGGL((lc_thresholded<PIX, C, true>), label_tile_grid(p.batch, p.H, p.W), dim3(LC_THREADS), 0, st, (const PIX*)p.image,
                           p.labels, p.exclude, p.H, p.W, p.vec, T, thr, rank, levels);
    else
        hipLaunchKernelGGL((lc_thresholded<PIX, C, false>), label_tile_grid(p.batch, p.H, p.W), dim3(LC_THREADS), 0, st, (const PIX*)p.image,
                           p.labels, p.exclude, p.H, p.W, p.vec, T, thr, rank, levels);
}

template <typename PIX> static void lc_launch_a_c(int C, const LcPlanes& p, const LcTables& T, unsigned char* presence, unsigned int* ctrl, hipStream_t st)
{
    switch (C) {
    case 2: lc_launch_a<PIX, 2>(p, T, presence, ctrl, st); break;
    case 3: lc_launch_a<PIX, 3>(p, T, presence, ctrl, st); break;
    default: lc_launch_a<PIX, 4>(p, T, presence, ctrl, st); break;
    }
}

template <typename PIX>
static void lc_launch_b_c(int C, const LcPlanes& p, const LcTables& T, const LcThreshold& thr, const unsigned short* rank, const int* levels,
                          hipStream_t st)
{
    switch (C) {
    case 2: lc_launch_b<PIX, 2>(p, T, thr, rank, levels, st); break;
    case 3: lc_launch_b<PIX, 3>(p, T, thr, rank, levels, st); break;
    default: lc_launch_b<PIX, 4>(p, T, thr, rank, levels, st); break;
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_colocalize(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                        int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, const cs_colocalize_params* params,
                        int64_t* geom, int64_t* chan, int64_t* pair, int32_t* levels, int out_kind)
{
    if (!image || !labels || !params || !geom || !chan || !pair || !levels) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 2) return fail(CS_ERR_INVALID, "channels %d: colocalization needs at least 2", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kLcMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kLcMaxChannels);
    if ((params->absolute != 0 && params->absolute != 1) || (params->rwc != 0 && params->rwc != 1))
        return fail(CS_ERR_INVALID, "cs_colocalize_params: absolute %d and rwc %d must be 0 or 1", (int)params->absolute, (int)params->rwc);
    if (!params->absolute && (params->thr_den < 1 || params->thr_den > 65536 || params->thr_num < 0 || params->thr_num > params->thr_den))
        return fail(CS_ERR_INVALID, "cs_colocalize_params: threshold %d / %d: 0 <= num <= den, den in 1..65536", (int)params->thr_num,
                    (int)params->thr_den);
    if (params->absolute)
        for (int c = 0; c < channels; ++c)
            if (params->abs_thr[c] < 0 || params->abs_thr[c] > 65536)
                return fail(CS_ERR_INVALID, "cs_colocalize_params: abs_thr[%d] = %d: must be in 0..65536", c, (int)params->abs_thr[c]);
    if ((rc = label_cap("max_label", max_label, batch, channels, kLcMaxCells, "the tables", "cells")) || (rc = image_limits(batch, height, width)))
        return rc;
    const bool rwc = params->rwc != 0;
    const size_t scratch = rwc ? (size_t)batch * channels * kLcScratchPer : 0;
    if (scratch > kLcMaxScratch)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x channels %d: the rank tables take %zu bytes, above %zu (split the batch)", (int)batch,
                    (int)channels, scratch, kLcMaxScratch);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width, C = channels, P = lc_pairs(C);
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const int64_t rows = (int64_t)batch * max_label;
    const size_t gbytes = (size_t)rows * 3 * sizeof(int64_t), cbytes = (size_t)rows * C * 5 * sizeof(int64_t),
                 pbytes = (size_t)rows * P * 9 * sizeof(int64_t), lbytes = (size_t)batch * C * sizeof(int32_t);
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rwc && (rc = S.co_rank.ensure(scratch)))) return rc;
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
    if (out_host && (rc = S.stage.ensure(gbytes + cbytes + pbytes + lbytes))) return rc;        // on their way to the host: geom, chan, pair, levels
    char* sg = S.stage.as<char>();
    unsigned long long* d_geom = out_host ? (unsigned long long*)sg : (unsigned long long*)geom;
    unsigned long long* d_chan = out_host ? (unsigned long long*)(sg + gbytes) : (unsigned long long*)chan;
    unsigned long long* d_pair = out_host ? (unsigned long long*)(sg + gbytes + cbytes) : (unsigned long long*)pair;
    int* d_levels = out_host ? (int*)(sg + gbytes + cbytes + pbytes) : (int*)levels;
    constexpr int PA[2][4] = {{4, 8, 4, 16}, {8, 16, 8, 16}};              // what lc_load assumes of 4 pixels: PXA
    const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0 &&
                    ((uintptr_t)d_img & (uintptr_t)(PA[esz - 1][C - 1] - 1)) == 0;
    const LcTables T{d_geom, d_chan, d_pair, (int)max_label};
    const LcPlanes planes{d_img, d_lab, d_ex, (int)batch, H, W, vec};
    unsigned char* d_pres = rwc ? S.co_rank.as<unsigned char>() : nullptr;  // [B][C][LC_LEVELS] bytes, then the ranks, uint16
    unsigned short* d_rank = rwc ? (unsigned short*)(d_pres + (size_t)batch * C * LC_LEVELS) : nullptr;
    LcThreshold thr{};
    thr.absolute = params->absolute;
    thr.num = params->absolute ? 0u : (unsigned int)params->thr_num;
    thr.den = params->absolute ? 1u : (unsigned int)params->thr_den;
    for (int c = 0; c < C; ++c) thr.abs_thr[c] = params->absolute ? (unsigned int)params->abs_thr[c] : 0u;

    if ((rc = S.clk_co.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(S.ctrl.p, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
    HIPCHK(hipMemsetAsync(d_chan, 0, cbytes, st));
    HIPCHK(hipMemsetAsync(d_pair, 0, pbytes, st));
    HIPCHK(hipMemsetAsync(d_levels, 0, lbytes, st));
    if (rwc) HIPCHK(hipMemsetAsync(d_pres, 0, (size_t)batch * C * LC_LEVELS, st));
    if ((rc = S.clk_co.record(1, st))) return rc;
    if (pixel_type == CS_PIX_U8) lc_launch_a_c<unsigned char>(C, planes, T, d_pres, S.ctrl.as<unsigned int>(), st);
    else lc_launch_a_c<unsigned short>(C, planes, T, d_pres, S.ctrl.as<unsigned int>(), st);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_co.record(2, st))) return rc;
    if (rwc) {
        hipLaunchKernelGGL(lc_ranks, dim3((unsigned)(batch * C)), dim3(LC_RANK_THREADS), 0, st, d_pres, d_rank, d_levels,
                           pixel_type == CS_PIX_U8 ? 256 : LC_LEVELS);
        HIPCHK(hipGetLastError());
    }
    if ((rc = S.clk_co.record(3, st, rwc))) return rc;
    if (pixel_type == CS_PIX_U8) lc_launch_b_c<unsigned char>(C, planes, T, thr, d_rank, d_levels, st);
    else lc_launch_b_c<unsigned short>(C, planes, T, thr, d_rank, d_levels, st);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_co.record(4, st))) return rc;
    unsigned int bad = 0u;
    HIPCHK(hipMemcpyAsync(&bad, S.ctrl.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(chan, d_chan, cbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(pair, d_pair, pbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(levels, d_levels, lbytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host tables
    if ((rc = S.clk_co.finish())) return rc;
    if (bad) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    return CS_OK;
}

int cs_label_colocalize_last_timing(const cs_preproc* p, double* clear_ms, double* moments_ms, double* ranks_ms, double* thresholded_ms)
{
    return clock_read(p, &SegmentState::clk_co, {clear_ms, moments_ms, ranks_ms, thresholded_ms});
}
