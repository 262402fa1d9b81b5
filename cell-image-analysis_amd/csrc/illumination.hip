// illumination.hip -- flat-field correction from a plate's own images on gfx950 (include/cellscreen.h, cs_illum_tile_stats,
// cs_illum_reduce and cs_illum_apply; the rule: DESIGN 3zj, restated in tests/illumination_reference.py).
//
// One multiplicative illumination function per channel: a rank statistic per tile of every field, a rank statistic (or the mean)
// per mesh node across the fields, and every pixel divided by the function interpolated between the tile centres.  The mesh is
// cs_segment_noise's (segment.hip): T = 1 << shift, m = max(1, n >> shift) tiles along an axis of n pixels, the last
// one runs to n and is at most 2T - 1 wide.
//   il_stats    one workgroup per tile and image, the channels looped: ns_stats' radix selection at the rank
//               (q_num (N - 1)) / q_den: a 256-bin LDS histogram of the high byte (wave-aggregated adds), a scan to the bucket
//               that holds the rank, then the low byte among that bucket's values (uint8: the one pass).  A tile of at most 4096
//               pixels is read once per channel and stays in 16 registers; larger ones (up to 511 x 511) are read again in each
//               pass, row by row.  It reads the interleaved image directly.
//   il_across   one thread per (channel, node): the stack is [n][C][my][mx], so adjacent lanes own adjacent nodes and every load
//               of the loop over the n images is coalesced.  The rank is found bit by bit: 16 passes that count the values below
//               a candidate, exact whatever n; the mean is an int64 sum.  Writes F8 = 256 max(value - offset, floor).
//   il_filter   ns_filter's median of the 3 x 3 mesh neighbourhood, one thread per node.
//   il_smooth_rows / il_smooth_cols   cs_segment_smooth's separable sum over the mesh, reflected at its edges, one thread per
//               node, and one rounding at the end.
//   il_apply    ns_cut's access shape: a thread owns 4 pixels a workgroup-stride apart, reads all channels of a pixel once, and per
//               channel the four nodes of its cell of the mesh from L2.
// Bounds (T <= 256, sides <= 4096, F8 < 2^24, G8 < 2^24, |v - offset| < 2^16):
//   an axis with m >= 2 nodes has D = 2T between regular centres and D = n - (m - 2) T in [2T, 3T) before the last one.  Left of
//   the first centre w1 = 2p - C2_0 >= -(T - 1) and w0 = D - w1 < 4T; right of the last one w1 = 2(n - 1) - C2_{m-2} =
//   2n - (2m - 3) T - 1 < 5T (n < (m + 1) T) and w0 = D - w1 > -3T.  So |w| < 5T = 1280 on either axis: at the widest last tile,
//   T = 256 and n = 767 (m = 2, the tile 511 wide), D = 767, w1 <= 2 * 766 - 255 = 1277 and w0 >= -510.
//   |wy wx| < 25 T^2 < 2^21, four terms of F8 < 2^24: |sum| < 100 * 2^40 < 2^47.  D = Dy Dx < 9 T^2 < 2^20.
//   numerator 2 (v - offset) G8 D + N: below 2 * 2^16 * 2^24 * 2^20 + 2^47 < 2^62; the denominator 2N is in [512 D, 2^48).
//   The Gaussian: row sums below 2^16 * 2^24 = 2^40, full sums below 2^56.  The mean: n * 65535 < 2^30.  All int64.
// The quotient: a float64 estimate (relative error below 2^-51) is taken only where it decides nothing: beyond +-2^17 the result
// is clamped whatever the exact value, and inside the estimate's floor is within one of the exact floor, which the remainder in
// integers then settles (il_quotient).  Where the remainder is not settled after one step the exact 64-bit division runs, so the
// result is the integer rule's for every input; no float reaches the output.
// A value of a device stack or a device function outside its range is cut to it and raises a sticky status word of the family's
// own, which the host reads and clears at its next synchronisation (il_end, cs_illum_last_timing): it is an operand, never an index.
// No float atomics; counts are integers, so the order of arrival cannot change them.
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int IL_THREADS = 256;
static constexpr int IL_WAVES = IL_THREADS / 64;
static constexpr int IL_REG = 16;                       // pixels a thread of il_stats keeps in registers
static constexpr int IL_CHUNK = 4 * IL_THREADS;         // linear pixels per workgroup of il_apply
static constexpr int kIlMaxChannels = 4;
static constexpr int kIlMaxImages = 16384;              // meshes of a stack
static constexpr int kIlMaxMesh = 256;                  // nodes along an axis: 4096 / 16
static constexpr int64_t kIlMaxStack = (int64_t)1 << 28;    // values of a stack: n * channels * my * mx
static constexpr int kIlMaxRadius = CS_ILLUM_MAX_RADIUS;
static constexpr int IL_F8_MIN = 256, IL_F8_END = 1 << 24;

// ---- the tile statistic ------------------------------------------------------------------------------------------------------
// hist_add of segment.hip: one LDS add per distinct value among the first rounds' leaders.  Called by whole waves.
__device__ inline void il_hist_add(unsigned int* bins, int v, bool valid)
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

// The bucket of a 256-bin histogram that holds `rank`, and the rank inside it: sel[0], sel[1].  All 256 threads call it; the
// bins are complete before and may be cleared after.
__device__ inline void il_find(const unsigned int* bins, int rank, int* sel, unsigned int* wsum)
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

// grid (mx, my, B); image: [B][H][W][C]; mesh: [B][C][my][mx]
template <typename PIX>
__global__ __launch_bounds__(IL_THREADS) void il_stats(const PIX* __restrict__ image, int C, int H, int W, int shift, int q_num, int q_den,
                                                       int* __restrict__ mesh)
{
    __shared__ unsigned int bins[256];
    __shared__ unsigned int wsum[IL_WAVES];
    __shared__ int sel[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int mx = gridDim.x, my = gridDim.y, b = blockIdx.z;
    const int x0 = blockIdx.x << shift, y0 = blockIdx.y << shift;
    const int tw = ((int)blockIdx.x == mx - 1 ? W : x0 + (1 << shift)) - x0, th = ((int)blockIdx.y == my - 1 ? H : y0 + (1 << shift)) - y0;
    const int N = tw * th, rank = (int)(((long long)q_num * (N - 1)) / q_den);     // q_num <= 2^16, N < 2^18
    const bool in_regs = N <= IL_REG * IL_THREADS;      // the whole workgroup decides alike
    for (int ch = 0; ch < C; ++ch) {
        const PIX* img = image + ((size_t)b * H * W + (size_t)y0 * W + x0) * C + ch;
        int reg[IL_REG];
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < IL_REG; ++k) {
                const int i = k * IL_THREADS + t;
                reg[k] = i < N ? (int)img[((size_t)(i / tw) * W + i % tw) * C] : 0;
            }
        }
        // f(value, valid) on every pixel of the tile, called by whole waves
        auto each = [&](auto&& f) {
            if (in_regs) {
#pragma unroll
                for (int k = 0; k < IL_REG; ++k) {
                    if (k * IL_THREADS >= N) break;
                    f(reg[k], k * IL_THREADS + t < N);
                }
            } else {
                for (int y = wave; y < th; y += IL_WAVES)
                    for (int xb = 0; xb < tw; xb += 64) {
                        const bool in = xb + lane < tw;
                        f(in ? (int)img[((size_t)y * W + xb + lane) * C] : 0, in);
                    }
            }
        };
        int hi = 0, r = rank;
        if (sizeof(PIX) > 1) {
            bins[t] = 0u;
            __syncthreads();
            each([&](int v, bool ok) { il_hist_add(bins, v >> 8, ok); });
            __syncthreads();
            il_find(bins, r, sel, wsum);
            hi = sel[0]; r = sel[1];
            __syncthreads();                            // sel is read before the next il_find writes it
        }
        bins[t] = 0u;
        __syncthreads();
        each([&](int v, bool ok) { il_hist_add(bins, v & 255, ok && (v >> 8) == hi); });
        __syncthreads();
        il_find(bins, r, sel, wsum);
        const int lo = sel[0];
        __syncthreads();
        if (t == 0) mesh[(((size_t)b * C + ch) * my + blockIdx.y) * mx + blockIdx.x] = (hi << 8) | lo;
    }
}

// ---- across the plate --------------------------------------------------------------------------------------------------------
struct IlChan { int v[kIlMaxChannels]; };

// a value of a device stack: 0..65535, or cut to it with the status raised
__device__ inline int il_value(int v, bool& bad)
{
    if (v < 0 || v > 65535) bad = true;
    return min(max(v, 0), 65535);
}

// grid ceil(nodes / 256), nodes = C * per_ch; stack: [n][nodes]; out: [nodes].  rank < n.
__global__ __launch_bounds__(IL_THREADS) void il_across(const int* __restrict__ stack, int n, int nodes, int per_ch, int rank, int mean,
                                                        IlChan offset, int floor_, int* __restrict__ out, unsigned int* __restrict__ ctrl)
{
    const int node = blockIdx.x * IL_THREADS + threadIdx.x;
    if (node >= nodes) return;
    const int* s = stack + node;
    bool bad = false;
    long long value;
    if (mean) {
        long long sum = 0;
        for (int k = 0; k < n; ++k) sum += il_value(s[(size_t)k * nodes], bad);
        value = (2 * sum + n) / (2 * (long long)n);
    } else {
        // the greatest x with #{v < x} <= rank is the value of that rank
        int res = 0;
        for (int bit = 15; bit >= 0; --bit) {
            const int cand = res | (1 << bit);
            int below = 0;
            for (int k = 0; k < n; ++k) below += il_value(s[(size_t)k * nodes], bad) < cand ? 1 : 0;
            if (below <= rank) res = cand;
        }
        value = res;
    }
    out[node] = 256 * max((int)value - offset.v[node / per_ch], floor_);
    if (bad) *ctrl = 1u;                                // a plain store of a constant
}

// grid (ceil(my * mx / 256), C): raw and out are [C][my][mx]
__global__ __launch_bounds__(IL_THREADS) void il_filter(const int* __restrict__ raw, int my, int mx, int* __restrict__ out)
{
    const int n = blockIdx.x * IL_THREADS + threadIdx.x;
    if (n >= my * mx) return;
    const int j = n / mx, i = n % mx;
    const size_t base = (size_t)blockIdx.y * my * mx;
    int v[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            v[(dy + 1) * 3 + dx + 1] = raw[base + (size_t)min(max(j + dy, 0), my - 1) * mx + min(max(i + dx, 0), mx - 1)];
    // the fifth of nine: Paeth's network of 19 exchanges
#define IL_SORT2(a, b) { const int lo_ = min(v[a], v[b]), hi_ = max(v[a], v[b]); v[a] = lo_; v[b] = hi_; }
    IL_SORT2(1, 2) IL_SORT2(4, 5) IL_SORT2(7, 8) IL_SORT2(0, 1) IL_SORT2(3, 4) IL_SORT2(6, 7) IL_SORT2(1, 2) IL_SORT2(4, 5)
    IL_SORT2(7, 8) IL_SORT2(0, 3) IL_SORT2(5, 8) IL_SORT2(4, 7) IL_SORT2(3, 6) IL_SORT2(1, 4) IL_SORT2(2, 5) IL_SORT2(4, 7)
    IL_SORT2(4, 2) IL_SORT2(6, 4) IL_SORT2(4, 2)
#undef IL_SORT2
    out[base + n] = v[4];
}

struct IlTaps {
    int radius;
    int w[kIlMaxRadius + 1];
};

// d c b a | a b c d | d c b a: the reflection of period 2n, so a radius may exceed the side
__device__ inline int il_fold(int i, int n)
{
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// grid (ceil(my * mx / 256), C).  in: [C][my][mx] int; rows: [C][my][mx] int64
__global__ __launch_bounds__(IL_THREADS) void il_smooth_rows(const int* __restrict__ in, int my, int mx, IlTaps taps, long long* __restrict__ rows)
{
    const int n = blockIdx.x * IL_THREADS + threadIdx.x;
    if (n >= my * mx) return;
    const int j = n / mx, i = n % mx;
    const int* row = in + ((size_t)blockIdx.y * my + j) * mx;
    long long s = (long long)taps.w[0] * row[i];
    for (int k = 1; k <= taps.radius; ++k) s += (long long)taps.w[k] * ((long long)row[il_fold(i - k, mx)] + row[il_fold(i + k, mx)]);
    rows[(size_t)blockIdx.y * my * mx + n] = s;
}

__global__ __launch_bounds__(IL_THREADS) void il_smooth_cols(const long long* __restrict__ rows, int my, int mx, IlTaps taps, int floor8,
                                                             int* __restrict__ out)
{
    const int n = blockIdx.x * IL_THREADS + threadIdx.x;
    if (n >= my * mx) return;
    const int j = n / mx, i = n % mx;
    const long long* col = rows + (size_t)blockIdx.y * my * mx + i;
    long long a = taps.w[0] * col[(size_t)j * mx];
    for (int k = 1; k <= taps.radius; ++k) a += taps.w[k] * (col[(size_t)il_fold(j - k, my) * mx] + col[(size_t)il_fold(j + k, my) * mx]);
    out[(size_t)blockIdx.y * my * mx + n] = max((int)((a + (1ll << 31)) >> 32), floor8);
}

// ---- apply -------------------------------------------------------------------------------------------------------------------
// One axis of the interpolation at pixel p: the first of the two nodes, the second's offset (0 with a single node), w0, w1.
// ns_axis of segment.hip with w1 left as it is: negative left of the first centre, above D right of the last.
struct IlAxis {
    int i0, step, w0, w1;
};
__device__ inline IlAxis il_axis(int p, int n, int m, int shift)
{
    if (m == 1) return IlAxis{0, 0, 1, 0};
    const int T = 1 << shift;
    const int i0 = min(max((2 * p - T + 1) >> (shift + 1), 0), m - 2);      // arithmetic shift: -1 left of the first centre
    const int c0 = 2 * i0 * T + T - 1;
    const int c1 = i0 + 1 == m - 1 ? (m - 1) * T + n - 1 : c0 + 2 * T;       // the last tile runs to n
    const int D = c1 - c0, w1 = 2 * p - c0;
    return IlAxis{i0, 1, D - w1, w1};
}

// floor(num / den), den > 0, exact wherever it lies in [-2^17, 2^17]; beyond, +-2^17: the caller clamps far inside that.
__device__ inline long long il_quotient(long long num, long long den)
{
    const double qf = (double)num / (double)den;        // relative error below 2^-51
    if (qf > 131072.0) return 131072;
    if (qf < -131072.0) return -131072;
    long long q = (long long)floor(qf);                 // within one of the exact floor: |qf| <= 2^17, an error below 2^-33
    // the remainder modulo 2^64: exact, since the true one is below 2 den < 2^49 in magnitude
    long long r = (long long)((unsigned long long)num - (unsigned long long)q * (unsigned long long)den);
    if (r < 0) { --q; r += den; }
    else if (r >= den) { ++q; r -= den; }
    if (r < 0 || r >= den) {                            // never taken if the estimate is what IEEE says; the integer rule itself
        q = num / den;
        if (num % den < 0) --q;
    }
    return q;
}

struct IlApply {
    int g8[kIlMaxChannels], off[kIlMaxChannels], ped[kIlMaxChannels];
    int floor8;                                         // 256 floor
};

__device__ inline long long il_f8(int v, bool& bad)
{
    if (v < IL_F8_MIN || v >= IL_F8_END) bad = true;
    return min(max(v, IL_F8_MIN), IL_F8_END - 1);
}

__device__ inline unsigned int il_wave_sum(unsigned int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// grid (ceil(HW / IL_CHUNK), B).  image, out: [B][H][W][C], out may be image; f8: [C][my][mx]; clipped: [B][C][2]
template <typename PIX, int C, bool COUNT>
__global__ __launch_bounds__(IL_THREADS) void il_apply(const PIX* image, PIX* out, int H, int W, int shift, int my, int mx,
                                                       const int* __restrict__ f8, IlApply A, unsigned long long* __restrict__ clipped,
                                                       unsigned int* __restrict__ ctrl)
{
    __shared__ unsigned int part[IL_WAVES][C][2];
    constexpr long long top = sizeof(PIX) == 1 ? 255 : 65535;
    const int b = blockIdx.y, HW = H * W;
    const PIX* img = image + (size_t)b * HW * C;
    PIX* o = out + (size_t)b * HW * C;
    unsigned int n_lo[C], n_hi[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) n_lo[ch] = n_hi[ch] = 0u;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * IL_CHUNK + k * IL_THREADS + threadIdx.x;
        if (i >= HW) continue;
        PIX v[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) v[ch] = img[(size_t)i * C + ch];
        const IlAxis ay = il_axis(i / W, H, my, shift), ax = il_axis(i % W, W, mx, shift);
        const int n00 = ay.i0 * mx + ax.i0, n01 = n00 + ax.step, n10 = n00 + ay.step * mx, n11 = n10 + ax.step;
        const long long w00 = (long long)ay.w0 * ax.w0, w01 = (long long)ay.w0 * ax.w1, w10 = (long long)ay.w1 * ax.w0,
                        w11 = (long long)ay.w1 * ax.w1;
        const long long D = (long long)(ay.w0 + ay.w1) * (ax.w0 + ax.w1);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const int* m = f8 + (size_t)ch * my * mx;
            long long N = w00 * il_f8(m[n00], bad) + w01 * il_f8(m[n01], bad) + w10 * il_f8(m[n10], bad) + w11 * il_f8(m[n11], bad);
            N = max(N, (long long)A.floor8 * D);
            const long long num = 2 * ((long long)v[ch] - A.off[ch]) * A.g8[ch] * D + N;
            long long y = A.ped[ch] + il_quotient(num, 2 * N);
            if (y < 0) { y = 0; ++n_lo[ch]; }
            else if (y > top) { y = top; ++n_hi[ch]; }
            o[(size_t)i * C + ch] = (PIX)y;
        }
    }
    if (bad) *ctrl = 1u;                                // a plain store of a constant
    if (COUNT) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const unsigned int lo = il_wave_sum(n_lo[ch]), hi = il_wave_sum(n_hi[ch]);
            if (lane == 0) { part[wave][ch][0] = lo; part[wave][ch][1] = hi; }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * C) {
            const int ch = threadIdx.x >> 1, side = threadIdx.x & 1;
            unsigned int s = 0u;
            for (int w = 0; w < IL_WAVES; ++w) s += part[w][ch][side];
            if (s) atomicAdd(&clipped[((size_t)b * C + ch) * 2 + side], (unsigned long long)s);
        }
    }
}

template <typename PIX, bool COUNT>
static void il_apply_launch(int C, dim3 grid, hipStream_t st, const void* image, void* out, int H, int W, int shift, int my, int mx, const int* f8,
                            const IlApply& A, unsigned long long* clipped, unsigned int* ctrl)
{
    const dim3 block(IL_THREADS);
    switch (C) {
    case 1: hipLaunchKernelGGL((il_apply<PIX, 1, COUNT>), grid, block, 0, st, (const PIX*)image, (PIX*)out, H, W, shift, my, mx, f8, A, clipped, ctrl); break;
    case 2: hipLaunchKernelGGL((il_apply<PIX, 2, COUNT>), grid, block, 0, st, (const PIX*)image, (PIX*)out, H, W, shift, my, mx, f8, A, clipped, ctrl); break;
    case 3: hipLaunchKernelGGL((il_apply<PIX, 3, COUNT>), grid, block, 0, st, (const PIX*)image, (PIX*)out, H, W, shift, my, mx, f8, A, clipped, ctrl); break;
    default: hipLaunchKernelGGL((il_apply<PIX, 4, COUNT>), grid, block, 0, st, (const PIX*)image, (PIX*)out, H, W, shift, my, mx, f8, A, clipped, ctrl); break;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// the shift of a tile side, or -1
static int il_shift(int tile)
{
    for (int s = 4; s <= 8; ++s)
        if (tile == (1 << s)) return s;
    return -1;
}

// What the three calls begin with, as plane_begin does for the segmenter's stages: the state, the two status words on their
// first use, and the upload of a host input into img.  d_src: where the input is on the device.
static int il_begin(cs_preproc* p, const void* src, size_t bytes, int kind, const void*& d_src)
{
    int rc;
    if ((rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    if (!S.il_status.p) {
        if ((rc = S.il_status.ensure(2 * sizeof(unsigned int)))) return rc;
        HIPCHK(hipMemsetAsync(S.il_status.p, 0, 2 * sizeof(unsigned int), p->stream));
    }
    d_src = src;
    if (kind == CS_MEM_HOST) {
        if ((rc = S.img.ensure(bytes))) return rc;
        HIPCHK(hipMemcpyAsync(S.img.p, src, bytes, hipMemcpyHostToDevice, p->stream));
        d_src = S.img.p;
    }
    return CS_OK;
}

// The status words are sticky: a kernel raises one, only the host clears them, after it has read them.  [0]: a value of a device
// stack was outside 0..65535 (cs_illum_reduce), [1]: a value of a device function was outside [256, 2^24) (cs_illum_apply).
// Enqueues the read and the clearing; the caller synchronises and then reports.
static int il_status_fetch(SegmentState& S, hipStream_t st, unsigned int* bad)
{
    HIPCHK(hipMemcpyAsync(bad, S.il_status.p, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemsetAsync(S.il_status.p, 0, 2 * sizeof(unsigned int), st));
    return CS_OK;
}

static int il_status_report(const unsigned int* bad)
{
    if (bad[0])
        return fail(CS_ERR_INVALID, "a value of a device stack was outside 0..65535 and was cut to it (cs_illum_reduce: this call, or one before it "
                                    "that did not synchronise)");
    if (bad[1])
        return fail(CS_ERR_INVALID, "a value of a device function was outside [256, 2^24) and was cut to it (cs_illum_apply: this call, or one "
                                    "before it that did not synchronise)");
    return CS_OK;
}

// The end of a call, its launches, its copies to the host and the clock's last record on the stream.  on_device: every buffer of
// the call is the caller's device memory, so nothing waits: the time and the status are read when cs_illum_last_timing, or the
// handle's next cs_illum_* call that synchronises, asks for them.
static int il_end(SegmentState& S, hipStream_t st, StageClock& clk, bool on_device)
{
    if (on_device) {
        clk.pending = true;
        S.il_unread = true;
        return CS_OK;
    }
    unsigned int bad[2] = {0u, 0u};
    int rc;
    if ((rc = il_status_fetch(S, st, bad))) return rc;
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the caller's host buffers are free / filled
    S.il_unread = false;
    if ((rc = clk.finish())) return rc;
    return il_status_report(bad);
}

// what the calls ask of an image stack, in cs_image_quality's order up to the rules of their own
static int il_image_check(const void* image, const void* other, int pixel_type, int32_t channels, int32_t batch, int32_t height, int32_t width,
                          int kind_a, int kind_b, const char* kinds)
{
    if (!image || !other) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(kind_a) || !mem_kind(kind_b)) return fail(CS_ERR_INVALID, "%s must be CS_MEM_HOST or CS_MEM_DEVICE", kinds);
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    return stack_dims(batch, height, width);
}

static int il_channel_cap(int32_t channels)
{
    if (channels > kIlMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are corrected per call (split the stack)", (int)channels, kIlMaxChannels);
    return CS_OK;
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_illum_tile_stats(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t batch, int32_t height, int32_t width,
                        int in_kind, int32_t tile, int32_t q_num, int32_t q_den, int32_t* mesh, int out_kind)
{
    int rc;
    if ((rc = il_image_check(image, mesh, pixel_type, channels, batch, height, width, in_kind, out_kind, "in_kind / out_kind"))) return rc;
    const int shift = il_shift(tile);
    if (shift < 0) return fail(CS_ERR_INVALID, "tile %d: a power of two in 16..256", (int)tile);
    if (q_den < 1 || q_den > 65536 || q_num < 0 || q_num > q_den)
        return fail(CS_ERR_INVALID, "quantile %d / %d: need 0 <= q_num <= q_den <= 65536", (int)q_num, (int)q_den);
    if ((rc = il_channel_cap(channels)) || (rc = image_limits(batch, height, width)) || (rc = handle_check(p))) return rc;
    const int H = height, W = width, C = channels;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const int my = std::max(1, H >> shift), mx = std::max(1, W >> shift);
    const size_t mbytes = (size_t)batch * C * my * mx * sizeof(int);
    const bool out_host = out_kind == CS_MEM_HOST;
    const void* d_img;
    if ((rc = il_begin(p, image, (size_t)batch * H * W * C * esz, in_kind, d_img))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    if (out_host && (rc = S.stage.ensure(mbytes))) return rc;
    int* d_mesh = out_host ? S.stage.as<int>() : mesh;
    if ((rc = S.clk_il_s.record(0, st))) return rc;
    const dim3 grid((unsigned)mx, (unsigned)my, (unsigned)batch);
    if (pixel_type == CS_PIX_U8)
        hipLaunchKernelGGL(il_stats<unsigned char>, grid, dim3(IL_THREADS), 0, st, (const unsigned char*)d_img, C, H, W, shift, (int)q_num, (int)q_den, d_mesh);
    else
        hipLaunchKernelGGL(il_stats<unsigned short>, grid, dim3(IL_THREADS), 0, st, (const unsigned short*)d_img, C, H, W, shift, (int)q_num, (int)q_den, d_mesh);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_il_s.record(1, st))) return rc;
    if (out_host) HIPCHK(hipMemcpyAsync(mesh, d_mesh, mbytes, hipMemcpyDeviceToHost, st));
    return il_end(S, st, S.clk_il_s, in_kind == CS_MEM_DEVICE && !out_host);
}

int cs_illum_reduce(cs_preproc* p, const int32_t* stack, int32_t n, int32_t channels, int32_t m_y, int32_t m_x, int in_kind,
                    const cs_illum_reduce_params* params, int32_t* f8, int out_kind)
{
    if (!stack || !params || !f8) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    if (n < 1 || m_y < 1 || m_x < 1) return fail(CS_ERR_INVALID, "n %d, mesh %d x %d: all must be >= 1", (int)n, (int)m_y, (int)m_x);
    const cs_illum_reduce_params& rp = *params;
    if (rp.mean != 0 && rp.mean != 1) return fail(CS_ERR_INVALID, "mean %d: 0 or 1", (int)rp.mean);
    if (!rp.mean && (rp.a_den < 1 || rp.a_den > 65536 || rp.a_num < 0 || rp.a_num > rp.a_den))
        return fail(CS_ERR_INVALID, "across %d / %d: need 0 <= a_num <= a_den <= 65536", (int)rp.a_num, (int)rp.a_den);
    for (int c = 0; c < kIlMaxChannels; ++c)
        if (rp.offset[c] < 0 || rp.offset[c] > 65535) return fail(CS_ERR_INVALID, "offset[%d] = %d: must be 0..65535", c, (int)rp.offset[c]);
    if (rp.floor < 1 || rp.floor > 4095) return fail(CS_ERR_INVALID, "floor %d outside 1..4095", (int)rp.floor);
    if (rp.mesh_median != 0 && rp.mesh_median != 1) return fail(CS_ERR_INVALID, "mesh_median %d: 0 or 1", (int)rp.mesh_median);
    if (rp.radius < 0 || rp.radius > kIlMaxRadius) return fail(CS_ERR_INVALID, "radius %d outside 0..%d", (int)rp.radius, kIlMaxRadius);
    if (rp.radius) {
        long long sum = rp.weights[0];
        bool ok = rp.weights[0] >= 1;
        for (int k = 1; k <= kIlMaxRadius; ++k) {
            ok = ok && rp.weights[k] >= 0 && (k <= rp.radius || rp.weights[k] == 0);
            sum += 2ll * rp.weights[k];
        }
        if (!ok || sum != 65536)
            return fail(CS_ERR_INVALID, "weights must be non-negative with w[0] >= 1, 0 beyond the radius and w[0] + 2 * sum(w[1..radius]) == 65536");
    }
    if (rp.reserved[0] != 0 || rp.reserved[1] != 0) return fail(CS_ERR_INVALID, "cs_illum_reduce_params.reserved must be 0");
    int rc;
    if ((rc = il_channel_cap(channels))) return rc;
    if (m_y > kIlMaxMesh || m_x > kIlMaxMesh)
        return fail(CS_ERR_UNSUPPORTED, "mesh %d x %d: at most %d nodes along an axis", (int)m_y, (int)m_x, kIlMaxMesh);
    if (n > kIlMaxImages) return fail(CS_ERR_UNSUPPORTED, "n %d: at most %d meshes per call", (int)n, kIlMaxImages);
    if ((int64_t)n * channels * m_y * m_x > kIlMaxStack)
        return fail(CS_ERR_UNSUPPORTED, "n %d x channels %d x mesh %d x %d: the stack is capped at %lld values", (int)n, (int)channels, (int)m_y,
                    (int)m_x, (long long)kIlMaxStack);
    if (in_kind == CS_MEM_HOST) {
        const size_t count = (size_t)n * channels * m_y * m_x;
        for (size_t i = 0; i < count; ++i)
            if (stack[i] < 0 || stack[i] > 65535) return fail(CS_ERR_INVALID, "a value of the stack is outside 0..65535");
    }
    if ((rc = handle_check(p))) return rc;
    const int C = channels, my = m_y, mx = m_x, per_ch = my * mx, nodes = C * per_ch;
    const size_t fbytes = (size_t)nodes * sizeof(int);
    const void* d_src;
    if ((rc = il_begin(p, stack, (size_t)n * fbytes, in_kind, d_src))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    if ((rc = S.ns_mesh.ensure(2 * fbytes))) return rc;
    if (rp.radius && (rc = S.sm_t.ensure((size_t)nodes * sizeof(long long)))) return rc;
    int *cur = S.ns_mesh.as<int>(), *other = cur + nodes;                // F8 between its filters
    IlChan off;
    for (int c = 0; c < kIlMaxChannels; ++c) off.v[c] = rp.offset[c];
    const int rank = rp.mean ? 0 : (int)(((long long)rp.a_num * (n - 1)) / rp.a_den);
    const dim3 block(IL_THREADS), ngrid((unsigned)((per_ch + IL_THREADS - 1) / IL_THREADS), (unsigned)C);
    if ((rc = S.clk_il_r.record(0, st))) return rc;
    hipLaunchKernelGGL(il_across, dim3((unsigned)((nodes + IL_THREADS - 1) / IL_THREADS)), block, 0, st, (const int*)d_src, (int)n, nodes, per_ch, rank,
                       (int)rp.mean, off, (int)rp.floor, cur, S.il_status.as<unsigned int>());
    if (rp.mesh_median) {
        hipLaunchKernelGGL(il_filter, ngrid, block, 0, st, (const int*)cur, my, mx, other);
        std::swap(cur, other);
    }
    if (rp.radius) {
        IlTaps taps;
        taps.radius = rp.radius;
        for (int k = 0; k <= kIlMaxRadius; ++k) taps.w[k] = rp.weights[k];
        hipLaunchKernelGGL(il_smooth_rows, ngrid, block, 0, st, (const int*)cur, my, mx, taps, S.sm_t.as<long long>());
        hipLaunchKernelGGL(il_smooth_cols, ngrid, block, 0, st, (const long long*)S.sm_t.as<long long>(), my, mx, taps, 256 * (int)rp.floor, other);
        std::swap(cur, other);
    }
    HIPCHK(hipGetLastError());
    const bool out_host = out_kind == CS_MEM_HOST;
    HIPCHK(hipMemcpyAsync(f8, cur, fbytes, out_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if ((rc = S.clk_il_r.record(1, st))) return rc;
    return il_end(S, st, S.clk_il_r, in_kind == CS_MEM_DEVICE && !out_host);
}

int cs_illum_apply(cs_preproc* p, const void* image, int pixel_type, int32_t channels, int32_t batch, int32_t height, int32_t width, int kind,
                   const int32_t* f8, int32_t m_y, int32_t m_x, int mesh_kind, const cs_illum_apply_params* params, void* out, int64_t* clipped)
{
    if (!f8 || !params) return fail(CS_ERR_INVALID, "NULL argument");
    int rc;
    if ((rc = il_image_check(image, out, pixel_type, channels, batch, height, width, kind, mesh_kind, "kind / mesh_kind"))) return rc;
    const cs_illum_apply_params& ap = *params;
    const int shift = il_shift(ap.tile);
    if (shift < 0) return fail(CS_ERR_INVALID, "tile %d: a power of two in 16..256", (int)ap.tile);
    if (ap.floor < 1 || ap.floor > 4095) return fail(CS_ERR_INVALID, "floor %d outside 1..4095", (int)ap.floor);
    IlApply A;
    for (int c = 0; c < kIlMaxChannels; ++c) {
        const bool used = c < channels;
        if (used && (ap.g8[c] < 1 || ap.g8[c] >= IL_F8_END)) return fail(CS_ERR_INVALID, "g8[%d] = %d: must be in [1, 2^24)", c, (int)ap.g8[c]);
        if (ap.offset[c] < 0 || ap.offset[c] > 65535) return fail(CS_ERR_INVALID, "offset[%d] = %d: must be 0..65535", c, (int)ap.offset[c]);
        if (ap.pedestal[c] < 0 || ap.pedestal[c] > 65535) return fail(CS_ERR_INVALID, "pedestal[%d] = %d: must be 0..65535", c, (int)ap.pedestal[c]);
        A.g8[c] = used ? ap.g8[c] : 1;
        A.off[c] = ap.offset[c];
        A.ped[c] = ap.pedestal[c];
    }
    A.floor8 = 256 * ap.floor;
    if (ap.reserved[0] != 0 || ap.reserved[1] != 0) return fail(CS_ERR_INVALID, "cs_illum_apply_params.reserved must be 0");
    if ((rc = il_channel_cap(channels)) || (rc = image_limits(batch, height, width))) return rc;
    if (m_y != std::max(1, height >> shift) || m_x != std::max(1, width >> shift))
        return fail(CS_ERR_INVALID, "mesh %d x %d: an image of %d x %d has %d x %d tiles of side %d", (int)m_y, (int)m_x, (int)height, (int)width,
                    std::max(1, height >> shift), std::max(1, width >> shift), (int)ap.tile);
    if (mesh_kind == CS_MEM_HOST) {
        const size_t count = (size_t)channels * m_y * m_x;
        for (size_t i = 0; i < count; ++i)
            if (f8[i] < IL_F8_MIN || f8[i] >= IL_F8_END) return fail(CS_ERR_INVALID, "a value of the function is outside [256, 2^24)");
    }
    if ((rc = handle_check(p))) return rc;
    const int H = height, W = width, C = channels, my = m_y, mx = m_x;
    const size_t esz = pixel_type == CS_PIX_U8 ? 1 : 2, ibytes = (size_t)batch * H * W * C * esz;
    const size_t fbytes = (size_t)C * my * mx * sizeof(int), cbytes = (size_t)batch * C * 2 * sizeof(int64_t);
    const bool host = kind == CS_MEM_HOST, mesh_host = mesh_kind == CS_MEM_HOST;
    const void* d_img;
    if ((rc = il_begin(p, image, ibytes, kind, d_img))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    void* d_out = host ? S.img.p : out;                 // a host stack is corrected in place in its upload, then copied out
    const int* d_f8 = f8;
    if (mesh_host) {
        if ((rc = S.lab.ensure(fbytes))) return rc;
        HIPCHK(hipMemcpyAsync(S.lab.p, f8, fbytes, hipMemcpyHostToDevice, st));
        d_f8 = S.lab.as<int>();
    }
    if (clipped && (rc = S.counts.ensure(cbytes))) return rc;
    unsigned long long* d_clip = clipped ? S.counts.as<unsigned long long>() : nullptr;
    if ((rc = S.clk_il_a.record(0, st))) return rc;
    if (clipped) HIPCHK(hipMemsetAsync(d_clip, 0, cbytes, st));
    const dim3 grid((unsigned)(((size_t)H * W + IL_CHUNK - 1) / IL_CHUNK), (unsigned)batch);
    unsigned int* status = S.il_status.as<unsigned int>() + 1;
    if (pixel_type == CS_PIX_U8) {
        if (clipped) il_apply_launch<unsigned char, true>(C, grid, st, d_img, d_out, H, W, shift, my, mx, d_f8, A, d_clip, status);
        else il_apply_launch<unsigned char, false>(C, grid, st, d_img, d_out, H, W, shift, my, mx, d_f8, A, d_clip, status);
    } else {
        if (clipped) il_apply_launch<unsigned short, true>(C, grid, st, d_img, d_out, H, W, shift, my, mx, d_f8, A, d_clip, status);
        else il_apply_launch<unsigned short, false>(C, grid, st, d_img, d_out, H, W, shift, my, mx, d_f8, A, d_clip, status);
    }
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_il_a.record(1, st))) return rc;
    if (host) HIPCHK(hipMemcpyAsync(out, d_out, ibytes, hipMemcpyDeviceToHost, st));
    if (clipped) HIPCHK(hipMemcpyAsync(clipped, d_clip, cbytes, hipMemcpyDeviceToHost, st));
    return il_end(S, st, S.clk_il_a, !host && !mesh_host && !clipped);
}

int cs_illum_last_timing(const cs_preproc* p, double* stats_ms, double* reduce_ms, double* apply_ms)
{
    int rc;
    if ((rc = clock_read(p, &SegmentState::clk_il_s, {stats_ms})) || (rc = clock_read(p, &SegmentState::clk_il_r, {reduce_ms})) ||
        (rc = clock_read(p, &SegmentState::clk_il_a, {apply_ms})))
        return rc;
    if (!p->seg || !p->seg->il_unread) return CS_OK;
    SegmentState& S = *p->seg;                            // a call left its status on the device: it is read and cleared here
    unsigned int bad[2] = {0u, 0u};
    HIPCHK(hipSetDevice(p->device));
    if ((rc = il_status_fetch(S, p->stream, bad))) return rc;
    HIPCHK(hipStreamSynchronize(p->stream));
    S.il_unread = false;
    return il_status_report(bad);
}
