// texture.hip -- per-object grey-level co-occurrence matrices of a label image on gfx950, reduced to the records Haralick's
// features follow from (include/cellscreen.h, cs_label_texture; the rule and the sizing: DESIGN 3w, restated in
// tests/texture_reference.py).
//
// Per object (cs_label_intensity's: a label > 0 of an image, less the pixels where `exclude` is non-zero), channel and direction
// k of (0, d), (d, d), (d, 0), (d, -d): the symmetric matrix G[k] of the quantised values of every pixel pair one step apart with
// both ends in the object.  Two steps, and the kernel boundary is the only ordering between workgroups:
//   tx_boxes     lb_pass of label_boxes.hpp, which cs_label_shape shares: the walk of label_tile.hpp over labels and exclude
//                alone; one open run per lane with its count and its extent, merged per wave, then per workgroup in a table of
//                1024 labels in LDS; only the distinct labels of a tile reach `count` (an integer add) and the bounding boxes
//                (integer maxima of an encoding that a cleared table starts).
//   tx_matrices  one workgroup per (object, channel), absent ones leave before they touch LDS.  It walks the object's box, a
//                thread per pixel and a loop over boxes of any size, and counts every pair once under (min, max) of its two
//                levels: the four upper triangles in LDS, 4 * L (L + 1) / 2 words, 33 KB at L = 64.  Equal bins of a wave are
//                added once (two rounds of ballot on the leader's bin, then an LDS add per remaining lane), so that a flat
//                object does not send 64 lanes to one address.  Then the same workgroup reduces the triangles in place: a
//                thread per entry of the three marginals, a fixed-order sum for sum G^2 and sum G log2 G, the copy to `glcm`.
//                No global atomics.
// The levels are exact: q = (v' * L) / span with v' = clamp(v) - lo < span <= 2^16 and L <= 64 is taken as
// (v' * L * m) >> 40, m = floor(2^40 / span) + 1.  With n = v' * L < 2^22 and e = m * span - 2^40 in 1..span:
// n * m / 2^40 = n / span + n * e / (span * 2^40), and n * e < 2^38 < 2^40 keeps the second term below 1 / span, the least
// distance of n / span from the next integer; n * m < 2^63.
// Everything is integers but clogc = sum G log2 G, which is summed in fp64 in a fixed order (per thread ascending, a shuffle
// tree, the waves in order), so the records are bit-identical run to run.  A label is range-checked before it is a key or an
// index, a box is clamped to the image before it is walked, and a neighbour is tested against the image before it is read: what
// fails the test reads the box's first pixel instead and is not counted.
#include "label_boxes.hpp"
#include "segment_internal.hpp"

namespace cs {

static constexpr int TX_THREADS = LT_THREADS;
static constexpr int kTxMaxChannels = 4;
static constexpr int kTxMinLevels = 2, kTxMaxLevels = 64;
static constexpr int kTxMaxDistance = 127;
static constexpr int kTxMaxValue = 65535;
static constexpr int64_t kTxMaxCells = 1 << 24;         // batch * max_label * channels * levels, and * levels^2 with glcm
static constexpr int TX_TRI = kTxMaxLevels * (kTxMaxLevels + 1) / 2;
static constexpr int TX_SHIFT = 40;
static constexpr int TX_ROUNDS = 2;                     // of the wave's merge of equal bins before the plain adds
static constexpr int TX_STEPS = 4;                      // steps of the walk over a box whose labels are loaded together

// tx_boxes is lb_pass of label_boxes.hpp without the moments: grid (ceil(W/256), ceil(H/64), B); count: [B][max_label],
// box: [B][max_label][4] (LbExtent), both cleared.
static constexpr auto tx_boxes = lb_pass<false>;

// ---- matrices -------------------------------------------------------------------------------------------------------------------
struct TxParams {
    int levels, distance;
    unsigned int lo[kTxMaxChannels], hi[kTxMaxChannels];
    unsigned long long magic[kTxMaxChannels];           // floor(2^40 / (hi - lo + 1)) + 1
};

__device__ inline unsigned int tx_level(unsigned int v, unsigned int lo, unsigned int hi, unsigned int L, unsigned long long magic)
{
    const unsigned int n = (min(max(v, lo), hi) - lo) * L;      // below 2^22
    return (unsigned int)(((unsigned long long)n * magic) >> TX_SHIFT);
}

// the place of the unordered pair {a, b} in a triangle
__device__ inline unsigned int tx_bin(unsigned int a, unsigned int b)
{
    const unsigned int lo = min(a, b), hi = max(a, b);
    return hi * (hi + 1u) / 2u + lo;
}

// G[i][j] of a triangle of pair counts: a pair of equal levels counts twice in its cell
__device__ inline unsigned int tx_cell(const unsigned int* t, int i, int j)
{
    const unsigned int v = t[tx_bin((unsigned int)i, (unsigned int)j)];
    return i == j ? 2u * v : v;
}

// One pair per lane where `valid`: t[bin] += 1.  The lanes that share the bin of the first valid lane add once, twice over;
// what is left then adds lane by lane.  Called by whole waves.
__device__ inline void tx_add(unsigned int* t, bool valid, unsigned int bin, int lane)
{
#pragma unroll
    for (int round = 0; round < TX_ROUNDS; ++round) {
        const unsigned long long m = __ballot(valid);
        if (m == 0ull) return;
        const int leader = __ffsll((long long)m) - 1;
        const unsigned int bw = (unsigned int)__shfl((int)bin, leader);
        const bool mine = valid && bin == bw;
        const unsigned long long mm = __ballot(mine);
        if (lane == leader) atomicAdd(&t[bw], (unsigned int)__popcll(mm));
        if (mine) valid = false;
    }
    if (valid) atomicAdd(&t[bin], 1u);
}

// grid (B * max_label * C): cell = row * C + channel.  image: [B][H][W][C] PIX; labels, exclude (or null): [B][H][W] int.
// count: [B][max_label], box: [B][max_label][4] from tx_boxes.  marg: [cells][4][4 L], sumsq, clogc: [cells][4], glcm (or null):
// [cells][4][L][L], all cleared.
template <typename PIX>
__global__ __launch_bounds__(TX_THREADS) void tx_matrices(const PIX* __restrict__ image, const int* __restrict__ labels,
                                                          const int* __restrict__ exclude, int H, int W, int C, int max_label, TxParams P,
                                                          const int* __restrict__ count, const int* __restrict__ box, int* __restrict__ marg,
                                                          long long* __restrict__ sumsq, double* __restrict__ clogc, int* __restrict__ glcm)
{
    const size_t cell = blockIdx.x, row = cell / (size_t)C;
    if (count[row] == 0) return;                        // an absent object keeps its zeros
    __shared__ unsigned int T[4][TX_TRI];               // per direction: the pairs under (min, max) of their levels
    __shared__ unsigned long long red_s[LT_WAVES][4];
    __shared__ double red_c[LT_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ch = (int)(cell - row * C), L = P.levels, d = P.distance, tri = L * (L + 1) / 2;
    for (int k = 0; k < 4; ++k)
        for (int s = tid; s < tri; s += TX_THREADS) T[k][s] = 0u;
    __syncthreads();

    const int b = (int)(row / (size_t)max_label), lab = (int)(row - (size_t)b * max_label) + 1;
    const int* bx = box + row * 4;
    const int r0 = max(kMaxSide - bx[0], 0), r1 = min(bx[1], H) - 1, c0 = max(kMaxSide - bx[2], 0), c1 = min(bx[3], W) - 1;
    const size_t plane = (size_t)b * H * W;
    const int* ll = labels + plane;
    const int* ee = exclude ? exclude + plane : nullptr;
    const PIX* im = image + plane * C + ch;
    const unsigned int lo = P.lo[ch], hi = P.hi[ch];
    const unsigned long long magic = P.magic[ch];
    if (r0 > r1 || c0 > c1) return;                     // cannot be, with a count above 0: the whole workgroup leaves
    // 2^sh threads side by side, 256 >> sh rows of them: a narrow box takes several rows per step
    int sh = 0;
    while ((1 << sh) < c1 - c0 + 1 && sh < 8) ++sh;
    const int tc = tid & ((1 << sh) - 1), tr = tid >> sh, rows_per = TX_THREADS >> sh, cols_per = 1 << sh;
    const size_t home = (size_t)r0 * W + c0;            // a pixel of the image: what a thread without a pixel, or a pair without a partner, reads
    for (int rb = r0; rb <= r1; rb += rows_per * TX_STEPS) {
        for (int cb = c0; cb <= c1; cb += cols_per) {   // both loops are uniform over the workgroup
            const int c = cb + tc;
            // The labels of TX_STEPS steps first, in flight together: the box of an object in two far pieces is mostly not the
            // object, and a wave without a pixel of it goes on after this one latency.
            int own_l[TX_STEPS], own_e[TX_STEPS];
#pragma unroll
            for (int u = 0; u < TX_STEPS; ++u) {
                const int r = rb + u * rows_per + tr;
                const size_t at = r <= r1 && c <= c1 ? (size_t)r * W + c : home;
                own_l[u] = ll[at];
                own_e[u] = ee ? ee[at] : 0;
            }
#pragma unroll
            for (int u = 0; u < TX_STEPS; ++u) {
                const int r = rb + u * rows_per + tr;
                const bool own = r <= r1 && c <= c1 && own_l[u] == lab && own_e[u] == 0;
                if (__ballot(own) == 0ull) continue;    // uniform over the wave
                // The pixel's value and its four partners.  A partner outside the image, or of a lane without a pixel, is replaced
                // by `home` and never counted, so the loads are unconditional and in flight together, not one behind the other's test.
                bool ok[4];
                size_t to[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int rr = r + (k == 0 ? 0 : d), cc = c + (k == 2 ? 0 : k == 3 ? -d : d);
                    ok[k] = own && rr < H && cc >= 0 && cc < W;         // never read outside the image
                    to[k] = ok[k] ? (size_t)rr * W + cc : home;
                }
                int lb[4], ex[4];
                unsigned int v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) lb[k] = ll[to[k]];
#pragma unroll
                for (int k = 0; k < 4; ++k) ex[k] = ee ? ee[to[k]] : 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (unsigned int)im[to[k] * C];
                const unsigned int q0 = tx_level((unsigned int)im[(own ? (size_t)r * W + c : home) * C], lo, hi, (unsigned int)L, magic);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool pair = ok[k] && lb[k] == lab && ex[k] == 0;
                    const unsigned int bin = pair ? tx_bin(q0, tx_level(v[k], lo, hi, (unsigned int)L, magic)) : 0u;
                    tx_add(T[k], pair, bin, lane);
                }
            }
        }
    }
    __syncthreads();

    // the marginals: entry m of direction k is one thread's sum; px[0 .. L), ps[0 .. 2 L) with its padding, pd[0 .. L)
    int* mrow = marg + cell * (size_t)(16 * L);
    for (int task = tid; task < 16 * L; task += TX_THREADS) {
        const int k = task / (4 * L), m = task - k * 4 * L;
        const unsigned int* t = T[k];
        unsigned int s = 0u;
        if (m < L) {
            for (int j = 0; j < L; ++j) s += tx_cell(t, m, j);
        } else if (m < 3 * L) {
            const int sum = m - L;                      // 2 L - 1 is the padding: no i fits
            for (int i = max(0, sum - (L - 1)); i <= min(L - 1, sum); ++i) s += tx_cell(t, i, sum - i);
        } else {
            const int dif = m - 3 * L;
            for (int i = 0; i + dif < L; ++i) s += tx_cell(t, i, i + dif);
            if (dif != 0) s *= 2u;                      // both sides of the diagonal
        }
        mrow[task] = (int)s;
    }
    // sum G^2 and sum G log2 G over the L x L cells, and the matrices themselves
    unsigned long long s2[4];
    double cl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s2[k] = 0ull;
        cl[k] = 0.0;
        for (int e = tid; e < L * L; e += TX_THREADS) {
            const int i = e / L, j = e - i * L;
            const unsigned int g = tx_cell(T[k], i, j);
            if (glcm) glcm[(cell * 4 + k) * (size_t)(L * L) + e] = (int)g;
            if (g != 0u) {
                s2[k] += (unsigned long long)g * g;
                cl[k] += (double)g * log2((double)g);
            }
        }
        s2[k] = wave_sum(s2[k]);
        cl[k] = wave_sum(cl[k]);                        // a fixed tree, and a + b is b + a: every lane holds the same bits
        if (lane == 0) {
            red_s[wave][k] = s2[k];
            red_c[wave][k] = cl[k];
        }
    }
    __syncthreads();
    if (tid < 4) {
        unsigned long long s = 0ull;
        double c = 0.0;
        for (int w = 0; w < LT_WAVES; ++w) {
            s += red_s[w][tid];
            c += red_c[w][tid];
        }
        sumsq[cell * 4 + tid] = (long long)s;
        clogc[cell * 4 + tid] = c;
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_texture(cs_preproc* p, const void* image, int pixel_type, int32_t channels, const int32_t* labels, const int32_t* exclude,
                     int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, int32_t levels, int32_t distance,
                     const int32_t* range_lo, const int32_t* range_hi, int32_t* count, int32_t* marg, int64_t* sumsq, double* clogc,
                     int32_t* glcm, int out_kind)
{
    if (!image || !labels || !range_lo || !range_hi || !count || !marg || !sumsq || !clogc) return fail(CS_ERR_INVALID, "NULL argument");
    if (pixel_type != CS_PIX_U8 && pixel_type != CS_PIX_U16) return fail(CS_ERR_INVALID, "pixel_type must be CS_PIX_U8 or CS_PIX_U16");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (channels < 1) return fail(CS_ERR_INVALID, "channels %d: must be >= 1", (int)channels);
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (channels > kTxMaxChannels)
        return fail(CS_ERR_UNSUPPORTED, "channels %d: at most %d are measured per call (split the stack)", (int)channels, kTxMaxChannels);
    if (levels < kTxMinLevels || levels > kTxMaxLevels)
        return fail(CS_ERR_INVALID, "levels %d: must lie in %d..%d", (int)levels, kTxMinLevels, kTxMaxLevels);
    if (distance < 1 || distance > kTxMaxDistance) return fail(CS_ERR_INVALID, "distance %d: must lie in 1..%d", (int)distance, kTxMaxDistance);
    for (int32_t c = 0; c < channels; ++c)
        if (range_lo[c] < 0 || range_lo[c] > range_hi[c] || range_hi[c] > kTxMaxValue)
            return fail(CS_ERR_INVALID, "range of channel %d is %d..%d: 0 <= lo <= hi <= %d is required", (int)c, (int)range_lo[c], (int)range_hi[c],
                        kTxMaxValue);
    const int64_t rows = max_label > kMaxLabel ? 0 : (int64_t)batch * max_label, cells = rows * channels;   // 0: refused here
    if (rows == 0 || cells * levels > kTxMaxCells || (glcm && cells * levels * levels > kTxMaxCells))
        return fail(CS_ERR_UNSUPPORTED, "max_label %d x batch %d x channels %d x levels %d: the tables are capped at %d labels per image and %lld "
                    "entries of a marginal%s", (int)max_label, (int)batch, (int)channels, (int)levels, kMaxLabel, (long long)kTxMaxCells,
                    glcm ? ", and as many cells of the matrices" : "");
    if ((rc = image_limits(batch, height, width)) || (rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width, C = channels, L = levels;
    const size_t npx = (size_t)batch * H * W, esz = pixel_type == CS_PIX_U8 ? 1 : 2;
    const size_t qbytes = (size_t)cells * 4 * sizeof(int64_t), lbytes = (size_t)cells * 4 * sizeof(double), cbytes = (size_t)rows * sizeof(int),
                 mbytes = (size_t)cells * 16 * L * sizeof(int), gbytes = glcm ? (size_t)cells * 4 * L * L * sizeof(int) : 0;
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;

    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rc = S.tx_box.ensure((size_t)rows * 4 * sizeof(int)))) return rc;
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
    // the records on their way to the host, the 8-byte ones first: sumsq, clogc, count, marg, glcm
    if (out_host && (rc = S.stage.ensure(qbytes + lbytes + cbytes + mbytes + gbytes))) return rc;
    char* base = S.stage.as<char>();
    long long* d_sumsq = out_host ? (long long*)base : (long long*)sumsq;
    double* d_clogc = out_host ? (double*)(base + qbytes) : clogc;
    int* d_count = out_host ? (int*)(base + qbytes + lbytes) : count;
    int* d_marg = out_host ? (int*)(base + qbytes + lbytes + cbytes) : marg;
    int* d_glcm = !glcm ? nullptr : out_host ? (int*)(base + qbytes + lbytes + cbytes + mbytes) : glcm;
    const int vec = (W & 3) == 0 && (((uintptr_t)d_lab | (uintptr_t)(d_ex ? d_ex : d_lab)) & 15) == 0;      // tx_matrices loads pixel by pixel
    int* d_box = S.tx_box.as<int>();
    unsigned int* d_ctrl = S.ctrl.as<unsigned int>();
    TxParams P{};
    P.levels = L;
    P.distance = distance;
    for (int c = 0; c < C; ++c) {
        P.lo[c] = (unsigned int)range_lo[c];
        P.hi[c] = (unsigned int)range_hi[c];
        P.magic[c] = (1ull << TX_SHIFT) / (unsigned long long)(range_hi[c] - range_lo[c] + 1) + 1ull;
    }

    if ((rc = S.clk_tx.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(d_ctrl, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_box, 0, (size_t)rows * 4 * sizeof(int), st));
    HIPCHK(hipMemsetAsync(d_sumsq, 0, qbytes, st));
    HIPCHK(hipMemsetAsync(d_clogc, 0, lbytes, st));
    HIPCHK(hipMemsetAsync(d_count, 0, cbytes, st));
    HIPCHK(hipMemsetAsync(d_marg, 0, mbytes, st));
    if (d_glcm) HIPCHK(hipMemsetAsync(d_glcm, 0, gbytes, st));
    hipLaunchKernelGGL(tx_boxes, label_tile_grid(batch, H, W), dim3(TX_THREADS), 0, st, d_lab, d_ex, H, W, vec, (int)max_label, d_count, d_box,
                       (unsigned long long*)nullptr, d_ctrl);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_tx.record(1, st))) return rc;
    if (pixel_type == CS_PIX_U8)
        hipLaunchKernelGGL(tx_matrices<unsigned char>, dim3((unsigned)cells), dim3(TX_THREADS), 0, st, (const unsigned char*)d_img, d_lab, d_ex, H, W, C,
                           (int)max_label, P, (const int*)d_count, (const int*)d_box, d_marg, d_sumsq, d_clogc, d_glcm);
    else
        hipLaunchKernelGGL(tx_matrices<unsigned short>, dim3((unsigned)cells), dim3(TX_THREADS), 0, st, (const unsigned short*)d_img, d_lab, d_ex, H, W, C,
                           (int)max_label, P, (const int*)d_count, (const int*)d_box, d_marg, d_sumsq, d_clogc, d_glcm);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_tx.record(2, st))) return rc;
    unsigned int bad = 0u;
    HIPCHK(hipMemcpyAsync(&bad, d_ctrl, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(sumsq, d_sumsq, qbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(clogc, d_clogc, lbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(count, d_count, cbytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(marg, d_marg, mbytes, hipMemcpyDeviceToHost, st));
        if (d_glcm) HIPCHK(hipMemcpyAsync(glcm, d_glcm, gbytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host records
    if ((rc = S.clk_tx.finish())) return rc;
    if (bad) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
    return CS_OK;
}

int cs_label_texture_last_timing(const cs_preproc* p, double* boxes_ms, double* matrices_ms)
{
    return clock_read(p, &SegmentState::clk_tx, {boxes_ms, matrices_ms});
}
