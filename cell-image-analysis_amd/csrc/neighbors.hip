// neighbors.hip -- per-object neighbours and contact of a label image on gfx950 (include/cellscreen.h, cs_label_neighbors; the rule
// and the sizing: DESIGN 3y, restated in tests/neighbors_reference.py).
//
// Per object a (a label > 0 of an image): area, sum r, sum c; the number of its border pixels (a 4-neighbour is not a's, outside the
// image included), how many of them have a foreign label within max_d2 (squared Euclidean distance between pixel centres), and its
// degree.  Per directed pair (a, b) with D2(a, b) <= max_d2: D2 and the number of a's border pixels whose nearest foreign label is b.
// The pairs leave as rows in CSR form, each row sorted by b.  Only border pixels look: the pixel of a closest to any outside pixel is
// one.  Scattered global atomics are slow (the guides put single-lane ones at about 1/17 of the shaped rate), so, as lm_count
// (match.hip) and li_pass (intensity.hip), the design makes them rare instead of fast:
//   nb_scan      one workgroup per tile of 32 x 64 pixels, the tile and a halo of R = floor(sqrt(max_d2)) pixels on every side in LDS
//                (zeros outside the image).  Pass A: a thread walks 8 pixels of a row, keeps one open run of area, sum r, sum c per
//                label and appends the border pixels to a list in LDS, compacted per wave by __ballot.  Pass B: the threads take the
//                border pixels from that list, so that every lane scans a disk, pixel by pixel over the rows of the halo; a lane keeps
//                one open (b, min d2) and flushes it when b changes, by idempotent minimum into a pair table the workgroup owns in LDS.
//                Its nearest foreign (d2, label) is one packed 32-bit minimum.  Per-object sums go to a second LDS table.  Only the
//                distinct entries of the two tables go on to global memory: 64-bit adds for geom, 32-bit adds for border / touching,
//                and for a pair a 64-bit atomicCAS on the key (image, a, b), a 32-bit atomicMin on D2 and a 32-bit atomicAdd on n_near.
//                An entry that finds no room in LDS goes to global memory directly.
//   nb_degree    over the occupied slots: the degree of a.
//   nb_offsets   one workgroup: the exclusive scan of the degrees into the CSR offsets.
//   nb_scatter   over the slots again: a pair into its row, in the order of arrival.
//   nb_sort      one thread per pair: its rank among the pairs of its row (the labels of a row are distinct), out of place.  A row of
//                any length comes out sorted; the threads of a long row read it from the caches together.
// A probe sequence that finds no room in the global table sets a flag the host reads at its one synchronisation; it then doubles the
// table and runs everything again.  No floating point; every result is a sum, a minimum or a count of integers, so it does not
// depend on the order of arrival, slot placement or capacity, and is bit-identical run to run.  A label is range-checked when the
// tile is loaded and held as 0 in LDS if it fails: no kernel forms a key or an index from an unchecked label.
#include "label_tile.hpp"
#include "segment_internal.hpp"

#include <algorithm>

namespace cs {

static constexpr int NB_THREADS = 256;
static constexpr int NB_TR = 32, NB_TC = 64;            // the tile: rows, columns
static constexpr int NB_RMAX = 32;                      // the widest halo: max_d2 <= 1024
static constexpr int NB_LDS_PIX = (NB_TR + 2 * NB_RMAX) * (NB_TC + 2 * NB_RMAX);       // 96 x 128 labels, 48 KB
static constexpr int NB_PER = NB_TR * NB_TC / NB_THREADS;                              // 8 pixels of a row per thread in pass A
static constexpr int NB_PAIR_LOG2 = 9, NB_PAIR_SLOTS = 1 << NB_PAIR_LOG2;              // 8 KB
static constexpr int NB_OBJ_LOG2 = 7, NB_OBJ_SLOTS = 1 << NB_OBJ_LOG2;                 // 3 KB
static constexpr int NB_LDS_PROBES = 16;
static constexpr int NB_PROBES = 64;                    // of the global table, before the call asks for a larger one
static constexpr int NB_SCAN_THREADS = 1024;            // nb_offsets
static constexpr int kNbMaxD2 = NB_RMAX * NB_RMAX;
static constexpr int64_t kNbMaxRows = 1 << 22;          // batch * max_label
static constexpr int kNbMinLog2 = 10, kNbMaxLog2 = 26, kNbAutoMinLog2 = 16, kNbAutoMaxLog2 = 24;
static constexpr unsigned long long kNbMul = 0x9E3779B97F4A7C15ull;
static constexpr unsigned int NB_NONE = 0xFFFFFFFFu;

// control word: 1 a label that is negative or above max_label, 8 a probe found no room
static constexpr unsigned int NB_BAD = 1u, NB_FULL = 8u;

struct NbTables {
    unsigned long long* geom;                           // [B][max_label][3]
    int* objects;                                       // [B][max_label][3]: border, touching, degree
    unsigned long long* keys;                           // the pair table: (image << 42) | (a << 21) | b, 0: empty
    unsigned int* d2;                                   // NB_NONE where cleared
    unsigned int* nn;
    int cap_log2, max_label;
};

// a pair of labels in 1..2^20 each; with the image above it the key of the global table
__device__ inline unsigned long long nb_key(int a, int b) { return ((unsigned long long)a << 21) | (unsigned long long)b; }

// d as a candidate of D2 and n more nearest border pixels under `key`, in LDS or global; false: no room within `probes` slots
__device__ inline bool nb_pair(unsigned long long* keys, unsigned int* d2, unsigned int* nn, int log2, int probes, unsigned long long key,
                               unsigned int d, unsigned int n)
{
    const int slot = table_claim(keys, log2, (unsigned int)((key * kNbMul) >> (64 - log2)), key, probes);
    if (slot < 0) return false;
    atomicMin(&d2[slot], d);
    if (n) atomicAdd(&nn[slot], n);
    return true;
}

// what a workgroup holds in LDS: 64648 bytes
struct NbLds {
    int pix[NB_LDS_PIX];                                // the tile with its halo, row stride NB_TC + 2 R; 0: background, outside, refused
    unsigned long long pkey[NB_PAIR_SLOTS];             // nb_key(a, b), 0: empty
    unsigned int pd2[NB_PAIR_SLOTS], pnn[NB_PAIR_SLOTS];
    int okey[NB_OBJ_SLOTS];                             // the label, 0: empty
    unsigned int osum[5][NB_OBJ_SLOTS];                 // area, sum r, sum c (tile coordinates), border, touching
    unsigned short list[NB_TR * NB_TC];                 // the border pixels: (row << 6) | column in the tile
    int cmax[NB_RMAX + 1];                              // per |dr|: the largest |dc| inside the disk
    int n_list;
};

// v[0..4] more of label (1..max_label) at tile origin (r0, c0), straight to the global tables
__device__ inline void nb_obj_global(const NbTables& T, int b, int label, const unsigned int (&v)[5], unsigned int r0, unsigned int c0)
{
    const size_t row = (size_t)b * T.max_label + (label - 1);
    if (v[0]) {
        atomicAdd(&T.geom[row * 3 + 0], (unsigned long long)v[0]);
        atomicAdd(&T.geom[row * 3 + 1], v[1] + (unsigned long long)v[0] * r0);
        atomicAdd(&T.geom[row * 3 + 2], v[2] + (unsigned long long)v[0] * c0);
    }
    if (v[3]) atomicAdd(&T.objects[row * 3 + 0], (int)v[3]);
    if (v[4]) atomicAdd(&T.objects[row * 3 + 1], (int)v[4]);
}

__device__ inline void nb_obj_add(NbLds& L, const NbTables& T, int b, int label, const unsigned int (&v)[5], unsigned int r0, unsigned int c0)
{
    const int slot = table_claim(L.okey, NB_OBJ_LOG2, ((unsigned int)label * 0x9E3779B1u) >> (32 - NB_OBJ_LOG2), label, NB_LDS_PROBES);
    if (slot < 0) {
        nb_obj_global(T, b, label, v, r0, c0);          // no room: straight to the global tables
        return;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j)
        if (v[j]) atomicAdd(&L.osum[j][slot], v[j]);
}

// grid (ceil(W/64), ceil(H/32), B).  labels: [B][H][W] int.  R = floor(sqrt(max_d2)) in 1..32.
__global__ __launch_bounds__(NB_THREADS) void nb_scan(const int* __restrict__ labels, int H, int W, int max_d2, int R, NbTables T,
                                                      unsigned int* __restrict__ ctrl)
{
    __shared__ NbLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.z, r0 = blockIdx.y * NB_TR, c0 = blockIdx.x * NB_TC;
    const int lw = NB_TC + 2 * R, lh = NB_TR + 2 * R;
    const int* ll = labels + (size_t)b * H * W;
    unsigned int flags = 0u;

    for (int s = tid; s < NB_PAIR_SLOTS; s += NB_THREADS) {
        L.pkey[s] = 0ull;
        L.pd2[s] = NB_NONE;
        L.pnn[s] = 0u;
    }
    for (int s = tid; s < NB_OBJ_SLOTS; s += NB_THREADS) {
        L.okey[s] = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) L.osum[j][s] = 0u;
    }
    if (tid <= R) {                                     // the disk: |dc| <= cmax[|dr|]
        const int rem = max_d2 - tid * tid;
        int k = 0;
        while ((k + 1) * (k + 1) <= rem) ++k;
        L.cmax[tid] = k;
    }
    if (tid == 0) L.n_list = 0;
    // the tile with its halo: consecutive threads read consecutive columns; a label is range-checked here, once for all its uses
    for (int i = tid; i < lh * lw; i += NB_THREADS) {
        const int lr = i / lw, lc = i - lr * lw;
        const int r = r0 - R + lr, c = c0 - R + lc;
        int v = 0;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            v = ll[(size_t)r * W + c];
            if (v < 0 || v > T.max_label) {
                flags |= NB_BAD;
                v = 0;
            }
        }
        L.pix[i] = v;
    }
    __syncthreads();

    // ---- pass A: area, sum r, sum c by runs; the border pixels into the list ----
    {
        const int tr = tid >> 3, tc0 = (tid & 7) * NB_PER;                // tile coordinates of the thread's 8 pixels
        const int* at = &L.pix[(tr + R) * lw + tc0 + R];
        int cur = 0;
        unsigned int run[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < NB_PER; ++k) {
            const int v = at[k];                        // 0 outside the image
            const bool edge = v != 0 && (at[k - lw] != v || at[k + lw] != v || at[k - 1] != v || at[k + 1] != v);
            const unsigned long long m = __ballot(edge);
            if (m != 0ull) {                            // uniform over the wave
                const int leader = __ffsll((long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&L.n_list, __popcll(m));
                base = __shfl(base, leader);
                if (edge) L.list[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)((tr << 6) | (tc0 + k));
            }
            if (v == 0) continue;
            if (v != cur) {
                if (run[0]) nb_obj_add(L, T, b, cur, run, r0, c0);
                cur = v;
                run[0] = run[1] = run[2] = 0u;
            }
            run[0] += 1u;
            run[1] += (unsigned int)tr;
            run[2] += (unsigned int)(tc0 + k);
        }
        if (run[0]) nb_obj_add(L, T, b, cur, run, r0, c0);
    }
    __syncthreads();

    // ---- pass B: every lane a border pixel and its disk ----
    const int n_list = L.n_list;
    for (int i = tid; i < n_list; i += NB_THREADS) {
        const int code = L.list[i];
        const int pr = (code >> 6) + R, pc = (code & 63) + R;
        const int a = L.pix[pr * lw + pc];
        unsigned int near = NB_NONE;                    // (d2 << 21) | label: the smallest d2, then the smallest label
        int cb = 0;                                     // the open pair: a sees cb at cd or nearer
        unsigned int cd = 0u;
        const auto put = [&](int bb, unsigned int d, unsigned int n) {
            const unsigned long long key = nb_key(a, bb);
            if (!nb_pair(L.pkey, L.pd2, L.pnn, NB_PAIR_LOG2, NB_LDS_PROBES, key, d, n) &&
                !nb_pair(T.keys, T.d2, T.nn, T.cap_log2, NB_PROBES, ((unsigned long long)b << 42) | key, d, n))
                flags |= NB_FULL;
        };
        for (int dr = -R; dr <= R; ++dr) {
            const int cm = L.cmax[dr < 0 ? -dr : dr];
            const int* row = &L.pix[(pr + dr) * lw + pc];
            const unsigned int dr2 = (unsigned int)(dr * dr);
            for (int dc = -cm; dc <= cm; ++dc) {
                const int v = row[dc];
                if (v == 0 || v == a) continue;
                const unsigned int d = dr2 + (unsigned int)(dc * dc);
                near = min(near, (d << 21) | (unsigned int)v);
                if (v == cb) {
                    cd = min(cd, d);
                } else {
                    if (cb) put(cb, cd, 0u);
                    cb = v;
                    cd = d;
                }
            }
        }
        if (cb) put(cb, cd, 0u);
        const bool touching = near != NB_NONE;
        if (touching) put((int)(near & 0x1FFFFFu), near >> 21, 1u);      // the pair is in a table already: one more nearest pixel
        const unsigned int v[5] = {0u, 0u, 0u, 1u, touching ? 1u : 0u};
        nb_obj_add(L, T, b, a, v, r0, c0);
    }
    __syncthreads();

    // ---- the distinct objects and pairs of the tile ----
    for (int s = tid; s < NB_OBJ_SLOTS; s += NB_THREADS) {
        const int label = L.okey[s];
        if (label == 0) continue;
        const unsigned int v[5] = {L.osum[0][s], L.osum[1][s], L.osum[2][s], L.osum[3][s], L.osum[4][s]};
        nb_obj_global(T, b, label, v, r0, c0);
    }
    for (int s = tid; s < NB_PAIR_SLOTS; s += NB_THREADS) {
        const unsigned long long key = L.pkey[s];
        if (key != 0ull && !nb_pair(T.keys, T.d2, T.nn, T.cap_log2, NB_PROBES, ((unsigned long long)b << 42) | key, L.pd2[s], L.pnn[s]))
            flags |= NB_FULL;
    }
    if (flags) atomicOr(ctrl, flags);
}

// the row of a key's first label
__device__ inline int64_t nb_row(unsigned long long key, int max_label)
{
    return (int64_t)(key >> 42) * max_label + (int64_t)((key >> 21) & 0x1FFFFFull) - 1;
}

__global__ __launch_bounds__(NB_THREADS) void nb_degree(const unsigned long long* __restrict__ keys, int64_t cap, int max_label, int* __restrict__ objects)
{
    const int64_t stride = (int64_t)gridDim.x * NB_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < cap; s += stride) {
        const unsigned long long key = keys[s];
        if (key != 0ull) atomicAdd(&objects[nb_row(key, max_label) * 3 + 2], 1);
    }
}

// one workgroup: offsets[i] = the sum of the degrees before row i, offsets[rows] = the number of pairs.  A thread owns a segment of
// consecutive rows; the 1024 segment sums are scanned by one thread.
__global__ __launch_bounds__(NB_SCAN_THREADS) void nb_offsets(const int* __restrict__ objects, int64_t rows, long long* __restrict__ offsets)
{
    __shared__ long long part[NB_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t seg = (rows + NB_SCAN_THREADS - 1) / NB_SCAN_THREADS;
    const int64_t lo = tid * seg < rows ? tid * seg : rows, hi = lo + seg < rows ? lo + seg : rows;
    long long sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += objects[i * 3 + 2];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int k = 0; k < NB_SCAN_THREADS; ++k) {
            const long long x = part[k];
            part[k] = run;
            run += x;
        }
        offsets[rows] = run;
    }
    __syncthreads();
    long long run = part[tid];
    for (int64_t i = lo; i < hi; ++i) {
        offsets[i] = run;
        run += objects[i * 3 + 2];
    }
}

// raw: [n_pairs] {row, b, D2, n_near}, the rows' entries in the order of arrival; cursor: [rows], cleared
__global__ __launch_bounds__(NB_THREADS) void nb_scatter(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ d2,
                                                         const unsigned int* __restrict__ nn, int64_t cap, int max_label,
                                                         const long long* __restrict__ offsets, int* __restrict__ cursor, int4* __restrict__ raw)
{
    const int64_t stride = (int64_t)gridDim.x * NB_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < cap; s += stride) {
        const unsigned long long key = keys[s];
        if (key == 0ull) continue;
        const int64_t row = nb_row(key, max_label);
        const long long at = offsets[row] + atomicAdd(&cursor[row], 1);
        raw[at] = make_int4((int)row, (int)(key & 0x1FFFFFull), (int)d2[s], (int)nn[s]);
    }
}

// pairs: [n_pairs][3] {b, D2, n_near}, every row sorted by b.  The labels of a row are distinct, so an entry's place is the number of
// smaller labels in its row.
__global__ __launch_bounds__(NB_THREADS) void nb_sort(const int4* __restrict__ raw, const long long* __restrict__ offsets, int64_t rows,
                                                      int* __restrict__ pairs)
{
    const int64_t n = offsets[rows], stride = (int64_t)gridDim.x * NB_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * NB_THREADS + threadIdx.x; e < n; e += stride) {
        const int4 me = raw[e];
        const long long lo = offsets[me.x], hi = offsets[me.x + 1];
        long long rank = 0;
        for (long long j = lo; j < hi; ++j) rank += raw[j].y < me.y ? 1 : 0;
        int* o = pairs + (lo + rank) * 3;
        o[0] = me.y;
        o[1] = me.z;
        o[2] = me.w;
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_neighbors(cs_preproc* p, const int32_t* labels, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                       const cs_neighbors_params* params, int64_t* geom, int32_t* objects, int64_t* offsets, int out_kind, int64_t* n_pairs)
{
    if (!labels || !params || !geom || !objects || !offsets || !n_pairs) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_label < 1) return fail(CS_ERR_INVALID, "max_label %d: must be >= 1", (int)max_label);
    if (params->max_d2 < 1) return fail(CS_ERR_INVALID, "max_d2 %d: must be >= 1", (int)params->max_d2);
    if (params->reserved != 0) return fail(CS_ERR_INVALID, "cs_neighbors_params.reserved must be 0");
    int log2 = params->table_log2;
    if (log2 != 0 && (log2 < kNbMinLog2 || log2 > kNbMaxLog2))
        return fail(CS_ERR_INVALID, "table_log2 %d: 0 (automatic) or %d..%d", log2, kNbMinLog2, kNbMaxLog2);
    if ((rc = image_limits(batch, height, width)) || (rc = label_cap("max_label", max_label, batch, 0, kNbMaxRows, "the tables", "rows"))) return rc;
    if (params->max_d2 > kNbMaxD2)
        return fail(CS_ERR_UNSUPPORTED, "max_d2 %d: distances above %d px (max_d2 %d) are not supported", (int)params->max_d2, NB_RMAX, kNbMaxD2);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    S.nb_n = -1;                                        // until this call has succeeded
    const int H = height, W = width, max_d2 = params->max_d2;
    int R = 1;
    while ((R + 1) * (R + 1) <= max_d2) ++R;
    const size_t npx = (size_t)batch * H * W;
    const int64_t rows = (int64_t)batch * max_label;
    const size_t gbytes = (size_t)rows * 3 * sizeof(int64_t), obytes = (size_t)rows * 3 * sizeof(int32_t), fbytes = (size_t)(rows + 1) * sizeof(int64_t);
    const bool out_host = out_kind == CS_MEM_HOST;
    if (log2 == 0) {
        log2 = kNbAutoMinLog2;
        while (log2 < kNbAutoMaxLog2 && ((int64_t)1 << log2) < 8 * rows) ++log2;
    }

    if ((rc = S.ctrl.ensure(8 * sizeof(int))) || (rc = S.counts.ensure((size_t)rows * sizeof(int)))) return rc;
    const int* d_lab = labels;
    if (in_kind == CS_MEM_HOST) {                       // the upload of the labels in lab
        if ((rc = S.lab.ensure(npx * sizeof(int)))) return rc;
        HIPCHK(hipMemcpyAsync(S.lab.p, labels, npx * sizeof(int), hipMemcpyHostToDevice, st));
        d_lab = S.lab.as<int>();
    }
    // the records on their way to the host, the 8-byte ones first: geom, offsets, objects
    if (out_host && (rc = S.stage.ensure(gbytes + fbytes + obytes))) return rc;
    char* base = S.stage.as<char>();
    unsigned long long* d_geom = out_host ? (unsigned long long*)base : (unsigned long long*)geom;
    long long* d_off = out_host ? (long long*)(base + gbytes) : (long long*)offsets;
    int* d_obj = out_host ? (int*)(base + gbytes + fbytes) : objects;
    unsigned int* d_ctrl = S.ctrl.as<unsigned int>();
    int* d_cursor = S.counts.as<int>();
    const dim3 grid((unsigned)((W + NB_TC - 1) / NB_TC), (unsigned)((H + NB_TR - 1) / NB_TR), (unsigned)batch);

    S.nb_grows = 0;
    for (;;) {
        const int64_t cap = (int64_t)1 << log2;
        if ((rc = S.key.ensure(cap * sizeof(unsigned long long))) || (rc = S.dq.ensure(cap * sizeof(unsigned int))) ||
            (rc = S.rec.ensure(cap * sizeof(unsigned int))) || (rc = S.slab.ensure(cap * sizeof(int4))) ||
            (rc = S.nb_pairs.ensure(cap * 3 * sizeof(int))))
            return rc;
        const NbTables T{d_geom, d_obj, S.key.as<unsigned long long>(), S.dq.as<unsigned int>(), S.rec.as<unsigned int>(), log2, (int)max_label};
        if ((rc = S.clk_nb.record(0, st))) return rc;
        HIPCHK(hipMemsetAsync(d_ctrl, 0, sizeof(int), st));
        HIPCHK(hipMemsetAsync(T.keys, 0, cap * sizeof(unsigned long long), st));
        HIPCHK(hipMemsetAsync(T.d2, 0xFF, cap * sizeof(unsigned int), st));
        HIPCHK(hipMemsetAsync(T.nn, 0, cap * sizeof(unsigned int), st));
        HIPCHK(hipMemsetAsync(d_geom, 0, gbytes, st));
        HIPCHK(hipMemsetAsync(d_obj, 0, obytes, st));
        HIPCHK(hipMemsetAsync(d_cursor, 0, (size_t)rows * sizeof(int), st));
        hipLaunchKernelGGL(nb_scan, grid, dim3(NB_THREADS), 0, st, d_lab, H, W, max_d2, R, T, d_ctrl);
        HIPCHK(hipGetLastError());
        if ((rc = S.clk_nb.record(1, st))) return rc;
        const unsigned sblocks = (unsigned)std::min<int64_t>((cap + NB_THREADS - 1) / NB_THREADS, 4096);
        hipLaunchKernelGGL(nb_degree, dim3(sblocks), dim3(NB_THREADS), 0, st, (const unsigned long long*)T.keys, cap, (int)max_label, d_obj);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nb_offsets, dim3(1), dim3(NB_SCAN_THREADS), 0, st, (const int*)d_obj, rows, d_off);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nb_scatter, dim3(sblocks), dim3(NB_THREADS), 0, st, (const unsigned long long*)T.keys, (const unsigned int*)T.d2,
                           (const unsigned int*)T.nn, cap, (int)max_label, (const long long*)d_off, d_cursor, S.slab.as<int4>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nb_sort, dim3(sblocks), dim3(NB_THREADS), 0, st, (const int4*)S.slab.as<int4>(), (const long long*)d_off, rows,
                           S.nb_pairs.as<int>());
        HIPCHK(hipGetLastError());
        if ((rc = S.clk_nb.record(2, st))) return rc;
        unsigned int flags = 0u;
        long long total = 0;
        HIPCHK(hipMemcpyAsync(&flags, d_ctrl, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&total, d_off + rows, sizeof(long long), hipMemcpyDeviceToHost, st));
        if (out_host) {                                 // wasted when the table has to grow, which is the rare case
            HIPCHK(hipMemcpyAsync(geom, d_geom, gbytes, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(offsets, d_off, fbytes, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(objects, d_obj, obytes, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));                 // the one host synchronisation of an attempt
        if ((rc = S.clk_nb.finish())) return rc;
        S.nb_log2 = log2;
        if (flags & NB_BAD) return fail(CS_ERR_INVALID, "a label is negative or exceeds max_label = %d", (int)max_label);
        if (!(flags & NB_FULL)) {
            S.nb_n = total;
            *n_pairs = total;
            return CS_OK;
        }
        if (log2 >= kNbMaxLog2) return fail(CS_ERR_NOMEM, "the pair table does not fit 2^%d slots", kNbMaxLog2);
        ++log2;
        ++S.nb_grows;
    }
}

int cs_label_neighbors_pairs(cs_preproc* p, int32_t* pairs, int64_t capacity, int pairs_kind)
{
    if (!pairs) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(pairs_kind)) return fail(CS_ERR_INVALID, "pairs_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    if (capacity < 0) return fail(CS_ERR_INVALID, "capacity %lld: must be >= 0", (long long)capacity);
    if (const int rc = handle_check(p)) return rc;
    const SegmentState* S = p->seg;
    if (!S || S->nb_n < 0) return fail(CS_ERR_INVALID, "no pair list on the handle: cs_label_neighbors has not succeeded on it");
    if (capacity < S->nb_n) return fail(CS_ERR_INVALID, "capacity %lld: the pair list has %lld pairs", (long long)capacity, (long long)S->nb_n);
    if (S->nb_n == 0) return CS_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(pairs, S->nb_pairs.p, (size_t)S->nb_n * 3 * sizeof(int32_t),
                          pairs_kind == CS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return CS_OK;
}

int cs_label_neighbors_last_timing(const cs_preproc* p, double* scan_ms, double* rows_ms)
{
    return clock_read(p, &SegmentState::clk_nb, {scan_ms, rows_ms});
}

int cs_label_neighbors_last_table(const cs_preproc* p, int32_t* table_log2, int32_t* grows)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    const SegmentState* S = p->seg;
    if (table_log2) *table_log2 = S ? S->nb_log2 : 0;
    if (grows) *grows = S ? S->nb_grows : 0;
    return CS_OK;
}
