// match.hip -- scoring a label image against ground truth on gfx950: the tables from which object matching by intersection
// over union follows (include/cellscreen.h, cs_label_match; the rule and why its matching is unique: DESIGN 3s).
//
// Per image the contingency table of (pred label, truth label) is sparse: an object meets a few objects of the other image and
// the background.  It lives in an open-addressing table in global memory, keyed by (image, p, t) in 58 bits with 0 for an empty
// slot: a 64-bit atomicCAS claims the key, a 32-bit atomicAdd adds the count.  Scattered global atomics are slow (the guides put
// single-lane ones at about 1/17 of the shaped rate), so the design makes them rare instead of fast:
//   lm_count     ONE read of the two planes, 8 bytes per pixel, 16-byte loads where width and pointers allow, on the tile
//                of label_tile.hpp.  A lane keeps one open run of (p, t) with its count and flushes when the pair changes;
//                flushes go into a table in LDS that the workgroup owns (1024 slots), the lanes' last runs merged per distinct
//                pair (merge_open_runs) first.
//                Only the distinct entries of the LDS table go on to the global one: one global atomic pair per distinct pair
//                and tile, not per run.  A pair that finds no room in LDS goes to the global table directly.  Pairs with one
//                side 0 are kept (they complete the areas); (0, 0) is not counted.
//   lm_reduce    over the occupied slots: areas by atomicAdd (A_p = sum over t of the counts of (p, t), t = 0 included), the
//                partner of either side by a 64-bit atomicMax on (I << 20) | (2^20 - label), which prefers the larger I and
//                then the smaller label, and the pairs per image.
//   lm_major     over the slots again, now that the areas are complete: n_major by atomicAdd.
//   lm_unpack    the partner words into the tables.
// A probe sequence that finds no room sets a flag the host reads at its one synchronisation; it then doubles the table and runs
// everything again.  No floating point; every result is a sum, a maximum or a count of integers, so it does not depend on
// insertion order, slot placement or capacity, and is bit-identical run to run.  A label is range-checked before it forms a key,
// and the reduction decodes only keys that passed: no kernel indexes with an unchecked label.
#include "label_tile.hpp"
#include "stage_host.hpp"

#include <algorithm>

namespace cs {

static constexpr int LM_THREADS = LT_THREADS;           // of the slot sweeps too
static constexpr int LM_LDS_LOG2 = 10;
static constexpr int LM_LDS_SLOTS = 1 << LM_LDS_LOG2;   // 12 KB of LDS
static constexpr int LM_LDS_PROBES = 16;
static constexpr int LM_PROBES = 64;                    // of the global table, before the call asks for a larger one
static constexpr int64_t kLmMaxRows = 1 << 22;          // batch * max, for each side
static constexpr int kLmMinLog2 = 10, kLmMaxLog2 = 26, kLmAutoMinLog2 = 16;
static constexpr unsigned long long kLmMul = 0x9E3779B97F4A7C15ull;

// control word: 1 a negative label, 2 a pred label above max_pred, 4 a truth label above max_truth, 8 a probe found no room
static constexpr unsigned int LM_NEG = 1u, LM_PRED = 2u, LM_TRUTH = 4u, LM_FULL = 8u;

__device__ inline unsigned long long lm_key(int b, int p, int t)
{
    return ((unsigned long long)b << 42) | ((unsigned long long)p << 21) | (unsigned long long)t;   // p, t <= 2^20; not both 0
}

// n more pixels of `key` in a table of 2^log2 slots, in LDS or global; false: no room within `probes` slots
__device__ inline bool lm_add(unsigned long long* keys, unsigned int* cnt, int log2, int probes, unsigned long long key, unsigned int n)
{
    const int slot = table_claim(keys, log2, (unsigned int)((key * kLmMul) >> (64 - log2)), key, probes);
    if (slot >= 0) atomicAdd(&cnt[slot], n);
    return slot >= 0;
}

// grid (ceil(W/256), ceil(H/64), B)
__global__ __launch_bounds__(LM_THREADS) void lm_count(const int* __restrict__ pred, const int* __restrict__ truth, int H, int W,
                                                       int max_pred, int max_truth, unsigned long long* __restrict__ keys,
                                                       unsigned int* __restrict__ cnt, int cap_log2, unsigned int* __restrict__ ctrl)
{
    __shared__ unsigned long long lk[LM_LDS_SLOTS];
    __shared__ unsigned int lc[LM_LDS_SLOTS];
    for (int s = threadIdx.x; s < LM_LDS_SLOTS; s += LM_THREADS) {
        lk[s] = 0ull;
        lc[s] = 0u;
    }
    __syncthreads();

    const LabelTile tile = label_tile();
    const int b = tile.b, c_base = tile.c_base;
    const int* pp = pred + (size_t)b * H * W;
    const int* tt = truth + (size_t)b * H * W;
    const bool vec = (W & 3) == 0 && (((uintptr_t)pred | (uintptr_t)truth) & 15) == 0 && c_base + 3 < W;
    // to the workgroup's table, or past it when that has no room
    const auto put = [&](unsigned long long key, unsigned int n) {
        return lm_add(lk, lc, LM_LDS_LOG2, LM_LDS_PROBES, key, n) || lm_add(keys, cnt, cap_log2, LM_PROBES, key, n);
    };

    unsigned int flags = 0u, n = 0u;
    int cp = 0, ct = 0;                                 // the open run: n pixels of (cp, ct)
#pragma unroll 4
    for (int i = 0; i < LT_ROWS; ++i) {
        const int r = tile.r_base + i;
        if (r >= H) break;                              // uniform over the wave
        int x[4], y[4];
        label_load4(pp + (size_t)r * W + c_base, W - c_base, vec, x);
        label_load4(tt + (size_t)r * W + c_base, W - c_base, vec, y);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = x[k], t = y[k];
            if ((p | t) == 0) continue;
            if ((p | t) < 0) { flags |= LM_NEG; continue; }
            if (p > max_pred) { flags |= LM_PRED; continue; }
            if (t > max_truth) { flags |= LM_TRUTH; continue; }
            if (n != 0u && p == cp && t == ct) {
                ++n;
            } else {
                if (n != 0u && !put(lm_key(b, cp, ct), n)) flags |= LM_FULL;
                cp = p; ct = t; n = 1u;
            }
        }
    }
    // the open run of every lane: one insertion per distinct pair of the wave
    merge_open_runs(n != 0u, lm_key(b, cp, ct), tile.lane, [&](unsigned long long key, bool mine, bool leader) {
        const unsigned int sum = wave_sum(mine ? n : 0u);
        if (leader && !put(key, sum)) flags |= LM_FULL;
    });
    __syncthreads();
    // the distinct pairs of the tile
    for (int s = threadIdx.x; s < LM_LDS_SLOTS; s += LM_THREADS) {
        const unsigned long long key = lk[s];
        if (key != 0ull && !lm_add(keys, cnt, cap_log2, LM_PROBES, key, lc[s])) flags |= LM_FULL;
    }
    if (flags) atomicOr(ctrl, flags);
}

struct LmTables {
    int* pred;                                          // [B][max_pred][4]: area, partner, overlap, n_major
    int* truth;                                         // [B][max_truth][4]
    unsigned long long* ppart;                          // [B][max_pred]: (I << 20) | (2^20 - partner), 0: none
    unsigned long long* tpart;                          // [B][max_truth]
    unsigned long long* pairs;                          // [B]
    int max_pred, max_truth;
};

__device__ inline void lm_decode(unsigned long long key, int& b, int& p, int& t)
{
    b = (int)(key >> 42);
    p = (int)((key >> 21) & 0x1fffffull);
    t = (int)(key & 0x1fffffull);
}

__global__ __launch_bounds__(LM_THREADS) void lm_reduce(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                                                        int64_t cap, LmTables T)
{
    const int64_t stride = (int64_t)gridDim.x * LM_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x; s < cap; s += stride) {
        const unsigned long long key = keys[s];
        if (key == 0ull) continue;
        const unsigned int I = cnt[s];
        int b, p, t;
        lm_decode(key, b, p, t);
        const int64_t prow = (int64_t)b * T.max_pred + p - 1, trow = (int64_t)b * T.max_truth + t - 1;
        if (p > 0) atomicAdd(&T.pred[prow * 4], (int)I);
        if (t > 0) atomicAdd(&T.truth[trow * 4], (int)I);
        if (p > 0 && t > 0) {
            atomicMax(&T.ppart[prow], ((unsigned long long)I << 20) | (unsigned long long)(kMaxLabel - t));
            atomicMax(&T.tpart[trow], ((unsigned long long)I << 20) | (unsigned long long)(kMaxLabel - p));
            atomicAdd(&T.pairs[b], 1ull);
        }
    }
}

__global__ __launch_bounds__(LM_THREADS) void lm_major(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                                                       int64_t cap, LmTables T)
{
    const int64_t stride = (int64_t)gridDim.x * LM_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x; s < cap; s += stride) {
        const unsigned long long key = keys[s];
        if (key == 0ull) continue;
        int b, p, t;
        lm_decode(key, b, p, t);
        if (p == 0 || t == 0) continue;
        const long long I2 = 2ll * cnt[s];
        const int64_t prow = (int64_t)b * T.max_pred + p - 1, trow = (int64_t)b * T.max_truth + t - 1;
        if (I2 > T.truth[trow * 4]) atomicAdd(&T.pred[prow * 4 + 3], 1);     // t lies mostly inside p
        if (I2 > T.pred[prow * 4]) atomicAdd(&T.truth[trow * 4 + 3], 1);     // p lies mostly inside t
    }
}

__global__ __launch_bounds__(LM_THREADS) void lm_unpack(LmTables T, int64_t prows, int64_t trows)
{
    const int64_t stride = (int64_t)gridDim.x * LM_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x; s < prows + trows; s += stride) {
        const bool ps = s < prows;
        const int64_t row = ps ? s : s - prows;
        const unsigned long long w = ps ? T.ppart[row] : T.tpart[row];
        if (w == 0ull) continue;                         // the table was cleared: partner 0, overlap 0
        int* out = (ps ? T.pred : T.truth) + row * 4;
        out[1] = kMaxLabel - (int)(w & (unsigned long long)(kMaxLabel - 1));
        out[2] = (int)(w >> 20);
    }
}

struct MatchState {
    DevBuf pred, truth;                                 // uploads of host inputs
    DevBuf keys, cnt, ppart, tpart, pairs, ctrl;
    DevBuf ptab, ttab;                                  // tables on their way to host buffers
    StageClock clk;                                     // spans: count, reduce
    int table_log2 = 0, grows = 0;
};

void match_state_free(MatchState* s) { delete s; }

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_match(cs_preproc* p, const int32_t* pred, const int32_t* truth, int32_t batch, int32_t height, int32_t width, int in_kind,
                   int32_t max_pred, int32_t max_truth, const cs_match_params* params, int32_t* pred_table, int32_t* truth_table,
                   int table_kind, int64_t* n_pairs)
{
    if (!pred || !truth || !pred_table || !truth_table) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(in_kind) || !mem_kind(table_kind)) return fail(CS_ERR_INVALID, "in_kind / table_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (max_pred < 1 || max_truth < 1) return fail(CS_ERR_INVALID, "max_pred %d, max_truth %d: both must be >= 1", (int)max_pred,
                                                   (int)max_truth);
    int log2 = 0;
    if (params) {
        if (params->reserved != 0) return fail(CS_ERR_INVALID, "cs_match_params.reserved must be 0");
        log2 = params->table_log2;
        if (log2 != 0 && (log2 < kLmMinLog2 || log2 > kLmMaxLog2))
            return fail(CS_ERR_INVALID, "table_log2 %d: 0 (automatic) or %d..%d", log2, kLmMinLog2, kLmMaxLog2);
    }
    if ((rc = image_limits(batch, height, width)) || (rc = label_cap("max_pred", max_pred, batch, 0, kLmMaxRows, "the tables", "per batch")) ||
        (rc = label_cap("max_truth", max_truth, batch, 0, kLmMaxRows, "the tables", "per batch")) || (rc = handle_check(p)))
        return rc;
    HIPCHK(hipSetDevice(p->device));
    if (!p->match) p->match = new MatchState();
    MatchState& S = *p->match;

    const size_t npx = (size_t)batch * height * width;
    const int64_t prows = (int64_t)batch * max_pred, trows = (int64_t)batch * max_truth;
    if (log2 == 0) {
        log2 = kLmAutoMinLog2;
        while (((int64_t)1 << log2) < 2 * (prows + trows)) ++log2;       // at most 2^24
    }
    const int *d_pred = pred, *d_truth = truth;
    if (in_kind == CS_MEM_HOST) {
        if ((rc = S.pred.ensure(npx * sizeof(int32_t))) || (rc = S.truth.ensure(npx * sizeof(int32_t)))) return rc;
        HIPCHK(hipMemcpyAsync(S.pred.p, pred, npx * sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipMemcpyAsync(S.truth.p, truth, npx * sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
        d_pred = S.pred.as<int>();
        d_truth = S.truth.as<int>();
    }
    const bool tdev = table_kind == CS_MEM_DEVICE;
    const size_t pbytes = (size_t)prows * 4 * sizeof(int32_t), tbytes = (size_t)trows * 4 * sizeof(int32_t);
    if (!tdev && ((rc = S.ptab.ensure(pbytes)) || (rc = S.ttab.ensure(tbytes)))) return rc;
    if ((rc = S.ppart.ensure(prows * sizeof(unsigned long long))) || (rc = S.tpart.ensure(trows * sizeof(unsigned long long))) ||
        (rc = S.pairs.ensure(batch * sizeof(unsigned long long))) || (rc = S.ctrl.ensure(sizeof(unsigned int))))
        return rc;
    const LmTables T{tdev ? pred_table : S.ptab.as<int>(), tdev ? truth_table : S.ttab.as<int>(), S.ppart.as<unsigned long long>(),
                     S.tpart.as<unsigned long long>(), S.pairs.as<unsigned long long>(), (int)max_pred, (int)max_truth};
    const dim3 cgrid = label_tile_grid(batch, height, width);
    S.grows = 0;
    for (;;) {
        const int64_t cap = (int64_t)1 << log2;
        if ((rc = S.keys.ensure(cap * sizeof(unsigned long long))) || (rc = S.cnt.ensure(cap * sizeof(unsigned int)))) return rc;
        if ((rc = S.clk.record(0, p->stream))) return rc;
        HIPCHK(hipMemsetAsync(S.keys.p, 0, cap * sizeof(unsigned long long), p->stream));
        HIPCHK(hipMemsetAsync(S.cnt.p, 0, cap * sizeof(unsigned int), p->stream));
        HIPCHK(hipMemsetAsync(S.ctrl.p, 0, sizeof(unsigned int), p->stream));
        hipLaunchKernelGGL(lm_count, cgrid, dim3(LM_THREADS), 0, p->stream, d_pred, d_truth, (int)height, (int)width, (int)max_pred,
                           (int)max_truth, S.keys.as<unsigned long long>(), S.cnt.as<unsigned int>(), log2, S.ctrl.as<unsigned int>());
        HIPCHK(hipGetLastError());
        if ((rc = S.clk.record(1, p->stream))) return rc;
        HIPCHK(hipMemsetAsync(T.pred, 0, pbytes, p->stream));
        HIPCHK(hipMemsetAsync(T.truth, 0, tbytes, p->stream));
        HIPCHK(hipMemsetAsync(T.ppart, 0, prows * sizeof(unsigned long long), p->stream));
        HIPCHK(hipMemsetAsync(T.tpart, 0, trows * sizeof(unsigned long long), p->stream));
        HIPCHK(hipMemsetAsync(T.pairs, 0, batch * sizeof(unsigned long long), p->stream));
        const unsigned rblocks = (unsigned)std::min<int64_t>((cap + LM_THREADS - 1) / LM_THREADS, 4096);
        hipLaunchKernelGGL(lm_reduce, dim3(rblocks), dim3(LM_THREADS), 0, p->stream, S.keys.as<unsigned long long>(),
                           S.cnt.as<unsigned int>(), cap, T);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(lm_major, dim3(rblocks), dim3(LM_THREADS), 0, p->stream, S.keys.as<unsigned long long>(),
                           S.cnt.as<unsigned int>(), cap, T);
        HIPCHK(hipGetLastError());
        const unsigned ublocks = (unsigned)std::min<int64_t>((prows + trows + LM_THREADS - 1) / LM_THREADS, 4096);
        hipLaunchKernelGGL(lm_unpack, dim3(ublocks), dim3(LM_THREADS), 0, p->stream, T, prows, trows);
        HIPCHK(hipGetLastError());
        if ((rc = S.clk.record(2, p->stream))) return rc;
        unsigned int flags = 0u;
        HIPCHK(hipMemcpyAsync(&flags, S.ctrl.p, sizeof(unsigned int), hipMemcpyDeviceToHost, p->stream));
        if (!tdev) {                                    // wasted when the table has to grow, which is the rare case
            HIPCHK(hipMemcpyAsync(pred_table, T.pred, pbytes, hipMemcpyDeviceToHost, p->stream));
            HIPCHK(hipMemcpyAsync(truth_table, T.truth, tbytes, hipMemcpyDeviceToHost, p->stream));
        }
        if (n_pairs) HIPCHK(hipMemcpyAsync(n_pairs, T.pairs, batch * sizeof(int64_t), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));          // the one host synchronisation of an attempt
        if ((rc = S.clk.finish())) return rc;
        S.table_log2 = log2;
        if (flags & LM_NEG) return fail(CS_ERR_INVALID, "negative label in the label images");
        if (flags & LM_PRED) return fail(CS_ERR_INVALID, "a pred label exceeds max_pred = %d", (int)max_pred);
        if (flags & LM_TRUTH) return fail(CS_ERR_INVALID, "a truth label exceeds max_truth = %d", (int)max_truth);
        if (!(flags & LM_FULL)) return CS_OK;
        if (log2 >= kLmMaxLog2) return fail(CS_ERR_NOMEM, "the pair table does not fit 2^%d slots", kLmMaxLog2);
        ++log2;
        ++S.grows;
    }
}

int cs_label_match_last_timing(const cs_preproc* p, double* count_ms, double* reduce_ms)
{
    return clock_read(p, p && p->match ? &p->match->clk : nullptr, {count_ms, reduce_ms});
}

int cs_label_match_last_table(const cs_preproc* p, int32_t* table_log2, int32_t* grows)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    const MatchState* S = p->match;
    if (table_log2) *table_log2 = S ? S->table_log2 : 0;
    if (grows) *grows = S ? S->grows : 0;
    return CS_OK;
}
