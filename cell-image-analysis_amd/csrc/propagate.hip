// propagate.hip -- growing the seeds of a label image inside a mask along the cheapest paths on gfx950 (include/cellscreen.h,
// cs_label_propagate; the rule: DESIGN 3zd, restated in tests/propagate_reference.py).
//
// A seed pixel (label 1..2^20) is a source of cost 0 and keeps its label.  A path leaves a seed and then moves through open pixels
// only (not a seed, mask non-zero) to 4- or 8-neighbours; a step q -> p costs w + |g(p) - g(q)| with w = lam * the metric's weight
// and g the guide's channel (0 without a guide); a candidate above max_cost is not taken.  A pixel's key is the lexicographic
// minimum over those paths of (cost, the label of the path's seed), packed (cost << 24) | label: cost < 2^40 by max_cost, label
// < 2^24 by the range check.  (c, l) -> (c + step, l) is monotone, so the keys are the least fixed point of
// K(p) = min(K(p), min over q of K(q) + step(q, p)), and any relaxation that only lowers keys to what some path justifies reaches it.
//   pg_init      ONE read of seeds, mask and guide: the key plane (the label at a seed, PG_NONE elsewhere), the byte plane `open`,
//                with a guide its channel as a planar uint16.  A seed is range-checked before it is a key.
//   pg_relax     one round, sp_flood's scheme (segment.hip) with gr_recon's stamps (granularity.hip): a 64 x 16 tile with a
//                one-pixel halo relaxes in LDS until it is quiet, relaxed atomic 64-bit loads and stores at workgroup scope in
//                LDS and at agent scope in HBM; only the keys that changed are stored.  Keys only fall and never pass the fixed
//                point, so a halo read while a neighbour writes is only late, never wrong; a round in which no tile changed
//                anything is the fixed point.  After a call's first round only the tiles at a moving front run: those that
//                changed, or had one of their 8 neighbours change, in the round before (a stamp per tile).  All images of the
//                batch go in one launch.
//   pg_advance   one thread: the round's "something changed" flag decides whether the call goes on.  The host enqueues rounds in
//                groups (8, 16, 32, then 64 at a time) and reads one int per group; a call takes at most H * W rounds that change
//                something, one more sets the cap flag and ends it.  No kernel waits for another workgroup.
//   pg_finish    keys -> int32 labels and, on request, int64 costs (-1 where nothing reached).
// No floating point, global atomics only on the control words; the result is the unique fixed point, so it is bit-identical run
// to run whatever the order of the tiles and the grouping of the rounds, and nothing crosses between the images of a batch.
// pg_finish reads the key plane only, so `out` may be the `seeds` buffer itself.
#include "segment_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace cs {

static constexpr int PG_THREADS = 256;
static constexpr int PG_TW = 64, PG_TH = 16;            // sg_tile's map: a wave reads one 64-pixel row
static constexpr int PG_TILE = PG_TW * PG_TH;
static constexpr int PG_LW = PG_TW + 2, PG_LH = PG_TH + 2;      // a tile with its halo
static constexpr int PG_PER = PG_TH / (PG_THREADS / PG_TW);     // pixels per thread: rows lw, lw + 4, ...
static constexpr int PG_CHUNK = 4 * PG_THREADS;         // linear pixels per workgroup in the per-pixel passes
static constexpr int PG_GROUP = 8, PG_GROUP_MAX = 64;   // rounds between two reads of the control word: the first group, the largest
static constexpr unsigned long long PG_NONE = ~0ull;
static constexpr int PG_LABEL_BITS = 24;
static constexpr unsigned long long PG_LABEL_MASK = (1ull << PG_LABEL_BITS) - 1ull;
static constexpr int64_t kPgMaxCost = ((int64_t)1 << 40) - 2;
static constexpr size_t kPgMaxBytes = (size_t)1 << 30;  // of the key plane
static constexpr int kPgMaxChannels = 4;
enum { PC_BAD = 0, PC_DONE, PC_CHANGED, PC_ROUNDS, PC_TOTAL, PC_CAPPED, PC_N = 8 };

struct PgRule {
    int axial, diag;                                    // lam * the metric's weights; diag 0: 4-neighbours only
    unsigned long long max_cost;
};

// ---- init ------------------------------------------------------------------------------------------------------------------------
// grid (ceil(H * W / 1024), B).  seeds: [B][H][W] int; mask: null or [B][H][W] bytes; guide: null or [B][H][W][C] PIX.
template <typename PIX>
__global__ __launch_bounds__(PG_THREADS) void pg_init(const int* seeds, const unsigned char* __restrict__ mask, const PIX* __restrict__ guide, int C,
                                                      int ch, int HW, unsigned long long* __restrict__ key, unsigned char* __restrict__ open,
                                                      unsigned short* __restrict__ g16, int* __restrict__ ctrl)
{
    const size_t base = (size_t)blockIdx.y * HW;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * PG_CHUNK + k * PG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const int s = seeds[base + i];
        bad |= s < 0 || s > kMaxLabel;
        const bool seed = s > 0 && s <= kMaxLabel;      // a label out of range never becomes a key
        key[base + i] = seed ? (unsigned long long)s : PG_NONE;
        open[base + i] = (unsigned char)(s == 0 && (!mask || mask[base + i] != 0));
        if (guide) g16[base + i] = (unsigned short)guide[(base + i) * C + ch];
    }
    if (bad) ctrl[PC_BAD] = 1;                          // a plain store of a constant
}

// ---- relax -----------------------------------------------------------------------------------------------------------------------
// one thread, after every round.  A round that changed something is counted against the cap; a path through the plane has fewer
// than H * W pixels, so the cap never binds on a correct run.
__global__ void pg_advance(int* __restrict__ ctrl, int cap)
{
    if (ctrl[PC_DONE] != 0) return;
    ++ctrl[PC_TOTAL];
    if (ctrl[PC_CHANGED] == 0) {
        ctrl[PC_DONE] = 1;
    } else if (++ctrl[PC_ROUNDS] > cap) {
        ctrl[PC_DONE] = 1;
        ctrl[PC_CAPPED] = 1;
    }
    ctrl[PC_CHANGED] = 0;
}

// grid (ceil(W/64), ceil(H/16), B), the thread-to-pixel map of sg_tile.  g16: null without a guide.
__global__ __launch_bounds__(PG_THREADS) void pg_relax(const unsigned char* __restrict__ open, const unsigned short* __restrict__ g16, int H, int W,
                                                       PgRule rule, unsigned long long* key, int* ctrl, int* stamp)
{
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP, AG = __HIP_MEMORY_SCOPE_AGENT;
    if (ctrl[PC_DONE] != 0) return;
    // Only a tile at a moving front can change: after the first round a tile runs when it or one of its eight neighbours changed
    // in the round before (a diagonal step crosses a corner).  stamp holds the round in which a tile last changed.  Neighbours
    // store into these words while this kernel runs: nine threads read one word each and the workgroup decides once, at a barrier
    // all of its threads reach, so it leaves whole or stays whole.  A neighbour that overwrites its stamp in this very round is
    // seen as well (>=), and a change missed now is seen in the next round, which then follows because that neighbour raised the
    // flag.  A tile that is skipped was quiet on its halo when it last ran and no neighbour has changed since, so a round
    // without a change is still the fixed point.
    const int round = ctrl[PC_TOTAL];
    const int tx = (int)gridDim.x, ty = (int)gridDim.y, bx = (int)blockIdx.x, by = (int)blockIdx.y;
    const int tile = ((int)blockIdx.z * ty + by) * tx + bx;
    {
        int go = round == 0;                            // the first round: every tile
        if (!go && threadIdx.x < 9) {
            const int ny = by + (int)threadIdx.x / 3 - 1, nx = bx + (int)threadIdx.x % 3 - 1;
            if (ny >= 0 && ny < ty && nx >= 0 && nx < tx)
                go = __hip_atomic_load(stamp + ((int)blockIdx.z * ty + ny) * tx + nx, __ATOMIC_RELAXED, AG) >= round - 1;
        }
        if (!__syncthreads_or(go)) return;
    }
    const int lx = threadIdx.x & 63, lw = threadIdx.x >> 6;
    const int x0 = bx * PG_TW, y0 = by * PG_TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    const int x = x0 + lx;
    bool op[PG_PER];
    int any_open = 0;
#pragma unroll
    for (int k = 0; k < PG_PER; ++k) {
        const int y = y0 + lw + 4 * k;
        op[k] = x < W && y < H && open[base + (size_t)y * W + x] != 0;
        any_open |= op[k];
    }
    if (!__syncthreads_or(any_open)) return;            // nothing here can take a key: seeds, closed pixels, the image's edge
    __shared__ unsigned long long sK[PG_LH * PG_LW];
    __shared__ unsigned short sG[PG_LH * PG_LW];
    for (int i = threadIdx.x; i < PG_LH * PG_LW; i += PG_THREADS) {
        const int y = y0 + i / PG_LW - 1, xx = x0 + i % PG_LW - 1;
        const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
        sK[i] = in ? __hip_atomic_load(key + base + (size_t)y * W + xx, __ATOMIC_RELAXED, AG) : PG_NONE;
        sG[i] = in && g16 ? g16[base + (size_t)y * W + xx] : (unsigned short)0;
    }
    __syncthreads();
    unsigned long long cur[PG_PER], was[PG_PER];
    int gp[PG_PER];
#pragma unroll
    for (int k = 0; k < PG_PER; ++k) {
        const int c = (lw + 4 * k + 1) * PG_LW + lx + 1;
        was[k] = cur[k] = sK[c];
        gp[k] = sG[c];
    }
    for (int it = 0; it < PG_TILE; ++it) {              // a path inside the tile has at most PG_TILE pixels
        int chg = 0;
#pragma unroll
        for (int k = 0; k < PG_PER; ++k) {
            if (!op[k]) continue;
            const int c = (lw + 4 * k + 1) * PG_LW + lx + 1;
            unsigned long long best = cur[k];
            auto look = [&](int n, int w) {
                const unsigned long long kn = __hip_atomic_load(&sK[n], __ATOMIC_RELAXED, WG);
                if (kn == PG_NONE) return;              // closed, unreached, or outside the image
                const int dg = gp[k] - (int)sG[n];
                const unsigned long long cost = (kn >> PG_LABEL_BITS) + (unsigned long long)(w + (dg < 0 ? -dg : dg));
                if (cost > rule.max_cost) return;
                const unsigned long long cand = (cost << PG_LABEL_BITS) | (kn & PG_LABEL_MASK);
                if (cand < best) best = cand;
            };
            look(c - 1, rule.axial); look(c + 1, rule.axial); look(c - PG_LW, rule.axial); look(c + PG_LW, rule.axial);
            if (rule.diag) {
                look(c - PG_LW - 1, rule.diag); look(c - PG_LW + 1, rule.diag); look(c + PG_LW - 1, rule.diag); look(c + PG_LW + 1, rule.diag);
            }
            if (best < cur[k]) {
                cur[k] = best;
                __hip_atomic_store(&sK[c], best, __ATOMIC_RELAXED, WG);
                chg = 1;
            }
        }
        if (!__syncthreads_or(chg)) break;
    }
    int any = 0;
#pragma unroll
    for (int k = 0; k < PG_PER; ++k) {
        if (cur[k] != was[k]) {                         // an open pixel: inside the image
            __hip_atomic_store(key + base + (size_t)(y0 + lw + 4 * k) * W + x, cur[k], __ATOMIC_RELAXED, AG);
            any = 1;
        }
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0 && any) {
        atomicOr(&ctrl[PC_CHANGED], 1);
        __hip_atomic_store(stamp + tile, round, __ATOMIC_RELAXED, AG);
    }
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// grid (ceil(H * W / 1024), B)
__global__ __launch_bounds__(PG_THREADS) void pg_finish(const unsigned long long* __restrict__ key, int HW, int* __restrict__ out,
                                                        long long* __restrict__ cost)
{
    const size_t base = (size_t)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * PG_CHUNK + k * PG_THREADS + threadIdx.x;
        if (i >= HW) continue;
        const unsigned long long kk = key[base + i];
        out[base + i] = kk == PG_NONE ? 0 : (int)(kk & PG_LABEL_MASK);
        if (cost) cost[base + i] = kk == PG_NONE ? -1ll : (long long)(kk >> PG_LABEL_BITS);
    }
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_propagate(cs_preproc* p, const int32_t* seeds, int32_t batch, int32_t height, int32_t width, int in_kind, const uint8_t* mask,
                       const void* guide, int32_t guide_channels, int guide_pixel_type, const cs_propagate_params* params, int32_t* out,
                       int64_t* cost, int out_kind)
{
    if (!seeds || !out || !params) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (params->metric != CS_PROPAGATE_CITYBLOCK && params->metric != CS_PROPAGATE_CHESSBOARD && params->metric != CS_PROPAGATE_CHAMFER)
        return fail(CS_ERR_INVALID, "cs_propagate_params.metric %d: must be CS_PROPAGATE_CITYBLOCK, _CHESSBOARD or _CHAMFER", (int)params->metric);
    if (params->lam < 1 || params->lam > 255) return fail(CS_ERR_INVALID, "cs_propagate_params.lam %d outside 1..255", (int)params->lam);
    if (params->max_cost < 1 || params->max_cost > kPgMaxCost)
        return fail(CS_ERR_INVALID, "cs_propagate_params.max_cost %lld outside 1..%lld", (long long)params->max_cost, (long long)kPgMaxCost);
    if (params->reserved != 0) return fail(CS_ERR_INVALID, "cs_propagate_params.reserved must be 0");
    if (guide) {
        if (guide_pixel_type != CS_PIX_U8 && guide_pixel_type != CS_PIX_U16)
            return fail(CS_ERR_INVALID, "guide_pixel_type must be CS_PIX_U8 or CS_PIX_U16");
        if (guide_channels < 1 || guide_channels > kPgMaxChannels)
            return fail(CS_ERR_INVALID, "guide_channels %d outside 1..%d", (int)guide_channels, kPgMaxChannels);
        if (params->guide_channel < 0 || params->guide_channel >= guide_channels)
            return fail(CS_ERR_INVALID, "cs_propagate_params.guide_channel %d outside 0..%d", (int)params->guide_channel, (int)guide_channels - 1);
    } else if (params->guide_channel != 0) {
        return fail(CS_ERR_INVALID, "cs_propagate_params.guide_channel %d without a guide: must be 0", (int)params->guide_channel);
    }
    if ((rc = image_limits(batch, height, width))) return rc;
    const int H = height, W = width, HW = H * W;
    const size_t npx = (size_t)batch * HW;
    if (npx * sizeof(unsigned long long) > kPgMaxBytes)
        return fail(CS_ERR_UNSUPPORTED, "batch %d x %d x %d: the key plane takes %zu bytes, above %zu (split the batch)", (int)batch, H, W,
                    npx * sizeof(unsigned long long), kPgMaxBytes);
    if ((rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;
    const int C = guide ? guide_channels : 1;
    const size_t esz = guide_pixel_type == CS_PIX_U8 ? 1 : 2;
    const int tx = (W + PG_TW - 1) / PG_TW, ty = (H + PG_TH - 1) / PG_TH;
    const size_t tbytes = (size_t)batch * tx * ty * sizeof(int);

    // the keys in key, the open plane in mask, the guide's channel in dq, the tiles' stamps in ttop, the control words in ctrl
    if ((rc = S.ctrl.ensure(PC_N * sizeof(int))) || (rc = S.key.ensure(npx * sizeof(unsigned long long))) || (rc = S.mask.ensure(npx)) ||
        (rc = S.ttop.ensure(tbytes)) || (guide && (rc = S.dq.ensure(npx * sizeof(unsigned short)))))
        return rc;
    // a host image's seeds and the labels on their way to the host in lab, a host mask in parent, a host guide in img, a host cost
    // plane in stage
    if ((in_host || out_host) && (rc = S.lab.ensure(npx * sizeof(int)))) return rc;
    if (in_host && ((mask && (rc = S.parent.ensure(npx))) || (guide && (rc = S.img.ensure(npx * C * esz))))) return rc;
    if (out_host && cost && (rc = S.stage.ensure(npx * sizeof(int64_t)))) return rc;
    const int* d_seeds = seeds;
    const unsigned char* d_mask = mask;
    const void* d_guide = guide;
    if (in_host) {
        HIPCHK(hipMemcpyAsync(S.lab.p, seeds, npx * sizeof(int), hipMemcpyHostToDevice, st));
        d_seeds = S.lab.as<int>();
        if (mask) {
            HIPCHK(hipMemcpyAsync(S.parent.p, mask, npx, hipMemcpyHostToDevice, st));
            d_mask = S.parent.as<unsigned char>();
        }
        if (guide) {
            HIPCHK(hipMemcpyAsync(S.img.p, guide, npx * C * esz, hipMemcpyHostToDevice, st));
            d_guide = S.img.p;
        }
    }
    int* d_out = out_host ? S.lab.as<int>() : out;      // pg_finish reads the keys only: a host image's upload is overwritten
    long long* d_cost = !cost ? nullptr : out_host ? S.stage.as<long long>() : (long long*)cost;
    int* d_ctrl = S.ctrl.as<int>();
    unsigned long long* d_key = S.key.as<unsigned long long>();
    const unsigned short* d_g16 = guide ? S.dq.as<const unsigned short>() : nullptr;

    static const int kAxial[3] = {1, 1, 5}, kDiag[3] = {0, 1, 7};
    const PgRule rule{params->lam * kAxial[params->metric], params->lam * kDiag[params->metric], (unsigned long long)params->max_cost};
    const dim3 pgrid((unsigned)((HW + PG_CHUNK - 1) / PG_CHUNK), (unsigned)batch), tgrid((unsigned)tx, (unsigned)ty, (unsigned)batch);
    const dim3 block(PG_THREADS), one(1);
    const int cap = HW;

    S.pg_rounds = 0;
    if ((rc = S.clk_pg.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(d_ctrl, 0, PC_N * sizeof(int), st));
    HIPCHK(hipMemsetAsync(S.ttop.p, 0xff, tbytes, st));  // -1: never
    if (guide && guide_pixel_type == CS_PIX_U16)
        hipLaunchKernelGGL(pg_init<unsigned short>, pgrid, block, 0, st, d_seeds, d_mask, (const unsigned short*)d_guide, C, (int)params->guide_channel,
                           HW, d_key, S.mask.as<unsigned char>(), S.dq.as<unsigned short>(), d_ctrl);
    else
        hipLaunchKernelGGL(pg_init<unsigned char>, pgrid, block, 0, st, d_seeds, d_mask, (const unsigned char*)d_guide, C, (int)params->guide_channel,
                           HW, d_key, S.mask.as<unsigned char>(), guide ? S.dq.as<unsigned short>() : nullptr, d_ctrl);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_pg.record(1, st))) return rc;
    // the rounds, read back once per group, every group twice as long as the one before; the cap ends the call on the device, so
    // this loop ends
    int group = PG_GROUP;
    for (int done = 0; !done; group = std::min(2 * group, PG_GROUP_MAX)) {
        for (int r = 0; r < group; ++r) {
            hipLaunchKernelGGL(pg_relax, tgrid, block, 0, st, S.mask.as<const unsigned char>(), d_g16, H, W, rule, d_key, d_ctrl, S.ttop.as<int>());
            hipLaunchKernelGGL(pg_advance, one, one, 0, st, d_ctrl, cap);
        }
        HIPCHK(hipGetLastError());
        int w[PC_DONE + 1] = {0};                       // one read: the seed check's word rides along with `done`
        HIPCHK(hipMemcpyAsync(w, d_ctrl, sizeof w, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        done = w[PC_DONE];
        if (w[PC_BAD])                                  // known since pg_init: the call ends at its first read, `out` stays unwritten
            return fail(CS_ERR_INVALID, "a seed is negative or exceeds %d", kMaxLabel);
    }
    if ((rc = S.clk_pg.record(2, st))) return rc;
    hipLaunchKernelGGL(pg_finish, pgrid, block, 0, st, (const unsigned long long*)d_key, HW, d_out, d_cost);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_pg.record(3, st))) return rc;
    int words[PC_N] = {0};
    HIPCHK(hipMemcpyAsync(words, d_ctrl, sizeof words, hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(out, d_out, npx * sizeof(int), hipMemcpyDeviceToHost, st));
        if (cost) HIPCHK(hipMemcpyAsync(cost, d_cost, npx * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the last host synchronisation: the round count, the host planes
    if ((rc = S.clk_pg.finish())) return rc;
    S.pg_rounds = words[PC_TOTAL];
    if (words[PC_CAPPED]) return fail(CS_ERR_UNSUPPORTED, "the propagation did not settle within %d rounds (the image is %d x %d)", cap, H, W);
    return CS_OK;
}

int cs_label_propagate_last_timing(const cs_preproc* p, double* init_ms, double* relax_ms, double* finish_ms, int32_t* rounds)
{
    if (const int rc = clock_read(p, &SegmentState::clk_pg, {init_ms, relax_ms, finish_ms})) return rc;
    if (rounds) *rounds = p->seg ? p->seg->pg_rounds : 0;
    return CS_OK;
}
