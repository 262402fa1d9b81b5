// train_internal.hpp -- the trainer handle shared by train_api.hip (reference graph, tuned kernels) and
// train_generic.hip (any instance of the layer grammar, run-time-shaped kernels).
#pragma once
#include "api_internal.hpp"

constexpr int TR_MAXL = CS_MAX_CONV;

// Pinned host slots for per-step parameters that stream work reads after the call has returned: a slot is written again only
// once the work recorded behind its last use has run.
template <int N>
struct PinnedRing {
    char* pin = nullptr;
    size_t slot_bytes = 0;
    hipEvent_t ev[N] = {nullptr};
    bool used[N] = {false};
    int next = 0, cur = 0;
    // *slot <- the next slot, at least `bytes` long (growing the ring drains `s` first)
    int acquire(size_t bytes, hipStream_t s, char** slot)
    {
        if (bytes > slot_bytes) {
            HIPCHK(hipStreamSynchronize(s));
            if (pin) { (void)hipHostFree(pin); pin = nullptr; slot_bytes = 0; }
            HIPCHK(hipHostMalloc((void**)&pin, bytes * N, hipHostMallocDefault));
            slot_bytes = bytes;
            for (int k = 0; k < N; ++k) {
                used[k] = false;
                if (!ev[k]) HIPCHK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
            }
        }
        cur = next;
        next = (cur + 1) % N;
        if (used[cur]) HIPCHK(hipEventSynchronize(ev[cur]));
        *slot = pin + (size_t)cur * slot_bytes;
        return CS_OK;
    }
    // the work that reads the slot acquired last is enqueued on s
    int release(hipStream_t s)
    {
        HIPCHK(hipEventRecord(ev[cur], s));
        used[cur] = true;
        return CS_OK;
    }
    ~PinnedRing()
    {
        if (pin) (void)hipHostFree(pin);
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    }
};

struct cs_trainer {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;      // weight gradients run here, beside the BatchNormalization-backward chain of the next layer
    hipEvent_t ev_dz[TR_MAXL] = {nullptr}, ev_wg = nullptr;
    cs_train_cfg cfg;
    int64_t maxb = 0;
    int64_t eval_maxb = 0;              // cells the forward-only buffers of cs_train_eval hold
    int64_t eval_chunk = 4096;          // cells per cs_train_eval chunk (1,024 for the generic form)
    // architecture: ref = the reference graph (64x64, 32-64-32 | 32-64-32-1) on the tuned kernels
    bool ref = true;
    int H = 64, W = 64, n_conv = 7, n_enc = 3;
    int ch[TR_MAXL] = {0}, gh[TR_MAXL] = {0}, gw[TR_MAXL] = {0};       // filters, conv grid of layer l
    size_t rfl[TR_MAXL] = {0}, afl[TR_MAXL] = {0};                     // per-cell floats: conv-grid tensor, stored (BN/pool) output
    int cin(int l) const { return l == 0 ? 1 : ch[l - 1]; }
    // flat parameter layout, Keras order: conv l kernel (HWIO), bias, [gamma, beta]
    long off_k[TR_MAXL], off_b[TR_MAXL], off_g[TR_MAXL], off_be[TR_MAXL], nparam = 0;
    long off_mm[TR_MAXL], off_mv[TR_MAXL], nmov = 0;
    cs::DevBuf P, Gown, M, V, MOV;
    float* G = nullptr;                 // gradient buffer in use (own or caller's)
    long step = 0;
    // packed operands, rebuilt after every update (reference graph: MFMA fragments; generic: flipped/transposed HWIO kernels)
    cs::DevBuf wf[TR_MAXL], wft[TR_MAXL], w7eff, ep_inf[TR_MAXL];
    // generic trainer: split-bf16 planes of the forward kernels / of the flipped kernels (conv_generic_x3.hip), re-packed with the weights
    cs::DevBuf wx3f[TR_MAXL], wx3t[TR_MAXL];
    bool x3f[TR_MAXL] = {false}, x3t[TR_MAXL] = {false};
    // batch tensors
    cs::DevBuf x, y, r[TR_MAXL], a[TR_MAXL], out, errpart, dz[TR_MAXL], da[TR_MAXL], stats[TR_MAXL], dup;
    cs::DevBuf aug_tf, aug_in, aug_out;
    cs::DevBuf part_stats, part_bwd, bwd_sums, dzsum_part[TR_MAXL], wpart[TR_MAXL], descs, scal;
    int np_w[TR_MAXL], np_b[TR_MAXL];
    // the reduction descriptors depend on the batch size only: uploaded when it changes, from memory that outlives the copy
    cs::ReduceDesc hdescs[2 * TR_MAXL];
    int64_t descs_batch = -1;
    float* hloss = nullptr;             // pinned {loss, mae}: read after the step's single synchronisation
    // cs_train_step_async: epoch metrics on the device {sum loss, sum mae, batches} (double), what synchronous steps add on the
    // host, and the event behind the step's input copies
    cs::DevBuf macc;
    double hacc[3] = {0.0, 0.0, 0.0};
    // synchronised BatchNormalization under data parallelism: the caller's all-gather in ONE of its two forms -- blocking
    // (cs_train_set_sync_bn: the library drains its stream before the call) or ordered on the stream
    // (cs_train_set_sync_bn_stream: the library only enqueues) -- and its exchange buffer
    cs_allgather_fn sync_fn = nullptr;
    cs_allgather_stream_fn sync_stream_fn = nullptr;
    bool sync_on() const { return sync_fn || sync_stream_fn; }
    int bn_cmax() const { int c = 0; for (int l = 0; l < n_conv - 1; ++l) c = ch[l] > c ? ch[l] : c; return c; }   // largest BatchNormalization layer
    void* sync_ctx = nullptr;
    float* sync_buf = nullptr;
    int64_t sync_cap = 0;
    int sync_rank = 0, sync_world = 1;
    cs::DevBuf sync_scratch;
    hipEvent_t ev_in = nullptr;
    PinnedRing<8> aug_ring;             // cs_train_augment: the transforms on their way to the device
    PinnedRing<16> fit_ring;            // cs_train_fit_step: per-step {transforms, indices} the gather kernel reads directly
    ~cs_trainer()
    {
        if (hloss) (void)hipHostFree(hloss);
        if (ev_in) (void)hipEventDestroy(ev_in);
        for (auto& e : ev_dz) if (e) (void)hipEventDestroy(e);
        if (ev_wg) (void)hipEventDestroy(ev_wg);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#define LCHK(call)                                                                             \
    do {                                                                                       \
        hipError_t le__ = (call);                                                              \
        if (le__ != hipSuccess) return cs::fail(CS_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(le__)); \
    } while (0)

// train_api.hip: the backward's two streams join, every partial sum -> the flat gradient t->G in workgroup order; errpart (the
// reference form) also reduces the forward pass's error partials to the batch's {loss, mae} in t->scal
int reduce_gradient(cs_trainer* t, int64_t B, const float* errpart);

// train_api.hip: the two points of a BatchNormalization layer at which a batch split over ranks is put together again, written once
// for both forms.  Without a hook they enqueue exactly the one final kernel of the single-process step.
//   forward:  the G1 {count, mean, M2} partials of layer l in t->part_stats -> t->stats[l] and the moving averages
//   backward: the G2 {sum dy, sum dy xhat} partials in t->part_bwd -> the two means in t->bwd_sums (over `local` elements per rank)
//             and this rank's dgamma / dbeta in t->G
int bn_forward_finish(cs_trainer* t, int l, int G1);
int bn_backward_finish(cs_trainer* t, int l, int G2, double local);

// train_generic.hip: the run-time-shaped form of the operations the two forms differ in (train_api.hip dispatches them)
int gen_train_setup(cs_trainer* t);                      // buffers that depend on the architecture only
int gen_train_repack(cs_trainer* t);                     // flipped / transposed kernels for the backward-data convs
int gen_train_ensure_batch(cs_trainer* t, int64_t b);
int gen_train_fb_enqueue(cs_trainer* t, int64_t B);      // the batch in t->x / t->y -> gradient in t->G, {loss, mae} in t->scal
int gen_train_eval_enqueue(cs_trainer* t, int64_t nc);   // inference forward of nc cells of t->x / t->y -> t->errpart
