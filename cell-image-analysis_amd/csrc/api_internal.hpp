// api_internal.hpp -- helpers shared by the C-ABI translation units (api.hip, train_api.hip, preprocess.hip, fit.hip and, through
// stage_host.hpp, the entry points on the preprocess handle): the error record, HIPCHK, DevBuf, and the handle itself.
#pragma once
#include "../../include/cellscreen.h"
#include "common.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace cs {

int fail(int code, const char* fmt, ...);      // records the thread-local message, returns code
const char* last_error_cstr();

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return cs::fail(CS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                            __FILE__, __LINE__);                                             \
    } while (0)

// ---- the reference graph (CAE_improved_modeltrain.py:184-229) ---------------------------
static const int kRefChannels[7] = {32, 64, 32, 32, 64, 32, 1};
static const int kNConv = 7, kNEnc = 3, kH = 64, kW = 64;
static const int kConvGrid[7] = {64, 32, 16, 8, 16, 32, 64};      // conv grid (= pre-pool output) side
// stored per-cell size (floats) of each conv's output tensor (after pool / before upsample)
static const size_t kLayerFloats[7] = {32 * 32 * 32, 16 * 16 * 64, 8 * 8 * 32, 8 * 8 * 32,
                                       16 * 16 * 64, 32 * 32 * 32, 64 * 64};
// conv MACs per cell, SURVEY.md Appendix A.1
static const double kLayerMacs[7] = {1179648, 18874368, 4718592, 589824, 4718592, 18874368, 1179648};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t need)
    {
        if (need <= bytes) return CS_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) { p = nullptr; return fail(CS_ERR_NOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e)); }
        bytes = need;
        return CS_OK;
    }
    template <class T> T* as() const { return (T*)p; }
};

// Orders `mine` (a handle's private stream) after everything enqueued so far on `other` (the caller's stream:
// torch's current stream, an RCCL stream, ...): the cs_*_wait_stream entry points.  other == nullptr is the
// legacy default stream, with which a hipStreamNonBlocking stream is NOT implicitly ordered either.
inline int wait_on_stream(hipStream_t mine, void* other)
{
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, (hipStream_t)other);
    if (e == hipSuccess) e = hipStreamWaitEvent(mine, ev, 0);
    (void)hipEventDestroy(ev);                 // released once the recorded work has completed
    if (e != hipSuccess) return fail(CS_ERR_HIP, "ordering the handle's stream after the caller's failed: %s", hipGetErrorString(e));
    return CS_OK;
}

// ---- crop preprocess (preprocess.hip), shared with the extraction front end (extract.hip) -------------------------------
struct CropDesc {
    long long off;      // element offset of the crop's first pixel in the ragged pixel buffer
    int H, W;
};
// What the preprocess accepts (include/cellscreen.h): output sides, crop sides, and per axis side <= kPreprocMaxRatio * out --
// the ratio that bounds the anti-aliasing Gaussian's radius (preprocess.hip PP_MAX_TAPS).  cs_preprocess checks crops on the
// host, the extraction's region pass on the device, both with preproc_side_beyond, so they cannot disagree about a crop.
static constexpr int kPreprocMin = 8, kPreprocMax = 1024, kPreprocMaxRatio = 16;
static constexpr int kPreprocOutMin = 8, kPreprocOutMax = 512;
__host__ __device__ inline bool preproc_side_beyond(int side, int out) { return side > kPreprocMax || side > kPreprocMaxRatio * out; }
// Enqueues the preprocess kernel on n crops whose descriptors are already in device (or mapped) memory; lds = the dynamic LDS
// bytes the largest crop needs (preprocess_lds_bytes); out: [n][out_h][out_w].  The arithmetic is cs_preprocess's, so the
// cells are bit-identical.
hipError_t launch_preprocess(const void* pix, int pixel_type, const CropDesc* desc, int64_t n, double clip_limit, size_t lds,
                             uint16_t* clahe, float* out, int out_h, int out_w, hipStream_t stream);
struct ExtractState;                            // extract.hip: the state between cs_extract_measure and cs_extract_fill
void extract_state_free(ExtractState* s);
struct SegmentState;                            // segment_internal.hpp: the buffers and clocks of cs_segment_* and of the label tools on its state
void segment_state_free(SegmentState* s);
struct MatchState;                              // match.hip: the buffers, the pair table and the clock of cs_label_match
void match_state_free(MatchState* s);

int upload(DevBuf& d, const void* src, size_t bytes);
int check_arch(const cs_cae_weights* w, int expect_convs, const char* what);
int require_gfx950(int device_id);

}  // namespace cs

// The preprocess handle (include/cellscreen.h); its extraction entry points live in extract.hip, its segmenter in segment.hip,
// its label scoring in match.hip, its label expansion in expand.hip, its intensity measurement in intensity.hip, its order
// statistics in quantile.hip, its texture records in texture.hip.  All seven take their argument rules, the handle check and
// their clocks from stage_host.hpp; each keeps a state of its own below (expand, intensity, quantile and texture share the
// segmenter's), since what must survive between calls differs: extract's uploads from measure to fill, match's pair table.
struct cs_preproc {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int out_h = 64, out_w = 64;         // cs_preproc_set_output_size; read by the next cs_preprocess / cs_extract_measure
    bool extract_pending = false;       // a cs_extract_measure whose cs_extract_fill has not run yet: the size is frozen
    cs::DevBuf pix, clahe, out;
    // crop descriptors: pinned host memory the kernel reads directly (24 B per crop).  A host-to-device COPY of them would
    // queue on the DMA engine behind whatever the caller has in flight there -- e.g. the raw pixels of the NEXT chunk it is
    // uploading while this one computes -- and the kernel would start only when that upload has finished.
    void* hdesc = nullptr;
    const void* ddesc = nullptr;        // the same memory as the device sees it
    double last_kernel_ms = 0.0;
    int64_t last_pixels = 0;
    cs::ExtractState* ext = nullptr;    // created by the first cs_extract_measure
    cs::SegmentState* seg = nullptr;    // created by the first cs_segment_* call
    cs::MatchState* match = nullptr;    // created by the first cs_label_match
    ~cs_preproc()
    {
        cs::extract_state_free(ext);
        cs::segment_state_free(seg);
        cs::match_state_free(match);
        if (hdesc) (void)hipHostFree(hdesc);
    }
};
