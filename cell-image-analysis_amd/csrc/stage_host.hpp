// stage_host.hpp -- what the entry points on the preprocess handle share on the host, whichever state they keep (segment.hip,
// expand.hip, intensity.hip, quantile.hip, texture.hip, shape.hip, neighbors.hip, colocalize.hip, radial.hip and granularity.hip on SegmentState, extract.hip on ExtractState, match.hip on
// MatchState): the limits, the argument rules with their texts, the handle check, and the one clock with its read.
#pragma once
#include "api_internal.hpp"

#include <hip/hip_runtime.h>

#include <initializer_list>

namespace cs {

static constexpr int kMaxSide = 4096;                   // image height / width
static constexpr int kMaxBatch = 65535;                 // grid.y / grid.z
static constexpr int kMaxLabel = 1 << 20;               // per image, wherever a table has a row per label

// ---- argument rules, in the order the entry points apply them; some have rules of their own between -------------------------
inline bool mem_kind(int kind) { return kind == CS_MEM_HOST || kind == CS_MEM_DEVICE; }

inline int stack_dims(int32_t batch, int32_t height, int32_t width)
{
    if (batch < 1 || height < 1 || width < 1)
        return fail(CS_ERR_INVALID, "batch %d, height %d, width %d: all must be >= 1", (int)batch, (int)height, (int)width);
    return CS_OK;
}

inline int side_limits(int32_t height, int32_t width)
{
    if (height > kMaxSide || width > kMaxSide)
        return fail(CS_ERR_UNSUPPORTED, "image %dx%d: sides above %d are not supported", (int)height, (int)width, kMaxSide);
    return CS_OK;
}

// sides above 4096 and batches above 65535: CS_ERR_UNSUPPORTED
inline int image_limits(int32_t batch, int32_t height, int32_t width)
{
    if (const int rc = side_limits(height, width)) return rc;
    if (batch > kMaxBatch) return fail(CS_ERR_UNSUPPORTED, "batch %d: at most %d images per call", (int)batch, kMaxBatch);
    return CS_OK;
}

// The cap of a dense table with a row per label: kMaxLabel labels per image and `cap` rows per call, or cells where the rows
// are per channel (channels 0: they are not).  name, tables and unit are the caller's words in the message.
inline int label_cap(const char* name, int32_t max_label, int32_t batch, int32_t channels, int64_t cap, const char* tables, const char* unit)
{
    if (max_label <= kMaxLabel && (int64_t)batch * max_label * (channels ? channels : 1) <= cap) return CS_OK;
    char ch[32] = "";
    if (channels) snprintf(ch, sizeof ch, " x channels %d", (int)channels);
    return fail(CS_ERR_UNSUPPORTED, "%s %d x batch %d%s: %s are capped at %d labels per image and %lld %s", name, (int)max_label, (int)batch,
                ch, tables, kMaxLabel, (long long)cap, unit);
}

// after the argument rules: without a handle the device's absence is reported before the handle's
inline int handle_check(const cs_preproc* p)
{
    if (p) return CS_OK;
    const int rc = require_gfx950(0);
    return rc ? rc : fail(CS_ERR_INVALID, "handle is NULL");
}

// The device times of one family of entry points: up to five events on the handle's stream, created on first use, and the
// spans between neighbours in milliseconds.  A new call records over the events of an earlier one whichever entry point it
// came through (cs_segment_hysteresis runs the local rule's launch), so the first record drops what was not read yet.
struct StageClock {
    static constexpr int kEvents = 5;
    hipEvent_t ev[kEvents] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ran[kEvents - 1] = {false, false, false, false};   // span k, ev[k] .. ev[k + 1]: its step ran in the call that recorded it
    int last = 0;                                       // the last event of that call
    bool pending = false;                               // the events of a call that left its plane on the device: not read yet
    double ms[kEvents - 1] = {0.0, 0.0, 0.0, 0.0};
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // event k on the stream; step_ran: whether the step of the span that ends here ran
    int record(int k, hipStream_t st, bool step_ran = true)
    {
        if (!ev[k]) HIPCHK(hipEventCreate(&ev[k]));
        HIPCHK(hipEventRecord(ev[k], st));
        if (k == 0) pending = false;
        else ran[k - 1] = step_ran;
        last = k;
        return CS_OK;
    }
    // waits for the last event and takes the spans
    int finish()
    {
        HIPCHK(hipEventSynchronize(ev[last]));
        pending = false;
        for (int k = 0; k < last; ++k) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
            ms[k] = ran[k] ? t : 0.0;                   // without its step a span's two records are back to back
        }
        return CS_OK;
    }
};

// What every *_last_timing does: the spans of the family's last call, read now if that call left them on the device, into the
// non-null pointers of `out` in span order.  clk null: the handle has not run that family yet, and reports zeros.
inline int clock_read(const cs_preproc* p, StageClock* clk, std::initializer_list<double*> out)
{
    if (!p) return fail(CS_ERR_INVALID, "handle is NULL");
    if (clk && clk->pending) {
        HIPCHK(hipSetDevice(p->device));
        if (const int rc = clk->finish()) return rc;
    }
    int k = 0;
    for (double* o : out) {
        if (o) *o = clk ? clk->ms[k] : 0.0;
        ++k;
    }
    return CS_OK;
}

}  // namespace cs
