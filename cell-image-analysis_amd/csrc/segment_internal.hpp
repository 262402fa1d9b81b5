// segment_internal.hpp -- the segmenter's host layer as its translation units share it (segment.hip, expand.hip, intensity.hip): the state
// behind cs_preproc::seg with its shared buffers, the one clock, and the argument checks every entry point on that state makes.
#pragma once
#include "api_internal.hpp"

#include <hip/hip_runtime.h>

#include <initializer_list>

namespace cs {

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

struct SegmentState {
    DevBuf img, lab, mask, parent, slab, hist, thr, chunks, counts;     // img: the upload of a host image, whichever entry point
    DevBuf med, stage;                                  // the 3 x 3 median's plane; a plane on its way to a host buffer
    DevBuf dq, rec, key, ttop, ctrl;                    // cs_segment_split and cs_segment_split_intensity only
    DevBuf si_guide;                                    // cs_segment_split_intensity only: a guide uploaded from the host
    DevBuf bg_a, bg_b;                                  // cs_segment_background only: two planes
    DevBuf lt_sum;                                      // cs_segment_local only: row sums
    DevBuf sm_t;                                        // cs_segment_smooth only: row pass
    DevBuf ns_mesh;                                     // cs_segment_noise only: the mesh before and after its filter
    // img, med and stage serve every stage: each use is ordered on the handle's one stream, a call that uploads or stages
    // synchronises before it returns, a median plane is consumed inside the call that made it, and DevBuf::ensure frees with
    // hipFree, which waits for the device.
    // cs_label_expand (expand.hip) has no buffer of its own: column distances in mask, column labels in parent, a host image's
    // labels in lab, a host d2 plane in stage, its status word in ctrl.
    // cs_label_intensity (intensity.hip) has none either: a host image in img, its labels in lab, its exclude plane in parent,
    // the two tables on their way to the host in stage, its status word in ctrl.
    StageClock clk_thr, clk_sp, clk_si, clk_bg, clk_lt, clk_cl, clk_sm, clk_hy, clk_ns, clk_ex, clk_in;
    int sp_recon_reads = 0, sp_flood_reads = 0;         // control-word reads (one host synchronisation each) of the last split of either kind
};

// sides above 4096 and batches above 65535: CS_ERR_UNSUPPORTED
int image_limits(int32_t batch, int32_t height, int32_t width);
// after the argument rules: without a handle the device's absence is reported before the handle's
int handle_check(const cs_preproc* p);
// the handle's device, and the state on its first use
int state_begin(cs_preproc* p);
// What every *_last_timing on this state does: the spans of the family's last call, read now if that call left them on the
// device; a handle that has not segmented yet reports zeros.
int clock_read(const cs_preproc* p, StageClock SegmentState::*which, std::initializer_list<double*> out);

}  // namespace cs
