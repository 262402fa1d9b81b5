// segment_internal.hpp -- the state behind cs_preproc::seg as its translation units share it (segment.hip, expand.hip,
// intensity.hip, quantile.hip, texture.hip, shape.hip, neighbors.hip, colocalize.hip, radial.hip, granularity.hip, propagate.hip, quality.hip, spots.hip, illumination.hip): the shared buffers and a clock per family of entry points.  The clock itself and
// the argument rules are stage_host.hpp's, which extract.hip and match.hip use with states of their own.
#pragma once
#include "stage_host.hpp"

namespace cs {

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
    // cs_label_quantiles (quantile.hip) shares img, lab, parent, stage and ctrl as cs_label_intensity does, and has two buffers of
    // its own: the objects' values gathered into segments, and the segments' starts with the cursors that fill them.
    DevBuf lq_val, lq_off;                              // [C][B * H * W] uint16; [2][B][max_label] uint32
    // cs_label_texture (texture.hip) shares img, lab, parent, stage and ctrl in the same way, and keeps the objects' bounding boxes.
    // cs_label_shape (shape.hip) shares lab, parent, stage and ctrl in the same way, and the bounding boxes with cs_label_texture.
    DevBuf tx_box;                                      // [B][max_label][4] int32, encoded (label_boxes.hpp, LbExtent)
    // cs_label_neighbors (neighbors.hip) shares lab, stage and ctrl in the same way; its pair table is in key (keys), dq (D2) and rec
    // (n_near), the unsorted rows in slab, the rows' cursors in counts.  Only the sorted pair list is its own: it stays on the
    // handle until cs_label_neighbors_pairs copies it out, whatever other stage runs between.
    DevBuf nb_pairs;                                    // [nb_n][3] int32
    int64_t nb_n = -1;                                  // -1: no successful cs_label_neighbors yet
    int nb_log2 = 0, nb_grows = 0;                      // the table the last call ended with, and its doublings
    // cs_label_colocalize (colocalize.hip) shares img, lab, parent, stage and ctrl as cs_label_intensity does, and keeps the presence
    // and rank tables of its rank-weighted sums.
    DevBuf co_rank;                                     // [B][C][65536] bytes, then [B][C][65536] uint16
    // cs_label_radial (radial.hip) shares img, lab, parent, stage and ctrl as cs_label_intensity does and has no buffer of its own:
    // column distances in mask, the depth plane in dq, the deepest pixels' keys in key, the caller's centres in rec.
    // cs_label_granularity (granularity.hip) shares img, lab, parent, stage and ctrl in the same way and has no buffer of its own: the
    // working plane P in dq, the erosion E in rec, the reconstruction R in key, uint16 [B][C][Hs][Ws] each, and in ttop an int per
    // reconstruction tile: the round in which it last changed.
    // cs_label_propagate (propagate.hip) has no buffer of its own: the 64-bit keys in key, the open plane in mask, the guide's channel
    // as a planar uint16 in dq, an int per tile in ttop (the round in which it last changed), its control words in ctrl; a host
    // image's seeds and the labels on their way back in lab, a host mask in parent, a host guide in img, a host cost plane in stage.
    // cs_image_quality and cs_object_focus (quality.hip) have no buffer of their own: a host image in img, its labels in lab, its
    // exclude plane in parent, the tables on their way to the host in stage, the status word in ctrl; the image pass keeps the
    // workgroups' (extreme, count) partials in slab and, without a mesh, a tile of sums per workgroup and channel in hist.
    StageClock clk_iq, clk_lf;
    // cs_spot_detect (spots.hip) shares img, lab, parent, stage and ctrl as cs_label_intensity does; its two planes of row sums are in
    // sm_t, the response in dq, the peak pass's ballot words in mask, the rows' counts in counts, the chunks' offsets in chunks, the
    // thresholds in thr.  Only the sorted list and its offsets are its own: they stay on the handle until cs_spot_fill copies them out.
    DevBuf sp_list, sp_off;                             // [sp_n][8] int32; [sp_batch + 1] int64
    int64_t sp_n = -1;                                  // -1: no successful cs_spot_detect yet
    int sp_batch = 0;
    StageClock clk_sd;
    // cs_illum_tile_stats, cs_illum_reduce and cs_illum_apply (illumination.hip) share the buffers: a host image (corrected in
    // place there and copied out) or a host stack in img, a host function in lab, a mesh on its way to the host in stage, the
    // function between its filters in ns_mesh, the Gaussian's row sums in sm_t, the clipped counts in counts.  Only the two sticky
    // status words are their own: a call that does not synchronise leaves them for the next one that does.  A clock per call.
    DevBuf il_status;                                   // [2] uint32: a bad value in a device stack, in a device function
    bool il_unread = false;                             // a call since the last read did not synchronise
    StageClock clk_il_s, clk_il_r, clk_il_a;
    StageClock clk_thr, clk_sp, clk_si, clk_bg, clk_lt, clk_cl, clk_sm, clk_hy, clk_ns, clk_ex, clk_in, clk_lq, clk_tx, clk_sh, clk_nb, clk_co, clk_ra, clk_gr, clk_gs, clk_pg;   // clk_gs: one sums pass of cs_label_granularity at a time
    int pg_rounds = 0;                                  // cs_label_propagate's last call: its rounds, the closing quiet one included
    double gr_ms[3] = {0.0, 0.0, 0.0};                  // cs_label_granularity's last call: prepare, erosions + reconstructions, sums
    int gr_rounds = 0, gr_reads = 0;                    // its reconstruction rounds (all steps) and control-word reads
    int sp_recon_reads = 0, sp_flood_reads = 0;         // control-word reads (one host synchronisation each) of the last split of either kind
};

// the handle's device, and the state on its first use
int state_begin(cs_preproc* p);
// clock_read of a clock of this state; a handle that has not segmented yet reports zeros
inline int clock_read(const cs_preproc* p, StageClock SegmentState::*which, std::initializer_list<double*> out)
{
    return clock_read(p, p && p->seg ? &(p->seg->*which) : nullptr, out);
}

}  // namespace cs
