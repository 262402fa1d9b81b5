// expand.hip -- growing the objects of a label image outwards by a fixed distance on gfx950 (include/cellscreen.h,
// cs_label_expand; the rule: DESIGN 3t, restated in tests/expand_reference.py).
//
// A background pixel within sqrt(max_d2) of a labelled pixel takes the label of the nearest one, the smallest label among
// those equally near: skimage.segmentation.expand_labels with the tie decided by the labels instead of by a scan order.  All
// integers: D2 is the exact squared Euclidean distance, found in two passes as the split's distance transform (segment.hip,
// sp_columns / sp_rows), with the label carried along.
//   ex_columns   per pixel the distance g to the nearest labelled pixel of its column, capped at 128, and that pixel's label;
//                where the one above and the one below are equally far, the smaller label (one thread per column, two sweeps,
//                16 rows per step in registers).  A negative label sets the status word by a plain store of a constant.
//   ex_rows      (D2, label) = the lexicographic minimum over |dx| <= r = isqrt(max_d2) of (dx^2 + g^2, column label), from a
//                row strip of both planes in LDS.  The window ends where dx^2 exceeds the best so far; it includes dx^2 == best,
//                where a g = 0 candidate can still win the tie with a smaller label.  A strip with no g <= r in reach, halo
//                included, writes background and leaves (one __syncthreads_or, which is also the barrier behind the loads).
// The two passes are exact together: within a column only its nearest labelled pixel, or the two of them, can be nearest
// overall, and ex_columns keeps the smaller label of the two.  No atomics, no floating point; every pixel is a function of its
// own image's labels, so the result is bit-identical run to run and nothing crosses between the images of a batch.  ex_rows
// reads the two scratch planes only, so `out` may be the `labels` buffer itself.
#include "segment_internal.hpp"

#include <hip/hip_runtime.h>

namespace cs {

static constexpr int EX_THREADS = 256;
static constexpr int EX_CAP = 128;                      // column distances are capped here: only D2 <= 127^2 matters
static constexpr int EX_HALO = EX_CAP - 1;
static constexpr int EX_ROW = EX_THREADS;               // pixels of one row per workgroup in the row pass
static constexpr int EX_STEP = 16;                      // rows a thread of the column pass loads before it uses the first
static constexpr int kExMaxD2 = EX_HALO * EX_HALO;
static constexpr int EX_FAR = 65535;                    // d2 of a pixel that nothing reaches

// grid (ceil(W / 256), B)
__global__ __launch_bounds__(EX_THREADS) void ex_columns(const int* __restrict__ labels, int H, int W, unsigned char* __restrict__ g,
                                                         int* __restrict__ cl, int* __restrict__ status)
{
    const int x = blockIdx.x * EX_THREADS + threadIdx.x;
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.y * H * W + x;
    int d = EX_CAP, lab = 0;                            // nothing above the image
    bool negative = false;
    for (int y0 = 0; y0 < H; y0 += EX_STEP) {
        int v[EX_STEP];
#pragma unroll
        for (int k = 0; k < EX_STEP; ++k) v[k] = y0 + k < H ? labels[base + (size_t)(y0 + k) * W] : 0;
#pragma unroll
        for (int k = 0; k < EX_STEP; ++k) {
            if (y0 + k >= H) continue;
            negative |= v[k] < 0;
            if (v[k] > 0) {
                d = 0;
                lab = v[k];
            } else {
                d = min(d + 1, EX_CAP);
            }
            g[base + (size_t)(y0 + k) * W] = (unsigned char)d;
            cl[base + (size_t)(y0 + k) * W] = lab;
        }
    }
    if (negative) *status = 1;
    d = EX_CAP;
    lab = 0;
    for (int y1 = H - 1; y1 >= 0; y1 -= EX_STEP) {
        unsigned char m[EX_STEP];
        int v[EX_STEP];
#pragma unroll
        for (int k = 0; k < EX_STEP; ++k) {
            m[k] = y1 - k >= 0 ? g[base + (size_t)(y1 - k) * W] : 0;
            v[k] = y1 - k >= 0 ? cl[base + (size_t)(y1 - k) * W] : 0;
        }
#pragma unroll
        for (int k = 0; k < EX_STEP; ++k) {
            if (y1 - k < 0) continue;
            if (m[k] == 0) {
                d = 0;
                lab = v[k];
            } else {
                d = min(d + 1, EX_CAP);
            }
            if (d < (int)m[k]) {
                g[base + (size_t)(y1 - k) * W] = (unsigned char)d;
                cl[base + (size_t)(y1 - k) * W] = lab;
            } else if (d == (int)m[k] && d < EX_CAP && lab < v[k]) {
                cl[base + (size_t)(y1 - k) * W] = lab;  // equally far above and below: the smaller label
            }
        }
    }
}

// grid (ceil(W / 256), H, B); r = isqrt(max_d2) <= 127
__global__ __launch_bounds__(EX_THREADS) void ex_rows(const unsigned char* __restrict__ g, const int* __restrict__ cl, int H, int W, int r,
                                                      int max_d2, int* __restrict__ out, unsigned short* __restrict__ d2)
{
    __shared__ unsigned char sg[EX_ROW + 2 * EX_HALO];
    __shared__ int sl[EX_ROW + 2 * EX_HALO];
    const int t = threadIdx.x, x0 = blockIdx.x * EX_ROW;
    const size_t row = ((size_t)blockIdx.z * H + blockIdx.y) * W;
    int near = 0;
    for (int i = t; i < EX_ROW + 2 * r; i += EX_THREADS) {
        const int xx = x0 - r + i;
        const int gv = xx >= 0 && xx < W ? (int)g[row + xx] : EX_CAP;       // outside the image there is nothing
        sg[i] = (unsigned char)gv;
        sl[i] = gv <= r ? cl[row + xx] : 0;             // beyond r a column cannot come within max_d2: its label is not read
        near |= gv <= r;
    }
    const int any = __syncthreads_or(near);
    const int x = x0 + t;
    if (x >= W) return;
    if (!any) {
        out[row + x] = 0;
        if (d2) d2[row + x] = (unsigned short)EX_FAR;
        return;
    }
    const int c = t + r, g0 = sg[c];
    int best = g0 * g0, bl = sl[c];                     // a labelled pixel: (0, its own label), and the window is empty
    for (int dx = 1; dx <= r && dx * dx <= best; ++dx) {                    // <=: a candidate at dx^2 == best can win the tie
        const int gl = sg[c - dx], gr = sg[c + dx];
        const int al = dx * dx + gl * gl, ar = dx * dx + gr * gr;
        if (al <= best) {
            const int l = sl[c - dx];
            if (al < best || l < bl) {
                best = al;
                bl = l;
            }
        }
        if (ar <= best) {
            const int l = sl[c + dx];
            if (ar < best || l < bl) {
                best = ar;
                bl = l;
            }
        }
    }
    const bool reached = best <= max_d2;
    out[row + x] = reached ? bl : 0;
    if (d2) d2[row + x] = (unsigned short)(reached ? best : EX_FAR);
}

}  // namespace cs

// ---- C ABI ----------------------------------------------------------------------------------
using namespace cs;

int cs_label_expand(cs_preproc* p, const int32_t* labels, int32_t batch, int32_t height, int32_t width, int in_kind,
                    const cs_expand_params* params, int32_t* out, uint16_t* d2, int out_kind)
{
    if (!labels || !out || !params) return fail(CS_ERR_INVALID, "NULL argument");
    if (!mem_kind(in_kind) || !mem_kind(out_kind)) return fail(CS_ERR_INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE");
    int rc;
    if ((rc = stack_dims(batch, height, width))) return rc;
    if (params->max_d2 < 1 || params->max_d2 > kExMaxD2)
        return fail(CS_ERR_INVALID, "max_d2 %d outside 1..%d (distances up to %d px)", (int)params->max_d2, kExMaxD2, EX_HALO);
    if (params->reserved != 0) return fail(CS_ERR_INVALID, "cs_expand_params.reserved must be 0");
    if ((rc = image_limits(batch, height, width)) || (rc = handle_check(p)) || (rc = state_begin(p))) return rc;
    SegmentState& S = *p->seg;
    hipStream_t st = p->stream;
    const int H = height, W = width, max_d2 = params->max_d2;
    int r = 1;
    while ((r + 1) * (r + 1) <= max_d2) ++r;
    const size_t npx = (size_t)batch * H * W;
    const bool in_host = in_kind == CS_MEM_HOST, out_host = out_kind == CS_MEM_HOST;
    if ((rc = S.mask.ensure(npx)) || (rc = S.parent.ensure(npx * sizeof(int))) || (rc = S.ctrl.ensure(8 * sizeof(int)))) return rc;
    if ((in_host || out_host) && (rc = S.lab.ensure(npx * sizeof(int)))) return rc;
    if (d2 && out_host && (rc = S.stage.ensure(npx * sizeof(uint16_t)))) return rc;
    const int* d_in = labels;
    if (in_host) {
        HIPCHK(hipMemcpyAsync(S.lab.p, labels, npx * sizeof(int), hipMemcpyHostToDevice, st));
        d_in = S.lab.as<int>();
    }
    int* d_out = out_host ? S.lab.as<int>() : out;      // a host image is grown in place in its upload
    unsigned short* d_d2 = !d2 ? nullptr : out_host ? S.stage.as<unsigned short>() : d2;

    if ((rc = S.clk_ex.record(0, st))) return rc;
    HIPCHK(hipMemsetAsync(S.ctrl.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(ex_columns, dim3((unsigned)((W + EX_THREADS - 1) / EX_THREADS), (unsigned)batch), dim3(EX_THREADS), 0, st, d_in, H, W,
                       S.mask.as<unsigned char>(), S.parent.as<int>(), S.ctrl.as<int>());
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ex.record(1, st))) return rc;
    hipLaunchKernelGGL(ex_rows, dim3((unsigned)((W + EX_ROW - 1) / EX_ROW), (unsigned)H, (unsigned)batch), dim3(EX_THREADS), 0, st,
                       S.mask.as<const unsigned char>(), S.parent.as<const int>(), H, W, r, max_d2, d_out, d_d2);
    HIPCHK(hipGetLastError());
    if ((rc = S.clk_ex.record(2, st))) return rc;
    int negative = 0;
    HIPCHK(hipMemcpyAsync(&negative, S.ctrl.p, sizeof(int), hipMemcpyDeviceToHost, st));
    if (out_host) {
        HIPCHK(hipMemcpyAsync(out, d_out, npx * sizeof(int), hipMemcpyDeviceToHost, st));
        if (d2) HIPCHK(hipMemcpyAsync(d2, d_d2, npx * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                     // the one host synchronisation: the status word, the host planes
    if ((rc = S.clk_ex.finish())) return rc;
    if (negative) return fail(CS_ERR_INVALID, "negative label in the label image");
    return CS_OK;
}

int cs_label_expand_last_timing(const cs_preproc* p, double* columns_ms, double* rows_ms)
{
    return clock_read(p, &SegmentState::clk_ex, {columns_ms, rows_ms});
}
