// conv12_fused.hip -- conv1 + conv2 of the encoder as ONE kernel: crop -> p2, p1 never leaves the CU.
//   conv1: Conv2D 1->32 on 64x64 + ReLU + BN + MaxPool   (CAE_improved_modeltrain.py:191-193)
//   conv2: Conv2D 32->64 on 32x32 + ReLU + BN + MaxPool  (:195-197)
//
// conv2 is Winograd F(4x4, 3x3) (interpolation points 0, +-1, +-2, inf): a 4x4 output tile costs 36
// multiplies per channel pair where F(2x2,3x3) needed 64.  Measured in fp32 emulation before adopting
// (tests/study_wino_error.py, tests/study_split_fp16.py): p2 error 1.1e-6 .. 1.6e-6 of its range, features 4.3e-7 of theirs
// (bar 1e-5).  conv1 (2.4 % of the path's MACs) is computed inside the staging of conv2's input rows, so the 131 KB/cell p1
// tensor (written by one kernel, read by the next) and one launch disappear.
//
// Two forms (template flag H = cs_model_options.precision): H (CS_PRECISION_SPLIT16) -- both contractions as two-term fp16 splits on
// v_mfma_f32_16x16x32_f16 with exact power-of-two operand scales from the crop's own maximum -- and !H (CS_PRECISION_FP32_EXACT) --
// everything on v_mfma_f32_16x16x4_f32.
//
// One 512-thread workgroup per CU (8 waves = 2 per SIMD, 159 KB of LDS) walks whole cells; a cell is four
// GROUPS of 16 tiles (two tile rows = 8 conv2 rows).  Per group, four phases, one barrier after each (H form; cycles per group
// and wave from the stamped build, tools/c12_diag.py, profiles/r04_*_conv12_phase_diag.txt):
//   P1 conv1   wave (x-tile, 16-channel slice) computes the 8 new p1 rows of the group from the crop's [hi | lo] records in LDS
//              (made IN PLACE from the staged fp32 crop, once per cell, by the threads that staged it): all nine taps of the 3x3
//              window in one K = 32 fragment, two MFMAs per 16 pixels x 16 filters; the vertical tile pair is the pool window;
//              bias -> ReLU -> BN -> max; rows go to a 10-slot ring in LDS (slot = row mod 10; two rows carry over).     2.5 k
//   P2 V=B^TdB thread (tile, channel PAIR, half of the transform rows): ds_read_b64, packed-fp32 transforms, one v_cvt_pk_f16_f32 +
//              two v_fma_mix per pair for [hi c | hi c+1] / [lo c | lo c+1], V written in the A-operand order of P3.        2.4 k
//   P3 MFMA    wave (column group g of 3 transform-domain columns, 16-filter slice): U = G g G^T of its
//              18 points x 32 channels stays in 144 VGPRs for the life of the workgroup; per point two ds_read_b128 and three
//              MFMAs; row fold s = A^T M in registers.  Output rows (2g, 2g+1) of s stay; the other two go to the partner wave
//              (same slice, other column group) through LDS that is dead at this point (the ring's 8 consumed slots + a 16 KB
//              area).  Bound by the LDS reads of V (every element is read by the four waves that share its columns): with
//              neither MFMAs nor fold the phase still takes 1.9 k of its                                              3.1 k
//   P4 Y=sA    column fold of the wave's two output rows over all six columns, bias -> ReLU -> BN -> 2x2
//              max (those two rows are one pool row), store p2.                                                        1.4 k
// (+ four barriers: 1.4 k.)  LDS map: V 73,728 | ring 10 x (34 x 32 + 8) x 4 = 43,840 | exchange 16,384 | crop 67 x 72 x 4 =
// 19,296 | conv1 fragments (both forms) and epilogue constants 9,344 | the crop's maximum 16.
#include "kernel_setup.hpp"
#include "split16.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace cs {

namespace {

constexpr int NTHR = 512;
constexpr int V_BYTES = 36 * 2048;                   // [xi][q][kq][slot][4]: 2 KB per transform point
constexpr int RING_SLOTS = 10;
constexpr int RING_ROWF = 34 * 32 + 8;               // floats per slot: 32 interior columns + 2 halo, 32 channels, + 8: four rows down is
                                                     // 32 banks on (P2's ds_read_b64 groups hold one tile of each tile row)
static_assert((4 * RING_ROWF) % 64 == 32 && RING_ROWF % 2 == 0, "ring pitch");
constexpr int RING_BYTES = RING_SLOTS * RING_ROWF * 4;
constexpr int E2_BYTES = 8 * 2048;
constexpr int INP_STRIDE = 72;                       // floats per crop row: interior at 4..67 (16-byte aligned), halo at 3 and 68
constexpr int INP_BYTES = 67 * INP_STRIDE * 4;         // crop rows -1 .. 64, + one zero row: P1's K = 32 fragments read one record row past
                                                     // their window (against zero weights: it has to be finite)
constexpr int OFF_RING = V_BYTES;
constexpr int OFF_E2 = OFF_RING + RING_BYTES;
constexpr int OFF_INP = OFF_E2 + E2_BYTES;
constexpr int OFF_B1 = OFF_INP + INP_BYTES;            // conv1's B fragments [2 slices][3 K steps][64 lanes]
constexpr int OFF_EP1 = OFF_B1 + 2 * 3 * 64 * 4;       // conv1 epilogue {bias, bn scale, bn shift, sign} per channel
constexpr int OFF_EP2 = OFF_EP1 + 32 * 16;             // conv2 epilogue, same
constexpr int OFF_B1X = OFF_EP2 + 64 * 16;             // conv1 on bf16 MFMAs: B fragments [2 slices][3 MFMAs][64 lanes][8 bf16]
constexpr int OFF_W9 = OFF_B1X + 2 * 3 * 64 * 16;      // ... and the fp32 weight of tap (2,2) per channel
constexpr int OFF_XMAX = OFF_W9 + 32 * 4;               // C2H: max|x| of the crop staged for the next cell (one word; 16 bytes kept)
constexpr int LDS_BYTES = OFF_XMAX + 16;
static_assert(LDS_BYTES <= 160 * 1024 && OFF_RING % 16 == 0 && OFF_E2 % 16 == 0 && OFF_INP % 16 == 0, "LDS map");

__device__ __forceinline__ float vmaxf(float a, float b) { float d; asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ float vminf(float a, float b) { float d; asm("v_min_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }

// pool_post's maxima are raw inline-asm v_max_f32 (no canonicalisation).  The compiler's hazard recogniser does not look inside
// inline asm, and the hardware does not interlock a VALU read of a register an MFMA has just written (8-pass XDL write -> VALU
// read: 11 wait states): an asm v_max placed right behind the MFMA that produces its input reads the OLD register contents
// -- measured: the last conv row of every P1 batch wrong once nothing else sat between the MFMAs and the pooling.  These fences
// take the accumulators as read-write operands, so they sit behind the producing MFMAs and ahead of every consumer, and spend
// the wait states explicitly (16 cycles per batch of 16 MFMAs).
__device__ __forceinline__ void mfma_result_fence(f32x4& a, f32x4& b)
{
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void mfma_result_fence(f32x4 (&a)[4], f32x4 (&b)[4])
{
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}

// bias -> ReLU -> BN -> 2x2 max of a window of raw conv sums.  The map v -> BN(relu(v + bias)) is monotone with the
// direction of the BN scale's sign, so the max over the window of the mapped values is the map of the window's max
// (scale >= 0) or min (scale < 0).  The min case is folded into the weights: channels with a negative BN scale carry
// NEGATED kernels (pack_conv12_*), so the MFMAs produce -z exactly (negation commutes with every fp32 rounding), the
// window's min is -max(-z), and v = sgn * max + bias with sgn = -1 for those channels -- one fma, no second path.
__device__ __forceinline__ float pool_post(float a, float b, float c, float d, float sgn, float bias, float bns, float bnt)
{
    float mx;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(mx) : "v"(a), "v"(b), "v"(c));       // raw, like vmaxf: see mfma_result_fence
    mx = vmaxf(mx, d);
    const float v = vmaxf(fmaf(sgn, mx, bias), 0.0f);   // raw v_max: never NaN for finite inputs, no canonicalisation needed
    return fmaf(v, bns, bnt);
}

// 1-D input transform B^T of F(4,3), points (0, 1, -1, 2, -2, inf): 12 operations
__device__ __forceinline__ void bt6(const float d[6], float o[6])
{
    o[0] = fmaf(4.0f, d[0], fmaf(-5.0f, d[2], d[4]));
    o[5] = fmaf(4.0f, d[1], fmaf(-5.0f, d[3], d[5]));
    const float t1 = fmaf(-4.0f, d[2], d[4]), t2 = fmaf(-4.0f, d[1], d[3]);
    o[1] = t1 + t2;
    o[2] = t1 - t2;
    const float t3 = d[4] - d[2], t4 = d[3] - d[1];
    o[3] = fmaf(2.0f, t4, t3);
    o[4] = fmaf(-2.0f, t4, t3);
}

// DIAG: diagnostic build (CS_C12_DIAG=1) that stamps s_memtime at the phase boundaries of every group and sums the
// differences per wave: [0] P1, [1] wait at barrier 1, [2] P2, [3] barrier 2,
// [4] P3, [5] barrier 3, [6] P4 (fold, epilogue, stores; the next cell's records), [7] barrier 4.
// Never used for results or timing.
#define C12_STAMP(k)                                                       \
    if constexpr (DIAG) {                                                  \
        const unsigned long long t__ = cycle_stamp();                        \
        dg[k] += t__ - dt;                                                 \
        dt = t__;                                                          \
    }

// A crop with a non-finite pixel is screened as if that pixel were 0: its NaN / Inf must not reach the LDS images other cells of this
// persistent workgroup are built in (zero weights against neighbouring records would turn a stale NaN into a NaN of the NEXT cell).
// The cell's error sums (conv67 reads x itself) come out NaN / Inf anyway, and finalize_kernel then reports NaN scores for it.
__device__ __forceinline__ void c12_sanitize(f32x4& v)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __builtin_fabsf(v[j]) <= 3.402823466e38f ? v[j] : 0.0f;
}

// one ds_read_b64 that the load / store optimiser leaves alone (a volatile access in the LDS address space)
__device__ __forceinline__ f32x2 lds_read_b64(const float* p)
{
    typedef const volatile __attribute__((address_space(3))) f32x2* lds_ptr;
    return *(lds_ptr)p;
}
__device__ __forceinline__ f32x2 pfma(float c, f32x2 a, f32x2 b) { return __builtin_elementwise_fma(f32x2{c, c}, a, b); }

// B^T of F(4,3) on a channel pair, the rows a thread of P2 owns: LO = outputs (0, 1, 2) from inputs d0 .. d4, otherwise outputs
// (3, 4, 5) from d1 .. d5 (d[] holds the five inputs in order).  The operations and their order are bt6's.
template <bool LO>
__device__ __forceinline__ void bt6_half(const f32x2 (&d)[5], f32x2 (&o)[3])
{
    if constexpr (LO) {
        o[0] = pfma(4.0f, d[0], pfma(-5.0f, d[2], d[4]));
        const f32x2 t1 = pfma(-4.0f, d[2], d[4]), t2 = pfma(-4.0f, d[1], d[3]);
        o[1] = t1 + t2;
        o[2] = t1 - t2;
    } else {
        const f32x2 t3 = d[3] - d[1], t4 = d[2] - d[0];
        o[0] = pfma(2.0f, t4, t3);
        o[1] = pfma(-2.0f, t4, t3);
        o[2] = pfma(4.0f, d[0], pfma(-5.0f, d[2], d[4]));
    }
}
__device__ __forceinline__ void bt6_pair(const f32x2 (&d)[6], f32x2 (&o)[6])
{
    o[0] = pfma(4.0f, d[0], pfma(-5.0f, d[2], d[4]));
    o[5] = pfma(4.0f, d[1], pfma(-5.0f, d[3], d[5]));
    const f32x2 t1 = pfma(-4.0f, d[2], d[4]), t2 = pfma(-4.0f, d[1], d[3]);
    o[1] = t1 + t2;
    o[2] = t1 - t2;
    const f32x2 t3 = d[4] - d[2], t4 = d[3] - d[1];
    o[3] = pfma(2.0f, t4, t3);
    o[4] = pfma(-2.0f, t4, t3);
}
// C2H: conv2's contraction M = V U (P3) as a TWO-term fp16 split on v_mfma_f32_16x16x32_f16 (conv_wino_up.hip, conv67_h2_kernel, has
// the algebra and the hardware facts; tests/study_split_fp16.py the error: p2 1.1e-6 of its range, the fp32 chain 1.2e-6).  A
// transform point's 32 channels are ONE K = 32 instruction, so 36 points x 4 tile groups x 4 filter slices x 3 products = 1,728
// MFMAs of 16 cycles per cell replace 4,608 fp32 ones of 32; U as two fp16 planes is the same 144 VGPRs per wave.
//   scale   |V| <= 100 max|p1| (B^T of F(4,3) has absolute row sums <= 10), and max|p1| <= a1 max|x| + b1 with a1, b1 from
//           conv1's weights and BN (host, pack_conv12_p1_bound): S puts 100 (a1 max|x| + b1) into [2^14, 2^15), max|x| is taken
//           where the crop is staged (once per cell).  The ring holds S p1 at no cost (conv1's BN constants times S: a
//           power of two commutes with every rounding), V = B^T d B comes out scaled, U carries the layer's S_w from the host, and
//           the conv2 epilogue's sign factor carries 1 / (S S_w).
//   P2      the 16-byte A fragments want 8 CHANNELS of one plane: a thread owns a channel PAIR, so its [hi c | hi c+1] and
//           [lo c | lo c+1] dwords are whole (one v_cvt_pk_f16_f32 + two v_fma_mix per pair; 36 ds_write_b32 per thread).
//   V       [point][tile 16][slot 8 ^ ((tile >> 1) & 7)][16 B]: slots 0-3 = hi of channels 8 kq .., 4-7 = lo; the XOR makes every
//           16-lane group of P3's ds_read_b128 land on 16 distinct slots, and a half wave's writes cover one tile's 128 bytes.
//   P3      per point two ds_read_b128 and three MFMAs (hi lo, lo hi, hi hi in that order on one accumulator: small terms first).
// C1H: conv1 (P1) likewise.  Its K is only 9 taps: a pixel is ONE dword record [hi | lo] and all nine taps of the 3x3 window
// (x 2 planes) sit in one K = 32 fragment (see P1); the large products and the cross terms are two MFMAs on the same A registers
// (one magnitude per instruction: the in-instruction adder truncates ~25 bits below its largest addend).
template <bool DIAG, bool H>
__global__ __launch_bounds__(NTHR, 2) void conv12_fused_kernel(const float* __restrict__ x, const float* __restrict__ w1frag,
                                                              const float* __restrict__ ep1, const float* __restrict__ ufrag,
                                                              const float* __restrict__ ep2, float* __restrict__ p2, long n_cells,
                                                              unsigned long long* __restrict__ diag, const unsigned int* __restrict__ w1x3,
                                                              float p1a, float p1b, float inv_sw, float inv_sw1)
{
    constexpr bool C2H = H, C1H = H;            // conv2's / conv1's contraction as a two-term fp16 split (the two always go together)
    unsigned long long dg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dt = 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const ring = (float*)(smem + OFF_RING);
    float* const inp = (float*)(smem + OFF_INP);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- P3 operands: U of this wave's 18 transform points, all 32 input channels, its 16 filters.  These 144 VGPRs
    // are the kernel's register budget; every other per-lane constant is kept in LDS or recomputed per group.
    const int gcol = w & 1, sl = w >> 1;
    float U[144];
#pragma unroll
    for (int s = 0; s < 144; ++s) U[s] = ufrag[((size_t)w * 144 + s) * 64 + lane];
#pragma unroll
    for (int s = 0; s < 144; ++s) asm volatile("" : "+v"(U[s]));     // first use inside the loop would put the wait for these loads there
    const int xt = w & 3, s1 = w >> 2;                                // P1: tile column, 16-channel slice of conv1

    const long my_cells = (n_cells - blockIdx.x + gridDim.x - 1) / gridDim.x;
    if (my_cells <= 0) return;

    // ---- LDS: zero everything once (halo columns / rows of the crop and the ring are never written again), then the
    // small tables: conv1's B fragments [2][3][64] and the epilogue constants {bias, bn scale, bn shift, sign} per channel
    for (int i = tid; i < LDS_BYTES / 16; i += NTHR) ((f32x4*)smem)[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();
    if (tid < 384) ((float*)(smem + OFF_B1))[tid] = w1frag[tid];
    if (tid < 32) {
        const float sc = ep1[32 + tid];
        ((f32x4*)(smem + OFF_EP1))[tid] = f32x4{ep1[tid], sc, ep1[64 + tid], sc >= 0.0f ? 1.0f : -1.0f};
    }
    if (tid >= 64 && tid < 128) {
        const int c = tid - 64;
        const float sc = ep2[64 + c];
        ((f32x4*)(smem + OFF_EP2))[c] = f32x4{ep2[c], sc, ep2[128 + c], sc >= 0.0f ? 1.0f : -1.0f};
    }
    if constexpr (C1H) {
        for (int i = tid; i < (2 * 2 * 64 * 16) / 4; i += NTHR) ((unsigned int*)(smem + OFF_B1X))[i] = w1x3[i];
    }
    {
        const int srow = tid >> 4, sc16 = tid & 15;
        const float* src = x + (size_t)blockIdx.x * 4096 + srow * 64 + 4 * sc16;
        float* dst = inp + (srow + 1) * INP_STRIDE + 4 + 4 * sc16;
        f32x4 c0 = *(const f32x4*)src, c1 = *(const f32x4*)(src + 32 * 64);
        c12_sanitize(c0);
        c12_sanitize(c1);
        *(f32x4*)dst = c0;
        *(f32x4*)(dst + 32 * INP_STRIDE) = c1;
        if constexpr (C2H) {
            const unsigned int mx = f16x2_rowmax(f16x2_absmax8(c0, c1));
            if ((lane & 15) == 0) atomicMax((unsigned int*)(smem + OFF_XMAX), mx);
        }
    }
    __syncthreads();
    // C2H: the scale of this cell's V (a wave-uniform power of two, kept in scalar registers) and what undoes it and the weights'
    float vscale = 1.0f, vunscale = 1.0f, xscale = 1.0f, xunscale = 1.0f;      // xscale: C1H, puts max|x| of the crop into [2^14, 2^15)
    auto set_scale = [&]() {
        const float xm = __builtin_bit_cast(float, *(const unsigned int*)(smem + OFF_XMAX));
        if constexpr (C1H) {
            int Ex = (int)((__builtin_bit_cast(unsigned int, xm) >> 23) & 0xffu);
            Ex = Ex < 40 ? 40 : (Ex > 254 ? 254 : Ex);
            Ex = __builtin_amdgcn_readfirstlane(Ex);
            xscale = __builtin_bit_cast(float, (unsigned int)(268 - Ex) << 23);
            xunscale = __builtin_bit_cast(float, (unsigned int)(Ex - 14) << 23) * inv_sw1;
        }
        const float vb = 100.0f * fmaf(p1a, xm, p1b);                       // >= every |V| of the cell
        int E = (int)((__builtin_bit_cast(unsigned int, vb) >> 23) & 0xffu);
        E = E < 40 ? 40 : (E > 254 ? 254 : E);
        E = __builtin_amdgcn_readfirstlane(E);
        vscale = __builtin_bit_cast(float, (unsigned int)(268 - E) << 23);      // puts vb into [2^14, 2^15)
        vunscale = __builtin_bit_cast(float, (unsigned int)(E - 14) << 23) * inv_sw;
    };
    if constexpr (C2H) set_scale();
    // C1H: conv1 reads the crop as one-dword records [fp16(S_x x) | fp16(S_x x - hi)].  The crop is staged as fp32 (its maximum fixes
    // S_x), then every thread turns the eight values it staged itself into records IN PLACE (same four bytes, no other thread's
    // data: no barrier of its own); the zero halo is the zero record.  INP then holds the whole cell's records until the next crop
    // replaces it, so P1 addresses them by crop row and nothing has to be rebuilt per group.
    auto records_in_place = [&](int t) {
        float* p0 = inp + ((t >> 4) + 1) * INP_STRIDE + 4 + 4 * (t & 15);
        float* p1 = p0 + 32 * INP_STRIDE;
        const f32x4 a = *(const f32x4*)p0, b = *(const f32x4*)p1;
        const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
        *(u32x4*)p0 = u32x4{f16x2_split_word_scaled(a0, xscale), f16x2_split_word_scaled(a1, xscale), f16x2_split_word_scaled(a2, xscale),
                            f16x2_split_word_scaled(a3, xscale)};
        *(u32x4*)p1 = u32x4{f16x2_split_word_scaled(b0, xscale), f16x2_split_word_scaled(b1, xscale), f16x2_split_word_scaled(b2, xscale),
                            f16x2_split_word_scaled(b3, xscale)};
    };
    if constexpr (C1H) {
        records_in_place(tid);
        __syncthreads();
    }

    if constexpr (DIAG) dt = cycle_stamp();
    for (long ci = 0; ci < my_cells; ++ci) {
        const long cell = blockIdx.x + ci * gridDim.x;
        const bool has_next = ci + 1 < my_cells;
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
            // per-lane offsets are recomputed from a laundered copy of the thread id in every group: hoisted out of the loop
            // they would be ~15 long-lived VGPRs next to the 144 of U, and the kernel would spill
            int t2 = tid;
            asm volatile("" : "+v"(t2));
            const int l2 = t2 & 63, li2 = l2 & 15, kq2 = l2 >> 4;
            if constexpr (C2H) {
                if (g == 1 && t2 == 0) *(unsigned int*)(smem + OFF_XMAX) = 0;   // last read (set_scale) several barriers ago, next atomics in g = 3
            }
            // ================= P1: the group's new p1 rows (ring positions q; p1 row y = q - 1; q = 0, 33: zero rows)
            f32x4 stg0 = {0.0f, 0.0f, 0.0f, 0.0f}, stg1 = stg0;
            if (g == 3 && has_next) {   // next cell's crop: in flight during this phase, written to LDS in P2
                const float* src = x + (size_t)(cell + gridDim.x) * 4096 + (t2 >> 4) * 64 + 4 * (t2 & 15);
                stg0 = *(const f32x4*)src;
                stg1 = *(const f32x4*)(src + 32 * 64);
            }
            if constexpr (C1H) {
                // conv1 as a two-term fp16 split.  A pixel's record is ONE dword [hi | lo]; a lane's K = 8 slots are the records at
                // offsets {0, 1, 72, 73} (two columns x two rows) from a per-kq base {0, 2, 144, 146} of its pixel's window: kq 0 gets
                // taps (0,0) (0,1) (1,0) (1,1), kq 1 (0,2) (1,2), kq 2 (2,0) (2,1), kq 3 (2,2); the other slots read neighbouring
                // records (finite) against zero weights.  Two MFMAs: B = [w_hi, 0] per tap gives hi w_hi, B = [w_lo, w_hi] gives
                // hi w_lo + lo w_hi -- all nine taps in one K = 32 instruction, no separate ninth tap.
                const int kb = (kq2 & 1) * 2 + (kq2 >> 1) * (2 * INP_STRIDE);
                const int offR = (kb + 16 * xt + li2 + 3) * 4;
                const f16x8 Bh = *(const f16x8*)(smem + OFF_B1X + ((s1 * 2 + 0) * 64 + l2) * 16);
                const f16x8 Bx = *(const f16x8*)(smem + OFF_B1X + ((s1 * 2 + 1) * 64 + l2) * 16);
                const int c1 = s1 * 16 + li2;
                f32x4 e1v = *(const f32x4*)(smem + OFF_EP1 + c1 * 16);                 // bias, bn scale, bn shift, sign
                e1v[1] *= vscale; e1v[2] *= vscale;                                     // the ring holds S p1
                e1v[3] *= xunscale;                                                     // the sums carry S_x S_w1
                const int pwoff = (8 * xt + 2 * kq2 + 1) * 32 + c1;
                auto frag = [&](int inp_row) -> f16x8 {
                    const unsigned int* b = (const unsigned int*)(smem + OFF_INP + inp_row * (INP_STRIDE * 4) + offR);
                    return __builtin_bit_cast(f16x8, u32x4{b[0], b[1], b[INP_STRIDE], b[INP_STRIDE + 1]});
                };
                auto conv_row = [&](const f16x8& a) -> f32x4 {
                    f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, Bx, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
                    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, Bh, acc, 0, 0, 0);
                };
                auto p1_rows4 = [&](int qb, bool last_is_zero_row) {
                    f16x8 a0[4], a1[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int q = (i == 3 && last_is_zero_row) ? qb + 2 : qb + i;        // a valid row; its result is discarded
                        a0[i] = frag(2 * (q - 1));
                        a1[i] = frag(2 * (q - 1) + 1);
                    }
                    f32x4 acc0[4], acc1[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { acc0[i] = conv_row(a0[i]); acc1[i] = conv_row(a1[i]); }
                    mfma_result_fence(acc0, acc1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float* const row = ring + ((qb + i) % RING_SLOTS) * RING_ROWF + pwoff;
                        float v0 = pool_post(acc0[i][0], acc0[i][1], acc1[i][0], acc1[i][1], e1v[3], e1v[0], e1v[1], e1v[2]);
                        float v1 = pool_post(acc0[i][2], acc0[i][3], acc1[i][2], acc1[i][3], e1v[3], e1v[0], e1v[1], e1v[2]);
                        if (i == 3 && last_is_zero_row) v0 = v1 = 0.0f;                     // q = 33: the bottom zero row
                        row[0] = v0;
                        row[32] = v1;
                    }
                };
                if (g == 0) {
                    if (t2 < 256) *(f32x4*)(ring + 32 + 4 * t2) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};      // q = 0 -> slot 0
                    f32x4 acc0 = conv_row(frag(0)), acc1 = conv_row(frag(1));                     // q = 1: conv rows 0, 1
                    mfma_result_fence(acc0, acc1);
                    float* const row = ring + RING_ROWF + pwoff;
                    row[0] = pool_post(acc0[0], acc0[1], acc1[0], acc1[1], e1v[3], e1v[0], e1v[1], e1v[2]);
                    row[32] = pool_post(acc0[2], acc0[3], acc1[2], acc1[3], e1v[3], e1v[0], e1v[1], e1v[2]);
                }
                p1_rows4(8 * g + 2, false);
                p1_rows4(8 * g + 6, g == 3);
            } else
            {
                // conv1 A operand: lane (pixel li, k = 4 s + kq) reads tap (k / 3, k % 3); the padded taps k >= 9 carry zero
                // weights and read tap 0 (finite whenever the true taps are)
                int toff[3];
                float B1[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int k = 4 * s + kq2, kk = k < 9 ? k : 0;
                    toff[s] = (kk / 3) * INP_STRIDE + (kk % 3) + 16 * xt + li2 + 3;
                    B1[s] = *(const float*)(smem + OFF_B1 + ((s1 * 3 + s) * 64 + l2) * 4);
                }
                const int c1 = s1 * 16 + li2;
                f32x4 e1v = *(const f32x4*)(smem + OFF_EP1 + c1 * 16);                 // bias, bn scale, bn shift, sign
                if constexpr (C2H) { e1v[1] *= vscale; e1v[2] *= vscale; }
                // pooled outputs of this lane: ring columns 8 xt + 2 kq + {0,1} (+1: halo), channel c1
                const int pwoff = (8 * xt + 2 * kq2 + 1) * 32 + c1;
                // One row: conv rows 2y, 2y+1 (y = q - 1) of this wave's 16 pixels x 16 channels -> two pooled values per lane.
                // Rows are processed four at a time in three explicit stages -- all 24 LDS reads, then the 24 MFMAs as eight
                // interleaved accumulation chains, then the four epilogues -- because left to itself the compiler serialises
                // each row (read -> wait -> 6 MFMAs -> s_nop -> pool -> write: ~440 cycles per row and wave, 8 rows per group).
                auto p1_rows4 = [&](int qb, bool last_is_zero_row) {
                    float a0[4][3], a1[4][3];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int q = (i == 3 && last_is_zero_row) ? qb + 2 : qb + i;        // a valid row; its result is discarded
                        const float* a = inp + (2 * (q - 1)) * INP_STRIDE;
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            a0[i][s] = a[toff[s]];
                            a1[i][s] = a[toff[s] + INP_STRIDE];
                        }
                    }
                    f32x4 acc0[4], acc1[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc0[i] = acc1[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int s = 0; s < 3; ++s)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i][s], B1[s], acc0[i], 0, 0, 0);
                            acc1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][s], B1[s], acc1[i], 0, 0, 0);
                        }
                    mfma_result_fence(acc0, acc1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float* const row = ring + ((qb + i) % RING_SLOTS) * RING_ROWF + pwoff;
                        float v0 = pool_post(acc0[i][0], acc0[i][1], acc1[i][0], acc1[i][1], e1v[3], e1v[0], e1v[1], e1v[2]);
                        float v1 = pool_post(acc0[i][2], acc0[i][3], acc1[i][2], acc1[i][3], e1v[3], e1v[0], e1v[1], e1v[2]);
                        if (i == 3 && last_is_zero_row) v0 = v1 = 0.0f;                     // q = 33: the bottom zero row
                        row[0] = v0;
                        row[32] = v1;
                    }
                };
                // rows q = 8 g + 2 .. 8 g + 9 of every group (g = 3: q = 33 is the bottom zero row), plus q = 0 (zero) and q = 1
                // for g = 0
                if (g == 0) {
                    if (t2 < 256) *(f32x4*)(ring + 32 + 4 * t2) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};      // q = 0 -> slot 0
                    const float* a = inp;                                                          // q = 1: conv rows 0, 1
                    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[toff[s]], B1[s], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[toff[s] + INP_STRIDE], B1[s], acc1, 0, 0, 0);
                    }
                    mfma_result_fence(acc0, acc1);
                    float* const row = ring + RING_ROWF + pwoff;
                    row[0] = pool_post(acc0[0], acc0[1], acc1[0], acc1[1], e1v[3], e1v[0], e1v[1], e1v[2]);
                    row[32] = pool_post(acc0[2], acc0[3], acc1[2], acc1[3], e1v[3], e1v[0], e1v[1], e1v[2]);
                }
                p1_rows4(8 * g + 2, false);
                p1_rows4(8 * g + 6, g == 3);
            }
            C12_STAMP(0)
            __syncthreads();
            C12_STAMP(1)

            // ================= P2: V = B^T d B
            if constexpr (C2H) {
                // A thread owns a channel PAIR of one tile and HALF of the transform rows: wave w = (row half h = w & 1, tile columns
                // 2 (w >> 1) + {0, 1}), lane = (pair p, tile row, tile column).  The pair is one ds_read_b64 and one packed-fp32
                // operation per step of the transform (v_pk_fma_f32 / v_pk_add_f32: both channels at once), its hi and lo dwords
                // [hi c | hi c+1], [lo c | lo c+1] are one v_cvt_pk_f16_f32 + two v_fma_mix with no lane exchange, and the rows of B^T d
                // split 3 | 3 without redundant work (outputs 0-2 need input rows 0-4, outputs 3-5 rows 1-5): 72 packed + 54 split
                // instructions per thread where the (tile, channel) form spent 144 + 144.
                // LDS: a ds_read_b64 is served 32 lanes at a time over 64 banks: lanes 0-15 read one tile's 16 pairs (32 consecutive
                // dwords), lanes 16-31 the tile four ring rows below -- 4 RING_ROWF = 32 banks on.  The ds_write_b32 groups (32
                // lanes, 32 banks) hold the same two tiles: their slots differ by the XOR's bit 2, so the 32 dwords are distinct.
                const int h = w & 1, p = l2 & 15, trow = (l2 >> 4) & 1, tx = 2 * (w >> 1) + (l2 >> 5), tile = 8 * trow + tx;
                // ring rows 4 trow + h + m, m = 0..4 -> slots (8 g + row) mod 10 (one conditional subtraction: the sum stays below 20)
                const int rbase = (8 * g) % RING_SLOTS + 4 * trow + h;
                const float* const rcol = ring + (4 * tx) * 32 + 2 * p;
                // the two halves are two instantiations of the body (h is wave-uniform: one scalar branch per phase)
                auto p2_body = [&](auto lo_c) {
                    constexpr bool LO = decltype(lo_c)::value;
                    f32x2 t[3][6];
                    {
                        const float* rrow[5];
    #pragma unroll
                        for (int m = 0; m < 5; ++m) {
                            const unsigned int sm = (unsigned int)(rbase + m);
                            const unsigned int slot = min(sm, sm - (unsigned int)RING_SLOTS);       // unsigned wrap: sm - 10 is huge below 10
                            rrow[m] = rcol + slot * RING_ROWF;
                        }
                        // reads column by column (a column's five rows feed its B^T d at once, so the transform starts while the later
                        // columns are still in flight); volatile keeps them single ds_read_b64 -- merged into ds_read2_b64 they are
                        // served 16 lanes at a time over 32 banks, at half the rate
                        f32x2 d[6][5];
    #pragma unroll
                        for (int j = 0; j < 6; ++j)
    #pragma unroll
                            for (int m = 0; m < 5; ++m) d[j][m] = lds_read_b64(rrow[m] + j * 32);
                        if (g == 3 && has_next) {   // the crop buffer is dead since the barrier above
                            float* dst = inp + ((t2 >> 4) + 1) * INP_STRIDE + 4 + 4 * (t2 & 15);
                            c12_sanitize(stg0);
                            c12_sanitize(stg1);
                            *(f32x4*)dst = stg0;
                            *(f32x4*)(dst + 32 * INP_STRIDE) = stg1;
                            const unsigned int mx = f16x2_rowmax(f16x2_absmax8(stg0, stg1));
                            if ((l2 & 15) == 0) atomicMax((unsigned int*)(smem + OFF_XMAX), mx);
                        }
                        // rows first (B^T d): this thread's three rows of every column
    #pragma unroll
                        for (int j = 0; j < 6; ++j) {
                            f32x2 o[3];
                            bt6_half<LO>(d[j], o);
    #pragma unroll
                            for (int rr = 0; rr < 3; ++rr) t[rr][j] = o[rr];
                        }
                    }
                    // then columns ((B^T d) B), split, store: [point][tile][slot ^ ((tile >> 1) & 7)][16 B], slots 0-3 = hi of channels
                    // 8 kq .., 4-7 = lo: the pair's hi dword goes to slot p >> 2, its lo dword to slot 4 + (p >> 2) (the XOR's bit 2)
                    const int sx = (tile >> 1) & 7;
                    char* const vhi = smem + (3 * h) * (6 * 2048) + (tile * 8 + ((p >> 2) ^ sx)) * 16 + (p & 3) * 4;
                    char* const vlo = smem + (3 * h) * (6 * 2048) + (tile * 8 + ((4 + (p >> 2)) ^ sx)) * 16 + (p & 3) * 4;
    #pragma unroll
                    for (int rr = 0; rr < 3; ++rr) {
                        f32x2 o[6];
                        bt6_pair(t[rr], o);
                        // both hi are fp16 of the SAME fp32 value: left to the compiler, the transform's last fma was folded into one of
                        // the conversions (v_fma_mixlo_f16: one rounding of the exact sum) and the residual taken against the wrong hi
                        unsigned int ph[6], pl[6];
                        f16x2_split6_pairs(o, ph, pl);
    #pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            *(unsigned int*)(vhi + (rr * 6 + c) * 2048) = ph[c];
                            *(unsigned int*)(vlo + (rr * 6 + c) * 2048) = pl[c];
                        }
                    }
                };
                if (h == 0) p2_body(std::true_type{});
                else p2_body(std::false_type{});
            } else {
                // thread (tile, channel): scalar LDS reads, conflict-free (a half wave reads 32 consecutive channels)
                const int tile = t2 >> 5, ch = t2 & 31, trow = w >> 2, tx = tile & 7;
                const int roff = (4 * tx) * 32 + ch;                              // first patch column of the tile, this channel
                const int vq = ch >> 4, vkq = (ch >> 2) & 3, vj = ch & 3;
                // V is stored in the A-operand order of P3: [point][q][kq][slot][4 channels], slot = tile rotated by
                // 2 (2 q + (kq >> 1)): the writes of a half wave (one tile, 32 channels) then spread over 16 banks x 2 (free for
                // ds_write_b32) instead of 4 banks x 8, and every 16-lane group of a ds_read_b128 still covers 16 distinct slots
                const int voff = (((vq * 4 + vkq) * 16 + ((tile + 2 * (2 * vq + (vkq >> 1))) & 15)) * 4 + vj) * 4;   // bytes
                float d[6][6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const int slot = (8 * g + 4 * trow + i) % RING_SLOTS;           // wave-uniform
                    const float* r = ring + slot * RING_ROWF + roff;
#pragma unroll
                    for (int j = 0; j < 6; ++j) d[i][j] = r[j * 32];
                }
                if (g == 3 && has_next) {   // the crop buffer is dead since the barrier above
                    float* dst = inp + ((t2 >> 4) + 1) * INP_STRIDE + 4 + 4 * (t2 & 15);
                    c12_sanitize(stg0);
                    c12_sanitize(stg1);
                    *(f32x4*)dst = stg0;
                    *(f32x4*)(dst + 32 * INP_STRIDE) = stg1;
                }
                // rows first (B^T d), then columns ((B^T d) B): V[r][c]
                float t[6][6];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    float col[6], o[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) col[i] = d[i][j];
                    bt6(col, o);
#pragma unroll
                    for (int i = 0; i < 6; ++i) t[i][j] = o[i];
                }
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    float o[6];
                    bt6(t[r], o);
#pragma unroll
                    for (int c = 0; c < 6; ++c) *(float*)(smem + (r * 6 + c) * 2048 + voff) = o[c];
                }
            }
            C12_STAMP(2)
            __syncthreads();
            C12_STAMP(3)

            // ================= P3: M = V U on the matrix pipe, row fold in registers
            f32x4 own[3][2];
            {
                // A operand slots of lane (tile li, channel quad kq) for q = 0, 1
                const int aoff0 = ((0 * 4 + kq2) * 16 + ((li2 + 2 * (0 + (kq2 >> 1))) & 15)) * 16;
                const int aoff1 = ((1 * 4 + kq2) * 16 + ((li2 + 2 * (2 + (kq2 >> 1))) & 15)) * 16;
                const int e1slot = (8 * g + w) % RING_SLOTS;                        // a consumed ring slot: this wave's exchange area
                char* const e1 = (char*)(ring + e1slot * RING_ROWF + 32) + l2 * 16;
                char* const e2 = smem + OFF_E2 + w * 2048 + l2 * 16;
                // three rows of one column: 6 LDS reads, then 24 MFMAs as three interleaved accumulation chains (an MFMA of a
                // chain issues 3 x 32 cycles after its predecessor, past the matrix pipe's result latency)
                // C2H: lane (tile li, kq): slots kq (hi) and 4 + kq (lo) of its tile, XORed as in P2
                const int hoffh = (li2 * 8 + (kq2 ^ ((li2 >> 1) & 7))) * 16;
                const int hoffl = (li2 * 8 + ((4 + kq2) ^ ((li2 >> 1) & 7))) * 16;
                auto trio = [&](int cc, int r0, f32x4 (&m)[3]) {
                    if constexpr (C2H) {
                        f16x8 ah[3], al[3];
#pragma unroll
                        for (int t = 0; t < 3; ++t) {
                            const int xi = (r0 + t) * 6 + 3 * gcol + cc;
                            ah[t] = *(const f16x8*)(smem + xi * 2048 + hoffh);
                            al[t] = *(const f16x8*)(smem + xi * 2048 + hoffl);
                        }
                        auto Uh = [&](int pt) { return __builtin_bit_cast(f16x8, f32x4{U[pt * 8], U[pt * 8 + 1], U[pt * 8 + 2], U[pt * 8 + 3]}); };
                        auto Ul = [&](int pt) { return __builtin_bit_cast(f16x8, f32x4{U[pt * 8 + 4], U[pt * 8 + 5], U[pt * 8 + 6], U[pt * 8 + 7]}); };
#pragma unroll
                        for (int t = 0; t < 3; ++t) m[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], Ul(cc * 6 + r0 + t), f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
                        for (int t = 0; t < 3; ++t) m[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], Uh(cc * 6 + r0 + t), m[t], 0, 0, 0);
#pragma unroll
                        for (int t = 0; t < 3; ++t) m[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], Uh(cc * 6 + r0 + t), m[t], 0, 0, 0);
                        return;
                    }
                    f32x4 a[3][2];
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const int xi = (r0 + t) * 6 + 3 * gcol + cc;
                        a[t][0] = *(const f32x4*)(smem + xi * 2048 + aoff0);
                        a[t][1] = *(const f32x4*)(smem + xi * 2048 + aoff1);
                        m[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int t = 0; t < 3; ++t)
                                m[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][h][j], U[(cc * 6 + r0 + t) * 8 + 4 * h + j], m[t], 0, 0, 0);
                };
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    // s = A^T m:  s0 = m0 + (m1+m2) + (m3+m4), s1 = (m1-m2) + 2 (m3-m4), s2 = (m1+m2) + 4 (m3+m4),
                    //             s3 = (m1-m2) + 8 (m3-m4) + m5
                    f32x4 ma[3], mb[3];
                    trio(cc, 0, ma);
                    const f32x4 p = ma[1] + ma[2], mq = ma[1] - ma[2];
                    trio(cc, 3, mb);
                    const f32x4 u = mb[0] + mb[1], v = mb[0] - mb[1];
                    const f32x4 s0 = ma[0] + p + u, s1 = mq + 2.0f * v, s2 = p + 4.0f * u, s3 = mq + 8.0f * v + mb[2];
                    // rows (2 gcol, 2 gcol + 1) stay, the other two go to the partner wave.  The asm statements keep the
                    // compiler from turning this wave-uniform branch into 16 v_cndmask per column.
                    f32x4 ta, tb;
                    if (gcol == 0) { asm volatile(""); own[cc][0] = s0; own[cc][1] = s1; ta = s2; tb = s3; }
                    else           { asm volatile(""); own[cc][0] = s2; own[cc][1] = s3; ta = s0; tb = s1; }
                    if (cc < 2) {
                        *(f32x4*)(e1 + (2 * cc) * 1024) = ta;
                        *(f32x4*)(e1 + (2 * cc + 1) * 1024) = tb;
                    } else {
                        *(f32x4*)(e2) = ta;
                        *(f32x4*)(e2 + 1024) = tb;
                    }
                }
            }
            C12_STAMP(4)
            __syncthreads();
            C12_STAMP(5)

            // ================= P4: column fold of this wave's two output rows, epilogue, store.  The group's last barrier stands BEHIND
            // the stores.  Right behind the partner rows' reads it would save the few hundred cycles the waves arrive apart here (-2.7 %
            // measured), but with the fold and the stores running straight into the next group's P1 the kernel stopped being
            // deterministic on gfx950: about one cell in 16,000 got one pooled value per filter of one wave computed as if its ReLU
            // input were 0 (always the wave's last-but-one store, lanes 48-63); 64 idle cycles behind the stores, a wait for them, or
            // this barrier each made it disappear, a late read of the stores' data registers was ruled out with sentinels.  The cause
            // was not found, so the arrangement that passes tools/determinism_stress.py stays.
            {
                const int wp = w ^ 1;
                const int pslot = (8 * g + wp) % RING_SLOTS;
                const char* const e1 = (const char*)(ring + pslot * RING_ROWF + 32) + l2 * 16;
                const char* const e2 = smem + OFF_E2 + wp * 2048 + l2 * 16;
                const int co = sl * 16 + li2;
                f32x4 e2v = *(const f32x4*)(smem + OFF_EP2 + co * 16);                // bias, bn scale, bn shift, sign
                if constexpr (C2H) e2v[3] *= vunscale;                                // the sums carry S S_w: undone in pool_post's fma
                // register r <-> tile 4 kq + r of the group (tile row kq >> 1, tile columns 4 (kq & 1) + r); output rows
                // (2 gcol, 2 gcol + 1) of a tile are pool row gcol: one base address per lane, the rest immediates
                float* const obase = p2 + ((((size_t)cell * 16 + 2 * (2 * g + (kq2 >> 1)) + gcol) * 16 + 8 * (kq2 & 1)) * 64 + co);
                auto finish = [&](auto first_c) {
                    constexpr bool FIRST = decltype(first_c)::value;
                    f32x4 y[2][4];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const f32x4 pa = *(const f32x4*)(e1 + (0 + i) * 1024), pb = *(const f32x4*)(e1 + (2 + i) * 1024),
                                    pc = *(const f32x4*)(e2 + i * 1024);
                        // this wave's columns are 0..2 (FIRST) or 3..5 of the transform domain
                        const f32x4 s0 = FIRST ? own[0][i] : pa, s1 = FIRST ? own[1][i] : pb, s2 = FIRST ? own[2][i] : pc;
                        const f32x4 s3 = FIRST ? pa : own[0][i], s4 = FIRST ? pb : own[1][i], s5 = FIRST ? pc : own[2][i];
                        const f32x4 p = s1 + s2, mq = s1 - s2, u = s3 + s4, v = s3 - s4;
                        y[i][0] = s0 + p + u;
                        y[i][1] = mq + 2.0f * v;
                        y[i][2] = p + 4.0f * u;
                        y[i][3] = mq + 8.0f * v + s5;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        obase[r * 128] = pool_post(y[0][0][r], y[0][1][r], y[1][0][r], y[1][1][r], e2v[3], e2v[0], e2v[1], e2v[2]);
                        obase[r * 128 + 64] = pool_post(y[0][2][r], y[0][3][r], y[1][2][r], y[1][3][r], e2v[3], e2v[0], e2v[1], e2v[2]);
                    }
                };
                if (gcol == 0) finish(std::true_type{});
                else finish(std::false_type{});
                if constexpr (C2H) {
                    if (g == 3 && has_next) set_scale();     // the next crop's maximum is complete since the barrier after P2 (this group's sums are out)
                }
                if constexpr (C1H) {
                    if (g == 3 && has_next) records_in_place(t2);     // the next cell's crop (this thread's own eight values, staged in P2)
                }
            }
            C12_STAMP(6)
            __syncthreads();   // the exchange area inside the ring is consumed before the next P1 refills those slots
            C12_STAMP(7)
        }
    }
    if constexpr (DIAG) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) diag[((size_t)blockIdx.x * 8 + w) * 8 + k] = dg[k];
        }
    }
}

}  // namespace

// U = G g G^T of F(4x4,3x3) per (cin, cout), evaluated in double and rounded once.
// ufrag[wave w = 2 sl + gcol][(cc * 6 + r) * 8 + 4 q + j][lane] = U[row r][col 3 gcol + cc][ci = 16 q + 4 kq + j][co = 16 sl + li]
size_t pack_conv12_fragments(const float* hwio /* [3][3][32][64] */, const float* bn_scale /* [64] */, float* dst)
{
    const size_t total = (size_t)8 * 144 * 64;
    if (!dst) return total;
    static const double G[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    for (int w = 0; w < 8; ++w) {
        const int gcol = w & 1, sl = w >> 1;
        for (int cc = 0; cc < 3; ++cc)
            for (int r = 0; r < 6; ++r)
                for (int kk = 0; kk < 8; ++kk)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int li = lane & 15, kq = lane >> 4, q = kk >> 2, j = kk & 3;
                        const int ci = 16 * q + 4 * kq + j, co = 16 * sl + li, c = 3 * gcol + cc;
                        double u = 0.0;
                        for (int a = 0; a < 3; ++a)
                            for (int b = 0; b < 3; ++b)
                                u += G[r][a] * (double)hwio[((size_t)(a * 3 + b) * 32 + ci) * 64 + co] * G[c][b];
                        if (bn_scale[co] < 0.0f) u = -u;      // the kernel pools -z for these filters (pool_post)
                        dst[((size_t)w * 144 + (cc * 6 + r) * 8 + kk) * 64 + lane] = (float)u;
                    }
    }
    return total;
}

// The same U for the fp16 form of P3 (C2H): two fp16 planes of S_w U, S_w the power of two that puts max|U| into [2^14, 2^15).
// dst[wave w][(cc * 6 + r) * 8 + plane * 4 + d][lane] = the dword {ci = 8 kq + 2 d (low half), ci + 1 (high half)} of that plane of
// U[row r][col 3 gcol + cc][ci][co = 16 sl + li]; *inv_sw = 1 / S_w.  Returns 32-bit words.
size_t pack_conv12_fragments_h2(const float* hwio /* [3][3][32][64] */, const float* bn_scale /* [64] */, unsigned int* dst, float* inv_sw)
{
    const size_t total = (size_t)8 * 144 * 64;
    if (!dst) return total;
    static const double G[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    std::vector<float> U((size_t)36 * 32 * 64);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c)
            for (int ci = 0; ci < 32; ++ci)
                for (int co = 0; co < 64; ++co) {
                    double u = 0.0;
                    for (int a = 0; a < 3; ++a)
                        for (int b = 0; b < 3; ++b) u += G[r][a] * (double)hwio[((size_t)(a * 3 + b) * 32 + ci) * 64 + co] * G[c][b];
                    if (bn_scale[co] < 0.0f) u = -u;          // the kernel pools -z for these filters (pool_post)
                    U[((size_t)(r * 6 + c) * 32 + ci) * 64 + co] = (float)u;
                }
    const float S = f16x2_weight_scale(U.data(), U.size());
    if (inv_sw) *inv_sw = 1.0f / S;
    for (int w = 0; w < 8; ++w) {
        const int gcol = w & 1, sl = w >> 1;
        for (int cc = 0; cc < 3; ++cc)
            for (int r = 0; r < 6; ++r)
                for (int pl = 0; pl < 2; ++pl)
                    for (int d = 0; d < 4; ++d)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int li = lane & 15, kq = lane >> 4, co = 16 * sl + li, c = 3 * gcol + cc;
                            uint16_t h[2][2];
                            for (int e = 0; e < 2; ++e)
                                f16x2_split(U[((size_t)(r * 6 + c) * 32 + 8 * kq + 2 * d + e) * 64 + co], S, h[e][0], h[e][1]);
                            dst[((size_t)w * 144 + (cc * 6 + r) * 8 + pl * 4 + d) * 64 + lane] = (unsigned int)h[0][pl] | ((unsigned int)h[1][pl] << 16);
                        }
    }
    return total;
}

// max|p1| <= a1 max|x| + b1 for every crop: |p1_c| = |s_c relu(w_c . x + b_c) + t_c| <= |s_c| (||w_c||_1 max|x| + max(b_c, 0)) + |t_c|
void pack_conv12_p1_bound(const float* hwio /* [3][3][1][32] */, const float* ep1 /* [3][32]: bias, bn scale, bn shift */, float* a1, float* b1)
{
    float a = 0.0f, b = 0.0f;
    for (int co = 0; co < 32; ++co) {
        float l1 = 0.0f;
        for (int t = 0; t < 9; ++t) l1 += fabsf(hwio[(size_t)t * 32 + co]);
        const float sc = fabsf(ep1[32 + co]);
        a = fmaxf(a, sc * l1);
        b = fmaxf(b, sc * fmaxf(ep1[co], 0.0f) + fabsf(ep1[64 + co]));
    }
    *a1 = a * 1.0001f;       // the sums above are rounded: keep the bound a bound
    *b1 = b * 1.0001f + 1e-30f;
}

// conv1's B fragments for the fused kernel: pack_conv_fragments(cin = 1) layout [slice][K step][lane] with the kernels of
// the filters whose BN scale is negative negated (pool_post).
size_t pack_conv12_conv1_fragments(const float* hwio /* [3][3][1][32] */, const float* bn_scale /* [32] */, float* dst)
{
    const size_t total = (size_t)2 * 3 * 64;
    if (!dst) return total;
    for (int nsl = 0; nsl < 2; ++nsl)
        for (int s = 0; s < 3; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int li = lane & 15, kq = lane >> 4, k = 4 * s + kq, co = nsl * 16 + li;
                float v = k < 9 ? hwio[(size_t)k * 32 + co] : 0.0f;
                if (bn_scale[co] < 0.0f) v = -v;
                dst[((size_t)nsl * 3 + s) * 64 + lane] = v;
            }
    return total;
}

// conv1 for the fp16 form of P1 (C1H): per (slice, MFMA m, lane (li, kq)) eight fp16 = the B slots (pair p, plane) of the lane's four
// record positions {0, 1, 72, 73} from its base {0, 2, 144, 146}[kq]: the taps of conv12_fused_kernel's comment, zero elsewhere.
// m = 0: [w_hi, 0] per tap, m = 1: [w_lo, w_hi]; w scaled by S_w1 (a power of two), negated for filters with a negative BN scale.
size_t pack_conv12_conv1_h2(const float* hwio /* [3][3][1][32] */, const float* bn_scale /* [32] */, unsigned int* dst, float* inv_sw1)
{
    const size_t total = (size_t)(2 * 2 * 64 * 16) / 4;
    if (!dst) return total;
    const float S = f16x2_weight_scale(hwio, 9 * 32);
    if (inv_sw1) *inv_sw1 = 1.0f / S;
    unsigned short* d16 = (unsigned short*)dst;
    for (int nsl = 0; nsl < 2; ++nsl)
        for (int m = 0; m < 2; ++m)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int li = lane & 15, kq = lane >> 4, p = j >> 1, plane = j & 1, co = nsl * 16 + li;
                    const int dy = (kq >> 1) * 2 + (p >> 1), dx = (kq & 1) * 2 + (p & 1);       // window position of slot pair p
                    unsigned short v = 0;
                    if (dy < 3 && dx < 3) {
                        float w = hwio[(size_t)(dy * 3 + dx) * 32 + co];
                        if (bn_scale[co] < 0.0f) w = -w;
                        uint16_t hi, lo;
                        f16x2_split(w, S, hi, lo);
                        v = m == 0 ? (plane == 0 ? hi : 0) : (plane == 0 ? lo : hi);
                    }
                    d16[(((size_t)nsl * 2 + m) * 64 + lane) * 8 + j] = v;
                }
    return total;
}

StampTable g_c12_stamps = {64};       // DIAG builds: 8 waves x 8 phases per workgroup

hipError_t launch_conv12_fused(const float* x, const float* w1frag, const float* ep1, const float* ufrag, const float* ep2, float* p2,
                               int64_t n_cells, hipStream_t stream, const unsigned int* ufrag_h2, float p1a, float p1b,
                               float inv_sw, const unsigned int* w1h2, float inv_sw1)
{
    static const bool diag = getenv("CS_C12_DIAG") != nullptr;       // tools/c12_diag.py: the stamped build, never for results
    if (n_cells <= 0) return hipSuccess;
    if ((w1h2 == nullptr) != (ufrag_h2 == nullptr)) return hipErrorInvalidValue;
    // one workgroup per CU (LDS-bound), persistent over cells
    auto go = [&](auto DIAG, auto H, const float* uf, const unsigned int* w1, float isw1) -> hipError_t {
        constexpr bool D = decltype(DIAG)::value;
        KernelSetup ks;
        const hipError_t e = kernel_setup<conv12_fused_kernel<D, decltype(H)::value>>(NTHR, LDS_BYTES, ks, D ? &g_c12_stamps : nullptr);
        if (e != hipSuccess) return e;
        const unsigned grid = (unsigned)(n_cells < ks.cus ? n_cells : ks.cus);
        hipLaunchKernelGGL((conv12_fused_kernel<D, decltype(H)::value>), dim3(grid), dim3(NTHR), LDS_BYTES, stream, x, w1frag, ep1, uf, ep2,
                           p2, (long)n_cells, D ? g_c12_stamps.begin(ks, grid) : nullptr, w1, p1a, p1b, inv_sw, isw1);
        return hipGetLastError();
    };
    const std::false_type F;
    const std::true_type T;
    if (!w1h2) return !diag ? go(F, F, ufrag, nullptr, 1.0f) : go(T, F, ufrag, nullptr, 1.0f);      // CS_PRECISION_FP32_EXACT
    // CS_PRECISION_SPLIT16: conv1 and conv2 as fp16 splits
    return !diag ? go(F, T, (const float*)ufrag_h2, w1h2, inv_sw1) : go(T, T, (const float*)ufrag_h2, w1h2, inv_sw1);
}

}  // namespace cs

// Diagnostic only (CS_C12_DIAG=1): per-wave phase cycles of the LAST launch of the fused conv1 + conv2 kernel, averaged over waves.
extern "C" int cs_debug_conv12_diag(double out8[8])
{
    return cs::stamp_table_average(cs::g_c12_stamps, 8, out8);
}
