// split16.hpp -- the pieces every two-term fp16 split kernel shares (CS_PRECISION_SPLIT16; conv_wino_up.hip,
// conv67_h2_kernel, has the algebra and the hardware facts).  The protocol: max|x| of a cell or strip (f16x2_absmax*, f16x2_rowmax,
// one LDS atomic max per 16 lanes), the exact power of two that puts it into [2^14, 2^15) (f16x2_scale), x S = hi + lo in fp16
// (the split forms below), three MFMAs per product, the scales undone in the epilogue's fma.  The weights take the same split on
// the host (f16x2_weight_scale, f16x2_split).  What is bound to one kernel's LDS layout stays in that kernel's file.
#pragma once
#include "common.hpp"

#include <cmath>
#include <cstring>

namespace cs {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// max over the 16 lanes of a DPP row of non-negative float bit patterns, which order like the floats (quad swaps, then row
// rotations by 4 and 8)
__device__ __forceinline__ unsigned int f16x2_rowmax(unsigned int m)
{
    unsigned int o;
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true);  m = m > o ? m : o;     // quad_perm [1,0,3,2]
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true);  m = m > o ? m : o;     // quad_perm [2,3,0,1]
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0x124, 0xF, 0xF, true); m = m > o ? m : o;     // row_ror:4
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0x128, 0xF, 0xF, true); m = m > o ? m : o;     // row_ror:8
    return m;
}

// the power of two S that puts 2^BIAS x (a maximum with float bits `mbits`, >= 0) into [2^14, 2^15), and 1 / S.  BIAS = 2 where
// what is split is bounded by 4 x the maximum (conv3's Winograd input transform).  The exponent is clamped so that both stay
// normal floats: a strip whose maximum is below 2^-87 (or zero) is scaled by 2^101 -- its values then sit in fp16's lowest
// binades or vanish, 2^-87 of anything the next layer can see.
template <int BIAS = 0>
__device__ __forceinline__ void f16x2_scale(unsigned int mbits, float& S, float& invS)
{
    int E = (int)((mbits >> 23) & 0xffu) + BIAS;
    E = E < 40 ? 40 : (E > 254 ? 254 : E);
    S = __builtin_bit_cast(float, (unsigned int)(268 - E) << 23);          // 2^(14 - (E - 127))
    invS = __builtin_bit_cast(float, (unsigned int)(E - 14) << 23);
}

// max|.| of four values.  The elements are copied to scalars first: __builtin_bit_cast applied to a vector ELEMENT expression
// reads element 0 whatever the index (clang 19 of ROCm 7.2 -- found as a scale taken from a quarter of the data), and every
// caller goes on to take the maximum's bits.
__device__ __forceinline__ float f16x2_absmax4(const f32x4& v)
{
    const float a = v[0], b = v[1], c = v[2], d = v[3];
    return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d)));
}
// ... into a running maximum kept as float bits
__device__ __forceinline__ void f16x2_absmax4(const f32x4& v, unsigned int& mx)
{
    const unsigned int u = __builtin_bit_cast(unsigned int, f16x2_absmax4(v));
    mx = mx > u ? mx : u;
}
// ... of eight values, as float bits
__device__ __forceinline__ unsigned int f16x2_absmax8(const f32x4& a, const f32x4& b)
{
    return __builtin_bit_cast(unsigned int, fmaxf(f16x2_absmax4(a), f16x2_absmax4(b)));
}

// ---- the split x S = hi + lo, hi = fp16(x S), lo = fp16(x S - hi) ---------------------------------------------------------------
// The convert / subtract form: what the kernels that split while staging under MFMAs use (conv3's strips aside, conv4, conv5,
// conv6 and the run-time-shaped convs).
// hi and the residual x S - hi (exact in fp32), for the callers that convert it where they store it
__device__ __forceinline__ f32x4 f16x2_residual4(const f32x4& x, float S, f16x4& hi)
{
    const f32x4 v = x * S;
    hi = __builtin_convertvector(v, f16x4);
    return v - __builtin_convertvector(hi, f32x4);
}
__device__ __forceinline__ void f16x2_split4(const f32x4& x, float S, f16x4& hi, f16x4& lo)
{
    lo = __builtin_convertvector(f16x2_residual4(x, S, hi), f16x4);
}

// On the mixed-precision fma: hi = fp16(x S) and lo = fp16(x S - hi) are ONE v_fma_mix*_f16 each (the product with a power of
// two and the residual are exact in fp32, so the instruction's single rounding is the conversion's): 2 VALU per value where
// scale / convert / convert back / subtract / convert took 3 to 4.  tools/microbench/fp16_split_probe.hip: bit-identical on
// 16.7 M values x 3 scales, except that fma(-0, S, +0) is +0 where the conversion kept -0.
// The instructions sit in inline asm (there is no builtin), and the hazard recogniser does not look inside: ordinary VALU
// consumers are interlocked by the hardware, but a DPP / MFMA read of a result needs two wait states.  Used where the split
// is a phase of its own (conv12_fused.hip: P2 3.6 k -> 3.0 k cycles per group, the kernel 83.2 -> 79.5 ms per 1 M cells).  In
// the kernels that split while staging under MFMAs (conv3, conv4, conv5, conv6) the same helpers measured SLOWER on the same
// box (conv3 24.2 -> 25.2 ms, conv5 15.6 -> 16.4): opaque asm blocks cost the compiler more scheduling freedom than the saved
// instructions return; those keep the convert / subtract form.
// One value -> the dword [fp16(x S) | fp16(x S - hi)] (conv1's crop records).
__device__ __forceinline__ unsigned int f16x2_split_word_scaled(float x, float S)
{
    unsigned int pk;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0\n\t"
        "v_fma_mixhi_f16 %0, %1, %2, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]"
        : "=&v"(pk) : "v"(x), "v"(S));
    return pk;
}
// Six values, already scaled -> six dwords for conv2's V (conv12_fused.hip, P2): [hi | lo] of each value, exchanged with the
// neighbouring lane (quad_perm [1,0,3,2]) and merged by `sel` (even lane [hi c | hi c+1], odd lane [lo c-1 | lo c]).  The DPP
// read of a VALU result needs two wait states: the six independent chains are interleaved so that five instructions separate them.
__device__ __forceinline__ void f16x2_split6_exchange(const float (&v)[6], unsigned int sel, unsigned int (&out)[6])
{
    unsigned int p0, p1, p2, p3, p4, p5;
    asm("v_cvt_f16_f32 %6, %12\n\t"
        "v_cvt_f16_f32 %7, %13\n\t"
        "v_cvt_f16_f32 %8, %14\n\t"
        "v_cvt_f16_f32 %9, %15\n\t"
        "v_cvt_f16_f32 %10, %16\n\t"
        "v_cvt_f16_f32 %11, %17\n\t"
        "v_fma_mixhi_f16 %6, %6, -1.0, %12 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %7, %7, -1.0, %13 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %8, %8, -1.0, %14 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %9, %9, -1.0, %15 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %10, %10, -1.0, %16 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %11, %11, -1.0, %17 op_sel_hi:[1,0,0]\n\t"
        "v_mov_b32_dpp %0, %6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %1, %7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %2, %8 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %3, %9 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %4, %10 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %5, %11 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_perm_b32 %0, %0, %6, %18\n\t"
        "v_perm_b32 %1, %1, %7, %18\n\t"
        "v_perm_b32 %2, %2, %8, %18\n\t"
        "v_perm_b32 %3, %3, %9, %18\n\t"
        "v_perm_b32 %4, %4, %10, %18\n\t"
        "v_perm_b32 %5, %5, %11, %18"
        : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3]), "=&v"(out[4]), "=&v"(out[5]),
          "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(p4), "=&v"(p5)
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(sel));
}
// Six channel pairs -> [hi c | hi c+1] and [lo c | lo c+1] dwords (hi = fp16(v), lo = fp16(v - hi)): one v_cvt_pk_f16_f32 and two
// v_fma_mix per pair, no lane exchange.  Both hi are fp16 of the fp32 value the transform stored (see conv12_fused.hip, P2's
// comment on the fold).
__device__ __forceinline__ void f16x2_split6_pairs(const f32x2 (&v)[6], unsigned int (&hi)[6], unsigned int (&lo)[6])
{
    float a[6], b[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { a[c] = v[c][0]; b[c] = v[c][1]; }
    asm("v_cvt_pk_f16_f32 %0, %12, %18\n\t"
        "v_cvt_pk_f16_f32 %1, %13, %19\n\t"
        "v_cvt_pk_f16_f32 %2, %14, %20\n\t"
        "v_cvt_pk_f16_f32 %3, %15, %21\n\t"
        "v_cvt_pk_f16_f32 %4, %16, %22\n\t"
        "v_cvt_pk_f16_f32 %5, %17, %23\n\t"
        "v_fma_mixlo_f16 %6, %12, 1.0, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %7, %13, 1.0, -%1 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %8, %14, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %9, %15, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %10, %16, 1.0, -%4 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %11, %17, 1.0, -%5 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %6, %18, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %7, %19, 1.0, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %8, %20, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %9, %21, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %10, %22, 1.0, -%4 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %11, %23, 1.0, -%5 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3]), "=&v"(hi[4]), "=&v"(hi[5]),
          "=&v"(lo[0]), "=&v"(lo[1]), "=&v"(lo[2]), "=&v"(lo[3]), "=&v"(lo[4]), "=&v"(lo[5])
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]),
          "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]));
}
// Eight values x S -> their hi and lo fragments as ONE block of 12 instructions (v_cvt_pk_f16_f32 per pair, then the residuals as
// v_fma_mix{lo,hi}_f16: exact in fp32, one rounding); in conv3 the convert / convert back / subtract / convert form compiled to ~ 20
// and the kernel ran 2.3 % slower (24.7 vs 24.1 ms per 1 M cells; per-VALUE asm blocks had measured slower in round 3, see above).
// -0 residuals come out +0.  The results feed MFMAs directly, which the hazard recogniser cannot see through the asm: the block
// ends with the two wait states a VALU write -> MFMA read needs.
__device__ __forceinline__ void f16x2_split8(const f32x4& lo4, const f32x4& hi4, float S, f16x8& ah, f16x8& al)
{
    const f32x4 a = lo4 * S, b = hi4 * S;
    const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    unsigned int h0, h1, h2, h3, l0, l1, l2, l3;
    asm("v_cvt_pk_f16_f32 %0, %8, %9\n\t"
        "v_cvt_pk_f16_f32 %1, %10, %11\n\t"
        "v_cvt_pk_f16_f32 %2, %12, %13\n\t"
        "v_cvt_pk_f16_f32 %3, %14, %15\n\t"
        "v_fma_mixlo_f16 %4, %8, 1.0, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %5, %10, 1.0, -%1 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %6, %12, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %7, %14, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %4, %9, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %5, %11, 1.0, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %6, %13, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %7, %15, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
        : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
    ah = __builtin_bit_cast(f16x8, u32x4{h0, h1, h2, h3});
    al = __builtin_bit_cast(f16x8, u32x4{l0, l1, l2, l3});
}

// The cycle counter, for the DIAG builds of the kernels: they sum the differences per wave and phase into a StampTable
// (kernel_setup.hpp).  Never used for results or timing.
__device__ __forceinline__ unsigned long long cycle_stamp()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

// ---- host: the weights' side of the split, for every packer ---------------------------------------------------------------------
// the power of two that puts max|w| into [2^14, 2^15)
inline float f16x2_weight_scale(const float* w, size_t n)
{
    float m = 0.0f;
    for (size_t i = 0; i < n; ++i) m = fmaxf(m, fabsf(w[i]));
    if (!(m > 0.0f) || !std::isfinite(m)) return 1.0f;
    int e;
    frexpf(m, &e);                       // m = f 2^e, f in [0.5, 1)
    return ldexpf(1.0f, 15 - e);         // S m = f 2^15 in [2^14, 2^15)
}
// one value -> its two fp16 terms (bit patterns): hi = fp16(S w), lo = fp16(S w - hi)
inline void f16x2_split(float w, float S, uint16_t& hi, uint16_t& lo)
{
    const float v = w * S;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    memcpy(&hi, &h, 2);
    memcpy(&lo, &l, 2);
}

}  // namespace cs
