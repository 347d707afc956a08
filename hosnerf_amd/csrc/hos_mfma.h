// Device helpers of the split-precision MFMA kernels (hos_gemm*.hip, hos_thin.hip, hos_mlpbwd.hip, hos_chain.hip, and the plane
// writers of hos_encode.hip): the ONE definition of how an fp32 value becomes a 16-bit (hi, lo) pair, in which order the three
// split products are issued, and how an accumulator tile is transposed inside a quad.  All __forceinline__; no argument structs.
#pragma once
#include "hos_common.h"

// Split element type: __bf16 (8-bit exponent: safe for gradients of any magnitude, ~2^-17 relative error per
// product) for DGRAD/WGRAD, _Float16 (11-bit mantissa: hi+lo carry 22 bits, ~2^-21 relative error -- fp32 grade)
// for the FORWARD GEMMs whose operands (features, activations, weights) are O(1e-3..1e3) by construction.
template <typename E> struct Vec { typedef E x8 __attribute__((ext_vector_type(8))); typedef E x4 __attribute__((ext_vector_type(4))); };
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- products ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x16 mfma16(const Vec<__bf16>::x8& a, const Vec<__bf16>::x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma16(const Vec<_Float16>::x8& a, const Vec<_Float16>::x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, issued in THIS order, fp32 accumulate (the dropped a_lo*b_lo term is 2^-18 relative
// for bf16)
template <typename E>
__device__ __forceinline__ f32x16 mma3(const typename Vec<E>::x8& ah, const typename Vec<E>::x8& al, const typename Vec<E>::x8& bh,
                                       const typename Vec<E>::x8& bl, f32x16 acc) {
    acc = mfma16(al, bh, acc);
    acc = mfma16(ah, bl, acc);
    acc = mfma16(ah, bh, acc);
    return acc;
}

// ---- the split: hi = (E)hi_src(x), lo = (E)(x - (float)hi), both round-to-nearest-even ----------------------------------------
template <typename E> __device__ __forceinline__ float hi_src(float x) { return x; }
// fp16 hi part saturates at +-65504 instead of overflowing to inf; the residual then lands in lo: the pair is exact to 2^-22 for
// |x| <= 65504 and carries x to 2^-11 relative up to |x| = 131008, beyond that it saturates (HOS_RANGE_LIMIT, hos_gemm_common.h).
// (one v_med3_f32; fminf(fmaxf()) costs a canonicalising v_max in front of it: 16 more VALU per staged tile and thread)
template <> __device__ __forceinline__ float hi_src<_Float16>(float x) { return __builtin_amdgcn_fmed3f(x, -65504.f, 65504.f); }

template <typename E>
__device__ __forceinline__ void split1(float x, E& hi, E& lo) {
    hi = (E)hi_src<E>(x);
    lo = (E)(x - (float)hi);
}
// (all four hi parts, then the four lo parts: written as four split1 calls the staging code of hos_gemm3.hip comes out differently)
template <typename E>
__device__ __forceinline__ void split4(const float4& v, typename Vec<E>::x4& hi, typename Vec<E>::x4& lo) {
    hi[0] = (E)hi_src<E>(v.x); hi[1] = (E)hi_src<E>(v.y); hi[2] = (E)hi_src<E>(v.z); hi[3] = (E)hi_src<E>(v.w);
    lo[0] = (E)(v.x - (float)hi[0]); lo[1] = (E)(v.y - (float)hi[1]);
    lo[2] = (E)(v.z - (float)hi[2]); lo[3] = (E)(v.w - (float)hi[3]);
}

// ---- memory -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// LDS-DMA: 16 bytes per lane from global memory straight to LDS (wave base + lane * 16), no VGPRs
__device__ __forceinline__ void dma16(const void* gsrc, void* ldst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)ldst, 16, 0, 0);
}
// ds_read_b64_tr_b16, the gfx950 LDS transpose read: inside a 16-lane group lane p supplies the address of row (p >> 2), columns
// 4 (p & 3) .. +3, and receives column p of the four rows
__device__ __forceinline__ s16x4 lds_tr(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
// fragment read the compiler does not count (the callers place their own s_waitcnt lgkmcnt)
#define HOS_RD128(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))

// ---- quad transpose ---------------------------------------------------------------------------------------------------------
// Exchange inside a quad of lanes (lane ^ 1, lane ^ 2) as v_mov_b32_dpp quad_perm -- a VALU move -- instead of __shfl_xor, which
// hipcc lowers to ds_bpermute_b32: 16 round trips through the LDS crossbar per 32 x 32 tile in the quad transposes.
__device__ __forceinline__ float quad_xor1(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
}
__device__ __forceinline__ float quad_xor2(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, true));      // quad_perm [2,3,0,1]
}
// 4x4 transpose across the four lanes of a quad (q = lane & 3), two xor-exchange stages.  In: lane q holds one column of four
// accumulator rows (the MFMA C/D layout, registers 4 g .. 4 g + 3) in the float lvalues V0..V3.  Out: (V0..V3) = row q, four
// CONSECUTIVE columns.
// A MACRO, not a function: the compiler simplifies a __forceinline__ function on its own before it inlines it, and every function
// form tried (float& parameters; by value with `q`; by value with the two bits of q tested by the caller) changed the
// instructions or their order in at least one of the kernels that use it.
#define HOS_QUAD_TRANSPOSE4(V0, V1, V2, V3, Q)                                                                     \
    {                                                                                                              \
        const float qt_s0 = ((Q) & 1) ? V0 : V1, qt_s1 = ((Q) & 1) ? V2 : V3;                                      \
        const float qt_r0 = quad_xor1(qt_s0), qt_r1 = quad_xor1(qt_s1);                                            \
        if ((Q) & 1) { V0 = qt_r0; V2 = qt_r1; } else { V1 = qt_r0; V3 = qt_r1; }                                  \
        const float qt_t0 = ((Q) & 2) ? V0 : V2, qt_t1 = ((Q) & 2) ? V1 : V3;                                      \
        const float qt_u0 = quad_xor2(qt_t0), qt_u1 = quad_xor2(qt_t1);                                            \
        if ((Q) & 2) { V0 = qt_u0; V1 = qt_u1; } else { V2 = qt_u0; V3 = qt_u1; }                                  \
    }

// ---- interleaved planes (hos_gemmp.hip) ---------------------------------------------------------------------------------------
// A split matrix [R][ld] (ld % 32 == 0) is ONE 16-bit array [R][ld/32][2][32]: per row and block of 32 columns, 32 hi values then
// the 32 lo values.  Element offset of (row r, column c): the hi part there, the lo part PL_LO further.
constexpr int PL_LO = 32;
__device__ __forceinline__ size_t pl_off(long r, int c, int ld) { return (size_t)r * (2 * ld) + (c >> 5) * 64 + (c & 31); }
