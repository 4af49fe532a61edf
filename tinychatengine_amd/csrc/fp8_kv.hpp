// fp8_kv.hpp -- the e4m3 KV pages' element format on the device (include/tce_matmul.h, "FP8 pages"): 8 elements at a time, as the kernels hold them.
//
//   dequant(b, e) = e4m3(b) * 2^e as binary16 -- EXACT for every finite byte and e in [-8, 7] (448 * 2^7 = 57344 <= 65504; 2^-9 * 2^-8 = 2^-17, a multiple of 2^-24)
//   quant(x, e)   = e4m3_rne(clamp(float(x) * 2^-e, -448, 448)): the product is exact in fp32, nearest with ties to the even mantissa, saturating (+-inf included),
//                   -0 stays -0 (0x80), NaN becomes the NaN byte 0x7f
// OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; subnormals m * 2^-9; 0x7f / 0xff NaN; no infinities -- gfx950's fp8, not the fnuz encoding.
// Both directions are held to the format's definition for every input by tests/test_gpu_fp8_kv.py (all 65536 binary16 patterns, all 256 bytes, the exponents).
#pragma once
#include "tce_common.hpp"

namespace tce {

constexpr int kFp8ScaleLog2Min = -8, kFp8ScaleLog2Max = 7;

// the host's side, what the paged launchers test and compute before a launch: a pool's exponent is in range; 2^e as a float; log2 of a page size that is a power of
// two in [16, 256], or -1
inline bool fp8_log2_ok(int e) { return e >= kFp8ScaleLog2Min && e <= kFp8ScaleLog2Max; }
inline float host_pow2(int e) {
    const unsigned bits = (unsigned)(127 + e) << 23;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}
inline int page_shift_of(int page_keys) {
    for (int s = 4; s <= 8; ++s)
        if (page_keys == 1 << s) return s;
    return -1;
}

__device__ __forceinline__ float fp8_pow2(int e) { return __builtin_bit_cast(float, (unsigned)(127 + e) << 23); }  // 2^e, -126 <= e <= 127

// 8 bytes -> 8 binary16, three instructions per pair: v_cvt_pk_f32_fp8 widens a pair exactly (NaN bytes to NaN), v_cvt_pkrtz_f16_f32 narrows it to binary16 -- every
// e4m3 value is a NORMAL binary16 number (the smallest is 2^-9), so nothing is rounded --, and v_pk_mul_f16 by 2^e is exact because the product is representable
// (subnormal products included: binary16 denormals are not flushed in this library's kernels, as the binary16 RoPE arithmetic already requires)
__device__ __forceinline__ half8_t fp8_dequant8(const uint2_t w, const float scale) {
    typedef float float2_t __attribute__((ext_vector_type(2)));
    const half_t sh = (half_t)scale;  // 2^-8 .. 2^7: exact
    const half2_t s2 = half2_t{sh, sh};
    half8_t o;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
        const half2_t a = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_pkrtz(lo[0], lo[1])) * s2;
        const half2_t b = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_pkrtz(hi[0], hi[1])) * s2;
        o[4 * d + 0] = a[0];
        o[4 * d + 1] = a[1];
        o[4 * d + 2] = b[0];
        o[4 * d + 3] = b[1];
    }
    return o;
}

// one fp32 (already times 2^-e) -> its byte, from the definition: sign, NaN, saturation; normals (>= 2^-6) by rounding the fp32 mantissa to 3 bits, nearest-even, in
// integer arithmetic (the carry runs into the exponent as it must; 448 stays 0x7e); below 2^-6 the spacing is 2^-9: adding 2^14, whose ulp that is, rounds to
// nearest-even in the adder and leaves the count m = 0 .. 8 in the low bits (8 = 0x08: the smallest normal)
__device__ __forceinline__ unsigned fp8_quant1(const float x) {
    const unsigned sign = (__builtin_bit_cast(unsigned, x) >> 24) & 0x80u;
    if (x != x) return 0x7fu;
    float a = __builtin_fabsf(x);
    a = a < 448.0f ? a : 448.0f;
    unsigned r;
    if (a >= 0.015625f) {
        unsigned bits = __builtin_bit_cast(unsigned, a);
        bits += 0x7FFFFu + ((bits >> 20) & 1u);
        r = (bits >> 20) - (120u << 3);
    } else {
        r = __builtin_bit_cast(unsigned, a + 16384.0f) - __builtin_bit_cast(unsigned, 16384.0f);
    }
    return sign | r;
}

// 8 binary16 -> 8 bytes; inv = 2^-e
__device__ __forceinline__ uint2_t fp8_quant8(const half8_t x, const float inv) {
    uint2_t w;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        unsigned v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) v |= fp8_quant1((float)x[4 * d + i] * inv) << (8 * i);
        w[d] = v;
    }
    return w;
}

}  // namespace tce
