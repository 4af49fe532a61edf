// w4a16_unpack16.hpp -- the int4 -> fp16 unpack of the fp16 GEMV family (w4a16_gemv.hip, w4a16_gemv_stream.hip, w4a16_gemv_ovl.hip,
// w4a16_skinny.hip): one q4_6 word -> MFMA operands holding 16 (q - z), exactly.  Plain functions, usable on the host
// (tests/host/test_w4a16_unpack.cc checks every nibble position, code and zero point against the integers).
//
// A q4_6 word holds the codes q0..q7 of k = 8j..8j+7, q_i in bits [4i, 4i+4).  The word shifted by 4, 0, -4, -8 bits puts the nibble
// pairs (q0,q4), (q1,q5), (q2,q6), (q3,q7) at bits 4..7 of the two 16-bit halves; masked with 0x00F000F0 and OR-ed into the mantissa of
// (1024.0h, 1024.0h) = 0x64006400 (ulp 1) each pair becomes the halves (1024 + 16 q, 1024 + 16 q'): 3 shifts + 4 v_and_or_b32 per word, no
// integer -> float conversion.  One packed subtraction of cz = 1024 + 16 z per two weights leaves 16 (q - z): both terms and the
// difference (a multiple of 16, |.| <= 240) are representable in binary16, so nothing is rounded.  The factor 16 leaves with the
// kernels' final 1/16.  So 7 VALU instructions per 8 weights, and the activations are staged in the matching pair order
// (x0,x4,x1,x5) / (x2,x6,x3,x7) (pair_permute, tce_common.hpp) so that no lane ever shuffles weights.
//
// The nibble mask is an ARGUMENT: the kernels keep it in a VGPR (gfx9 VOP3 reads one scalar / literal operand only: with the mask and the
// magic both literals every v_and_or_b32 splits in two) behind an asm the constant folder cannot see through.
// (History -- the algebraic zero-point removal these forms replaced, and what it cost in accuracy: DESIGN.md 4.2, DESIGN_HISTORY.md.)
#pragma once

#ifndef TCE_HD
#if defined(__HIPCC__)
#define TCE_HD __host__ __device__ inline
#else
#define TCE_HD inline
#endif
#endif

namespace tce {

typedef _Float16 half_t;
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

namespace unpack16 {

constexpr unsigned kMaskHi = 0x00F000F0u;  // bits 4..7 of both halves (the kernels' VGPR copy: v_mov_b32 ..., 0x00F000F0)
constexpr unsigned kMagic = 0x64006400u;   // (1024.0h, 1024.0h)
constexpr unsigned kCz8Bits = 0x64806480u; // (1152.0h, 1152.0h) = 1024 + 16 * 8: zero point 8, what the reference quantizer writes

// ---- cz = 1024 + 16 z ----
// zero point 8: from the packed constant, which the kernels hold in a SCALAR register (the packed subtraction reads it from there, no VGPR is spent)
TCE_HD half4_t cz4_of_8(unsigned cz8_bits) { return __builtin_bit_cast(half4_t, uint2_t{cz8_bits, cz8_bits}); }
// a general z (0..15), as it comes out of the packed zeros word: exact (an integer <= 1264 in fp32, then in binary16)
TCE_HD half_t cz_of(unsigned z) { return (half_t)__builtin_fmaf((float)z, 16.0f, 1024.0f); }
TCE_HD half4_t cz4_of(unsigned z) {
    const half_t c = cz_of(z);
    return half4_t{c, c, c, c};
}
TCE_HD half8_t cz8_splat(half_t c) { return half8_t{c, c, c, c, c, c, c, c}; }  // (the skinny kernels read a row's cz from their LDS table)

// ---- word -> operand: one call, one MFMA operand ----
// the 4x4x4 kernels: two operands per word, 16 (q - z) in the order (q0,q4,q1,q5) and (q2,q6,q3,q7)
TCE_HD half4_t operand_lo(unsigned w, unsigned mask_hi, half4_t cz) {
    const unsigned t0 = ((w << 4) & mask_hi) | kMagic;  // (1024 + 16 q0, 1024 + 16 q4)
    const unsigned t1 = (w & mask_hi) | kMagic;         // (q1, q5)
    return __builtin_bit_cast(half4_t, uint2_t{t0, t1}) - cz;
}
TCE_HD half4_t operand_hi(unsigned w, unsigned mask_hi, half4_t cz) {
    const unsigned t2 = ((w >> 4) & mask_hi) | kMagic;  // (q2, q6)
    const unsigned t3 = ((w >> 8) & mask_hi) | kMagic;  // (q3, q7)
    return __builtin_bit_cast(half4_t, uint2_t{t2, t3}) - cz;
}
// the 16x16x32 (skinny) kernels: the whole word is one operand, (q0,q4,q1,q5,q2,q6,q3,q7)
TCE_HD half8_t operand8(unsigned w, unsigned mask_hi, half8_t cz) {
    const unsigned t0 = ((w << 4) & mask_hi) | kMagic;
    const unsigned t1 = (w & mask_hi) | kMagic;
    const unsigned t2 = ((w >> 4) & mask_hi) | kMagic;
    const unsigned t3 = ((w >> 8) & mask_hi) | kMagic;
    return __builtin_bit_cast(half8_t, uint4_t{t0, t1, t2, t3}) - cz;
}

}  // namespace unpack16
}  // namespace tce
