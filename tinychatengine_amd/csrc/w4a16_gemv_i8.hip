// w4a16_gemv_i8.hip -- the decode GEMV (M <= 4) as an EXACT int8 contraction on the matrix pipe, on the pre-packed copy of a linear (q4_mfma words + the
// tile-major fp16 scales / zero points tce_w4a16_prepack writes beside them, w4a16_mfma_layout.hpp).  Round 4; replaces the unpack-to-halves GEMV
// (w4a16_gemv.hip) wherever a packed copy comes with the descriptor.  Same math as gemv_kernel_g128 / g64 (reference kernels/cuda/gemv_cuda.cu:140-194, 68-123):
//     C[m][n] = fp16( sum_g fp32(s[n][g]) * sum_{k in g} (q[n][k] - z[n][g]) * A[m][k] )
// Why another kernel: the fp16 form spends 7 vector instructions per 8 weights on the unpack alone and is issue-bound; measured issue rates
// (profiles/r4/valu_probe.jsonl): v_and_or / v_perm / v_cvt / v_dot8_i32_i4 4.2 cycles per wave instruction, plain VOP2 logic 2.4, an i8 16x16x64 MFMA 16, and
// MFMA time ADDS to VALU time on a SIMD.  Here:
//   * WEIGHTS  a lane's 16 bytes of the packed copy (row n16 of a 16-row tile, 32 codes of one 128-wide k unit) become the A operands of two
//              v_mfma_i32_16x16x64_i8 as signed bytes 16 * (q - 8): one v_bitop3 for the high nibbles, shift + v_bitop3 for the low ones -- 3 instructions per
//              8 weights, no zero-point term for the reference's zero point 8 (other zero points: (8 - z) * sum_k X_k from one more MFMA pair with A = 16).
//   * X        every wave converts the 128 * UW activations IT consumes: x * 2^sh truncated to a 31-bit integer under ONE block exponent per wave and row
//              (sh from the block's largest exponent: every element within 2^19 of the block maximum is represented exactly), split into four balanced
//              base-256 digit planes ((I + 0x808080) ^ 0x808080: 2 instructions), byte-transposed into the B operand image in the wave's OWN LDS region: no
//              workgroup barrier in front of the contraction.  The planes are COLUMNS of B: one MFMA contracts all four at once, products and sums exact.
//   * COLUMNS  M = 1 uses 4 of the 16 output columns per 128-k unit, so four units (four quantization groups) share one accumulator: unit c of a pass presents
//              its planes in columns 4c..4c+3 and zeros elsewhere (the B registers of the other lanes are never written -- or, in the ring of two sets that
//              keeps the plain forms at seven or eight waves per SIMD, read from a block of zeros: section 3).  One v_cvt_f32_i32 + one v_fma_mix
//              (fp16 scale) per output register then serve FOUR groups; M = 2 / 4 rows of A take the columns instead (2 / 1 units per pass).
//   * STREAM   a wave owns ROWS tiles x UW units: every weight byte it will use is requested at once (after the few x / scale bytes: loads retire in order,
//              a wait for x must not be a wait for the weights), 1 KiB of consecutive memory per load instruction, non-temporal.
//   * HEAD     nothing stands between wave entry and those requests: the arguments they need are flat leading parameters that arrive preloaded in SGPRs (I8SegHead
//              below); everything else -- the store's fields, the residual's old values -- is asked for behind them.
//   * K        the waves of a workgroup split K (UW depends on K only: a row's bits do not depend on N, so column shards are bit-identical to the whole);
//              partial rows meet in LDS and are added in wave order.
// Numerics: integer part exact; the roundings are one fp32 fma per (row, group), the plane / group / wave additions in a fixed order, the fp16 store.
// Activations holding inf / NaN: every output of that row is NaN (the reference yields NaN or +-inf there).
#include "tce_common.hpp"
#include "w4a16_kernels.hpp"
#include "w4a16_mfma_layout.hpp"

namespace tce {

namespace {

// ---- the ordinary launch's arguments: FLAT, in the order the wave needs them (decode-head round; profiles/decode_head/).
// A kernel argument struct passed by value cannot be preloaded; scalar and pointer parameters can: with -mllvm -amdgpu-kernarg-preload-count the first 14 dwords below
// arrive in SGPRs with the wave (kernel descriptor: kernarg_preload_length 14 -- the 16 user SGPRs less the kernarg pointer), so x, the scales and all weight requests of a
// single-linear launch issue without ONE scalar-memory round trip (before: header + block_begin words -> wait -> the chosen segment's fields at a computed offset + the
// hidden blockDim word -> wait -> first request).  Hardware or firmware that does not preload enters 256 bytes earlier, through the compiler's compatible prologue: one
// batch of scalar loads and one wait.
//     dword  0- 1  words      linear 0's packed words          8- 9  dscales    linear 0's tile-major scales
//            2     bytes_w    their byte count                10     bytes_s
//            3     U          K / 128                          11     N          linear 0's rows
//            4- 5  A          activations                      12     M
//            6     lda                                         13     geom       waves that split K (the workgroup's width / 64; not read from the hidden
//            7     K                                                             arguments any more) | linears of the launch << 8 | members of a group copy << 16
// Everything else -- what is used BEHIND the weight requests (C, ldc, epilogue flags, zero points), linears 1.. of a grouped launch, gamma, the RNORM / COMB fields -- is the
// tail struct: ordinary scalar loads, issued with the wave's first instructions and waited for where first used (a grouped launch: ONE batch holding every further
// linear's addressing fields, chosen by scalar selects -- at most one wait in front of the weight requests; nothing behind the K reduction's barrier).
struct I8SegHead {  // what the requests need, linears 1.. of a grouped launch (linear 0: the leading parameters)
    const void *words;
    const half_t *dscales;
    int bytes_w, bytes_s, N;
    int block_begin;  // first blockIdx.x of this linear
};
struct I8SegRest {  // what the epilogue (and the general-zero-point forms) need
    half_t *C;               // fp16 [M][ldc]
    const unsigned *dzeros;  // u32 [NT16][NG][2]
    int ldc, epilogue, bytes_z, pad_;
};
struct I8Tail {
    I8SegRest rest[TCE_MAX_GROUP];
    I8SegHead head[TCE_MAX_GROUP - 1];
    // a launch on a GROUP COPY (tce_w4a16_prepack_group: q/k/v, gate+up packed as one row-concatenated linear; geom: one linear, members << 16): the leading parameters
    // address the whole copy exactly like a single linear's, rest[0] carries its zero points; what differs per member -- rest[i].C / ldc / epilogue -- is chosen by the
    // member's first 16-row tile, behind the weight requests
    int mtile[TCE_MAX_GROUP];
    const float *gamma;  // non-null: the activation is the UN-normalised hidden state; the conversion stages RMSNorm(A) * gamma (generalT5LayerNorm arithmetic; M = 1)
    float eps;
    // RNORM (tce_w4a16_forward_residual_rmsnorm): the residual epilogue also produces the NEXT RMSNorm of the updated row -- out_gamma fp32 [N], xn_out fp16 [N],
    // ws = float slots[2048] (the row's piece sums) + unsigned counter at word 2048 (zero between launches)
    float out_eps;
    const float *out_gamma;
    half_t *xn_out;
    float *ws;
    // COMB (tce_w4a16_forward_deferred_attention, round 5): the activation row is the output of a deferred attention step -- per query head `comb_slots` partial
    // states (M, L, -, -, O[128]; `comb_stride` floats each) of which the first ceil((position + 1) / comb_chunk) are live; the prologue combines them exactly as the
    // attention kernel's own last workgroup would (attention_fast.hip) and rounds to binary16 -- the same row, bit for bit -- while the weights are in flight
    const float *comb_part;
    const int *comb_pos_dev;
    int comb_pos, comb_slots, comb_chunk, comb_stride, comb_heads;
    unsigned long long *dbg;  // the lab build's stamped form only (null otherwise): [workgroup][8] clock readings of wave 0, see I8Stamps
};

// The time budget of a launch (lab build, debug mode 7704; scripts/decode_head_timeline.py): wave 0 of every workgroup reads the 100 MHz clock (s_memrealtime) at
// [0] wave entry, [1] the last weight request issued, [2] x converted and staged (its loads have arrived), [3] the contraction done (the last weight has arrived and
// been used), [4] the output stored; [5] / [6]: the shader clock (s_memtime) at [0] / [1], for the head in cycles.  The readings stay in scalar registers until the end.
struct I8Stamps {
    unsigned long long t[7];
};

// one linear as the body uses it (the mixed launch passes it in this form)
struct I8Seg {
    const void *words;       // u32 [NT16][U][64][4]
    const half_t *dscales;   // fp16 [NT16][NG][16]
    const unsigned *dzeros;  // u32 [NT16][NG][2]
    half_t *C;               // fp16 [M][ldc]
    int N, ldc, epilogue;
    int bytes_w, bytes_s, bytes_z;
    int block_begin;  // first blockIdx.x of this linear
};

// ---- the MIXED launch (round 6): up to kI8MixMax decode linears that share NOTHING -- own activation, own K -- as one launch.
// What it is for: with the linears sharded over P ranks and the activations replicated (north_star's one-gather-per-block form) a rank's five linears of a block read
// independent inputs; issued one by one they are 4 launches of 2-6 MB at P = 8, each paying the same ~2.5 us of boundary and ramp as a 60 MB launch.
// Geometry: the workgroup has as many waves as the LONGEST K needs (K / 1024, e.g. 14 for down_proj of Llama-3-8B); a linear with a shorter K packs floor(waves / its own
// waves) tiles into one workgroup -- wave groups of ITS K-split width, each with its own LDS region, running the unchanged body.  A row's bits are therefore exactly those
// of the ordinary launch (same waves per tile, same order of every sum).  The workgroup barrier of the K reduction is shared by the wave groups (each reaches it once);
// waves that belong to no group end at once (a barrier counts the surviving waves only).
constexpr int kI8MixMax = 8;
struct I8MixSeg {
    const half_t *A;
    int lda, K;
    I8Seg seg;  // block_begin: first blockIdx.x of this linear
};
struct I8MixArgs {
    int nseg, M;
    // (what the body reads from the launch's arguments whatever the form; the prologues / epilogues that use them are not compiled into the mixed form)
    const float *gamma = nullptr;
    float eps = 0.f;
    const float *out_gamma = nullptr;
    float out_eps = 0.f;
    half_t *xn_out = nullptr;
    float *ws = nullptr;
    const float *comb_part = nullptr;
    const int *comb_pos_dev = nullptr;
    int comb_pos = 0, comb_slots = 0, comb_chunk = 0, comb_stride = 0, comb_heads = 0;
    // the exchange of ONE linear's output slice with the other ranks inside this launch (tce_w4a16_forward_independent_gather): linear g_seg (-1: none), its g_tiles
    // 16-row tiles count themselves in on the slot's arrival counter
    int g_seg = -1;
    unsigned g_tiles = 0;
    PeerGatherEpi g;
    I8MixSeg s[kI8MixMax];
};

template <int DPP_CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ unsigned dpp_max_u32(unsigned v) {
    const unsigned t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_CTRL, ROW_MASK, 0xF, false);
    return v > t ? v : t;
}
template <int DPP_CTRL>
__device__ __forceinline__ float dpp_add_f32(float v) {
    const int t = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), DPP_CTRL, 0xF, 0xF, false);
    return v + __builtin_bit_cast(float, t);
}

// MB rows of A per pass over the weights (1 / 2 / 4), GPU groups per 128-k unit (1 / 2 / 4 for G = 128 / 64 / 32), ROWS tiles per wave, UW units per wave.
// Output column j of the MFMA = ((uu * GPU + gi) * MB + m) * 4 + p: unit-in-pass uu, group-in-unit gi, activation row m, digit plane p.
// NORM: the fused RMSNorm prologue (LlamaRMSNorm.cu:68-93 in front of q/k/v and gate/up, Int4llamaDecoderLayer.cu:78, 92-99): the waves' piece sums of x^2 meet in LDS
// (tce_common.hpp's shape-independent order: the same rs, bit for bit, as tce_rmsnorm_half and the fp16 GEMV's prologue), one barrier, then every wave normalises the
// activations it converts.  (A form that factors rs out of the row -- x * gamma kept in fp32, rs applied to the finished rows behind the barrier the K reduction needs
// anyway: no barrier and no second pass in front of the contraction -- ran the whole token 2.6 % faster and FAILED parity: the reference rounds the normalised
// activation to binary16 before the linear, and that rounding is 2.8e-4 of the output's rms, 18 x the tolerance floor of outputs near zero.  Round 4, not kept.)
// RNORM: o_proj / down_proj + residual add + the RMSNorm that FOLLOWS (post_attention_layernorm / the next layer's input_layernorm, Int4llamaDecoderLayer.cu:86-99,
// 107-108 + :78 of the next layer) as one launch: every workgroup stores its 16 updated residual values and their two piece sums of squares write-through (system
// scope: the per-XCD L2s are not coherent), counts itself in; the workgroup that arrives LAST forms rs in tce_common.hpp's order from all piece sums and writes the
// normalised row once -- instead of every workgroup of the NEXT launch normalising all of x behind a barrier (its fused prologue: +1.7 / +5.5 us on the q/k/v and
// gate/up launches; the next launch is then the plain kernel).  Bits: C as TCE_W4_ADD_TO_C, xn as tce_rmsnorm_half on the updated row.
// MEASURED (round 4): correct and SLOWER than the prologue it replaces -- the write-through stores must be acknowledged before a workgroup may count itself in and the last
// workgroup's pass is serial: +3.8 us per producer launch, a whole token 1.65 against 1.41 ms.  Kept as an entry point (tests pin its bits); DecoderBlock.step does not use it.
// a scalar the compiler must keep in its register from here on: kernel arguments are invariant loads, which the register allocator re-loads at the use rather than
// keep (the parent's `args.M` was fetched again, with its own wait, between the final LDS sum and the store)
template <typename T>
__device__ __forceinline__ void keep_scalar(T &v) {
    asm volatile("" : "+s"(v));
}
typedef __attribute__((address_space(1))) half_t c16_t;  // an output element, as device memory

// The forms whose contraction stages the B operand in a ring of two register sets (section 3 of the body): four units per pass -- one decode row, groups of 128 -- of
// the ordinary launch.  They end the workgroup's LDS with two 16-byte blocks of zeros 256 bytes apart (kI8ZeroBlock; ONE rule for the body and for launch_i8).  The other forms hold two
// sets or one per pass as it is; the mixed launch and the deferred-attention prologue keep the whole pass (their waves per SIMD are set by the workgroup's width and by
// the prologue's registers, not by the contraction).
constexpr bool i8_ring_staging(int MB, int GPU, bool MIX, int COMB) { return MB * GPU == 1 && !MIX && COMB == 0; }
constexpr int kI8ZeroBlock = 256 + 16;

// The body: everything behind the choice of the workgroup's linear.  `seg`, `A_` ... are VALUES (registers, or scalar loads still in flight: waited for at the first use);
// `args` is the launch's tail (I8Tail) or the mixed launch's struct, for the prologue / epilogue fields.
template <int MB, int GPU, int ROWS, int UW, bool Z8, bool NORM, bool RNORM, int COMB, bool MIX, typename ARGS, bool STAMPS = false>
__device__ __forceinline__ void w4a16_gemv_i8_body(const ARGS &args, unsigned char *smem, int tid, const int WK, const int U, const int K_, const int lda_, int M_, const half_t *A_,
                                                   I8Seg seg, const int tile0, const bool gathers, const unsigned g_epoch, I8Stamps *st = nullptr, const int nmem = 0) {
    static_assert(!MIX || (MB == 1 && GPU == 1 && ROWS == 1 && UW == 8 && !NORM && !RNORM && !COMB), "the mixed launch: one decode row, groups of 128, one tile per wave group");
    static_assert(!COMB || (MB == 1 && ROWS == 1 && GPU == 1 && UW == 8 && !NORM && !RNORM), "the deferred-attention prologue: one decode row, groups of 128, K a multiple of 1024");
    static_assert(MB * GPU <= 4, "sixteen output columns: rows x groups-per-unit x 4 planes");
    static_assert(!RNORM || (MB == 1 && ROWS == 1 && !NORM), "the residual + next-norm epilogue: one decode row, one tile per workgroup");
    static_assert(!NORM || MB == 1, "the fused RMSNorm prologue is a decode (M = 1) feature");
    constexpr int UPP = 4 / (MB * GPU);  // units per pass
    static_assert(UW % UPP == 0 && UW % 4 == 0, "whole passes; whole 16-byte x loads per lane");
    constexpr int NP = UW / UPP;         // passes
    constexpr int XC = UW / 4;           // 8-element activation chunks per lane and row (64 lanes x 8 = 4 units)
    constexpr int SPG = 4 / GPU;         // dwords of a lane's B operand that belong to one group
    const int NG = U * GPU;              // groups of a row
    const int lane = tid & 63;
    const int wk = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u0 = wk * UW;
    const int kq = lane >> 4, j = lane & 15;
    const int m0 = blockIdx.y * MB;
    const int ntiles = (seg.N + 15) >> 4;
    auto tile_of = [&](int r) { return tile0 + r < ntiles ? tile0 + r : ntiles - 1; };  // a surplus tile of the last workgroup re-reads the last one; its stores are masked

    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(seg.words), 0, seg.bytes_w, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t *>(seg.dscales), 0, seg.bytes_s, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(seg.dzeros), 0, seg.bytes_z, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_none = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(seg.words), 0, 0, 0x00020000);

    // column of this lane
    const int p_l = j & 3;
    const int m_l = (j >> 2) % MB;
    const int gi_l = ((j >> 2) / MB) % GPU;
    const int uu_l = (j >> 2) / (MB * GPU);

    // ---- 1. requests, in the order they are needed: activations, scales (zero points), then every weight byte of the wave ----
    uint4_t xv[MB][XC];
    // COMB: how many chunk slots of the deferred attention step are live (wave-uniform; one: that launch wrote the row itself and it is read like any other)
    int nact = 1;
    if constexpr (COMB) {
        const int pos = args.comb_pos_dev ? __builtin_amdgcn_readfirstlane(*args.comb_pos_dev) : args.comb_pos;
        nact = (pos + args.comb_chunk) / args.comb_chunk;  // ceil((pos + 1) / chunk)
        nact = nact < args.comb_slots ? nact : args.comb_slots;
    }
    constexpr int kSlots = COMB ? COMB : 1;              // COMB = the slots the prologue is compiled for: 4 or 8 (kAttnDeferMaxSlots); the launch's slots <= COMB
    uint2_t cml[COMB ? XC : 1][kSlots];                  // (M, L) of the lane's head per slot
    uint4_t co[COMB ? XC : 1][kSlots][2];                // O[d0 .. d0 + 7] per slot
    if constexpr (COMB) {
        if (nact > 1) {
            const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(args.comb_part), 0, args.comb_heads * args.comb_slots * args.comb_stride * 4, 0x00020000);
#pragma unroll
            for (int c = 0; c < XC; ++c) {
                const int kpos = u0 * 128 + (lane + 64 * c) * 8;       // the lane's 8 columns: head kpos / 128, dimensions kpos % 128 ..
                const int hbase = ((kpos >> 7) * args.comb_slots) * args.comb_stride * 4 + (kpos & 127) * 4;
#pragma unroll
                for (int i = 0; i < kSlots; ++i) {
                    // dead slots re-read the first one (their weights are never formed): plain loads -- every lane's addresses are valid, nothing needs a range check
                    const int ii = i < nact ? i : 0;
                    const unsigned char *src = reinterpret_cast<const unsigned char *>(args.comb_part) + hbase + ii * args.comb_stride * 4;
                    cml[c][i] = *reinterpret_cast<const uint2_t *>(src - (kpos & 127) * 4);
                    co[c][i][0] = *reinterpret_cast<const uint4_t *>(src + 16);
                    co[c][i][1] = *reinterpret_cast<const uint4_t *>(src + 32);
                }
                (void)rs_p;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        if (COMB && nact > 1) break;
        int mrow = m0 + m;
        mrow = mrow < M_ ? mrow : M_ - 1;
        // a descriptor per row, K halves long: chunks past K (a ragged last wave) read as zeros
        const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t *>(A_ + (size_t)mrow * lda_), 0, K_ * 2, 0x00020000);
#pragma unroll
        for (int c = 0; c < XC; ++c) xv[m][c] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, u0 * 256 + (lane + 64 * c) * 16, 0, 0);  // (the scalar offset of a buffer load is NOT range-checked: everything that may run past K sits in the vector offset)
    }
    float4_t gm[NORM ? XC : 1][2];  // gamma of the lane's 8 columns per chunk
    if constexpr (NORM) {
        const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(args.gamma), 0, K_ * 4, 0x00020000);
#pragma unroll
        for (int c = 0; c < XC; ++c) {
            gm[c][0] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_g, u0 * 512 + (lane + 64 * c) * 32, 0, 0));
            gm[c][1] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_g, u0 * 512 + (lane + 64 * c) * 32 + 16, 0, 0));
        }
    }
    uint2_t sc[ROWS][NP];
    unsigned zq[ROWS][(NP + 1) / 2];  // zero points other than 8: the lane's four rows' nibbles of pass ps in half (ps & 1) of word ps / 2 (two passes per register: the general-zero-point forms are the ones short of registers)
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int g = (ps * UPP + uu_l) * GPU + gi_l;  // group of this lane's column, relative to the wave's first group
            const int ga = (tile_of(r) * NG + u0 * GPU) + g;  // groups past K (a ragged last wave) read the next tile's values or, behind the last tile, zeros: their products are zero
            sc[r][ps] = __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(rs_s, (ga * 16 + 4 * kq) * 2, 0, 0));
            if constexpr (!Z8) {
                const unsigned z16 = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs_z, ga * 8 + 2 * kq, 0, 0);
                zq[r][ps >> 1] = (ps & 1) ? (zq[r][ps >> 1] | (z16 << 16)) : z16;
            }
        }
    __builtin_amdgcn_sched_barrier(0);
    uint4_t w[ROWS][UW];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int t = 0; t < UW; ++t) {
            // units past K (a ragged last wave): an empty descriptor -- answered with zeros by the buffer unit, no memory traffic
            w[r][t] = __builtin_amdgcn_raw_buffer_load_b128(u0 + t < U ? rs_w : rs_none, lane * 16, (tile_of(r) * U + u0 + t) * 1024, /*nt*/ 2);
        }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STAMPS) {
        st->t[1] = __builtin_amdgcn_s_memrealtime();
        st->t[6] = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
    }

    if constexpr (COMB) {
        if (nact > 1) {
            // attention_fast.hip's combine, operation for operation: Mx = max M_i; w_i = exp(M_i - Mx); L = sum L_i w_i, O = sum O_i w_i in slot order (products and sums
            // rounded separately: this file is compiled without contraction); x = half(O / L)
#pragma unroll
            for (int c = 0; c < XC; ++c) {
                // (an element of a vector goes through a scalar before its bits are reinterpreted: __builtin_bit_cast applied to `v[k]` directly read v[0] for every k --
                //  found by tests/test_gpu_deferred_attention.py: M for L, O[0] for O[1..3])
                auto f32 = [](unsigned u) { return __builtin_bit_cast(float, u); };
                float Mx = -1.0e30f;
#pragma unroll
                for (int i = 0; i < kSlots; ++i)
                    if (i < nact) Mx = __builtin_fmaxf(Mx, f32(cml[c][i][0]));
                float Lx = 0.f, Ox[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) Ox[e] = 0.f;
#pragma unroll
                for (int i = 0; i < kSlots; ++i) {
                    if (i < nact) {  // (wave-uniform)
                        const float w = __expf(f32(cml[c][i][0]) - Mx);
                        Lx += f32(cml[c][i][1]) * w;
#pragma unroll
                        for (int e = 0; e < 8; ++e) Ox[e] += f32(co[c][i][e >> 2][e & 3]) * w;
                    }
                }
                half8_t y;
#pragma unroll
                for (int e = 0; e < 8; ++e) y[e] = (half_t)(Ox[e] / Lx);
                xv[0][c] = __builtin_bit_cast(uint4_t, y);
            }
        }
    }
    // ---- 2. the wave's activations -> digit planes, image [unit][lo/hi][m][plane][kq][word s] in its own LDS region ----
    unsigned *planes = reinterpret_cast<unsigned *>(smem) + wk * (UW * MB * 128);
    // the workgroup's two blocks of zeros (section 3's ring; bytes 0 .. 15 and 256 .. 271), behind everything else in LDS.  Every wave writes them -- the same zeros -- in front of its own wave barrier:
    // what a wave reads there follows its own write in program order, whatever the other waves are doing
    unsigned char *zero_blk = smem + (size_t)WK * UW * MB * 512 + (size_t)WK * ROWS * MB * 16 * sizeof(float) + (NORM ? (size_t)(K_ >> 3) * sizeof(float) + 1024 : 0);
    if constexpr (i8_ring_staging(MB, GPU, MIX, COMB)) reinterpret_cast<unsigned *>(zero_blk)[(lane & 3) + (lane & 4) * 16] = 0u;
    if constexpr (NORM) {
        // slot[p] = the sum of squares of the row's p-th 16-byte piece (fmaf chain over its 8 values); K <= 16384: at most two pieces per slot of the
        // 1024-slot order, and a two-term sum does not depend on which wave wrote which
        float *slots = reinterpret_cast<float *>(smem + (size_t)WK * UW * MB * 512 + (size_t)WK * ROWS * MB * 16 * sizeof(float));  // [2048]
        const int pieces = K_ >> 3;
#pragma unroll
        for (int c = 0; c < XC; ++c) {
            const int p = u0 * 16 + lane + 64 * c;
            if (p < pieces + 128) slots[p] = rmsnorm_piece_sum(__builtin_bit_cast(half8_t, xv[0][c]));  // (pieces past K: zeros were loaded)
        }
        lds_barrier();  // (LDS only: every weight byte of the wave stays in flight)
        // (the order's sixteen terms per lane; the terms past the row's pieces are zeros: only the first ceil(pieces / 64) are read -- 8 for K = 4096)
        float tot = 0.f;
        const int nc = pieces >= 1024 ? 16 : (pieces + 63) >> 6;
        if (pieces <= 1024 && (pieces & 63) == 0) {
            // whole 64-piece terms, no second piece per slot (K = 4096: 8 reads at fixed offsets and 8 adds; the same sum, without the bounds arithmetic of the
            // general form below -- measured 0.25 / 0.65 us per launch on norm + q/k/v and norm + gate/up of a 4096-wide layer)
            const float *sl = slots + lane;
            for (int c = 0; c < nc; ++c) tot += sl[c * 64];
        } else {
            for (int c = 0; c < nc; ++c) {
                const int q = c * 64 + lane;
                float slot = 0.f;
                slot += q < pieces ? slots[q] : 0.f;
                if (q + 1024 < pieces) slot += slots[q + 1024];
                tot += slot;
            }
        }
        tot = wave_sum_dpp_lane63(tot);
        tot = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tot), 63));
        const float rs = 1.0f / sqrtf(tot / (float)K_ + args.eps);
#pragma unroll
        for (int c = 0; c < XC; ++c) {
            const half8_t v = __builtin_bit_cast(half8_t, xv[0][c]);
            half8_t y;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // rmsnorm_out's arithmetic -- half(clamp((x * rs) * gamma)) -- with the clamp as ONE v_med3_f32: the same value for every finite product, and for a NaN
                // product too (v_med3_f32 returns the minimum of the other two, -64504, which is where rmsnorm_out's fmaxf sends it: a row that holds a NaN is
                // normalised to FINITE values and is not poisoned below): 3 vector instructions fewer per element, 48 per wave, in a kernel that is bound by issue
                const float f = ((float)v[e] * rs) * (e < 4 ? gm[c][0][e] : gm[c][1][e - 4]);
                y[e] = (half_t)__builtin_amdgcn_fmed3f(f, -(65504.f - 1000.f), 65504.f - 1000.f);
            }
            xv[0][c] = __builtin_bit_cast(uint4_t, y);
        }
        // A ragged last wave (K no multiple of the wave's block): its chunks past K hold zeros and must STAY zero -- the weights they meet are the next tile's.  With a
        // finite rs they do (0 * rs * 0); a row that holds a NaN has rs = NaN, and 0 * NaN is NaN, which the clamp above turns into -64504.  One scalar test for the
        // launches that have no ragged wave (every K that is a multiple of 1024: the models' hidden sizes), a select per chunk for the others.
        // (the lane against a scalar bound per chunk: no vector register beside the ones the prologue holds -- tests/test_decode_occupancy_isa.py)
        if (K_ % (UW * 128) != 0) {
            const int left = __builtin_amdgcn_readfirstlane(pieces - u0 * 16);  // the wave's pieces inside the row
#pragma unroll
            for (int c = 0; c < XC; ++c)
                if (lane >= left - 64 * c) xv[0][c] = uint4_t{0u, 0u, 0u, 0u};
        }
    }
    int sh[MB];
    bool bad[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        unsigned mx = 0;
#pragma unroll
        for (int c = 0; c < XC; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned v = xv[m][c][q] & 0x7FFF7FFFu;
                const unsigned v2 = v << 16;
                const unsigned m2 = v > v2 ? v : v2;  // bits 30..26: the larger exponent field of the two halves
                mx = mx > m2 ? mx : m2;
            }
        // wave-wide maximum on the VALU: row_shr 1 2 4 8 inside rows of 16, then row_bcast15 / row_bcast31; the total sits in lane 63
        mx = dpp_max_u32<0x111>(mx);
        mx = dpp_max_u32<0x112>(mx);
        mx = dpp_max_u32<0x114>(mx);
        mx = dpp_max_u32<0x118>(mx);
        mx = dpp_max_u32<0x142, 0xA>(mx);
        mx = dpp_max_u32<0x143, 0xC>(mx);
        const int E = (int)((unsigned)__builtin_amdgcn_readlane((int)mx, 63) >> 26);  // exponent field of the block's largest magnitude: |x| < 2^(E - 14)
        bad[m] = E == 31;
        sh[m] = 44 - E;  // |x * 2^sh| < 2^30
        const float scale = __builtin_bit_cast(float, (unsigned)(127 + sh[m]) << 23);
#pragma unroll
        for (int c = 0; c < XC; ++c) {
            unsigned d[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const half_t lo = __builtin_bit_cast(half_t, (unsigned short)(xv[m][c][q] & 0xFFFFu));
                const half_t hi = __builtin_bit_cast(half_t, (unsigned short)(xv[m][c][q] >> 16));
                // exact product (11 significant bits), truncated to an integer; balanced digits: the bytes of (I + 0x808080) ^ 0x808080
                d[2 * q] = ((unsigned)(int)__builtin_fmaf((float)lo, scale, 0.0f) + 0x00808080u) ^ 0x00808080u;
                d[2 * q + 1] = ((unsigned)(int)__builtin_fmaf((float)hi, scale, 0.0f) + 0x00808080u) ^ 0x00808080u;
            }
            // chunk cc of the wave's block = the 8 activations of (unit tu, word s, k-quarter q): k = 128 tu + 32 s + 8 q + e
            const int cc = lane + 64 * c;
            const int tu = cc >> 4, s = (cc >> 2) & 3, q4 = cc & 3;
            // a packed word's low nibbles are the codes e = (0, 4, 1, 5), its high nibbles e = (2, 6, 3, 7) (pk::nibble_index)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned a0 = d[2 * h], a1 = d[2 * h + 4], a2 = d[2 * h + 1], a3 = d[2 * h + 5];
                const unsigned t0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);  // (a0.b0, a1.b0, a0.b1, a1.b1)
                const unsigned t1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);  // (a0.b2, a1.b2, a0.b3, a1.b3)
                const unsigned t2 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
                const unsigned t3 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
                const int base = ((((tu * 2 + h) * MB + m) * 4) * 4 + q4) * 4 + s;  // + plane * 16
                planes[base + 0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
                planes[base + 16] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
                planes[base + 32] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
                planes[base + 48] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (STAMPS) st->t[2] = __builtin_amdgcn_s_memrealtime();

    // a launch on a group copy (nmem > 0): the member each of the wave's tiles belongs to -- where its rows are stored and how.  Up to here the launch was one linear of
    // the members' rows together (seg.N: all of them); member rows are whole tiles, so a tile that exists lies inside exactly one member
    half_t *mC[ROWS];
    int mldc[ROWS], mepi[ROWS], mrow0[ROWS];  // mrow0: the member's first row in the copy
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        mC[r] = seg.C;
        mldc[r] = seg.ldc;
        mepi[r] = seg.epilogue;
        mrow0[r] = 0;
    }
    if constexpr (!MIX) {
        if (nmem > 0) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                int mi = 0;
#pragma unroll
                for (int i = 1; i < TCE_MAX_GROUP; ++i) mi = (i < nmem && tile0 + r >= args.mtile[i]) ? i : mi;
                mC[r] = args.rest[mi].C;
                mldc[r] = args.rest[mi].ldc;
                mepi[r] = args.rest[mi].epilogue;
                mrow0[r] = args.mtile[mi] * 16;
            }
        }
    }
    // (the thread's own tile r: wave-uniform for one tile per wave)
    auto of_tile = [&](auto *v, int r) {
        auto x = v[0];
#pragma unroll
        for (int r2 = 1; r2 < ROWS; ++r2) x = r == r2 ? v[r2] : x;
        return x;
    };
    // the residual epilogue's old values (TCE_W4_ADD_TO_C): requested by the lanes that will add to them, BEHIND the weight requests and the conversion (the flags, C and
    // ldc are tail arguments: asking here, not in front of the weights, keeps every scalar wait out of the head; loads return in order, and the value is needed behind
    // the K reduction's barrier only -- where a load issued there was a memory round trip at the very end of every o_proj / down_proj launch)
    // What the store needs is formed HERE as well, where the wave is parked on its weight loads and the issue slots are free (decode-tail round; profiles/decode_tail/):
    // whether the thread's output row exists, its member's epilogue, and its element as a scalar base per tile plus one 32-bit byte offset per lane.  Behind the K
    // reduction's barrier wave 0 then does only what needs the contraction's result: the sum over the waves, the rounding, the epilogue its flags name, one store -- no
    // select, no bounds compare, no multiply.
    // Thread tid of wave 0 finishes output (tile t_r, activation row t_m, tile row t_i16): tid = (t_r * MB + t_m) * 16 + t_i16.
    const int t_i16 = tid & 15, t_m = (tid >> 4) % MB, t_r = tid / (16 * MB);
    const int t_row = (tile0 + t_r) * 16 + t_i16;  // (unclamped: a surplus tile's rows are >= N)
    const bool t_live = wk == 0 && tid < ROWS * MB * 16 && m0 + t_m < M_ && t_row < seg.N;
    c16_t *cbase[ROWS];  // the element of (activation row m0, the tile's first row) in the tile's member: C is device memory, addressed as such (a scalar base + a lane's offset in ONE instruction)
    int any_pair = 0;    // (wave-uniform: the SiLU arithmetic sits behind a scalar branch)
    int pshift[ROWS];    // 1: the tile's member stores pairs
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        keep_scalar(mepi[r]);  // (the flags stay in their registers from here on: nothing behind the barrier waits on scalar memory)
        const int first = (tile0 + r) * 16 - mrow0[r];  // the tile's first row inside its member (a group copy; otherwise in the linear): a multiple of 16
        // the pair epilogue: rows 2n, 2n + 1 -> element n
        cbase[r] = (c16_t *)mC[r] + ((size_t)m0 * mldc[r] + ((mepi[r] & TCE_W4_SILU_MUL_PAIRS) ? first >> 1 : first));
        keep_scalar(cbase[r]);
        pshift[r] = (mepi[r] & TCE_W4_SILU_MUL_PAIRS) ? 1 : 0;
        keep_scalar(pshift[r]);
        any_pair |= mepi[r] & TCE_W4_SILU_MUL_PAIRS;
    }
    const int t_epi = of_tile(mepi, t_r);
    const bool t_pair = (t_epi & TCE_W4_SILU_MUL_PAIRS) != 0;
    const bool t_add = !t_pair && (t_epi & TCE_W4_ADD_TO_C);
    const bool t_store = t_live && !(t_pair && (t_i16 & 1));  // (the pair is stored by the even row's lane)
    // thread t's element of tile r: bytes from the tile's base -- its activation row's ldc (nothing for one row per pass) and the tile row, halved by a pair member
    auto c_at = [&](int r, int t) {
        const unsigned off = (unsigned)(((t >> 4) % MB) * mldc[r] + ((t & 15) >> pshift[r])) * 2u;
        return reinterpret_cast<c16_t *>(reinterpret_cast<__attribute__((address_space(1))) unsigned char *>(cbase[r]) + off);
    };
    half_t c_old = (half_t)0.0f;
    if constexpr (!RNORM) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
            if (t_live && t_add && (ROWS == 1 || t_r == r)) c_old = *c_at(r, tid);
    }

    // ---- 3. contraction.  B set uu: the operand of unit uu of the pass in the lanes of ITS columns, zeros in the others (never written) ----
    // RING (four units per pass: one decode row, groups of 128): the sets are a ring of TWO -- unit t's operand is read into set t & 1 behind the MFMAs of unit t - 2,
    // two units ahead of its own -- where a whole pass of four sets (32 registers, refilled a pass ahead) was what kept the kernel at five waves per SIMD
    // (profiles/decode_occupancy/).  A reused set must hold zeros again in the lanes of the other units' columns: those lanes READ zeros, through the same two
    // instructions, from the workgroup's zero blocks -- two of 16 bytes, as far apart (256 bytes) as a unit's low and high image, so that ONE select on the address
    // serves both reads of a unit: an add and a select per unit, 16 vector instructions per wave.  (Re-zeroing a set instead: four 64-bit moves and a second exec mask
    // per reuse, 24 moves per wave; a select per read with the offset in the instruction: a move of the scalar operand on top of every select, 31.)
    // Same LDS image, same addresses, same columns, the same MFMAs in the same order per accumulator: the integer sums are what they were.
    constexpr bool RING = i8_ring_staging(MB, GPU, MIX, COMB);
    constexpr int NB = RING ? 2 : UPP;
    int4_t B[NB][2];
    if constexpr (!RING) {
#pragma unroll
        for (int uu = 0; uu < UPP; ++uu) B[uu][0] = B[uu][1] = int4_t{0, 0, 0, 0};
    }
    typedef __attribute__((address_space(3))) const uint4_t lds_u4_t;
    // (LDS byte addresses; RING only: MB == 1 and GPU == 1, the lane's part of a unit's image is (plane, k-quarter))
    const unsigned lane_a = (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) unsigned *)planes + (unsigned)((p_l * 4 + kq) * 16);
    const unsigned zero_a = (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) unsigned char *)zero_blk;
    auto read_unit = [&](int t) {  // unit t of the wave (t = ps * UPP + uu) -> set t & 1
        const unsigned a = uu_l == t % UPP ? lane_a + (unsigned)t * 512u : zero_a;  // the unit's low image, or the first zero block
#pragma unroll
        for (int h = 0; h < 2; ++h) B[t & 1][h] = __builtin_bit_cast(int4_t, *reinterpret_cast<lds_u4_t *>(a + (unsigned)h * 256u));
    };
    auto read_b = [&](int ps) {
#pragma unroll
        for (int uu = 0; uu < UPP; ++uu)
#pragma unroll
            for (int gi = 0; gi < GPU; ++gi)
                if (uu_l == uu && gi_l == gi) {  // exec-masked reads
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const unsigned *src = planes + ((((((ps * UPP + uu) * 2 + h) * MB + m_l) * 4 + p_l) * 4 + kq) * 4 + gi * SPG);
                        if constexpr (GPU == 1) {
                            B[uu][h] = __builtin_bit_cast(int4_t, *reinterpret_cast<const uint4_t *>(src));
                        } else if constexpr (GPU == 2) {
                            const uint2_t v = *reinterpret_cast<const uint2_t *>(src);
                            B[uu][h][gi * 2] = (int)v[0];
                            B[uu][h][gi * 2 + 1] = (int)v[1];
                        } else {
                            B[uu][h][gi] = (int)*src;
                        }
                    }
                }
    };
    (void)read_unit;
    (void)read_b;
    if constexpr (RING) {
        read_unit(0);
        read_unit(1);
    } else {
        read_b(0);
    }

    float acc[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[r][q] = 0.f;
    const int4_t zero4 = int4_t{0, 0, 0, 0};
    const int4_t sixteens = int4_t{0x10101010, 0x10101010, 0x10101010, 0x10101010};
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        // general zero points: the scheduler would otherwise unpack every pass's (8 - z) nibbles ahead of the first MFMA (NP x 4 registers: 19 spilled in the
        // M = 2 / G = 64 form under the 128-register bound of a 16-wave workgroup).  A pass's work stays inside the pass.
        if constexpr (!Z8) __builtin_amdgcn_sched_barrier(0);
        int4_t dd[ROWS][2];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) dd[r][0] = dd[r][1] = zero4;
        int4_t dz = zero4;  // 16 * sum of the digits of the column's group (zero points other than 8)
#pragma unroll
        for (int uu = 0; uu < UPP; ++uu) {
            const int t = ps * UPP + uu;
            const int bs = RING ? (t & 1) : uu;  // the unit's B set
            if constexpr (!Z8) {
                dz = __builtin_amdgcn_mfma_i32_16x16x64_i8(sixteens, B[bs][0], dz, 0, 0, 0);
                dz = __builtin_amdgcn_mfma_i32_16x16x64_i8(sixteens, B[bs][1], dz, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                int4_t alo, ahi;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // signed bytes 16 (q - 8): (nibble in the high half of the byte) ^ 0x80.  Written as two independent and-xor forms so that each is ONE
                    // v_bitop3 (a shared w ^ 0x88888888 costs a fourth instruction per word)
                    const unsigned wq = w[r][t][q];
                    ahi[q] = (int)((wq & 0xF0F0F0F0u) ^ 0x80808080u);
                    alo[q] = (int)(((wq << 4) & 0xF0F0F0F0u) ^ 0x80808080u);
                }
                dd[r][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(alo, B[bs][0], dd[r][0], 0, 0, 0);
                if constexpr (Z8) dd[r][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ahi, B[bs][1], dd[r][1], 0, 0, 0);
                else dd[r][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ahi, B[bs][1], dd[r][0], 0, 0, 0);  // (one accumulator chain: integer sums, the same value; four registers fewer beside dz and the sixteens)
            }
            if constexpr (RING) {
                // the set is free once this unit's MFMAs have been issued: the read of unit t + 2 stays BEHIND them (left alone the scheduler hoists every read to the
                // top of the pass -- one set per unit again) and in front of the next unit's
                __builtin_amdgcn_sched_barrier(0);
                if (t + 2 < UW) read_unit(t + 2);
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const half_t s0 = __builtin_bit_cast(half_t, (unsigned short)(sc[r][ps][0] & 0xFFFFu));
            const half_t s1 = __builtin_bit_cast(half_t, (unsigned short)(sc[r][ps][0] >> 16));
            const half_t s2 = __builtin_bit_cast(half_t, (unsigned short)(sc[r][ps][1] & 0xFFFFu));
            const half_t s3 = __builtin_bit_cast(half_t, (unsigned short)(sc[r][ps][1] >> 16));
            int4_t tot = dd[r][0] + dd[r][1];
            if constexpr (!Z8) {
                // sum (q - z) X = sum (q - 8) X + (8 - z) sum X, in the same units of 16
#pragma unroll
                for (int q = 0; q < 4; ++q) tot[q] += __mul24(8 - (int)((zq[r][ps >> 1] >> (16 * (ps & 1) + 4 * q)) & 0xFu), dz[q]);
            }
            acc[r][0] = __builtin_fmaf((float)tot[0], (float)s0, acc[r][0]);
            acc[r][1] = __builtin_fmaf((float)tot[1], (float)s1, acc[r][1]);
            acc[r][2] = __builtin_fmaf((float)tot[2], (float)s2, acc[r][2]);
            acc[r][3] = __builtin_fmaf((float)tot[3], (float)s3, acc[r][3]);
        }
        if constexpr (!RING) {
            if (ps + 1 < NP) read_b(ps + 1);
        }
    }

    // ---- 4. planes and groups -> the wave's partial rows (fixed lane order), waves -> rows (wave order), store ----
    if constexpr (STAMPS) {
        // (behind the last accumulator: the reading must not be taken before the contraction's results exist)
        asm volatile("" ::"v"(acc[ROWS - 1][3]));
        st->t[3] = __builtin_amdgcn_s_memrealtime();
    }
    int sh_l = sh[0];
    bool bad_l = bad[0];
#pragma unroll
    for (int m = 1; m < MB; ++m) {
        sh_l = m_l == m ? sh[m] : sh_l;
        bad_l = m_l == m ? bad[m] : bad_l;
    }
    // 2^(8 p) * 2^(-sh) / 16 (the A operand carries 16 (q - 8))
    const float cj = bad_l ? __builtin_nanf("") : __builtin_bit_cast(float, (unsigned)(127 + 8 * p_l - sh_l - 4) << 23);
    float *red = reinterpret_cast<float *>(smem + (size_t)WK * UW * MB * 512);  // [WK][ROWS][MB][16]
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        // (step by step over the four registers: four independent chains, so that no DPP step waits on the add in front of it; each chain's own order is what it was)
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[r][q] * cj;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = dpp_add_f32<0xB1>(v[q]);  // quad_perm [1,0,3,2]: planes
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = dpp_add_f32<0x4E>(v[q]);  // quad_perm [2,3,0,1]
        if constexpr (MB <= 2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = dpp_add_f32<0x128>(v[q]);  // row_ror 8
        }
        if constexpr (MB == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = dpp_add_f32<0x124>(v[q]);  // row_ror 4
        }
        // (the chains end as four scalars: seen from the 16-byte write the vectoriser pairs them up -- a zeroing move, a DPP move and a packed add per step and pair
        //  where the scalar form is ONE v_add_f32 with a DPP operand)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(v[q]));
        // a lane that holds a finished partial row holds four consecutive floats of it: one 16-byte LDS write
        if (p_l == 0 && (j >> 2) < MB) *reinterpret_cast<float4_t *>(red + ((wk * ROWS + r) * MB + m_l) * 16 + kq * 4) = float4_t{v[0], v[1], v[2], v[3]};
    }
    keep_scalar(seg.N);
    keep_scalar(M_);
    float *ws_ = nullptr, *out_gamma_ = nullptr;
    half_t *xn_out_ = nullptr;
    unsigned out_eps_ = 0, last_wg_ = 0;
    if constexpr (RNORM) {
        ws_ = args.ws;
        out_gamma_ = const_cast<float *>(args.out_gamma);
        xn_out_ = args.xn_out;
        out_eps_ = __builtin_bit_cast(unsigned, args.out_eps);
        last_wg_ = gridDim.x - 1;
        keep_scalar(ws_);
        keep_scalar(out_gamma_);
        keep_scalar(xn_out_);
        keep_scalar(out_eps_);
        keep_scalar(last_wg_);
    }
    __syncthreads();
    if (tid < ROWS * MB * 16) {
        // The sum over the WK waves that exist (wave-uniform, 1..16): exactly their partial rows, at one address plus immediate offsets, chosen by scalar branches.
        // Added in wave order starting from 0.f, as ever: what the sixteen-slot form added for the waves that do not exist was `+ 0.f` on a value that is never -0
        // (the chain starts at +0, and +0 plus anything is not -0), so every output bit is what it was.
        constexpr int S = ROWS * MB * 16;  // floats per set of partial rows
        const float *part = red + tid;
        float v = 0.f;
        if (WK <= 4) {
            // K <= 4096, four of the token's five launch shapes: straight-line, the reads issued together
            if (WK == 4) {
                const float p0 = part[0], p1 = part[S], p2 = part[2 * S], p3 = part[3 * S];
                v += p0;
                v += p1;
                v += p2;
                v += p3;
            } else if (WK == 3) {
                const float p0 = part[0], p1 = part[S], p2 = part[2 * S];
                v += p0;
                v += p1;
                v += p2;
            } else if (WK == 2) {
                const float p0 = part[0], p1 = part[S];
                v += p0;
                v += p1;
            } else {
                v += part[0];
            }
        } else {
            // 5 .. 16 waves: four rows per trip, then the 0 .. 3 rows that are left.  (Written with the next trip's reads in front of this trip's adds; the compiler
            //  reuses the four registers and issues them behind the adds, so a trip still costs an LDS round trip: profiles/decode_tail/instruction_budget.md)
            float p0 = part[0], p1 = part[S], p2 = part[2 * S], p3 = part[3 * S];
            int left = WK - 4;
            part += 4 * S;
#pragma unroll 1
            while (left >= 4) {
                const float q0 = part[0], q1 = part[S], q2 = part[2 * S], q3 = part[3 * S];
                v += p0;
                v += p1;
                v += p2;
                v += p3;
                p0 = q0, p1 = q1, p2 = q2, p3 = q3;
                left -= 4;
                part += 4 * S;
            }
            float r0 = 0.f, r1 = 0.f, r2 = 0.f;
            if (left >= 1) r0 = part[0];
            if (left >= 2) r1 = part[S];
            if (left >= 3) r2 = part[2 * S];
            v += p0;
            v += p1;
            v += p2;
            v += p3;
            if (left >= 1) v += r0;
            if (left >= 2) v += r1;
            if (left >= 3) v += r2;
        }
        const half_t y = (half_t)v;
        half_t out = y, hnew = (half_t)0.0f;
        (void)hnew;
        if (any_pair) {  // (wave-uniform)
            // the (gate, up) neighbour of the pair epilogue: rows 2n, 2n + 1 are adjacent lanes
            const half_t y_other = __builtin_bit_cast(half_t, (unsigned short)__builtin_amdgcn_update_dpp(0, (int)__builtin_bit_cast(unsigned short, y), 0xB1, 0xF, 0xF, false));
            if (t_pair) out = silu_mul_half(y, y_other);
        }
        if constexpr (RNORM) {
            if (t_live && t_add) hnew = *c_at(0, tid) + y;  // (stored below, write-through)
            else if (t_store) *c_at(0, tid) = out;
        } else {
            if (t_add) out = c_old + y;
            // (several tiles per wave are the forms short of registers: there the lane's offset -- two shifts -- is formed again here and not carried through the contraction)
            int t_late = tid;
            if constexpr (ROWS > 1) asm volatile("" : "+v"(t_late));
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
                if (t_store && (ROWS == 1 || t_r == r)) *c_at(r, t_late) = out;
        }
        if constexpr (MIX) {
            if (gathers && t_live) {
                // (a) the tile's 16 values into EVERY rank's window -- buffer (slot, parity of the epoch), this rank's slice -- past every cache (comm.hip's protocol)
                const half_t outv = (t_epi & TCE_W4_ADD_TO_C) ? (half_t)(c_old + y) : y;
                const size_t off = ((size_t)args.g.slot * 2 + (g_epoch & 1u)) * args.g.vec_bytes + ((size_t)args.g.rank * args.g.slice_elems + (size_t)t_row) * 2;
#pragma unroll
                for (int p = 0; p < kCommMaxRanks; ++p)
                    if (p < args.g.world)
                        __hip_atomic_store(reinterpret_cast<unsigned short *>(args.g.peer[p] + off), __builtin_bit_cast(unsigned short, outv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if constexpr (RNORM) {
            // the tile's 16 updated values -> memory, past every cache (the last workgroup reads them from another XCD); their two piece sums likewise
            const int row = t_row;
            if (row < seg.N) __hip_atomic_store(reinterpret_cast<unsigned short *>(seg.C) + row, __builtin_bit_cast(unsigned short, hnew), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const float hf = row < seg.N ? (float)hnew : 0.f;
            float s0 = 0.f, s1 = 0.f;  // fmaf chains over the two pieces' 8 values, in order (rmsnorm_piece_sum), formed by every lane from broadcasts
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hf), e));
                const float v1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hf), 8 + e));
                s0 = __builtin_fmaf(v0, v0, s0);
                s1 = __builtin_fmaf(v1, v1, s1);
            }
            if (tid < 2) __hip_atomic_store(ws_ + 2 * tile0 + tid, tid == 0 ? s0 : s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if constexpr (STAMPS) {
        if (tid < 64 && args.dbg) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have been acknowledged
            st->t[4] = __builtin_amdgcn_s_memrealtime();
#pragma unroll
            for (int i = 0; i < 7; ++i)
                if (tid == i) args.dbg[(size_t)blockIdx.x * 8 + i] = st->t[i];
        }
    }
    if constexpr (MIX) {
        if (gathers && tid < 64) {  // (the tile's first wave: the one that stored)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores above have been acknowledged before the tile counts itself in
            unsigned *const counter = args.g.epochs + args.g.slots + 1 + args.g.slot;
            unsigned last = 0;
            if (tid == 0) last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == args.g_tiles - 1u ? 1u : 0u;
            last = (unsigned)__builtin_amdgcn_readfirstlane((int)last);
            if (last) {
                // ---- the last tile of the slice: flags out, the other ranks' flags in, the complete vector to the consumer's buffer (allgather_peer_kernel's b, c, d) ----
                const unsigned e = g_epoch, par = e & 1u;
                __threadfence_system();
                if (tid < args.g.world) {
                    unsigned *flag = reinterpret_cast<unsigned *>(args.g.peer[tid] + args.g.flags_off) + (((size_t)args.g.slot * 2 + par) * kCommMaxRanks + args.g.rank) * kCommFlagStride;
                    __hip_atomic_store(flag, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                if (tid < args.g.world) {
                    const unsigned *flag = reinterpret_cast<const unsigned *>(args.g.peer[args.g.rank] + args.g.flags_off) + (((size_t)args.g.slot * 2 + par) * kCommMaxRanks + tid) * kCommFlagStride;
                    const unsigned long long t0 = wall_clock64();
                    const bool dead = __hip_atomic_load(args.g.epochs + args.g.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                    while (!dead && (int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - e) < 0) {
                        __builtin_amdgcn_s_sleep(8);
                        if (wall_clock64() - t0 > args.g.timeout_ticks) {  // a rank that never arrives: give up, flag the communicator (tce_comm_status; tce_comm_reset re-arms)
                            __hip_atomic_store(args.g.epochs + args.g.slots, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            break;
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                __threadfence_system();  // acquire: the peers' data behind their flags
                const unsigned char *full = args.g.peer[args.g.rank] + ((size_t)args.g.slot * 2 + par) * args.g.vec_bytes;
                const unsigned total16 = args.g.slice_elems * (unsigned)args.g.world / 8u;
                for (unsigned base = 0; base < total16; base += 64 * 8) {
                    uint4_t v[8];  // eight pieces per lane in flight (one wave carries the whole vector: 8 KiB at 4096 halves)
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const unsigned i = base + q * 64 + tid;
                        const unsigned ic = i < total16 ? i : total16 - 1;
                        asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v[q]) : "v"(full + (size_t)ic * 16) : "memory");
                    }
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const unsigned i = base + q * 64 + tid;
                        if (i < total16) reinterpret_cast<uint4_t *>(args.g.dst)[i] = v[q];
                    }
                }
                if (tid == 0) {
                    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next exchange on this slot (ordered by the kernel boundary)
                    __hip_atomic_store(args.g.epochs + args.g.slot, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    if constexpr (RNORM) {
        unsigned *flag = reinterpret_cast<unsigned *>(smem);  // (the planes are dead)
        if (tid < 64) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores above have left this wave before it counts itself in
            if (tid == 0) {
                const unsigned old = __hip_atomic_fetch_add(reinterpret_cast<unsigned *>(ws_) + 2048, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                flag[0] = old == last_wg_ ? 1u : 0u;
            }
        }
        __syncthreads();
        if (flag[0] == 0u) return;
        // ---- the last workgroup: rs, then the normalised row ----
        if (tid == 0) reinterpret_cast<unsigned *>(ws_)[2048] = 0u;  // for the next launch on this workspace (ordered by the kernel boundary)
        const int n = seg.N, pieces = n >> 3;
        auto sys_load_f32 = [](const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
        float tot = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int q = c * 64 + lane;
            float slot = 0.f;
            slot += q < pieces ? sys_load_f32(ws_ + q) : 0.f;
            if (q + 1024 < pieces) slot += sys_load_f32(ws_ + q + 1024);
            tot += slot;
        }
        tot = wave_sum_dpp_lane63(tot);
        tot = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tot), 63));
        const float rs = 1.0f / sqrtf(tot / (float)n + __builtin_bit_cast(float, out_eps_));
        const half_t *hrow = seg.C;
        for (int p = tid; p < pieces; p += WK * 64) {
            uint4_t raw;
            asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(raw) : "v"(hrow + p * 8) : "memory");
            const half8_t hv = __builtin_bit_cast(half8_t, raw);
            const float4_t g0 = *reinterpret_cast<const float4_t *>(out_gamma_ + p * 8), g1 = *reinterpret_cast<const float4_t *>(out_gamma_ + p * 8 + 4);
            half8_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = rmsnorm_out(hv[e], rs, g0[e]);
                o[4 + e] = rmsnorm_out(hv[4 + e], rs, g1[e]);
            }
            *reinterpret_cast<half8_t *>(xn_out_ + p * 8) = o;
        }
    }
}

// The ordinary launch: flat arguments (the layout and the reason: above I8SegHead).  MB rows per pass ... as the body.
template <int MB, int GPU, int ROWS, int UW, bool Z8, int MAXT, bool NORM = false, bool RNORM = false, int COMB = 0, bool STAMPS = false>
__global__ __launch_bounds__(MAXT) void w4a16_gemv_i8_kernel(const void *words, int bytes_w, int U, const void *A_, int lda, int K, const void *dscales_, int bytes_s, int N, int M,
                                                            int geom, const I8Tail t) {
    // (A, dscales: fp16; untyped in the signature so that every demangler in use can print the kernel's name)
    const half_t *A = static_cast<const half_t *>(A_), *dscales = static_cast<const half_t *>(dscales_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_wg[];
    I8Stamps st;
    if constexpr (STAMPS) {
        st.t[0] = __builtin_amdgcn_s_memrealtime();
        st.t[5] = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
    }
    const int WK = geom & 0xFF, nseg = (geom >> 8) & 0xFF, nmem = geom >> 16;
    int si = 0, block_begin = 0;
    if (nseg > 1) {
        // a grouped launch (q/k/v, gate+up): every further linear's addressing fields in ONE batch of scalar loads, the workgroup's own by scalar selects
        static_assert(TCE_MAX_GROUP == 4, "the batch below names three further linears");
        I8SegHead h[TCE_MAX_GROUP - 1] = {t.head[0], t.head[1], t.head[2]};
        // (all 24 dwords requested before the first select: left alone the compiler asks for the third linear's behind the wait for the first two -- a second round trip)
        asm volatile("" : "+s"(h[0].words), "+s"(h[0].dscales), "+s"(h[0].bytes_w), "+s"(h[0].bytes_s), "+s"(h[0].N), "+s"(h[0].block_begin),
                          "+s"(h[1].words), "+s"(h[1].dscales), "+s"(h[1].bytes_w), "+s"(h[1].bytes_s), "+s"(h[1].N), "+s"(h[1].block_begin),
                          "+s"(h[2].words), "+s"(h[2].dscales), "+s"(h[2].bytes_w), "+s"(h[2].bytes_s), "+s"(h[2].N), "+s"(h[2].block_begin));
#pragma unroll
        for (int s = 1; s < TCE_MAX_GROUP; ++s) {
            const bool mine = s < nseg && (int)blockIdx.x >= h[s - 1].block_begin;
            si = mine ? s : si;
            words = mine ? h[s - 1].words : words;
            dscales = mine ? h[s - 1].dscales : dscales;
            bytes_w = mine ? h[s - 1].bytes_w : bytes_w;
            bytes_s = mine ? h[s - 1].bytes_s : bytes_s;
            N = mine ? h[s - 1].N : N;
            block_begin = mine ? h[s - 1].block_begin : block_begin;
        }
    }
    const I8SegRest &r = t.rest[si];
    const I8Seg seg{words, dscales, r.dzeros, r.C, N, r.ldc, r.epilogue, bytes_w, bytes_s, r.bytes_z, block_begin};
    w4a16_gemv_i8_body<MB, GPU, ROWS, UW, Z8, NORM, RNORM, COMB, false, I8Tail, STAMPS>(t, smem_wg, (int)threadIdx.x, WK, U, K, lda, M, A, seg, ((int)blockIdx.x - block_begin) * ROWS, false, 0u, &st, nmem);
}

// The mixed launch (I8MixArgs, above): the linear, its activation and k range per WORKGROUP, the tile per wave group.  Its arguments stay one struct by value (P > 1
// plans only; not on the single-GPU token's path).
template <bool Z8>
__global__ __launch_bounds__(1024) void w4a16_gemv_i8_mixed_kernel(const I8MixArgs args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_wg[];
    unsigned char *smem = smem_wg;
    int tid = threadIdx.x;
    int si = 0;
#pragma unroll
    for (int s = 1; s < kI8MixMax; ++s)
        if (s < args.nseg && (int)blockIdx.x >= args.s[s].seg.block_begin) si = s;
    const half_t *A_ = args.s[si].A;
    const int lda_ = args.s[si].lda;
    const int K_ = args.s[si].K;
    const I8Seg seg = args.s[si].seg;
    const int U = K_ >> 7;
    const int wl = blockDim.x >> 6;                  // waves of the launch's workgroups
    const int WK = (U + 8 - 1) / 8;                  // waves that split THIS linear's K
    const int nsub = wl / WK;                        // its tiles per workgroup
    const int sub = __builtin_amdgcn_readfirstlane(tid >> 6) / WK;
    const int tile0 = ((int)blockIdx.x - seg.block_begin) * nsub + sub;
    if (sub >= nsub || tile0 >= ((seg.N + 15) >> 4)) return;  // (whole wave groups: the barrier of the K reduction counts the surviving waves)
    tid -= sub * WK * 64;
    smem += (size_t)sub * ((size_t)WK * 8 * 512 + (size_t)WK * 16 * sizeof(float));
    const bool gathers = si == args.g_seg;  // this workgroup's linear is the one whose slice is exchanged inside the launch
    // the exchange's epoch: the slot's count of completed exchanges + 1 (the same on every rank: they all run the same sequence per slot)
    // (read before any tile of this launch can have counted itself in: the word changes only after ALL of them have)
    unsigned g_epoch = 0;
    if (gathers) g_epoch = __hip_atomic_load(args.g.epochs + args.g.slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    w4a16_gemv_i8_body<1, 1, 1, 8, Z8, false, false, 0, true>(args, smem, tid, WK, U, K_, lda_, args.M, A_, seg, tile0, gathers, g_epoch);
}

static int i8_units_per_wave(int U) { return U <= 128 ? 8 : (U <= 256 ? 16 : 0); }
thread_local int g_i8_mode = 0;  // 0 automatic (wherever the shape allows and a packed copy is given), 1 off
thread_local int g_i8_rows = 0;  // 0 the rule, 1 / 2 forced tiles per wave
thread_local unsigned long long *g_i8_stamps = nullptr;  // lab build: the plain M = 1 / G = 128 / zero-point-8 launches run the stamped form and write [workgroup][8] readings here

// host side: the leading parameters of a launch and its tail
struct I8Launch {
    const void *words;
    const half_t *dscales, *A;
    int bytes_w, bytes_s, U, lda, K, N, M, nseg, nmem;
    I8Tail t;
};

template <int MB, int GPU, int ROWS, int UW, bool Z8, int MAXT, bool NORM = false, bool RNORM = false, int COMB = 0, bool STAMPS = false>
hipError_t launch_i8(const I8Launch &a, int blocks, int m_blocks, int wk, hipStream_t stream) {
    const size_t lds = (size_t)wk * UW * MB * 512 + (size_t)wk * ROWS * MB * 16 * sizeof(float) + (NORM ? (size_t)(a.K >> 3) * sizeof(float) + 1024 : 0)  // the row's piece sums (+ the ragged last wave's zero pieces)
                       + (i8_ring_staging(MB, GPU, false, COMB) ? kI8ZeroBlock : 0);                                                           // the ring's blocks of zeros, last
    auto kfn = w4a16_gemv_i8_kernel<MB, GPU, ROWS, UW, Z8, MAXT, NORM, RNORM, COMB, STAMPS>;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kfn, dim3(blocks, m_blocks, 1), dim3(64 * wk, 1, 1), lds, stream, a.words, a.bytes_w, a.U, static_cast<const void *>(a.A), a.lda, a.K, static_cast<const void *>(a.dscales), a.bytes_s, a.N, a.M, wk | (a.nseg << 8) | (a.nmem << 16), a.t);
    return hipGetLastError();
}

}  // namespace

// rows of A per pass of the weights: 1 / 2 / 4, bounded by the sixteen columns of the MFMA and by the digit planes fitting LDS twice per CU (M = 4 at K = 11008 / 14336:
// one row per pass).  ONE rule for the launcher and for tce_w4a16_describe_dispatch.
int gemv_i8_rows_per_pass(int M, int K, int group_size) {
    const int U = K / 128, gpu = 128 / group_size;
    const int uw = i8_units_per_wave(U);
    const int wk = (U + uw - 1) / uw;
    int mb = M >= 3 ? 4 : M;
    while (mb > 1 && (mb * gpu > 4 || (size_t)wk * uw * mb * 512 > 72 * 1024)) mb >>= 1;
    return mb;
}

void set_gemv_i8_stamps(void *buf) { g_i8_stamps = static_cast<unsigned long long *>(buf); }

void set_gemv_i8_mode(int mode, int rows) {
    g_i8_mode = mode == 1 ? 1 : 0;
    g_i8_rows = rows == 1 || rows == 2 ? rows : 0;
}

// units per wave: a function of K (and of the rows / groups per pass) ONLY, so that a row's arithmetic does not depend on N

bool gemv_i8_supports(const tce_w4a16_desc *descs, int count, bool with_norm) {
    if (g_i8_mode == 1) return false;
    const tce_w4a16_desc &d0 = descs[0];
    if (d0.M < 1 || d0.M > 4 || d0.K % 128 != 0) return false;
    if ((d0.rmsnorm_gamma || with_norm) && (d0.M != 1 || d0.group_size != 128 || d0.K > 16384)) return false;  // the fused RMSNorm prologue: decode rows, groups of 128
    if (d0.group_size != 128 && d0.M > (d0.group_size == 64 ? 2 : 1)) return false;
    const int uw = i8_units_per_wave(d0.K / 128);
    if (uw == 0 || (uw == 16 && (d0.M > 1 || d0.group_size != 128))) return false;  // (very long K: single rows only -- the registers hold 16 KiB of weights per wave)
    for (int i = 0; i < count; ++i) {
        const tce_w4a16_desc &d = descs[i];
        if (!d.prepacked || (reinterpret_cast<uintptr_t>(d.prepacked) & 255) || !pk::group_member_ok(d.N, d.reserved, d.reserved2)) return false;
        if ((long long)pk::nt16(d.N) * (d.K / 2) * 16 >= (1LL << 31)) return false;  // buffer descriptors address 32-bit byte offsets
        if (d.flags & TCE_W4_FORCE_GEMM) return false;
    }
    return true;
}

// > 0: the `count` (> 1) linears are members of ONE group copy (tce_w4a16_prepack_group), named in the copy's order with consecutive tile ranges -- the launch addresses
// them as one linear (the count is returned); 0: today's grouped launch, every linear through its own addressing fields (individual copies, or members out of order / with a gap)
int gemv_i8_group_copy_members(const tce_w4a16_desc *descs, int count) {
    if (count < 2 || count > TCE_MAX_GROUP || descs[0].reserved2 <= 0) return 0;
    long long tiles = 0;
    for (int i = 0; i < count; ++i) {
        const tce_w4a16_desc &d = descs[i];
        if (d.prepacked != descs[0].prepacked || d.reserved2 != descs[0].reserved2 || !pk::group_member_ok(d.N, d.reserved, d.reserved2)) return 0;
        if (i > 0 && d.reserved != descs[i - 1].reserved + descs[i - 1].N / 16) return 0;
        tiles += d.N / 16;
    }
    if (tiles * (descs[0].K / 2) * 16 >= (1LL << 31)) return 0;  // (the whole range behind one buffer descriptor)
    return count;
}

int launch_w4a16_gemv_i8(const tce_w4a16_desc *descs, int count, hipStream_t stream, hipError_t *hip_err, const float *gamma, float eps, const I8ResidualNorm *rn,
                         const AttnDeferred *comb, const int *comb_pos_dev, int comb_pos) {
    const tce_w4a16_desc &d0 = descs[0];
    if (!gamma && d0.rmsnorm_gamma) {
        gamma = static_cast<const float *>(d0.rmsnorm_gamma);
        eps = d0.rmsnorm_eps;
    }
    I8Launch a{};
    a.t.gamma = gamma;
    a.t.eps = eps;
    a.A = static_cast<const half_t *>(d0.A);
    a.lda = d0.lda ? d0.lda : d0.K;
    a.M = d0.M;
    a.K = d0.K;
    a.U = d0.K / 128;
    a.nseg = count;
    const int gpu = 128 / d0.group_size;
    const int uw = i8_units_per_wave(a.U);
    const int wk = (a.U + uw - 1) / uw;
    bool z8 = true;
    long long total_tiles = 0;
    for (int i = 0; i < count; ++i) {
        z8 = z8 && (descs[i].flags & TCE_W4_ZERO_POINT_IS_8);
        total_tiles += pk::nt16(descs[i].N);
    }
    const int mb = gemv_i8_rows_per_pass(d0.M, d0.K, d0.group_size);
    const int m_blocks = (d0.M + mb - 1) / mb;
    // tiles per wave: one.  Two (the conversion of x amortised over twice the bytes, one generation of workgroups for the gate+up launch) measured slower on every
    // launch of the token (profiles/r4/gemv_i8_ab.jsonl: qkv 6.6 -> 7.4 us, o 3.9 -> 4.5, gate+up 9.9 -> 10.2, down a tie); compiled, forceable (tce_w4a16_set_gemv_i8)
    // With the RMSNorm prologue -- x, gamma, the piece sums and the normalisation on top of the conversion, all per wave -- two tiles per wave win where one tile per
    // workgroup leaves a short second generation of workgroups behind the resident ones (256 CUs x 20 waves at five per SIMD: 1280 four-wave workgroups): norm + gate/up of
    // a 4096 x 11008 layer, 1376 tiles, 11.84 -> 11.31 us.  Elsewhere one tile per wave is level or ahead (scripts/probes/norm_tiles_ab.py: 768 tiles 7.1 / 8.3 us,
    // 1024: 8.65 / 9.04, 1280: 10.4 / 11.1, 1536: 11.6 / 11.75, 1792: 12.9 / 13.5, 2000: 14.2 / 14.0, 8016: 43.3 / 43.8).  (The tile count per wave does not enter
    // the arithmetic: same bits.)
    int rows = 1;
    const bool two_ok = mb == 1 && gpu == 1 && uw == 8 && wk <= 8;
    // Those figures are of the prologue kernel at five waves per SIMD.  With the B operand staged two units deep (section 3 of the body) it holds seven, and all of the
    // window's workgroups are resident at once -- and two tiles per wave STILL win there (profiles/decode_occupancy/norm_tiles_ab.jsonl, one tile / two tiles:
    // 1280 tiles 10.28 / 10.48 us, 1376: 11.26 / 10.77, 1536: 11.68 / 11.35, 1792: 13.17 / 13.19): what they save is the conversion per byte, not a generation.  The
    // window is a measured one and stays as it is; `resident` is its anchor, no longer the number of workgroups the chip holds.
    const long long resident = 256LL * (20 / wk);
    if (gamma && two_ok && total_tiles > resident && total_tiles * 5 <= resident * 6) rows = 2;
    if (g_i8_rows && two_ok) rows = g_i8_rows;
    // members of ONE group copy, in the copy's order and without a gap: the launch is one linear of their rows together (gemv_i8_group_copy_members)
    const bool shared = gemv_i8_group_copy_members(descs, count) > 0;
    int blocks = 0;
    for (int i = 0; i < count; ++i) {
        const tce_w4a16_desc &d = descs[i];
        const unsigned char *base = static_cast<const unsigned char *>(d.prepacked);
        const pk::PackedView pv = pk::packed_view(d.N, d.K, d.group_size, d.reserved, d.reserved2);  // (a member of a group copy: its slice of every part)
        I8SegHead h{};
        h.words = base + pv.words;
        h.dscales = reinterpret_cast<const half_t *>(base + pv.dscales);
        h.bytes_w = (int)pk::words_bytes(d.N, d.K);
        h.bytes_s = (int)pk::dscales_bytes(d.N, d.K, d.group_size);
        h.N = d.N;
        h.block_begin = blocks;
        if (i == 0) {  // linear 0: the leading (preloaded) parameters
            a.words = h.words;
            a.dscales = h.dscales;
            a.bytes_w = h.bytes_w;
            a.bytes_s = h.bytes_s;
            a.N = h.N;
        } else {
            a.t.head[i - 1] = h;
        }
        I8SegRest &r = a.t.rest[i];
        r.C = static_cast<half_t *>(d.C);
        r.dzeros = reinterpret_cast<const unsigned *>(base + pv.dzeros);
        r.epilogue = d.flags & (TCE_W4_SILU_MUL_PAIRS | TCE_W4_ADD_TO_C);
        r.ldc = d.ldc ? d.ldc : ((r.epilogue & TCE_W4_SILU_MUL_PAIRS) ? d.N / 2 : d.N);
        r.bytes_z = (int)pk::dzeros_bytes(d.N, d.K, d.group_size);
        blocks += (pk::nt16(d.N) + rows - 1) / rows;
    }
    for (int i = count; i < TCE_MAX_GROUP; ++i) {  // (never chosen: the kernel's selects stop at the launch's count)
        a.t.rest[i] = a.t.rest[0];
        a.t.head[i - 1] = I8SegHead{a.words, a.dscales, a.bytes_w, a.bytes_s, a.N, 0};
    }
    if (shared) {
        // member 0's slices are where the launch's rows begin; the sizes become those of all members' rows, the workgroups walk their tiles as one range
        const int rows_all = (int)total_tiles * 16;
        a.nseg = 1;
        a.nmem = count;
        a.N = rows_all;
        a.bytes_w = (int)pk::words_bytes(rows_all, d0.K);
        a.bytes_s = (int)pk::dscales_bytes(rows_all, d0.K, d0.group_size);
        a.t.rest[0].bytes_z = (int)pk::dzeros_bytes(rows_all, d0.K, d0.group_size);
        for (int i = 0; i < TCE_MAX_GROUP; ++i) a.t.mtile[i] = i < count ? descs[i].reserved - d0.reserved : 0;
        blocks = (int)((total_tiles + rows - 1) / rows);
    }
    hipError_t e = hipErrorInvalidConfiguration;
    if (rn) {  // residual add + the next RMSNorm: one decode row, one linear, groups of 128, N <= 16384 (the 2048 slots of the order)
        if (count != 1 || gamma || mb != 1 || gpu != 1 || d0.M != 1 || !(d0.flags & TCE_W4_ADD_TO_C) || d0.N > 16384 || d0.N % 8 != 0) return TCE_ERR_UNSUPPORTED_SHAPE;
        a.t.out_gamma = rn->gamma;
        a.t.out_eps = rn->eps;
        a.t.xn_out = static_cast<half_t *>(rn->xn_out);
        a.t.ws = static_cast<float *>(rn->workspace);
        if (uw == 8) e = z8 ? launch_i8<1, 1, 1, 8, true, 1024, false, true>(a, blocks, m_blocks, wk, stream) : launch_i8<1, 1, 1, 8, false, 1024, false, true>(a, blocks, m_blocks, wk, stream);
        else if (z8) e = launch_i8<1, 1, 1, 16, true, 1024, false, true>(a, blocks, m_blocks, wk, stream);
        else return TCE_ERR_UNSUPPORTED_SHAPE;  // K > 16384 with general zero points: the epilogue's registers on top of 16 KiB of weights per wave and the zero-point chain do not fit 128 (the form spilled; no instantiation spills: build.py NO_VGPR_SPILL)
        if (e != hipSuccess) {
            if (hip_err) *hip_err = e;
            return TCE_ERR_HIP;
        }
        return TCE_OK;
    }
    if (comb && comb->slots > 1) {  // the activation row = a deferred attention step's partial states (one decode row, one linear, groups of 128, K = heads x 128 in whole 1024-k waves)
        if (count != 1 || gamma || mb != 1 || gpu != 1 || uw != 8 || d0.M != 1 || d0.K != comb->heads * 128 || d0.K % 1024 != 0 || comb->slots > kAttnDeferMaxSlots || comb->stride != 132)
            return TCE_ERR_UNSUPPORTED_SHAPE;
        a.t.comb_part = comb->part;
        a.t.comb_pos_dev = comb_pos_dev;
        a.t.comb_pos = comb_pos;
        a.t.comb_slots = comb->slots;
        a.t.comb_chunk = comb->chunk;
        a.t.comb_stride = comb->stride;
        a.t.comb_heads = comb->heads;
        // (compiled for at most four waves -- K <= 4096, the 7B / 8B widths --: eight slots of partial states in flight beside the wave's weights need more registers than
        //  sixteen waves per CU leave)
        if (wk > 4) return TCE_ERR_UNSUPPORTED_SHAPE;
        if (comb->slots <= 4) e = z8 ? launch_i8<1, 1, 1, 8, true, 256, false, false, 4>(a, blocks, m_blocks, wk, stream) : launch_i8<1, 1, 1, 8, false, 256, false, false, 4>(a, blocks, m_blocks, wk, stream);
        else e = z8 ? launch_i8<1, 1, 1, 8, true, 256, false, false, 8>(a, blocks, m_blocks, wk, stream) : launch_i8<1, 1, 1, 8, false, 256, false, false, 8>(a, blocks, m_blocks, wk, stream);
        if (e != hipSuccess) {
            if (hip_err) *hip_err = e;
            return TCE_ERR_HIP;
        }
        return TCE_OK;
    }
    if (gamma) {
        if (mb != 1 || gpu != 1 || uw != 8) return TCE_ERR_UNSUPPORTED_SHAPE;
        if (rows == 2) e = z8 ? launch_i8<1, 1, 2, 8, true, 512, true>(a, blocks, m_blocks, wk, stream) : launch_i8<1, 1, 2, 8, false, 512, true>(a, blocks, m_blocks, wk, stream);
        else e = z8 ? launch_i8<1, 1, 1, 8, true, 1024, true>(a, blocks, m_blocks, wk, stream) : launch_i8<1, 1, 1, 8, false, 1024, true>(a, blocks, m_blocks, wk, stream);
        if (e != hipSuccess) {
            if (hip_err) *hip_err = e;
            return TCE_ERR_HIP;
        }
        return TCE_OK;
    }
#ifdef TCE_LAB  // (the stamped instantiation: the lab build, build.py --lab)
    if (g_i8_stamps && z8 && mb == 1 && gpu == 1 && rows == 1 && uw == 8) {
        a.t.dbg = g_i8_stamps;
        e = launch_i8<1, 1, 1, 8, true, 1024, false, false, 0, true>(a, blocks, m_blocks, wk, stream);
        if (e != hipSuccess) {
            if (hip_err) *hip_err = e;
            return TCE_ERR_HIP;
        }
        return TCE_OK;
    }
#endif
#define TCE_I8(MB_, GPU_, ROWS_, UW_, MAXT_)                                                                                        \
    if (mb == MB_ && gpu == GPU_ && rows == ROWS_ && uw == UW_) {                                                                   \
        e = z8 ? launch_i8<MB_, GPU_, ROWS_, UW_, true, MAXT_>(a, blocks, m_blocks, wk, stream)                                     \
               : launch_i8<MB_, GPU_, ROWS_, UW_, false, MAXT_>(a, blocks, m_blocks, wk, stream);                                   \
    } else
    TCE_I8(1, 1, 1, 8, 1024)
    TCE_I8(1, 1, 2, 8, 512)
    TCE_I8(1, 1, 1, 16, 1024)
    TCE_I8(2, 1, 1, 8, 1024)
    TCE_I8(4, 1, 1, 8, 1024)
    TCE_I8(1, 2, 1, 8, 1024)
    TCE_I8(2, 2, 1, 8, 1024)
    TCE_I8(1, 4, 1, 8, 1024)
    return TCE_ERR_UNSUPPORTED_SHAPE;
#undef TCE_I8
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

// ---- the mixed launch: up to TCE_MAX_INDEPENDENT decode linears with their own activations and K as ONE launch (w4a16_gemv_i8_mixed_kernel) ----
static_assert(kI8MixMax == TCE_MAX_INDEPENDENT, "include/tce_matmul.h");

bool gemv_i8_mixed_supports(const tce_w4a16_desc *descs, int count) {
    if (g_i8_mode == 1 || count < 1 || count > kI8MixMax) return false;
    for (int i = 0; i < count; ++i) {
        const tce_w4a16_desc &d = descs[i];
        // one decode row, groups of 128, eight units per wave (K <= 16384), no prologue: the <1, 1, 1, 8> body
        if (d.M != 1 || d.group_size != 128 || d.K % 128 != 0 || d.K > 16384 || d.rmsnorm_gamma) return false;
        if (!d.prepacked || (reinterpret_cast<uintptr_t>(d.prepacked) & 255) || !pk::group_member_ok(d.N, d.reserved, d.reserved2)) return false;
        if ((long long)pk::nt16(d.N) * (d.K / 2) * 16 >= (1LL << 31)) return false;
        if (d.flags & TCE_W4_FORCE_GEMM) return false;
    }
    return true;
}

// workgroups of the mixed launch and the waves of each (what tce_w4a16_forward_independent reports through describe; ONE rule with the launcher)
thread_local int g_i8_mix_waves = 0;  // tuning: waves per workgroup of the mixed launch forced (>= what the longest K needs; 0: the rule)
void set_gemv_i8_mixed_waves(int w) { g_i8_mix_waves = w >= 1 && w <= 16 ? w : 0; }

void gemv_i8_mixed_geometry(const tce_w4a16_desc *descs, int count, int *waves, int *workgroups) {
    // (a host issues the same block shapes launch after launch: the last answer is kept per thread)
    struct Memo {
        int count = 0, forced = -1, n[kI8MixMax], k[kI8MixMax], waves = 0, workgroups = 0;
    };
    thread_local Memo memo;
    bool hit = memo.count == count && memo.forced == g_i8_mix_waves;
    for (int i = 0; i < count && hit; ++i) hit = memo.n[i] == descs[i].N && memo.k[i] == descs[i].K;
    if (hit) {
        *waves = memo.waves;
        *workgroups = memo.workgroups;
        return;
    }
    int need = 1;
    for (int i = 0; i < count; ++i) need = need > (descs[i].K / 128 + 7) / 8 ? need : (descs[i].K / 128 + 7) / 8;
    auto blocks_at = [&](int wl) {
        int blocks = 0;
        for (int i = 0; i < count; ++i) {
            const int nsub = wl / ((descs[i].K / 128 + 7) / 8);
            blocks += (pk::nt16(descs[i].N) + nsub - 1) / nsub;
        }
        return blocks;
    };
    // The workgroup is at least as wide as the longest K needs and at most 16 waves.  What a width costs is the most loaded CU -- workgroups go to the 256 CUs in
    // index order, a workgroup's bytes are its live waves' 8 KiB each -- and, between widths that load it alike (within 5 %), the number of workgroups.  Fitted to
    // profiles/r6/mixed_block_waves_sweep.jsonl (a Llama-3-8B block's shards at 8 / 4 / 2 / 1 ranks: 14 waves 6.29 / 11.08 / 16.45 / 26.26 us, 16 waves 6.66 / 7.89 / 13.73 /
    // 24.71; Llama-2-13B: 14 waves 7.01 / 11.4 / 20.07 / 36.3, 15 waves 6.98 / 12.0 / 18.03 / 33.4): the rule picks the faster (or a tie) in all eight.
    // (workgroups b0 .. b0 + n - 1 of a linear go to CUs b0 % 256 ...: every CU gets n / 256 of them, the first n % 256 from b0 on one more; the linear's last workgroup may
    //  carry fewer tiles -- O(256) per linear, not O(tiles): this runs on the launch path)
    auto max_load = [&](int wl) {
        int load[256] = {0};
        int b0 = 0;
        for (int i = 0; i < count; ++i) {
            const int wk = (descs[i].K / 128 + 7) / 8, nsub = wl / wk, tiles = pk::nt16(descs[i].N);
            const int n = (tiles + nsub - 1) / nsub, units = nsub * wk, last_units = (tiles - (n - 1) * nsub) * wk;
            const int every = n / 256, extra = n % 256;
            for (int c = 0; c < 256; ++c) load[c] += every * units;
            for (int e = 0; e < extra; ++e) load[(b0 + every * 256 + e) & 255] += units;
            load[(b0 + n - 1) & 255] -= units - last_units;
            b0 += n;
        }
        int worst = 0;
        for (int c = 0; c < 256; ++c) worst = worst > load[c] ? worst : load[c];
        return worst;
    };
    int best_load = 1 << 30;
    for (int w = need; w <= 16; ++w) best_load = best_load < max_load(w) ? best_load : max_load(w);
    int wl = need;
    long best_blocks = 1L << 40;
    for (int w = need; w <= 16; ++w)
        if (max_load(w) * 20 <= best_load * 21 && blocks_at(w) < best_blocks) best_blocks = blocks_at(w), wl = w;
    if (g_i8_mix_waves >= need) wl = g_i8_mix_waves;
    *waves = wl;
    *workgroups = blocks_at(wl);
    memo.count = count;
    memo.forced = g_i8_mix_waves;
    for (int i = 0; i < count; ++i) memo.n[i] = descs[i].N, memo.k[i] = descs[i].K;
    memo.waves = wl;
    memo.workgroups = *workgroups;
}

int launch_w4a16_gemv_i8_mixed(const tce_w4a16_desc *descs, int count, hipStream_t stream, hipError_t *hip_err, const PeerGatherEpi *gather, int gathered) {
    if (!gemv_i8_mixed_supports(descs, count)) return TCE_ERR_UNSUPPORTED_SHAPE;
    I8MixArgs a{};
    a.nseg = count;
    a.M = 1;
    if (gather) {  // linear `gathered`'s slice is exchanged inside the launch: plain or residual-add store (the pair epilogue halves the row index), the slice is the whole linear
        if (gathered < 0 || gathered >= count) return TCE_ERR_BAD_ARG;
        const tce_w4a16_desc &dg = descs[gathered];
        if ((dg.flags & TCE_W4_SILU_MUL_PAIRS) || (unsigned)dg.N != gather->slice_elems) return TCE_ERR_UNSUPPORTED_SHAPE;
        a.g = *gather;
        a.g_seg = gathered;
        a.g_tiles = (unsigned)pk::nt16(dg.N);
    }
    int wl = 1, total = 0;
    gemv_i8_mixed_geometry(descs, count, &wl, &total);
    bool z8 = true;
    int blocks = 0;
    for (int i = 0; i < count; ++i) {
        const tce_w4a16_desc &d = descs[i];
        z8 = z8 && (d.flags & TCE_W4_ZERO_POINT_IS_8);
        I8MixSeg &m = a.s[i];
        m.A = static_cast<const half_t *>(d.A);
        m.lda = d.lda ? d.lda : d.K;
        m.K = d.K;
        I8Seg &s = m.seg;
        const unsigned char *base = static_cast<const unsigned char *>(d.prepacked);
        const pk::PackedView pv = pk::packed_view(d.N, d.K, d.group_size, d.reserved, d.reserved2);  // (a member of a group copy: its slice of every part)
        s.words = base + pv.words;
        s.dscales = reinterpret_cast<const half_t *>(base + pv.dscales);
        s.dzeros = reinterpret_cast<const unsigned *>(base + pv.dzeros);
        s.C = static_cast<half_t *>(d.C);
        s.N = d.N;
        s.epilogue = d.flags & (TCE_W4_SILU_MUL_PAIRS | TCE_W4_ADD_TO_C);
        s.ldc = d.ldc ? d.ldc : ((s.epilogue & TCE_W4_SILU_MUL_PAIRS) ? d.N / 2 : d.N);
        s.bytes_w = (int)pk::words_bytes(d.N, d.K);
        s.bytes_s = (int)pk::dscales_bytes(d.N, d.K, d.group_size);
        s.bytes_z = (int)pk::dzeros_bytes(d.N, d.K, d.group_size);
        s.block_begin = blocks;
        const int nsub = wl / ((d.K / 128 + 7) / 8);
        blocks += (pk::nt16(d.N) + nsub - 1) / nsub;
    }
    for (int i = count; i < kI8MixMax; ++i) a.s[i] = a.s[0];
    const size_t lds = (size_t)wl * 8 * 512 + (size_t)wl * 16 * sizeof(float);  // the wave groups' regions side by side: never more than `wl` waves' worth
    auto launch = [&](auto kfn) -> hipError_t {
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kfn, dim3(blocks, 1, 1), dim3(64 * wl, 1, 1), lds, stream, a);
        return hipGetLastError();
    };
    const hipError_t e = z8 ? launch(w4a16_gemv_i8_mixed_kernel<true>) : launch(w4a16_gemv_i8_mixed_kernel<false>);
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace tce
