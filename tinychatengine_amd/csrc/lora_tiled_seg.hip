// lora_tiled_seg.hip -- the SEGMENTED tiled expands (include/tce_matmul.h, "Multi-LoRA", THE SEGMENTED TILED EXPANDS: tce_lora_expand_silu_mul_tiled_f16,
// tce_lora_expand_add_segmented_tiled_f16), gfx950.  Both stand behind tce_lora_shrink_tiled_f16 and are lora_tiled.hip's expand with ONE change: a column tile walks only
// the rows of B, and the columns of t, that belong to ITS columns -- where the pool's layout puts zeros for every other j, lora_tiled.hip's expand loads, converts and
// multiplies them.
//
//     gate/up     g = fp16(fmaf(scale[a], sum_{j < R} t[i][j]     * Bg[a][j][n], float(y[i][2n])))        t fp32 [rows][2R]: the shrink of gate's and up's As stacked
//                 u = fp16(fmaf(scale[a], sum_{j < R} t[i][R + j] * Bu[a][j][n], float(y[i][2n + 1])))    y fp16 [rows][2N], only read
//                 C[i][n] = silu_mul_half(g, u)             for EVERY row below `rows`; a row whose word names no adapter takes g and u from y as they are
//     segmented   C[i][n] = fp16(fmaf(scale[a], sum_{j in block s} t[i][j] * B[a][j][n], float(C[i][n])))   n in [seg_cols[s], seg_cols[s + 1]), block s = R / segments rows of B
//
// One kernel body, two instantiations.  256 threads = 4 waves, a tile of kTileRows = 32 rows, the tile's distinct adapters walked by ballot (lora_tiled.hpp), t formed from
// the K slices in slice order while it is staged -- all as in lora_tiled.hip.  A workgroup stages chunks of 64 j x 128 fp32 columns of its adapter (the same LDS footprint
// and the same request view, four 16-byte pieces per thread, the next chunk's requests in flight under the MFMAs) and a wave holds acc[2 row blocks][2 column blocks]:
//   SEGMENTED  the 128 staged columns are 128 columns of C; the workgroup finds the segment its tile lies in (bounds are multiples of 128, so a tile never straddles
//     two) and stages that block's R / segments columns of t alone.  Wave w: staged columns 32 w + 16 cb + r16.
//   GATE/UP    the 128 staged columns are 64 columns of Bg beside the SAME 64 columns of Bu: the workgroup's tile is 64 ffn columns = 128 contiguous halves of a row of y.
//     t is staged whole, [32][2R + 4].  Wave w owns ffn columns 16 w .. 16 w + 15 for gate (cb 0: staged column 16 w + r16, t columns j) and for up (cb 1: staged column
//     64 + 16 w + r16, t columns R + j).  B's columns are on the MFMA's M side, so lane (r16, kq) ends with ffn columns 4 kq .. 4 kq + 3 of row r16 for BOTH g and u: ONE
//     16-byte load of y (the 8 interleaved halves), two fmaf + one rounding per pair, four silu_mul_half, ONE 8-byte store.  The tile's rows that no pass covered (a word
//     outside [0, n), row < rows) take the same epilogue without the fmaf in a last step; a tile of such rows does only that -- no LDS, no barrier, nothing of the pool.
// The sums: v_mfma_f32_16x16x4_f32 from +0, j ascending in super-steps of 8 (lane group kq on j0 + 2 kq, then j0 + 2 kq + 1) -- lora_tiled.hip's order, begun at the
// block's first j.  A block begins at a multiple of 8, so for finite t the result is BIT-IDENTICAL to tce_lora_expand_add_tiled_f16 on the block-structured B (every
// product it adds beyond these is an exact zero, and the accumulator began at +0) -- GIVEN that kernel's rounding to fp16, which is not the same for every column: see
// silu_mul_store.  No atomics; a row's bits depend on that row's y / C, its partials, its adapter, K and R.
// Built like lora_tiled.hip: no packed fp32 arithmetic, -ffp-contract=off.  On the disassembly: gate/up 91 VGPRs + 16 AGPRs, segmented 84 + 16, no scratch
// (build.py NO_VGPR_SPILL); LDS at most 59904 B, inside a kernel's default, two workgroups per CU; the js loop carries no unroll pragma (the compiler refused 2).
#include "lora_tiled.hpp"

namespace tce {

int lora_tiled_slices(int K);  // lora_tiled.hip

namespace {

constexpr int kGateUpCols = kExpandCols / 2;  // ffn columns of a gate/up workgroup
constexpr int kMaxSegments = 4;

struct SegExpandArgs {
    const float *partial;      // [slices][rows][Rt], Rt = 2 R (gate/up) or R
    const half_t *B0, *B1;     // gate/up: Bg, Bu [n][R][N]; segmented: B [n][R][N] and nothing
    const float *scale;
    const int32_t *row_adapter;
    const half_t *y;           // gate/up only
    long long ldy;
    half_t *C;
    long long ldc;
    int rows, N, R, n_adapters, slices;
    int segments;                   // segmented only
    int seg_cols[kMaxSegments + 1];
};

// one lane's four ffn columns of one row: g and u from y's 8 interleaved halves (ADAPTED: with the deltas added), SiLU * mul, one store
template <bool ADAPTED>
__device__ __forceinline__ void silu_mul_store(const half_t *yp, half_t *cp, float sc, float4_t dg, float4_t du) {
    const half8_t yh = __builtin_bit_cast(half8_t, *reinterpret_cast<const uint4_t *>(yp));
    half4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        half_t g = yh[2 * i], u = yh[2 * i + 1];
        if constexpr (ADAPTED) {
            float fg = __builtin_fmaf(sc, dg[i], (float)g), fu = __builtin_fmaf(sc, du[i], (float)u);
            // THE ROUNDING OF lora_tiled.hip's EPILOGUE, column by column.  There a lane's 4 adjacent columns c .. c + 3 (c % 4 == 0) are compiled to v_fma_mixlo/hi_f16
            // for c, c + 1 -- ONE rounding, of the exact sum, to fp16 -- and to v_fma_mix_f32 + v_cvt_pk_f16_f32 for c + 2, c + 3 -- the sum rounded to fp32 FIRST.  The two
            // differ where the fp32 value is a tie of fp16 (measured: 1 element in 20000 .. 70000).  In the interleaved y, ffn column n sits at c = 2n, 2n + 1: an even n
            // is rounded once, an odd n twice.  Here a lane's columns are n = 4 kq + i: odd i keeps fg / fu as fp32 values (the empty asm), which leaves v_cvt_f16_f32;
            // even i is left to the same fold.  Held by tests/test_gpu_lora_tiled_seg.py on both kernels' bits.
            if (i & 1) asm volatile("" : "+v"(fg), "+v"(fu));
            g = (half_t)fg, u = (half_t)fu;
        }
        o[i] = silu_mul_half(g, u);
    }
    *reinterpret_cast<uint2_t *>(cp) = __builtin_bit_cast(uint2_t, o);
}

template <bool SILU>
__global__ __launch_bounds__(kThreads) void lora_expand_seg_tiled_kernel(const SegExpandArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // t [kTileRows][W + 4], then the chunk [kChunkJ][kLdB]
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * kTileRows, n0 = blockIdx.y * (SILU ? kGateUpCols : kExpandCols);
    int seg = 0;
    if constexpr (!SILU) {
#pragma unroll
        for (int s = 1; s < kMaxSegments; ++s) seg += s < a.segments && n0 >= a.seg_cols[s];
    }
    const int R = a.R, N = a.N, rows = a.rows;
    const int Rs = SILU ? R : R / a.segments;  // the j of one sum
    const int Rt = SILU ? 2 * R : R;           // a row of partial
    const int W = SILU ? 2 * R : Rs;           // the columns of t staged: t0 .. t0 + W
    const int t0 = seg * Rs;
    const int ldt = W + 4;
    float *Ts = lds, *Bs = lds + kTileRows * ldt;
    const int nchunks = (Rs + kChunkJ - 1) / kChunkJ;

    unsigned plain = 0;  // gate/up: the tile's rows below `rows` whose word names no adapter
    if constexpr (SILU) {
        const int i = row0 + (tid & 31);
        const int w = i < rows ? a.row_adapter[i] : 0;
        plain = (unsigned)__ballot(i < rows && !(w >= 0 && w < a.n_adapters));
    }

    walk_adapters(a.row_adapter, row0, rows, a.n_adapters, [&](int ad, unsigned same) {
        const half_t *Ba0 = a.B0 + (size_t)ad * R * (size_t)N + (size_t)t0 * N, *Ba1 = SILU ? a.B1 + (size_t)ad * R * (size_t)N : nullptr;
        const float sc = a.scale[ad];
        // request view: piece u of thread t is the 16-byte piece (t + 256 u) % 16 of chunk row (t + 256 u) / 16; gate/up: pieces 0 .. 7 are Bg's, 8 .. 15 Bu's
        uint4_t Bq[4];
        auto request = [&](int c) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + kThreads * u, j = c * kChunkJ + (idx >> 4), p = idx & 15;
                const int n = n0 + (SILU ? p & 7 : p) * 8;
                const half_t *src = SILU && p >= 8 ? Ba1 : Ba0;
                Bq[u] = uint4_t{0u, 0u, 0u, 0u};
                if (j < Rs && n < N) Bq[u] = *reinterpret_cast<const uint4_t *>(src + (size_t)j * N + n);  // (N % 8 == 0: a piece is all inside or all outside)
            }
        };
        auto land = [&]() {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + kThreads * u;
                const half8_t h = __builtin_bit_cast(half8_t, Bq[u]);
                float *dst = Bs + (idx >> 4) * kLdB + (idx & 15) * 8;
                *reinterpret_cast<float4_t *>(dst) = float4_t{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                *reinterpret_cast<float4_t *>(dst + 4) = float4_t{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
            }
        };
        request(0);
        // t of the pass's rows (the staged columns alone), the K slices added in slice order; zeros for the other rows
        for (int e = tid; e < kTileRows * W; e += kThreads) {
            const int row = e / W, j = e - row * W;
            float v = 0.f;
            if ((same >> row) & 1u) {
                const float *p = a.partial + (size_t)(row0 + row) * Rt + t0 + j;
                v = p[0];
                for (int s = 1; s < a.slices; ++s) v += p[(size_t)s * rows * Rt];
            }
            Ts[row * ldt + j] = v;
        }

        float4_t acc[2][2];  // D[staged column + 4 kq + i][row 16 rb + r16], [rb][cb]
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nchunks; ++c) {
            land();
            __syncthreads();
            if (c + 1 < nchunks) request(c + 1);
            const int jn = Rs - c * kChunkJ < kChunkJ ? Rs - c * kChunkJ : kChunkJ;  // a multiple of 8
            const float *tp = Ts + r16 * ldt + c * kChunkJ + 2 * kq, *bp = Bs + 2 * kq * kLdB + (SILU ? wave * 16 : wave * 32) + r16;
            for (int js = 0; js < jn; js += 8) {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    float2 tf[2];  // (segmented: the same pair for both column blocks)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) tf[rb] = *reinterpret_cast<const float2 *>(tp + rb * 16 * ldt + (SILU ? cb * R : 0) + js);
                    const int col = cb * (SILU ? kGateUpCols : 16);
                    const float b0 = bp[js * kLdB + col], b1 = bp[(js + 1) * kLdB + col];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0, tf[rb].x, acc[rb][cb], 0, 0, 0);
                        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1, tf[rb].y, acc[rb][cb], 0, 0, 0);
                    }
                }
            }
            __syncthreads();  // (the next chunk, or the next pass, writes the staged tiles again)
        }

#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            if (!((same >> (rb * 16 + r16)) & 1u)) continue;
            const size_t row = (size_t)(row0 + rb * 16 + r16);
            if constexpr (SILU) {
                const int n = n0 + wave * 16 + 4 * kq;
                if (n < N) silu_mul_store<true>(a.y + row * (size_t)a.ldy + 2 * n, a.C + row * (size_t)a.ldc + n, sc, acc[rb][0], acc[rb][1]);  // (N % 8 == 0: all inside or all outside)
            } else {
                half_t *crow = a.C + row * (size_t)a.ldc;
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const int n = n0 + wave * 32 + cb * 16 + 4 * kq;
                    if (n >= N) continue;
                    uint2_t *cp = reinterpret_cast<uint2_t *>(crow + n);
                    const half4_t ch = __builtin_bit_cast(half4_t, *cp);
                    half4_t o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = (half_t)__builtin_fmaf(sc, acc[rb][cb][i], (float)ch[i]);
                    *cp = __builtin_bit_cast(uint2_t, o);
                }
            }
        }
    });

    if constexpr (SILU) {  // the rows without an adapter: y as it is
        const int n = n0 + wave * 16 + 4 * kq;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            if (!((plain >> (rb * 16 + r16)) & 1u) || n >= N) continue;
            const size_t row = (size_t)(row0 + rb * 16 + r16);
            silu_mul_store<false>(a.y + row * (size_t)a.ldy + 2 * n, a.C + row * (size_t)a.ldc + n, 0.f, float4_t{0.f, 0.f, 0.f, 0.f}, float4_t{0.f, 0.f, 0.f, 0.f});
        }
    }
}

template <bool SILU>
int launch(const SegExpandArgs &a, int staged_t, hipStream_t stream, hipError_t *hip_err) {
    const size_t bytes = ((size_t)kTileRows * (staged_t + 4) + (size_t)kChunkJ * kLdB) * sizeof(float);  // at most 59904 (192 columns of t): inside a kernel's default
    const int cols = SILU ? kGateUpCols : kExpandCols;
    hipLaunchKernelGGL(lora_expand_seg_tiled_kernel<SILU>, dim3((a.rows + kTileRows - 1) / kTileRows, (a.N + cols - 1) / cols), dim3(kThreads), bytes, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace

int launch_lora_expand_silu_mul_tiled_f16(const float *partial, const void *Bg, const void *Bu, const float *scale, const int32_t *row_adapter, const void *y, int ldy, void *C,
                                          int ldc, int rows, int N, int K, int R, int n_adapters, hipStream_t stream, hipError_t *hip_err) {
    SegExpandArgs a{};
    a.partial = partial, a.B0 = static_cast<const half_t *>(Bg), a.B1 = static_cast<const half_t *>(Bu), a.scale = scale, a.row_adapter = row_adapter;
    a.y = static_cast<const half_t *>(y), a.ldy = ldy, a.C = static_cast<half_t *>(C), a.ldc = ldc;
    a.rows = rows, a.N = N, a.R = R, a.n_adapters = n_adapters, a.slices = lora_tiled_slices(K), a.segments = 1;
    return launch<true>(a, 2 * R, stream, hip_err);
}

// seg_cols: segments + 1 bounds, checked by the caller (tce_capi.hip); they travel in the kernel's arguments
int launch_lora_expand_add_segmented_tiled_f16(const float *partial, const void *B, const float *scale, const int32_t *row_adapter, void *C, int ldc, int rows, int N, int K,
                                               int R, int n_adapters, const int *seg_cols, int segments, hipStream_t stream, hipError_t *hip_err) {
    SegExpandArgs a{};
    a.partial = partial, a.B0 = static_cast<const half_t *>(B), a.scale = scale, a.row_adapter = row_adapter, a.C = static_cast<half_t *>(C), a.ldc = ldc;
    a.rows = rows, a.N = N, a.R = R, a.n_adapters = n_adapters, a.slices = lora_tiled_slices(K), a.segments = segments;
    for (int s = 0; s <= segments; ++s) a.seg_cols[s] = seg_cols[s];
    return launch<false>(a, R / segments, stream, hip_err);
}

}  // namespace tce
