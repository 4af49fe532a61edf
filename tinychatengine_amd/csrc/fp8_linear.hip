// fp8_linear.hip -- FP8 (OCP e4m3fn) W8A8 linears with one fp32 scale per token and per output channel (include/tce_matmul.h, "FP8 linears"), gfx950:
// tce_fp8_quantize_rows_f16 and the two forms of tce_w8a8_fp8_forward_f16.  The contraction is v_mfma_f32_16x16x128_f8f6f4 with both formats e4m3 and no scale operand.
//
// The matrix instruction's operands, as this file uses them: lane l holds 32 bytes of operand row (l & 15), the bytes k = 32 (l >> 4) .. + 31 of a 128-byte K step, in
// BOTH operands -- a dot product does not care which k sits in which slot as long as the two operands agree, so the 32 bytes are simply the row's next 32 (two 16-byte
// loads) and no byte is ever shuffled.  The FIRST operand is the weights, the second the activations: D[4 (l >> 4) + r][l & 15] is then C[m = l & 15][n = 4 (l >> 4) + r],
// four consecutive columns of one output row per lane -- one 8-byte store (and one 8-byte load with TCE_W4_ADD_TO_C).  tests/test_gpu_fp8_linear.py's one-hot cases
// pin both statements, bit for bit.
//
//   quantiser   one workgroup per row: the row is read once (16-byte loads, up to 16 per thread: K <= 32768) and stays in registers; |x|'s maximum by a DPP tree in the
//               wave and through LDS across the four waves (a maximum has no order: every thread ends with the same bits); two correctly rounded divisions; bytes by
//               fp8_kv.hpp's fp8_quant1 -- the definition, held for every input by tests/test_gpu_fp8_kv.py --, 8 per store.
//   skinny      M <= 16.  A workgroup of 8 waves owns ONE band of 16 weight rows; wave w contracts the K steps [w S / 8, (w + 1) S / 8) of S = K / 128 -- a function of K
//               alone.  Weights go global -> VGPR in operand order (non-temporal: every byte is used once) and straight into the MFMA, four K steps (128 bytes per
//               lane) requested before the first is used.  The activation operand is rows 0 .. M - 1 (lanes of rows >= M hold zeros): a wave needs only ITS slice of
//               them, once, so it takes the slice global -> VGPR as well -- staging all 16 x K bytes in LDS would put bytes there that one wave reads one time, and does
//               not fit from K = 10240 on.  The waves' 16 x 16 fp32 tiles meet in LDS and wave 0 adds them in wave order, scales and stores.
//   tiled       128 x 128 outputs per workgroup, four waves of 64 x 64 (4 x 4 accumulator tiles); a K step is 128 bytes: a 16 KiB panel per operand, two buffers of
//               both = 64 KiB of LDS.  Step t + 1 is requested into registers (8 x 16 bytes per thread, eight lanes per 128-byte row piece) before step t is contracted
//               and written to the other buffer behind it: one barrier per step.  Fragments come back with two ds_read_b128 per lane; 16-byte chunk c of row r lies at
//               chunk c ^ sw(r), sw(r) = ((r & 7) + (r >> 3 & 1)) & 7 for r = row & 15 -- the 16 rows of a fragment read (stride 128 bytes unswizzled: two bank
//               groups) then cover all sixteen 16-byte bank groups of a 64-bank LDS, and each half of them all eight of a 32-bank one; the writes (a row's eight
//               chunks from eight neighbouring lanes) are a permutation inside the row either way.
// Both forms: acc by the matrix instruction in fp32, K steps ascending, then (acc * sx[m]) * sw[n], two roundings, then binary16 (or float(C) + v first).  No atomics, no
// K cut across workgroups; an output's bits are a function of its own operand rows and K.  The two forms cut K differently (eight slices / one chain) and need not agree.
// Rows past M or N inside a tile are clamped re-reads whose outputs are never stored.  This file is compiled without packed fp32 arithmetic (build.py): the epilogue's
// multiplies are plain v_mul_f32.
#include "fp8_kv.hpp"

namespace tce {

namespace {

typedef int int8v_t __attribute__((ext_vector_type(8)));

constexpr int kQuantThreads = 256, kQuantPieces = 16;  // 16 x 256 pieces of 8 values: K <= 32768
constexpr int kSkWaves = 8, kSkDepth = 4;              // the skinny form: waves per band, K steps in flight per wave
constexpr int kTile = 128, kTiledThreads = 256, kPanelBytes = kTile * 128, kTiledLds = 4 * kPanelBytes;

__device__ __forceinline__ int8v_t operand(const uint4_t lo, const uint4_t hi) {
    return int8v_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// e4m3 x e4m3, no scale operand (both scale arguments the constant 0 select the unscaled instruction)
__device__ __forceinline__ float4_t mfma_e4m3(const int8v_t w, const int8v_t x, const float4_t acc) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, acc, 0, 0, 0, 0, 0, 0);
}

// the maximum of 64 non-negative values, in lane 63 (tce_common.hpp's wave_sum_dpp_lane63 with a maximum: the lanes a step leaves out see 0)
__device__ __forceinline__ float wave_max_dpp_lane63(float v) {
    auto dpp = [](float x, auto ctrl, auto row_mask) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, decltype(row_mask)::value, 0xF, false));
    };
    v = __builtin_fmaxf(v, dpp(v, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xF>{}));   // quad_perm [1,0,3,2]
    v = __builtin_fmaxf(v, dpp(v, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xF>{}));   // quad_perm [2,3,0,1]
    v = __builtin_fmaxf(v, dpp(v, std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xF>{}));  // row_half_mirror
    v = __builtin_fmaxf(v, dpp(v, std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xF>{}));  // row_mirror
    v = __builtin_fmaxf(v, dpp(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{}));  // row_bcast15 into rows 1 and 3
    v = __builtin_fmaxf(v, dpp(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{}));  // row_bcast31 into rows 2 and 3
    return v;
}

__global__ __launch_bounds__(kQuantThreads) void fp8_quantize_rows_kernel(const half_t *x, long long ldx, uint8_t *xq, long long ldq, float *sx, int K) {
    __shared__ float wmax[kQuantThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = blockIdx.x;
    const half8_t *xr = reinterpret_cast<const half8_t *>(x + row * ldx);
    const int pieces = K >> 3;
    half8_t v[kQuantPieces];
#pragma unroll
    for (int i = 0; i < kQuantPieces; ++i) {
        const int p = tid + i * kQuantThreads;
        v[i] = xr[p < pieces ? p : pieces - 1];  // (past the row: a re-read of its last piece -- a maximum does not mind seeing it again, and it is not stored)
    }
    float amax = 0.f;  // fmaxf: a NaN element does not enter the maximum
#pragma unroll
    for (int i = 0; i < kQuantPieces; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = __builtin_fmaxf(amax, __builtin_fabsf((float)v[i][e]));
    amax = wave_max_dpp_lane63(amax);
    if (lane == 63) wmax[wave] = amax;
    __syncthreads();
    amax = __builtin_fmaxf(__builtin_fmaxf(wmax[0], wmax[1]), __builtin_fmaxf(wmax[2], wmax[3]));
    const bool zero = amax == 0.f;
    const float s = zero ? 1.0f : amax / 448.0f, inv = zero ? 1.0f : 448.0f / amax;
    if (tid == 0) sx[row] = s;
    uint2_t *qr = reinterpret_cast<uint2_t *>(xq + row * ldq);
#pragma unroll
    for (int i = 0; i < kQuantPieces; ++i) {
        const int p = tid + i * kQuantThreads;
        if (p < pieces) qr[p] = fp8_quant8(v[i], inv);
    }
}

// four consecutive columns of output row m: (acc * sx[m]) * sw[n], then binary16 -- with `add` float(C) + v first
__device__ __forceinline__ void scale_store4(const float4_t acc, const float sxm, const float4_t sw4, half_t *dst, const int add) {
    half4_t old = half4_t{0, 0, 0, 0}, out;
    if (add) old = *reinterpret_cast<const half4_t *>(dst);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v = (acc[r] * sxm) * sw4[r];
        out[r] = add ? (half_t)((float)old[r] + v) : (half_t)v;
    }
    *reinterpret_cast<half4_t *>(dst) = out;
}

__global__ __launch_bounds__(64 * kSkWaves) void w8a8_fp8_skinny_kernel(const uint8_t *xq, long long ldq, const float *sx, const uint8_t *wq, const float *sw, half_t *C,
                                                                         long long ldc, int M, int K, int add) {
    __shared__ float4_t part[kSkWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const bool live = r16 < M;  // this lane's activation row exists; the others' operand bytes are zeros
    const uint8_t *pw = wq + (size_t)(n0 + r16) * K + kq * 32;
    const uint8_t *px = xq + (size_t)(live ? r16 : 0) * ldq + kq * 32;
    const int steps = K >> 7;
    const int s_begin = wave * steps / kSkWaves, s_end = (wave + 1) * steps / kSkWaves;  // this wave's K steps (none when there are fewer steps than waves)
    float4_t acc = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int s = s_begin; s < s_end; s += kSkDepth) {
        uint4_t w[kSkDepth][2], a[kSkDepth][2];
#pragma unroll
        for (int d = 0; d < kSkDepth; ++d) {
            const size_t k0 = (size_t)(s + d < s_end ? s + d : s_end - 1) * 128;  // (past the slice: a clamped re-read, not contracted)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                w[d][h] = load_nt(reinterpret_cast<const uint4_t *>(pw + k0) + h);
                a[d][h] = reinterpret_cast<const uint4_t *>(px + k0)[h];
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // (every request of the kSkDepth steps is out before the first contraction: the scheduler otherwise sinks the loads to their uses)
#pragma unroll
        for (int d = 0; d < kSkDepth; ++d) {
            if (s + d >= s_end) break;
            const uint4_t z = uint4_t{0u, 0u, 0u, 0u};
            acc = mfma_e4m3(operand(w[d][0], w[d][1]), operand(live ? a[d][0] : z, live ? a[d][1] : z), acc);
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    float4_t sum = part[0][lane];
#pragma unroll
    for (int w = 1; w < kSkWaves; ++w) {  // wave order
        const float4_t o = part[w][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[r] = sum[r] + o[r];
    }
    if (!live) return;
    const int n = n0 + 4 * kq;
    scale_store4(sum, sx[r16], *reinterpret_cast<const float4_t *>(sw + n), C + (size_t)r16 * ldc + n, add);
}

// chunk c of panel row `row` lies at chunk c ^ tiled_swizzle(row)
__device__ __forceinline__ int tiled_swizzle(const int row) { return ((row & 7) + ((row >> 3) & 1)) & 7; }

__global__ __launch_bounds__(kTiledThreads) void w8a8_fp8_tiled_kernel(const uint8_t *xq, long long ldq, const float *sx, const uint8_t *wq, const float *sw, half_t *C,
                                                                        long long ldc, int M, int N, int K, int add) {
    extern __shared__ __attribute__((aligned(16))) uint4_t lds_fp8[];  // [2 buffers][weights: 128 rows x 8 chunks | activations: 128 rows x 8 chunks]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_tile = blockIdx.x * kTile, m_tile = blockIdx.y * kTile;
    // load view: eight lanes per 128-byte row piece, four rows (32 apart) of each panel per thread
    const int lrow = tid >> 3, lchunk = tid & 7;
    const uint8_t *pw[4], *px[4];
    int ws[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = lrow + 32 * i;
        int n = n_tile + row, m = m_tile + row;
        n = n < N ? n : N - 1;
        m = m < M ? m : M - 1;
        pw[i] = wq + (size_t)n * K + lchunk * 16;
        px[i] = xq + (size_t)m * ldq + lchunk * 16;
        ws[i] = row * 8 + (lchunk ^ tiled_swizzle(row));
    }
    // MFMA view: the two chunks of this lane's 32 bytes in fragment row r16 of a 16-row block
    const int f0 = r16 * 8 + ((2 * kq) ^ tiled_swizzle(r16)), f1 = r16 * 8 + ((2 * kq + 1) ^ tiled_swizzle(r16));
    const int fw = (wn * 64) * 8, fx = kTile * 8 + (wm * 64) * 8;
    float4_t acc[4][4];  // [weight block i: n][activation block j: m]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    uint4_t rw[4], rx[4];
    auto request = [&](int t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rw[i] = *reinterpret_cast<const uint4_t *>(pw[i] + (size_t)t * 128);
            rx[i] = *reinterpret_cast<const uint4_t *>(px[i] + (size_t)t * 128);
        }
    };
    auto stage_write = [&](int buf) {
        uint4_t *base = lds_fp8 + buf * (2 * kTile * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            base[ws[i]] = rw[i];
            base[kTile * 8 + ws[i]] = rx[i];
        }
    };
    const int T = K >> 7;
    request(0);
    stage_write(0);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        if (t + 1 < T) request(t + 1);  // in flight through this step's contraction
        const uint4_t *base = lds_fp8 + (t & 1) * (2 * kTile * 8);
        int8v_t bx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bx[j] = operand(base[fx + j * 128 + f0], base[fx + j * 128 + f1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int8v_t aw = operand(base[fw + i * 128 + f0], base[fw + i * 128 + f1]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma_e4m3(aw, bx[j], acc[i][j]);
        }
        if (t + 1 < T) stage_write((t + 1) & 1);  // (the buffer step t - 1 was read from: every wave passed the barrier behind that step)
        __syncthreads();
    }
    // acc[i][j][r]: C[m = m_base + 16 j + r16][n = n_base + 16 i + 4 kq + r]
    const int n_base = n_tile + wn * 64 + 4 * kq, m_base = m_tile + wm * 64 + r16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m_base + 16 * j;
        if (m >= M) continue;
        const float sxm = sx[m];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n_base + 16 * i;
            if (n < N) scale_store4(acc[i][j], sxm, *reinterpret_cast<const float4_t *>(sw + n), C + (size_t)m * ldc + n, add);
        }
    }
}

int launched(hipError_t *hip_err) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return TCE_OK;
    if (hip_err) *hip_err = e;
    return TCE_ERR_HIP;
}

}  // namespace

int launch_fp8_quantize_rows_f16(const void *x, int ldx, void *xq, int ldq, float *sx, int rows, int K, hipStream_t stream, hipError_t *hip_err) {
    hipLaunchKernelGGL(fp8_quantize_rows_kernel, dim3(rows), dim3(kQuantThreads), 0, stream, static_cast<const half_t *>(x), (long long)ldx, static_cast<uint8_t *>(xq),
                       (long long)ldq, sx, K);
    return launched(hip_err);
}

// The dispatcher's choice with no form bit: the skinny form while it can take the rows.  (The threshold is the smallest measured M from which the tiled form wins at
// every larger one -- DESIGN.md 3.11: measured, there is none up to 16 rows, where the skinny form ends.)
bool fp8_linear_tiled(int M, int flags) {
    constexpr int kTiledFromM = 17;
    if (flags & TCE_FP8_FORM_TILED) return true;
    if (flags & TCE_FP8_FORM_SKINNY) return false;
    return M >= kTiledFromM;
}

int launch_w8a8_fp8_forward_f16(const void *xq, int ldq, const float *sx, const void *wq, const float *sw, void *C, int ldc, int M, int N, int K, int flags, hipStream_t stream,
                                hipError_t *hip_err) {
    const uint8_t *xb = static_cast<const uint8_t *>(xq), *wb = static_cast<const uint8_t *>(wq);
    const int add = (flags & TCE_W4_ADD_TO_C) != 0;
    if (!fp8_linear_tiled(M, flags)) {
        hipLaunchKernelGGL(w8a8_fp8_skinny_kernel, dim3(N / 16), dim3(64 * kSkWaves), 0, stream, xb, (long long)ldq, sx, wb, sw, static_cast<half_t *>(C), (long long)ldc, M, K,
                           add);
        return launched(hip_err);
    }
    static hipError_t raised = hipErrorNotReady;  // 64 KiB of LDS is more than a kernel gets by default: the limit is raised once
    if (raised != hipSuccess) raised = hipFuncSetAttribute(reinterpret_cast<const void *>(w8a8_fp8_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kTiledLds);
    if (raised != hipSuccess) {
        if (hip_err) *hip_err = raised;
        return TCE_ERR_HIP;
    }
    hipLaunchKernelGGL(w8a8_fp8_tiled_kernel, dim3((N + kTile - 1) / kTile, (M + kTile - 1) / kTile), dim3(kTiledThreads), kTiledLds, stream, xb, (long long)ldq, sx, wb, sw,
                       static_cast<half_t *>(C), (long long)ldc, M, N, K, add);
    return launched(hip_err);
}

}  // namespace tce
