// lora_tiled.hip -- the adapted linear's two launches on prompt-sized row counts (include/tce_matmul.h, "Multi-LoRA", THE TILED FORM: tce_lora_shrink_tiled_f16,
// tce_lora_expand_add_tiled_f16), gfx950.  The second form of lora.hip's shrink and expand: the same operands and the same definition,
//
//     shrink   t[i][j]  = sum_k x[i][k] * A[a][j][k]                                       fp32, never rounded to fp16
//     expand   C[i][n]  = fp16(float(C[i][n]) + scale[a] * sum_j t[i][j] * B[a][j][n])     in place, behind the base linear
//
// on matrix instructions and on tiles of 32 rows, so that a prompt's rows share ONE read of their adapter per tile instead of one per block of 4 rows.  The sums
// are taken in another order than lora.hip's, so the results are NOT its bits (they meet the same bound against float64): the form is opt-in.
//
// Both kernels: 256 threads = 4 waves, a tile of kTileRows = 32 rows, NO adapter dimension in the grid.  Every wave reads the tile's 32 words (lane i and lane 32 + i
// word i; a row past `rows` counts as -1) and walks the DISTINCT valid adapters among them by ballot: the lowest pending lane's word is the pass's adapter, the lanes
// with that word leave the pending set.  A prompt's tile is one pass, a tile that straddles two admissions two, a tile of -1 none (the workgroup leaves).  In a pass
// the rows on other adapters are zero-filled operands: nothing of x, t or the pool is read for them, and nothing is stored.  An MFMA's rows and columns do not mix,
// so a row's bits depend on that row's operands and its adapter alone -- not on its index, `rows`, its neighbours' words or data (a NaN included), or the grid.
//
// SHRINK  grid (row tile, K slice).  K is cut into S(K) runs of `run` k (1024, lengthened in steps of 128 where that would give more than 16 slices: a function of K
//   ALONE); slice s of a row goes to partial[s][row][0 .. R) fp32.  The four waves deal the slice's super-steps of 128 k (wave w: w, w + 4, ...).  A super-step
//   is four v_mfma_f32_16x16x32_f16 per accumulator block, adapter rows on the instruction's M side and the tile's rows on its N side: lane (r16, kq) takes for step
//   s the 8 halves at k0 + 32 kq + 8 s of row r16 -- straight from global memory in 16-byte pieces, the four lanes of a row covering 256 contiguous bytes.  (The k
//   index inside a super-step is a permutation of the natural one, the same for both operands.)  A wave holds 2 row blocks x NJB = ceil(R / 16) column blocks of
//   accumulators (96 registers at R = 192); an x fragment meets every column block, an A fragment both row blocks.  Zero-filled and never loaded: rows past `rows` or
//   on another adapter, pieces past the slice's end (K % 8 == 0, not % 32), adapter rows past R (R % 8 == 0, not % 16).  fp16 x fp16 is exact in fp32; the
//   instruction adds in fp32.  The four waves' tiles meet in LDS and are added ((w0 + w1) + w2) + w3 by all 256 threads, which store the pass's rows.
// EXPAND  grid (row tile, tile of kExpandCols = 128 columns).  t = ((p[0] + p[1]) + ...) + p[S - 1] is formed in slice order while the tile's t [32][R] is staged in
//   LDS (rows of the pass; the others are zeros and their partials are never read): no third launch, no atomics, t is never rounded.  B[a]'s column tile streams through
//   LDS in chunks of 64 j, 16-byte global loads converted fp16 -> fp32 (exact) on the way, the next chunk's requests in flight under the MFMAs.  j ascends in super-steps
//   of 8 = two v_mfma_f32_16x16x4_f32 (lane group kq on j0 + 2 kq, then j0 + 2 kq + 1), B's columns on the M side and the rows on the N side: a lane ends with 4
//   adjacent columns of one row.  Epilogue fmaf(scale[a], acc, float(C)) and ONE rounding to fp16, stored for the pass's rows only.
// The unit is built without packed fp32 arithmetic (build.py) and with -ffp-contract=off: the sums beside the MFMAs are plain v_add_f32.
#include "lora_tiled.hpp"  // the tile, the staged chunk, walk_adapters: shared with lora_tiled_seg.hip

namespace tce {
namespace {

constexpr int kRun = 1024;         // k of a slice, unless K would need more than TCE_LORA_TILED_MAX_SLICES of them
constexpr int kSuper = 128;        // k of one wave iteration of the shrink: four MFMA steps

__host__ __device__ inline int tiled_run(int K) {
    if ((K + kRun - 1) / kRun <= TCE_LORA_TILED_MAX_SLICES) return kRun;
    const int per = (K + TCE_LORA_TILED_MAX_SLICES - 1) / TCE_LORA_TILED_MAX_SLICES;
    return (per + kSuper - 1) / kSuper * kSuper;
}

__device__ __forceinline__ half8_t load8_or_zero(const half_t *p, bool ok) {
    uint4_t v = {0u, 0u, 0u, 0u};
    if (ok) v = *reinterpret_cast<const uint4_t *>(p);
    return __builtin_bit_cast(half8_t, v);
}

template <int NJB>
__global__ __launch_bounds__(kThreads) void lora_shrink_tiled_kernel(const half_t *__restrict__ x, long long ldx, const half_t *__restrict__ A,
                                                                      const int32_t *__restrict__ row_adapter, float *__restrict__ partial, int rows, int K, int R,
                                                                      int n_adapters, int run) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [kWaves][kTileRows][kLd]
    constexpr int kLd = NJB * 16 + 4;
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * kTileRows, slice = blockIdx.y;
    const int kbeg = slice * run, kend = kbeg + run < K ? kbeg + run : K;
    const int nss = (kend - kbeg + kSuper - 1) / kSuper;

    walk_adapters(row_adapter, row0, rows, n_adapters, [&](int a, unsigned same) {
        const half_t *Aa = A + (size_t)a * R * (size_t)K;
        const half_t *xr[2];
        bool xok[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            xok[rb] = (same >> (rb * 16 + r16)) & 1u;
            xr[rb] = x + (size_t)(row0 + rb * 16 + r16) * (size_t)ldx;  // (read under xok only)
        }
        float4_t acc[2][NJB];  // D[j = 16 jb + 4 kq + i][row 16 rb + r16]
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) acc[rb][jb] = float4_t{0.f, 0.f, 0.f, 0.f};

        for (int ss = wave; ss < nss; ss += kWaves) {
            const int k0 = kbeg + ss * kSuper + kq * 32;
            half8_t xf[2][4];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int s = 0; s < 4; ++s) xf[rb][s] = load8_or_zero(xr[rb] + k0 + 8 * s, xok[rb] && k0 + 8 * s < kend);
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) {
                const int j = jb * 16 + r16;
                const half_t *aj = Aa + (size_t)j * K + k0;  // (read under j < R only)
                half8_t af[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) af[s] = load8_or_zero(aj + 8 * s, j < R && k0 + 8 * s < kend);
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[rb][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], xf[rb][s], acc[rb][jb], 0, 0, 0);
            }
        }

        float *mine = lds + wave * (kTileRows * kLd);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) *reinterpret_cast<float4_t *>(mine + (rb * 16 + r16) * kLd + jb * 16 + 4 * kq) = acc[rb][jb];
        __syncthreads();
        float *out = partial + ((size_t)slice * rows + row0) * R;
        for (int e = tid; e < kTileRows * R; e += kThreads) {
            const int row = e / R, j = e - row * R;
            if ((same >> row) & 1u) {
                const float *p = lds + row * kLd + j;
                out[e] = ((p[0] + p[kTileRows * kLd]) + p[2 * kTileRows * kLd]) + p[3 * kTileRows * kLd];
            }
        }
        __syncthreads();  // (the next pass writes the tiles again)
    });
}

__global__ __launch_bounds__(kThreads) void lora_expand_add_tiled_kernel(const float *__restrict__ partial, const half_t *__restrict__ B, const float *__restrict__ scale,
                                                                         const int32_t *__restrict__ row_adapter, half_t *__restrict__ C, long long ldc, int rows, int N,
                                                                         int R, int n_adapters, int slices) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // t [kTileRows][R + 4], then B's chunk [kChunkJ][kLdB]
    const int ldt = R + 4;
    float *Ts = lds, *Bs = lds + kTileRows * ldt;
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * kTileRows, n0 = blockIdx.y * kExpandCols;
    const int nchunks = (R + kChunkJ - 1) / kChunkJ;

    walk_adapters(row_adapter, row0, rows, n_adapters, [&](int a, unsigned same) {
        const half_t *Ba = B + (size_t)a * R * (size_t)N;
        const float sc = scale[a];
        // request view: piece u of thread t is the 16-byte piece (t + 256 u) % 16 of chunk row (t + 256 u) / 16
        uint4_t Bq[4];
        auto request = [&](int c) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + kThreads * u, j = c * kChunkJ + (idx >> 4), n = n0 + (idx & 15) * 8;
                Bq[u] = uint4_t{0u, 0u, 0u, 0u};
                if (j < R && n < N) Bq[u] = *reinterpret_cast<const uint4_t *>(Ba + (size_t)j * N + n);  // (N % 8 == 0: a piece is all inside or all outside)
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
        // t of the pass's rows, the K slices added in slice order; zeros for the other rows
        for (int e = tid; e < kTileRows * R; e += kThreads) {
            const int row = e / R, j = e - row * R;
            float v = 0.f;
            if ((same >> row) & 1u) {
                const float *p = partial + (size_t)row0 * R + e;
                v = p[0];
                for (int s = 1; s < slices; ++s) v += p[(size_t)s * rows * R];
            }
            Ts[row * ldt + j] = v;
        }

        float4_t acc[2][2];  // D[n = n0 + 32 wave + 16 nb + 4 kq + i][row 16 rb + r16]
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[rb][nb] = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nchunks; ++c) {
            land();
            __syncthreads();
            if (c + 1 < nchunks) request(c + 1);
            const int jn = R - c * kChunkJ < kChunkJ ? R - c * kChunkJ : kChunkJ;  // a multiple of 8
            const float *tp = Ts + r16 * ldt + c * kChunkJ + 2 * kq, *bp = Bs + 2 * kq * kLdB + wave * 32 + r16;
#pragma unroll 2
            for (int js = 0; js < jn; js += 8) {
                float2 tf[2];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) tf[rb] = *reinterpret_cast<const float2 *>(tp + rb * 16 * ldt + js);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const float b0 = bp[js * kLdB + nb * 16], b1 = bp[(js + 1) * kLdB + nb * 16];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0, tf[rb].x, acc[rb][nb], 0, 0, 0);
                        acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1, tf[rb].y, acc[rb][nb], 0, 0, 0);
                    }
                }
            }
            __syncthreads();  // (the next chunk, or the next pass, writes the staged tiles again)
        }

#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            if (!((same >> (rb * 16 + r16)) & 1u)) continue;
            half_t *crow = C + (size_t)(row0 + rb * 16 + r16) * (size_t)ldc;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int n = n0 + wave * 32 + nb * 16 + 4 * kq;
                if (n >= N) continue;  // (N % 8 == 0: a lane's 4 columns are all inside or all outside)
                uint2_t *cp = reinterpret_cast<uint2_t *>(crow + n);
                const half4_t ch = __builtin_bit_cast(half4_t, *cp);
                half4_t o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (half_t)__builtin_fmaf(sc, acc[rb][nb][i], (float)ch[i]);
                *cp = __builtin_bit_cast(uint2_t, o);
            }
        }
    });
}

template <int NJB>
int launch_shrink(const half_t *x, long long ldx, const half_t *A, const int32_t *row_adapter, float *partial, int rows, int K, int R, int n_adapters, hipStream_t stream,
                  hipError_t *hip_err) {
    constexpr size_t bytes = (size_t)kWaves * kTileRows * (NJB * 16 + 4) * sizeof(float);
    if constexpr (bytes > 48 * 1024) {  // more than a kernel gets by default: the limit is raised ONCE per instantiation
        static hipError_t raised = hipErrorNotReady;
        if (raised != hipSuccess)
            raised = hipFuncSetAttribute(reinterpret_cast<const void *>(lora_shrink_tiled_kernel<NJB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (raised != hipSuccess) {
            if (hip_err) *hip_err = raised;
            return TCE_ERR_HIP;
        }
    }
    const int run = tiled_run(K);
    hipLaunchKernelGGL(lora_shrink_tiled_kernel<NJB>, dim3((rows + kTileRows - 1) / kTileRows, (K + run - 1) / run), dim3(kThreads), bytes, stream, x, ldx, A, row_adapter,
                       partial, rows, K, R, n_adapters, run);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace

int lora_tiled_slices(int K) {
    const int run = tiled_run(K);
    return (K + run - 1) / run;
}

int launch_lora_shrink_tiled_f16(const void *x, int ldx, const void *A, const int32_t *row_adapter, float *partial, int rows, int K, int R, int n_adapters, hipStream_t stream,
                                 hipError_t *hip_err) {
    const half_t *xh = static_cast<const half_t *>(x), *Ah = static_cast<const half_t *>(A);
    const int njb = (R + 15) / 16;  // the instantiation with the fewest column blocks that hold R (blocks past R are zero operands)
    if (njb <= 1) return launch_shrink<1>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
    if (njb <= 2) return launch_shrink<2>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
    if (njb <= 3) return launch_shrink<3>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
    if (njb <= 4) return launch_shrink<4>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
    if (njb <= 6) return launch_shrink<6>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
    if (njb <= 8) return launch_shrink<8>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
    return launch_shrink<12>(xh, ldx, Ah, row_adapter, partial, rows, K, R, n_adapters, stream, hip_err);
}

int launch_lora_expand_add_tiled_f16(const float *partial, const void *B, const float *scale, const int32_t *row_adapter, void *C, int ldc, int rows, int N, int K, int R,
                                     int n_adapters, hipStream_t stream, hipError_t *hip_err) {
    const size_t bytes = ((size_t)kTileRows * (R + 4) + (size_t)kChunkJ * kLdB) * sizeof(float);  // at most 59904: inside a kernel's default
    hipLaunchKernelGGL(lora_expand_add_tiled_kernel, dim3((rows + kTileRows - 1) / kTileRows, (N + kExpandCols - 1) / kExpandCols), dim3(kThreads), bytes, stream, partial,
                       static_cast<const half_t *>(B), scale, row_adapter, static_cast<half_t *>(C), (long long)ldc, rows, N, R, n_adapters, lora_tiled_slices(K));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace tce
