// lora.hip -- per-row fp16 LoRA adapters beside the W4A16 linears (include/tce_matmul.h: tce_lora_shrink_f16, tce_lora_expand_add_f16, tce_lora_expand_silu_mul_f16).
//
// The base weights are packed int4, so an adapter cannot be merged into them: it is a run-time path of two launches per adapted linear,
//
//     shrink   t[i][j]  = sum_k x[i][k] * A[a][j][k]                                       fp32, never rounded to fp16
//     expand   C[i][n]  = fp16(float(C[i][n]) + scale[a] * sum_j t[i][j] * B[a][j][n])     in place, behind the base linear
//
// with a = row_adapter[i] read ON THE DEVICE when the kernel runs: the rows of one launch pick different adapters, and a captured graph follows a slot that
// changes its adapter.  A word outside [0, n_adapters) leaves the row alone: nothing of the pool is read for it, C[i] keeps its bits, t[i] is not written.
//
// Both grids are (piece of the adapter, adapter, block of 4 rows).  A workgroup reads its block's 4 words and leaves at once when none names its adapter; the matching
// rows are served by ONE read of the workgroup's piece of the adapter, so rows that share an adapter share its read (the SGMV property, with no sorting on the host;
// across blocks the adapter comes from the L2).  The row-block dimension keeps a prefill of several hundred rows on one adapter from serialising.
//
// Arithmetic ("Multi-LoRA"): every step is ONE explicit fmaf in fp32.  fp16 * fp16 is exact in fp32, so the shrink's steps round once, at the add.
//   shrink: a workgroup of 256 threads owns j = 4 * blockIdx.x .. + 3 and the whole K; thread T takes the 8-element pieces T, T + 256, T + 512, ... in ascending order,
//           the 8 elements of a piece in ascending k, into one accumulator per (j, row); a wave's 64 accumulators meet in the xor butterfly 32, 16, 8, 4, 2, 1, the four
//           waves' sums in LDS as (w0 + w1) + (w2 + w3).  The order depends on K alone -- not on the row, its place in the launch, how many rows match, or which rows
//           share the pass (every count of rows per pass is the same instructions per row).
//   expand: a lane owns 8 adjacent columns; j ascends into one accumulator per column; then fmaf(scale, acc, float(C)) and ONE rounding to fp16.
// No atomics: a row has exactly one adapter, so one workgroup owns each element it writes.
//
// Gate / up (tce_lora_expand_silu_mul_f16): the project runs gate, up and SiLU * mul as ONE launch, and a delta has to land in front of the nonlinearity.  An adapted
// gate/up is the shrink on the shared input (A stacked: t fp32 [rows][2R], gate's sums in front), the base gate_up linear WITHOUT the pair flag (y fp16 [rows][2N],
// column 2n = gate n, column 2n + 1 = up n) and
//     expand   g = fp16(float(y[i][2n]) + scale[a] * sum_j t[i][j] * Bg[a][j][n]),  u = fp16(float(y[i][2n+1]) + scale[a] * sum_j t[i][R + j] * Bu[a][j][n]),
//              C[i][n] = silu_mul_half(g, u)                                          -- every row; a row without an adapter takes g and u from y as they are
// The expand is SEGMENTED: gate's sum walks gate's R rows of t and Bg, up's sum up's -- the zero blocks of the block-structured form (B' [2R][2N], gate in the even
// columns of the first R rows, up in the odd columns of the last R) are never read.  It is that form's result bit for bit all the same: a sum that starts at +0 never
// becomes -0, so the steps fmaf(t, 0, acc) it leaves out change no bit of acc (finite t).  Grid (piece of N, adapter, block of 4 rows) as above, with ONE PLANE MORE:
// plane n_adapters serves the block's rows without an adapter.  An adapter's plane serves the block's rows on it with ONE read of Bg and Bu, gate's pass in front of up's.
#include "tce_common.hpp"

namespace tce {
namespace {

constexpr int kRowBlock = 4;      // rows one workgroup scans and serves in one pass (both kernels)
constexpr int kShrinkJ = 4;       // the j rows of A a shrink workgroup owns
constexpr int kShrinkThreads = 256;
constexpr int kExpandCols = 512;  // columns of an expand workgroup: 64 lanes x 8

// the rows of this workgroup's block whose word names adapter `a` (uniform: every lane reads the same words): their offsets in r[0 .. n), the last one repeated behind
__device__ __forceinline__ int matching_rows(const int32_t *__restrict__ row_adapter, int row0, int rows, int a, int (&r)[kRowBlock]) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < kRowBlock; ++i) {
        const bool hit = row0 + i < rows && row_adapter[row0 + i] == a;
#pragma unroll
        for (int p = 0; p < kRowBlock; ++p)
            if (hit && p >= n) r[p] = i;
        n += hit ? 1 : 0;
    }
    return n;
}

template <int NR>
__device__ __forceinline__ void shrink_pass(const half_t *__restrict__ x, long long ldx, const half_t *__restrict__ A0, float *__restrict__ t, const int (&r)[kRowBlock],
                                            int row0, int j0, int K, int R, float (*part)[kShrinkJ * kRowBlock]) {
    const int tid = threadIdx.x, pieces = K >> 3;
    const uint4_t *Aj[kShrinkJ], *xr[NR];
#pragma unroll
    for (int jj = 0; jj < kShrinkJ; ++jj) Aj[jj] = reinterpret_cast<const uint4_t *>(A0 + (size_t)jj * K);
#pragma unroll
    for (int p = 0; p < NR; ++p) xr[p] = reinterpret_cast<const uint4_t *>(x + (size_t)(row0 + r[p]) * (size_t)ldx);
    float acc[kShrinkJ][NR];
#pragma unroll
    for (int jj = 0; jj < kShrinkJ; ++jj)
#pragma unroll
        for (int p = 0; p < NR; ++p) acc[jj][p] = 0.f;
#pragma unroll 2
    for (int c = tid; c < pieces; c += kShrinkThreads) {
        half8_t ah[kShrinkJ], xh[NR];
#pragma unroll
        for (int jj = 0; jj < kShrinkJ; ++jj) ah[jj] = __builtin_bit_cast(half8_t, Aj[jj][c]);
#pragma unroll
        for (int p = 0; p < NR; ++p) xh[p] = __builtin_bit_cast(half8_t, xr[p][c]);
#pragma unroll
        for (int jj = 0; jj < kShrinkJ; ++jj)
#pragma unroll
            for (int p = 0; p < NR; ++p)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[jj][p] = fmaf((float)xh[p][e], (float)ah[jj][e], acc[jj][p]);
    }
#pragma unroll
    for (int jj = 0; jj < kShrinkJ; ++jj)
#pragma unroll
        for (int p = 0; p < NR; ++p) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) acc[jj][p] += __shfl_xor(acc[jj][p], s, 64);
            if ((tid & 63) == 0) part[tid >> 6][jj * kRowBlock + p] = acc[jj][p];
        }
    __syncthreads();
    if (tid < kShrinkJ * kRowBlock) {
        const int jj = tid / kRowBlock, p = tid % kRowBlock;
        if (p < NR) t[(size_t)(row0 + r[p]) * R + j0 + jj] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    }
}

__global__ __launch_bounds__(kShrinkThreads) void lora_shrink_kernel(const half_t *__restrict__ x, long long ldx, const half_t *__restrict__ A,
                                                                      const int32_t *__restrict__ row_adapter, float *__restrict__ t, int rows, int K, int R) {
    __shared__ float part[kShrinkThreads / 64][kShrinkJ * kRowBlock];
    const int a = blockIdx.y, row0 = blockIdx.z * kRowBlock, j0 = blockIdx.x * kShrinkJ;  // (R % 8 == 0: all four j exist)
    int r[kRowBlock] = {0, 0, 0, 0};
    const int n = matching_rows(row_adapter, row0, rows, a, r);
    if (n == 0) return;
    const half_t *A0 = A + ((size_t)a * R + j0) * (size_t)K;
    if (n == 1)  // (one instantiation per count: NR == n, no row slot is computed and thrown away)
        shrink_pass<1>(x, ldx, A0, t, r, row0, j0, K, R, part);
    else if (n == 2)
        shrink_pass<2>(x, ldx, A0, t, r, row0, j0, K, R, part);
    else if (n == 3)
        shrink_pass<3>(x, ldx, A0, t, r, row0, j0, K, R, part);
    else
        shrink_pass<4>(x, ldx, A0, t, r, row0, j0, K, R, part);
}

template <int NR>
__device__ __forceinline__ void expand_pass(const float *__restrict__ t, const half_t *__restrict__ Ba, float s, half_t *__restrict__ C, long long ldc, const int (&r)[kRowBlock],
                                            int n, int row0, int col, int N, int R) {
    const float *tr[NR];
#pragma unroll
    for (int p = 0; p < NR; ++p) tr[p] = t + (size_t)(row0 + r[p]) * R;
    float acc[NR][8];
#pragma unroll
    for (int p = 0; p < NR; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[p][e] = 0.f;
#pragma unroll 2
    for (int j0 = 0; j0 < R; j0 += 8) {  // (R % 8 == 0) eight rows of B requested together
        half8_t bh[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) bh[u] = __builtin_bit_cast(half8_t, *reinterpret_cast<const uint4_t *>(Ba + (size_t)(j0 + u) * N));
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const float tj = p < n ? tr[p][j0 + u] : 0.f;  // (a repeated slot adds nothing and is not stored)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[p][e] = fmaf(tj, (float)bh[u][e], acc[p][e]);
            }
    }
#pragma unroll
    for (int p = 0; p < NR; ++p) {
        if (p >= n) break;
        uint4_t *cp = reinterpret_cast<uint4_t *>(C + (size_t)(row0 + r[p]) * (size_t)ldc + col);
        const half8_t ch = __builtin_bit_cast(half8_t, *cp);
        half8_t out;
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] = (half_t)fmaf(s, acc[p][e], (float)ch[e]);
        *cp = __builtin_bit_cast(uint4_t, out);
    }
}

__global__ __launch_bounds__(64) void lora_expand_add_kernel(const float *__restrict__ t, const half_t *__restrict__ B, const float *__restrict__ scale,
                                                             const int32_t *__restrict__ row_adapter, half_t *__restrict__ C, long long ldc, int rows, int N, int R) {
    const int a = blockIdx.y, row0 = blockIdx.z * kRowBlock;
    int r[kRowBlock] = {0, 0, 0, 0};
    const int n = matching_rows(row_adapter, row0, rows, a, r);
    if (n == 0) return;
    const int col = blockIdx.x * kExpandCols + threadIdx.x * 8;
    if (col >= N) return;  // (N % 8 == 0: a lane's 8 columns are all inside or all outside)
    const half_t *Ba = B + (size_t)a * R * (size_t)N + col;
    const float s = scale[a];
    if (n == 1)
        expand_pass<1>(t, Ba, s, C, ldc, r, n, row0, col, N, R);
    else if (n == 2)
        expand_pass<2>(t, Ba, s, C, ldc, r, n, row0, col, N, R);
    else  // three rows run the 4-row form with t = 0 in the repeated slot: with a <3> instantiation beside these the compiler keeps 6 .. 8 instead of 16 rows of B in
          // flight in EVERY form (73 against 103 registers) and the one-row pair was measured 1.3 .. 4 us slower ("Multi-LoRA")
        expand_pass<4>(t, Ba, s, C, ldc, r, n, row0, col, N, R);
}

// one segment (gate's or up's) of the rows r[0 .. n): out[p] = fp16(fmaf(s, sum_j t[r[p]][j] * Ba[j][:], float(yv[p]))) -- expand_pass's sums and its one rounding
template <int NR>
__device__ __forceinline__ void segment_pass(const float *__restrict__ t, int ldt, const half_t *__restrict__ Ba, float s, const half8_t (&yv)[NR], half8_t (&out)[NR],
                                             const int (&r)[kRowBlock], int n, int row0, int N, int R) {
    const float *tr[NR];
#pragma unroll
    for (int p = 0; p < NR; ++p) tr[p] = t + (size_t)(row0 + r[p]) * ldt;
    float acc[NR][8];
#pragma unroll
    for (int p = 0; p < NR; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[p][e] = 0.f;
#pragma unroll 2
    for (int j0 = 0; j0 < R; j0 += 8) {  // (R % 8 == 0)
        half8_t bh[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) bh[u] = __builtin_bit_cast(half8_t, *reinterpret_cast<const uint4_t *>(Ba + (size_t)(j0 + u) * N));
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const float tj = p < n ? tr[p][j0 + u] : 0.f;  // (a repeated slot adds nothing and is not stored)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[p][e] = fmaf(tj, (float)bh[u][e], acc[p][e]);
            }
    }
#pragma unroll
    for (int p = 0; p < NR; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) out[p][e] = (half_t)fmaf(s, acc[p][e], (float)yv[p][e]);
}

// a lane's 16 columns of one row of y (8 gate / up pairs), de-interleaved
__device__ __forceinline__ void load_pairs(const half_t *__restrict__ yp, half8_t &g, half8_t &u) {
    const half8_t lo = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4_t *>(yp)[0]), hi = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4_t *>(yp)[1]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        g[e] = lo[2 * e];
        u[e] = lo[2 * e + 1];
        g[4 + e] = hi[2 * e];
        u[4 + e] = hi[2 * e + 1];
    }
}

__device__ __forceinline__ void store_silu_mul(half_t *__restrict__ cp, const half8_t &g, const half8_t &u) {
    half8_t out;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = silu_mul_half(g[e], u[e]);
    *reinterpret_cast<uint4_t *>(cp) = __builtin_bit_cast(uint4_t, out);
}

template <int NR>
__device__ __forceinline__ void gate_up_pass(const float *__restrict__ t, const half_t *__restrict__ Bga, const half_t *__restrict__ Bua, float s, const half_t *__restrict__ y,
                                             long long ldy, half_t *__restrict__ C, long long ldc, const int (&r)[kRowBlock], int n, int row0, int col, int N, int R) {
    half8_t yg[NR], yu[NR], g[NR], u[NR];
#pragma unroll
    for (int p = 0; p < NR; ++p) load_pairs(y + (size_t)(row0 + r[p]) * (size_t)ldy + 2 * (size_t)col, yg[p], yu[p]);
    segment_pass<NR>(t, 2 * R, Bga, s, yg, g, r, n, row0, N, R);
    segment_pass<NR>(t + R, 2 * R, Bua, s, yu, u, r, n, row0, N, R);
#pragma unroll
    for (int p = 0; p < NR; ++p) {
        if (p >= n) break;
        store_silu_mul(C + (size_t)(row0 + r[p]) * (size_t)ldc + col, g[p], u[p]);
    }
}

__global__ __launch_bounds__(64) void lora_expand_silu_mul_kernel(const float *__restrict__ t, const half_t *__restrict__ Bg, const half_t *__restrict__ Bu,
                                                                  const float *__restrict__ scale, const int32_t *__restrict__ row_adapter, const half_t *__restrict__ y,
                                                                  long long ldy, half_t *__restrict__ C, long long ldc, int rows, int N, int R, int n_adapters) {
    const int a = blockIdx.y, row0 = blockIdx.z * kRowBlock;  // plane n_adapters: the block's rows without an adapter
    const int col = blockIdx.x * kExpandCols + threadIdx.x * 8;
    if (a == n_adapters) {
        if (col >= N) return;  // (N % 8 == 0: a lane's 8 columns -- 8 pairs of y -- are all inside or all outside)
        for (int i = 0; i < kRowBlock && row0 + i < rows; ++i) {
            const int w = row_adapter[row0 + i];
            if (w >= 0 && w < n_adapters) continue;
            half8_t g, u;  // g and u are y's bits
            load_pairs(y + (size_t)(row0 + i) * (size_t)ldy + 2 * (size_t)col, g, u);
            store_silu_mul(C + (size_t)(row0 + i) * (size_t)ldc + col, g, u);
        }
        return;
    }
    int r[kRowBlock] = {0, 0, 0, 0};
    const int n = matching_rows(row_adapter, row0, rows, a, r);
    if (n == 0 || col >= N) return;
    const half_t *Bga = Bg + (size_t)a * R * (size_t)N + col, *Bua = Bu + (size_t)a * R * (size_t)N + col;
    const float s = scale[a];
    if (n == 1)
        gate_up_pass<1>(t, Bga, Bua, s, y, ldy, C, ldc, r, n, row0, col, N, R);
    else if (n == 2)
        gate_up_pass<2>(t, Bga, Bua, s, y, ldy, C, ldc, r, n, row0, col, N, R);
    else  // (three rows run the 4-row form, as in lora_expand_add_kernel)
        gate_up_pass<4>(t, Bga, Bua, s, y, ldy, C, ldc, r, n, row0, col, N, R);
}

}  // namespace

int launch_lora_shrink_f16(const void *x, int ldx, const void *A, const int32_t *row_adapter, float *t, int rows, int K, int R, int n_adapters, hipStream_t stream,
                           hipError_t *hip_err) {
    hipLaunchKernelGGL(lora_shrink_kernel, dim3(R / kShrinkJ, n_adapters, (rows + kRowBlock - 1) / kRowBlock), dim3(kShrinkThreads), 0, stream,
                       static_cast<const half_t *>(x), (long long)ldx, static_cast<const half_t *>(A), row_adapter, t, rows, K, R);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

int launch_lora_expand_add_f16(const float *t, const void *B, const float *scale, const int32_t *row_adapter, void *C, int ldc, int rows, int N, int R, int n_adapters,
                               hipStream_t stream, hipError_t *hip_err) {
    hipLaunchKernelGGL(lora_expand_add_kernel, dim3((N + kExpandCols - 1) / kExpandCols, n_adapters, (rows + kRowBlock - 1) / kRowBlock), dim3(64), 0, stream, t,
                       static_cast<const half_t *>(B), scale, row_adapter, static_cast<half_t *>(C), (long long)ldc, rows, N, R);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

int launch_lora_expand_silu_mul_f16(const float *t, const void *Bg, const void *Bu, const float *scale, const int32_t *row_adapter, const void *y, int ldy, void *C, int ldc,
                                    int rows, int N, int R, int n_adapters, hipStream_t stream, hipError_t *hip_err) {
    hipLaunchKernelGGL(lora_expand_silu_mul_kernel, dim3((N + kExpandCols - 1) / kExpandCols, n_adapters + 1, (rows + kRowBlock - 1) / kRowBlock), dim3(64), 0, stream, t,
                       static_cast<const half_t *>(Bg), static_cast<const half_t *>(Bu), scale, row_adapter, static_cast<const half_t *>(y), (long long)ldy,
                       static_cast<half_t *>(C), (long long)ldc, rows, N, R, n_adapters);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace tce
