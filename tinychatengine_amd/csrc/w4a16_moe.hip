// w4a16_moe.hip -- a sparse mixture-of-experts FFN on W4A16 (include/tce_matmul.h, "Mixture of experts": tce_moe_route_f16, tce_moe_gate_up_f16, tce_moe_down_f16,
// tce_moe_combine_add_f16), gfx950.
//
// The expert a row uses is decided per token ON THE DEVICE, so neither a weight pointer nor a row count of these launches is known to the host: every launch has a
// fixed grid, reads the routing words when it runs, and a captured graph follows a routing that changes from replay to replay.
//
//     route     l[e] = x_i . Wr[e] (fp32), the k largest in descending order (ties to the lower index, NaN below every number), softmax weights of the selected;
//               then a STABLE grouping of the rows * k pairs by expert: count[e], list[e][0 .. count[e]) = the pair indices p = i * k + s that name e, ascending
//     gate_up   act[p] = silu_mul_half(fp16(gate_e . x_i), fp16(up_e . x_i))         e = ids[p], i = p / k; gate / up rows interleaved (row 2n gate n, 2n + 1 up n)
//     down      y[p]   = down_e . act[p]                                             fp32, never rounded to fp16
//     combine   C[i][n] = fp16(float(C[i][n]) + sum_s w[i][s] * y[i * k + s][n])    s ascending, one fmaf per slot from +0
//
// The expert-grouped contraction (w4a16_moe_kernel, one template, two epilogues).  Grid (16-row weight tiles of N) x (experts); the experts' linears are the stacked
// q4_6 arrays qweight [E][N][K/8], scales [E][N][scales_stride], zeros [E][N][zeros_stride], read as they are (no second copy).
//   * workgroup (tile, e) reads count[e] -- a uniform address: one scalar load -- and leaves when it is 0;
//   * its 8 waves cut K: wave w owns the k-blocks (128 k) w * gpw .. + gpw - 1, gpw = ceil(K / 128 / 8): a function of K alone.  A wave with no k-block adds zeros;
//   * up to 16 pairs of list[e] are the B operand of v_mfma_f32_16x16x32_f16 (32 k x 16 pairs), gathered per k-block through the wave's LDS slot from the rows the list
//     names (x[p / k] for the up stage, act[p] for the down stage); the unpacked weight tile (16 rows x 32 k) is A: every weight of an active expert meets all rows
//     that chose it in one instruction, and the tile is streamed from HBM once however many of the first 16 pairs name the expert.  Pairs 16 .., 32 .. run further
//     passes over the same tile in list order (from the L2: the kernel is built for decode-sized rows * k); a column past count[e] repeats the last pair and is
//     not stored;
//   * the weight requests of a pass (a group of four k-blocks per wave in flight) are issued BEFORE the list is read, i.e. before anything that depends on the gathered rows;
//   * weights: w4a16_unpack16.hpp's 16 (q - z), exactly; one fp32 scale per (row, group): acc = fmaf(scale, block sum, acc), k-blocks ascending; the final 1 / 16;
//   * no workgroup barrier inside the k-loop (a wave's LDS slot is its own); the waves' fp32 partial tiles meet in LDS and wave 0 adds them in wave order.
// No atomics: a pair is in exactly one list, so every (pair, column) has one writer.  A pair's bits depend on its row's input, its expert's weights, K and the group
// size: not on the other pairs of the pass (MFMA columns are independent), its column, rows, or the grid.
// The weight stream is ROW-MAJOR over the wave's own run of k-blocks: a wave instruction asks for four k-blocks (256 contiguous bytes) of each of 4 tile rows -- 16
// lanes x 16 bytes along one row -- and four such instructions bring a group of four k-blocks of the whole tile.  At K = 4096 that is the wave's whole run of every
// row in one piece.  The q4_6 row pitch (K / 2 bytes) keeps the tile's rows apart, so 1 KiB in one piece would be 16 k-blocks of one row: 16 KiB of staged weights
// per wave for the tile, which the workgroup's LDS does not hold beside the gathered rows.  The wave's LDS slot takes the group in fragment order, so the request
// order and the MFMA order are decoupled.
#include "w4a16_moe.hpp"
#include "w4a16_unpack16.hpp"

namespace tce {
namespace {

constexpr int kWSub = 68;           // 16-byte slots between the k-blocks of a staged group: 64 + 4, so the 16 lanes that write one row's 256 bytes fall on 16 different bank groups
constexpr int kWBuf = 4 * kWSub * 16;  // packed weight group of one wave: 4 k-blocks x 16 rows x 64 bytes
constexpr int kXBuf = 256 * 16;     // gathered activation block of one wave: 16 pairs x 256 bytes
constexpr int kRedBytes = kMoeWaves * 64 * 16;
constexpr int kRouteThreads = 256;  // 4 waves: wave w forms the logits of experts w, w + 4, ...
constexpr int kGroupChunk = 1024;

// fp32 -> a word whose unsigned order is the numbers' order (-0 was made +0 by the caller); every number maps to >= 0x007FFFFF, so 0 ("taken" / no such expert) and
// 1 (NaN) sit below all of them
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kRouteThreads) void moe_route_kernel(const half_t *__restrict__ x, long long ldx, const half_t *__restrict__ Wr, int32_t *__restrict__ ids,
                                                                    float *__restrict__ weights, int hidden, int E, int k, int renormalize) {
    __shared__ float logit[64], ex[64];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint4_t *xr = reinterpret_cast<const uint4_t *>(x + (size_t)row * (size_t)ldx);
    const int pieces = hidden >> 3;
    // logits: lane L takes the 8-element pieces L, L + 64, ... ascending, the 8 elements ascending, one fmaf each; then the xor butterfly 32 .. 1: hidden alone fixes the order
    for (int e = wave; e < E; e += kRouteThreads / 64) {
        const uint4_t *wr = reinterpret_cast<const uint4_t *>(Wr + (size_t)e * hidden);
        float acc = 0.f;
        for (int c = lane; c < pieces; c += 64) {
            const half8_t xh = __builtin_bit_cast(half8_t, xr[c]), wh = __builtin_bit_cast(half8_t, wr[c]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf((float)xh[j], (float)wh[j], acc);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (lane == 0) logit[e] = acc;
    }
    __syncthreads();
    if (wave != 0) return;
    const bool have = lane < E;
    const float l = have ? logit[lane] + 0.0f : 0.f;  // (-0 -> +0: equal numbers are a tie)
    const bool isnan = l != l;
    unsigned key = have ? (isnan ? 1u : order_key(l)) : 0u;
    float m = (have && !isnan) ? l : -INFINITY;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    float p = have ? expf(l - m) : 0.f;
    ex[lane] = p;
    __builtin_amdgcn_wave_barrier();
    float den = 0.f;
    for (int e = 0; e < E; ++e) den += ex[e];  // e ascending (every lane the same sum)
    p = p / den;
    int sel[8];
    float ps[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        sel[s] = 0;
        ps[s] = 0.f;
        if (s < k) {  // the largest key left; equal keys: the larger 63 - lane, i.e. the lower expert
            unsigned long long best = ((unsigned long long)key << 32) | (unsigned)(63 - lane);
#pragma unroll
            for (int t = 32; t >= 1; t >>= 1) {
                const unsigned long long o = __shfl_xor(best, t, 64);
                best = o > best ? o : best;
            }
            const int win = 63 - (int)(best & 63u);  // (k <= E: a lane below E is always left, so win < E)
            sel[s] = win;
            ps[s] = __shfl(p, win, 64);
            if (lane == win) key = 0u;
        }
    }
    if (lane != 0) return;
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (s < k) sum += ps[s];  // slot order
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (s < k) {
            ids[(size_t)row * k + s] = sel[s];
            weights[(size_t)row * k + s] = renormalize ? ps[s] / sum : ps[s];
        }
}

// the stable grouping: lane e walks the pairs in ascending order and keeps those that name e.  One workgroup; the ids pass through LDS a chunk at a time.
__global__ __launch_bounds__(64) void moe_group_kernel(const int32_t *__restrict__ ids, int32_t *__restrict__ count, int32_t *__restrict__ list, int P, int E) {
    __shared__ int32_t chunk[kGroupChunk];
    const int e = threadIdx.x;
    int c = 0;
    for (int base = 0; base < P; base += kGroupChunk) {
        const int n = P - base < kGroupChunk ? P - base : kGroupChunk;
        for (int j = e; j < n; j += 64) chunk[j] = ids[base + j];
        __syncthreads();
        if (e < E)
            for (int j = 0; j < n; ++j)
                if (chunk[j] == e) list[(size_t)e * P + c++] = base + j;
        __syncthreads();
    }
    if (e < E) count[e] = c;
}

template <bool UP, bool Z8>
__global__ __launch_bounds__(64 * kMoeWaves) void w4a16_moe_kernel(const MoeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.y;
    int cnt = a.count[e];
    if (cnt == 0) return;
    cnt = cnt < 0 ? 0 : (cnt > a.P ? a.P : cnt);  // (a count the caller wrote itself is not followed past the lists)
    if (cnt == 0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * 16;
    const int nkb = a.K >> 7, gpw = a.gpw, kb0 = wave * gpw;
    const int my = kb0 < nkb ? (nkb - kb0 < gpw ? nkb - kb0 : gpw) : 0;
    const int nchunks = a.K >> 5;

    // LDS: per wave a weight block, an activation block and its groups' scale / (1024 + 16 z) tables [gpw][16] halves; behind them the partial tiles of the K sum
    unsigned char *wv = smem + (size_t)wave * (kWBuf + kXBuf + (size_t)gpw * 64);
    uint4_t *lds_w = reinterpret_cast<uint4_t *>(wv);
    uint4_t *lds_x = reinterpret_cast<uint4_t *>(wv + kWBuf);
    half_t *tab_s = reinterpret_cast<half_t *>(wv + kWBuf + kXBuf);
    half_t *tab_c = tab_s + gpw * 16;
    float4_t *red = reinterpret_cast<float4_t *>(smem + (size_t)kMoeWaves * (kWBuf + kXBuf + (size_t)gpw * 64));

    const int r16 = lane & 15, kq = lane >> 4;      // MFMA view: A row / B column r16, k-slice kq
    // weight request view: instruction j asks for rows 4 j + lane / 16; along a row the 16 lanes take k-block (lane / 4) % 4 of the group, 16-byte chunk lane % 4 of it
    const int lkb = (lane >> 2) & 3, lchunk = lane & 3;
    const uint4_t *wsrc[4];
    int w_wslot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * j + (lane >> 4);
        const int wrow = n0 + r < a.N ? n0 + r : a.N - 1;
        wsrc[j] = a.qweight + ((size_t)e * a.N + wrow) * nchunks + lchunk + (size_t)kb0 * 4;
        w_wslot[j] = lkb * kWSub + r * 4 + (lchunk ^ j);  // ((r >> 2) & 3 == j: the read side's swizzle)
    }
    const int w_rslot = r16 * 4 + (kq ^ ((r16 >> 2) & 3));
    const int32_t *mylist = a.list + (size_t)e * a.P;
    unsigned mask_hi;  // the unpack's nibble mask in a VGPR (w4a16_unpack16.hpp)
    asm volatile("v_mov_b32 %0, 0x00F000F0" : "=v"(mask_hi));

    bool tables = false;
    for (int pass0 = 0; pass0 < cnt; pass0 += 16) {
        // ---- the pass's first weight requests: nothing in front of them but count[e] ----
        uint4_t W[4];
        auto request = [&](int g4) {  // the group of k-blocks g4 .. g4 + 3 of the wave's run (a k-block past the run repeats its last one: in bounds, never used)
            const int kb = g4 + lkb < my ? g4 + lkb : my - 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) W[j] = wsrc[j][kb * 4];
        };
        if (my > 0) request(0);
        if (!tables) {  // once: the tables of this wave's groups (strided 2-byte reads)
            for (int idx = lane; idx < my * 16; idx += 64) {
                const int g = idx >> 4, r = idx & 15;
                int n = n0 + r;
                n = n < a.N ? n : a.N - 1;
                const int kb = kb0 + g;
                tab_s[idx] = a.scales[((size_t)e * a.N + n) * a.scales_stride + kb];
                unsigned z = 8u;
                if constexpr (!Z8) z = (a.zeros[((size_t)e * a.N + n) * a.zeros_stride + (kb >> 3)] >> ((kb & 7) * 4)) & 0xFu;
                tab_c[idx] = (half_t)(float)(1024u + 16u * z);  // cz of w4a16_unpack16.hpp, in integers: exact in binary16
            }
            tables = true;
        }
        // ---- the pass's pairs: column xm reads the row its list word names (piece j * 64 + lane -> column 4 j + lane / 16, 16-byte piece lane % 16 of the row's 256 bytes) ----
        const half_t *xsrc[4];
        int x_wslot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xm = 4 * j + (lane >> 4), pc = lane & 15;
            const int idx = pass0 + xm < cnt ? pass0 + xm : cnt - 1;  // columns past the list repeat its last pair; they are not stored
            int p = mylist[idx];
            p = p < 0 ? 0 : (p >= a.P ? a.P - 1 : p);  // (no address is formed from a word outside the pairs)
            const int row = UP ? p / a.k : p;
            xsrc[j] = a.X + (size_t)row * (size_t)a.ldx + (size_t)kb0 * 128 + pc * 8;
            x_wslot[j] = pc * 16 + (xm ^ pc);
        }
        float4_t acc = float4_t{0.f, 0.f, 0.f, 0.f};  // D[n = 4 kq + i][pair column r16]
        if (my > 0) {
            uint4_t X[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) X[0][j] = *reinterpret_cast<const uint4_t *>(xsrc[j]);
            for (int g4 = 0; g4 < my; g4 += 4) {
                // registers -> the wave's LDS slot in fragment-friendly order (a wave's LDS operations complete in order: no barrier), then the next group's requests
                // land in the registers this group has just left
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_w[w_wslot[j]] = W[j];
                __builtin_amdgcn_sched_barrier(0);
                if (g4 + 4 < my) request(g4 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int g = g4 + j;
                    if (g < my) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) lds_x[x_wslot[q]] = pair_permute(X[j & 1][q]);
                        __builtin_amdgcn_sched_barrier(0);
                        if (g + 1 < my) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) X[(j + 1) & 1][q] = *reinterpret_cast<const uint4_t *>(xsrc[q] + (g + 1) * 128);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        __builtin_amdgcn_wave_barrier();
                        const uint4_t wq = lds_w[j * kWSub + w_rslot];  // k-block j of the group, row r16, k-chunk kq: word s feeds MFMA step s
                        float4_t blk = float4_t{0.f, 0.f, 0.f, 0.f};
                        const half8_t cz8 = unpack16::cz8_splat(tab_c[g * 16 + r16]);
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int pc = kq * 4 + s;
                            const half8_t xb = __builtin_bit_cast(half8_t, lds_x[pc * 16 + (r16 ^ pc)]);  // pair column r16, its piece pc
                            blk = __builtin_amdgcn_mfma_f32_16x16x32_f16(unpack16::operand8(wq[s], mask_hi, cz8), xb, blk, 0, 0, 0);
                        }
                        __builtin_amdgcn_wave_barrier();
                        const half4_t s4 = *reinterpret_cast<const half4_t *>(tab_s + g * 16 + 4 * kq);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf((float)s4[i], blk[i], acc[i]);
                    }
                }
            }
        }
        // ---- the K slices meet in LDS; wave 0 adds them in wave order, scales by 1 / 16, runs the epilogue ----
        red[wave * 64 + lane] = acc;
        __syncthreads();
        if (wave == 0) {
            acc = red[lane];
#pragma unroll
            for (int w = 1; w < kMoeWaves; ++w) {
                const float4_t o = red[w * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += o[i];
            }
            if (pass0 + r16 < cnt) {
                int p = mylist[pass0 + r16];
                p = p < 0 ? 0 : (p >= a.P ? a.P - 1 : p);
                const int nb = n0 + 4 * kq;
                if constexpr (UP) {  // tile rows (2n, 2n + 1) = (gate n, up n), each rounded to fp16 first: the arithmetic of TCE_W4_SILU_MUL_PAIRS
                    half_t *arow = static_cast<half_t *>(a.out) + (size_t)p * a.ld_out;
                    if (nb + 1 < a.N) arow[nb >> 1] = silu_mul_half((half_t)(acc[0] * 0.0625f), (half_t)(acc[1] * 0.0625f));
                    if (nb + 3 < a.N) arow[(nb >> 1) + 1] = silu_mul_half((half_t)(acc[2] * 0.0625f), (half_t)(acc[3] * 0.0625f));
                } else {
                    float *yrow = static_cast<float *>(a.out) + (size_t)p * a.ld_out;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (nb + i < a.N) yrow[nb + i] = acc[i] * 0.0625f;
                }
            }
        }
        if (pass0 + 16 < cnt) __syncthreads();  // (the next pass writes `red` again)
    }
}

// 16-byte pieces over C: a thread owns 8 adjacent columns of one row and walks the row's k slots in ascending order
__global__ __launch_bounds__(256) void moe_combine_add_kernel(half_t *__restrict__ C, long long ldc, const int32_t *__restrict__ ids, const float *__restrict__ weights,
                                                               const float *__restrict__ y, int N, int k, int E, int blocks_per_row) {
    const int row = blockIdx.x / blocks_per_row;
    const int col = ((blockIdx.x % blocks_per_row) * 256 + threadIdx.x) * 8;
    if (col >= N) return;  // (N % 8 == 0: a thread's 8 columns are all inside or all outside)
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int s = 0; s < k; ++s) {
        const size_t p = (size_t)row * k + s;
        const int id = ids[p];
        if (id < 0 || id >= E) continue;  // such a pair is in no list: nothing was written for it
        const float w = weights[p];
        const float4_t *yp = reinterpret_cast<const float4_t *>(y + p * (size_t)N + col);
        const float4_t y0 = yp[0], y1 = yp[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = fmaf(w, y0[j], acc[j]);
            acc[4 + j] = fmaf(w, y1[j], acc[4 + j]);
        }
    }
    uint4_t *cp = reinterpret_cast<uint4_t *>(C + (size_t)row * (size_t)ldc + col);
    const half8_t ch = __builtin_bit_cast(half8_t, *cp);
    half8_t out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (half_t)((float)ch[j] + acc[j]);
    *cp = __builtin_bit_cast(uint4_t, out);
}

int launched(hipError_t *hip_err) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace

size_t moe_workspace_bytes(int rows, int k, int E, int n_max) { return moe_layout(rows, k, E, n_max).total; }

size_t moe_lds_bytes(int K) { return (size_t)kMoeWaves * (kWBuf + kXBuf + (size_t)moe_gpw(K) * 64) + kRedBytes; }

// the route's first launch alone: ids and weights (the grouping behind it is moe_group_kernel below, or w4a16_moe_group.hip's pair of launches)
int launch_moe_route_select_f16(const void *x, int ldx, const void *Wr, int rows, int hidden, int E, int k, int renormalize, int n_max, void *workspace, hipStream_t stream,
                                hipError_t *hip_err) {
    const MoeLayout L = moe_layout(rows, k, E, n_max);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    hipLaunchKernelGGL(moe_route_kernel, dim3(rows), dim3(kRouteThreads), 0, stream, static_cast<const half_t *>(x), (long long)ldx, static_cast<const half_t *>(Wr),
                       reinterpret_cast<int32_t *>(ws + L.ids), reinterpret_cast<float *>(ws + L.weights), hidden, E, k, renormalize);
    return launched(hip_err);
}

int launch_moe_route_f16(const void *x, int ldx, const void *Wr, int rows, int hidden, int E, int k, int renormalize, int n_max, void *workspace, hipStream_t stream,
                         hipError_t *hip_err) {
    if (const int rc = launch_moe_route_select_f16(x, ldx, Wr, rows, hidden, E, k, renormalize, n_max, workspace, stream, hip_err)) return rc;
    const MoeLayout L = moe_layout(rows, k, E, n_max);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const int32_t *>(ws + L.ids), reinterpret_cast<int32_t *>(ws + L.count),
                       reinterpret_cast<int32_t *>(ws + L.list), rows * k, E);
    return launched(hip_err);
}

// one contraction stage: up (x fp16 [rows][ldx] -> act fp16 [P][N / 2]) or down (act fp16 [P][K] -> y fp32 [P][N])
int launch_moe_stage(bool up, const void *x, int ldx, const void *qweight, const void *scales, const void *zeros, int rows, int k, int E, int N, int K, int scales_stride,
                     int zeros_stride, bool z8, int n_max, void *workspace, hipStream_t stream, hipError_t *hip_err) {
    const MoeArgs a = moe_stage_args(up, x, ldx, qweight, scales, zeros, rows, k, E, N, K, scales_stride, zeros_stride, n_max, workspace);
    const size_t lds = moe_lds_bytes(K);
    auto kfn = up ? (z8 ? w4a16_moe_kernel<true, true> : w4a16_moe_kernel<true, false>) : (z8 ? w4a16_moe_kernel<false, true> : w4a16_moe_kernel<false, false>);
    // every K needs more than the 64 KiB a kernel gets by default: the limit is raised ONCE per instantiation, to what the largest accepted K (32768) needs, not per launch
    static hipError_t raised[4] = {hipErrorNotReady, hipErrorNotReady, hipErrorNotReady, hipErrorNotReady};
    hipError_t &r = raised[(up ? 2 : 0) + (z8 ? 1 : 0)];
    if (r != hipSuccess) r = hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)moe_lds_bytes(32768));
    if (r != hipSuccess) {
        if (hip_err) *hip_err = r;
        return TCE_ERR_HIP;
    }
    hipLaunchKernelGGL(kfn, dim3((N + 15) / 16, E), dim3(64 * kMoeWaves), lds, stream, a);
    return launched(hip_err);
}

int launch_moe_combine_add_f16(void *C, int ldc, int rows, int k, int E, int N, int n_max, const void *workspace, hipStream_t stream, hipError_t *hip_err) {
    const MoeLayout L = moe_layout(rows, k, E, n_max);
    const unsigned char *ws = static_cast<const unsigned char *>(workspace);
    const int bpr = (N / 8 + 255) / 256;
    hipLaunchKernelGGL(moe_combine_add_kernel, dim3((unsigned)rows * bpr), dim3(256), 0, stream, static_cast<half_t *>(C), (long long)ldc,
                       reinterpret_cast<const int32_t *>(ws + L.ids), reinterpret_cast<const float *>(ws + L.weights), reinterpret_cast<const float *>(ws + L.y), N, k, E, bpr);
    return launched(hip_err);
}

}  // namespace tce
