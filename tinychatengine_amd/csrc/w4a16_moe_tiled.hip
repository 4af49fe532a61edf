// w4a16_moe_tiled.hip -- the expert-grouped W4A16 contraction on prompt-sized pair counts (include/tce_matmul.h, "Mixture of experts": tce_moe_gate_up_tiled_f16,
// tce_moe_down_tiled_f16), gfx950.  The second form of w4a16_moe.hip's two contractions: the same operands, workspace and epilogues, and per pair THE SAME BITS.
//
// w4a16_moe.hip cuts K over a workgroup's eight waves and runs the pairs of an expert in passes of 16 over a 16-row weight tile: one MFMA per unpacked weight fragment,
// the tile re-read and re-unpacked per pass.  Here a workgroup owns, for one expert, kTN = 128 weight rows x kTM = 128 pairs of its list over the WHOLE K:
//   * 8 waves lie 4 x 2 on the tile: wave (wr, wc) owns weight rows 32 wr .. + 31 and pair columns 64 wc .. + 63, i.e. 2 x 4 MFMA tiles and 32
//     v_mfma_f32_16x16x32_f16 per k-block (128 k).  An unpacked A fragment (w4a16_unpack16.hpp, unchanged) meets 4 column blocks, a B fragment read from LDS 2 row blocks;
//   * per k-block the workgroup stages 128 x 64 bytes of packed q4_6 weights (the stacked arrays as they lie), 128 x 256 bytes of activation rows gathered through
//     list[e] (x[p / k] or act[p]) and the 128 rows' scale / (1024 + 16 z) halves: 40.5 KiB per stage, TWO stages (81 KiB of the 160), one workgroup barrier per
//     k-block.  Global -> registers -> LDS with plain loads: the rows pass pair_permute on the way (the LDS-DMA path cannot permute), and the requests of k-block
//     kb + 1 are issued before the MFMAs of kb and land in LDS after them;
//   * LDS order: weights [row][4 chunks of 16 bytes], the chunk index xor (row / 4) % 4 -- the 16 lanes of an A read (16 rows, one chunk) fall on 16 different 16-byte
//     bank groups; activations per block of 16 columns [16 pieces][16 columns] of 16 bytes, the column xor the piece -- the 16 lanes of a B read (16 columns, one
//     piece) are 256 contiguous bytes and the 16 lanes that write one row's 256 bytes fall on 16 different bank groups (both as in w4a16_moe.hip);
//   * grid (ceil(N / 128)) x (P / 128 + min(E, P)): the host-known bound on sum_e ceil(count[e] / 128).  Every wave reads count[0 .. E) (lane e, clamped to [0, P]),
//     takes the prefix sum of the experts' tile counts and finds its slot's (expert, first pair); a slot past the total leaves at once.  Nothing is added to the
//     workspace, nothing is read back, and a captured graph follows a routing that changes;
//   * no split of K across workgroups, no atomics: every (pair, column) has one writer.
// THE BITS.  Per (pair, weight row) w4a16_moe.hip computes: per k-block blk = four chained MFMA steps from +0, step s of lane group kq on the 8-half piece 4 kq + s
// (weights A, pairs B); acc = fmaf(scale, blk, acc) over the k-blocks of one of EIGHT K slices of gpw = ceil(K / 128 / 8) k-blocks, ascending from +0; the slices added
// in slice order (total = slice 0; total += slice 1; ...; an empty slice is +0); x 1/16; the epilogue.  This kernel issues the same instruction on the same operands
// in the same lanes (an MFMA column's result does not depend on the other columns, a row's not on the other rows), keeps a slice accumulator and folds it into the
// total at every slice edge, and adds +0 for the slices K leaves empty.  The unit is built without packed fp32 arithmetic and with -ffp-contract=off, as w4a16_moe.hip
// is: the K sum is v_fma_f32 / v_add_f32.  tests/test_gpu_moe_tiled.py compares the two forms word for word.
#include "w4a16_moe.hpp"
#include "w4a16_unpack16.hpp"

namespace tce {
namespace {

constexpr int kTN = TCE_MOE_TILE_ROWS, kTM = TCE_MOE_TILE_PAIRS;
constexpr int kWavesN = 4, kWavesM = 2, kThreads = 64 * kWavesN * kWavesM;
constexpr int kRB = kTN / kWavesN / 16, kCB = kTM / kWavesM / 16;  // MFMA row / column blocks of a wave: 2 x 4
constexpr int kStageW = kTN * 64;   // packed weights of a k-block
constexpr int kStageX = kTM * 256;  // gathered rows of a k-block
constexpr int kStageT = 2 * kTN * 2;  // halves [0, kTN): the rows' scales; [kTN, 2 kTN): their 1024 + 16 z
constexpr int kStage = kStageW + kStageX + kStageT;
constexpr int kStages = 2;
static_assert(kThreads == 512 && kTN * 4 == kThreads && kTM * 16 == 4 * kThreads && 2 * kTN <= kThreads, "the request views below: one weight piece, four row pieces, at most one table half per thread");
static_assert(kTM % 16 == 0 && kRB >= 1 && kCB >= 1, "whole MFMA blocks per wave");

template <bool UP, bool Z8>
__global__ __launch_bounds__(kThreads) void w4a16_moe_tiled_kernel(const MoeArgs a, const int E) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- the slot's (expert, first pair): every wave for itself, lane e on count[e] (E <= 64) ----
    int c = lane < E ? a.count[lane] : 0;
    c = c < 0 ? 0 : (c > a.P ? a.P : c);  // (a count the caller wrote itself is not followed past the lists)
    const int tiles = (c + kTM - 1) / kTM;
    int incl = tiles;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(incl, s, 64);
        incl += lane >= s ? o : 0;
    }
    const unsigned long long beyond = __ballot(incl > (int)blockIdx.y);  // the experts whose tiles end past this slot: the first of them owns it
    if (beyond == 0) return;
    const int e = __builtin_amdgcn_readfirstlane(__builtin_ctzll(beyond));
    const int cnt = __builtin_amdgcn_readlane(c, e);  // >= 1: the expert has a tile
    const int first = ((int)blockIdx.y - (__builtin_amdgcn_readlane(incl, e) - __builtin_amdgcn_readlane(tiles, e))) * kTM;  // < cnt

    const int n0 = blockIdx.x * kTN;
    const int nkb = a.K >> 7, nchunks = a.K >> 5, gpw = a.gpw;
    const int32_t *mylist = a.list + (size_t)e * a.P;
    const int r16 = lane & 15, kq = lane >> 4;  // MFMA view: A row / B column r16, k-slice kq
    const int wr = wave >> 1, wc = wave & 1;

    // ---- request views ----
    // weights: thread t asks for the 16-byte chunk t % 4 of row t / 4 (4 lanes = a row's 64 bytes of the k-block)
    const int w_row = tid >> 2, w_chunk = tid & 3;
    const uint4_t *wsrc = a.qweight + ((size_t)e * a.N + (n0 + w_row < a.N ? n0 + w_row : a.N - 1)) * nchunks + w_chunk;
    const int w_wslot = w_row * 4 + (w_chunk ^ ((w_row >> 2) & 3));
    // tables: threads [0, kTN) ask for their row's scale, threads [kTN, 2 kTN) for its zero point (whole waves each)
    const int t_row = n0 + (tid & (kTN - 1)) < a.N ? n0 + (tid & (kTN - 1)) : a.N - 1;
    const half_t *ssrc = a.scales + ((size_t)e * a.N + t_row) * a.scales_stride;
    const unsigned *zsrc = a.zeros + ((size_t)e * a.N + t_row) * a.zeros_stride;
    // rows: piece j of thread t is the 16-byte piece t % 16 of pair column 32 j + t / 16 (16 lanes = a row's 256 bytes of the k-block)
    const half_t *xsrc[4];
    int x_wslot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xm = 32 * j + (tid >> 4), pc = tid & 15;
        const int idx = first + xm < cnt ? first + xm : cnt - 1;  // columns past the list repeat its last pair; they are not stored
        int p = mylist[idx];
        p = p < 0 ? 0 : (p >= a.P ? a.P - 1 : p);  // (no address is formed from a word outside the pairs)
        const int row = UP ? p / a.k : p;
        xsrc[j] = a.X + (size_t)row * (size_t)a.ldx + pc * 8;
        x_wslot[j] = (xm >> 4) * 256 + pc * 16 + ((xm & 15) ^ pc);
    }
    uint4_t Wq, Xq[4];
    half_t tq = (half_t)0.f;
    auto request = [&](int kb) {
        Wq = wsrc[kb * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) Xq[j] = *reinterpret_cast<const uint4_t *>(xsrc[j] + (size_t)kb * 128);
        if (tid < kTN) {
            tq = ssrc[kb];
        } else if (tid < 2 * kTN) {
            unsigned z = 8u;
            if constexpr (!Z8) z = (zsrc[kb >> 3] >> ((kb & 7) * 4)) & 0xFu;
            tq = (half_t)(float)(1024u + 16u * z);  // cz of w4a16_unpack16.hpp, in integers: exact in binary16
        }
    };
    auto land = [&](int stage) {
        unsigned char *st = smem + stage * kStage;
        reinterpret_cast<uint4_t *>(st)[w_wslot] = Wq;
#pragma unroll
        for (int j = 0; j < 4; ++j) reinterpret_cast<uint4_t *>(st + kStageW)[x_wslot[j]] = pair_permute(Xq[j]);
        if (tid < 2 * kTN) reinterpret_cast<half_t *>(st + kStageW + kStageX)[tid] = tq;
    };

    // ---- read views ----
    int a_rslot[kRB], row16[kRB];
#pragma unroll
    for (int rb = 0; rb < kRB; ++rb) {
        row16[rb] = (wr * kRB + rb) * 16;
        a_rslot[rb] = (row16[rb] + r16) * 4 + (kq ^ ((r16 >> 2) & 3));
    }
    int live = (cnt - first - wc * (kTM / kWavesM) + 15) >> 4;  // the wave's column blocks that hold a pair; the others are neither multiplied nor stored
    live = live < 0 ? 0 : (live > kCB ? kCB : live);
    unsigned mask_hi;  // the unpack's nibble mask in a VGPR (w4a16_unpack16.hpp)
    asm volatile("v_mov_b32 %0, 0x00F000F0" : "=v"(mask_hi));

    float4_t total[kRB][kCB], slice[kRB][kCB];  // D[n = 4 kq + i][pair column r16] of block (rb, cb)
#pragma unroll
    for (int rb = 0; rb < kRB; ++rb)
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) total[rb][cb] = slice[rb][cb] = float4_t{0.f, 0.f, 0.f, 0.f};

    request(0);
    land(0);
    __syncthreads();
    int in_slice = 0, slices = 0;
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb + 1 < nkb) request(kb + 1);
        const unsigned char *st = smem + (kb & 1) * kStage;
        const uint4_t *lds_w = reinterpret_cast<const uint4_t *>(st);
        const uint4_t *lds_x = reinterpret_cast<const uint4_t *>(st + kStageW) + wc * kCB * 256;
        const half_t *tab = reinterpret_cast<const half_t *>(st + kStageW + kStageX);
        half8_t A[kRB][4];
        half4_t s4[kRB];
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb) {
            const uint4_t wq = lds_w[a_rslot[rb]];  // row r16 of the block, k-chunk kq: word s feeds MFMA step s
            const half8_t cz8 = unpack16::cz8_splat(tab[kTN + row16[rb] + r16]);
#pragma unroll
            for (int s = 0; s < 4; ++s) A[rb][s] = unpack16::operand8(wq[s], mask_hi, cz8);
            s4[rb] = *reinterpret_cast<const half4_t *>(tab + row16[rb] + 4 * kq);
        }
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            if (cb < live) {
                half8_t B[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int pc = kq * 4 + s;
                    B[s] = __builtin_bit_cast(half8_t, lds_x[cb * 256 + pc * 16 + (r16 ^ pc)]);  // pair column r16 of the block, its piece pc
                }
#pragma unroll
                for (int rb = 0; rb < kRB; ++rb) {
                    float4_t blk = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 4; ++s) blk = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[rb][s], B[s], blk, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) slice[rb][cb][i] = __builtin_fmaf((float)s4[rb][i], blk[i], slice[rb][cb][i]);
                }
            }
        }
        if (++in_slice == gpw || kb + 1 == nkb) {  // a slice edge: what wave `slices` of w4a16_moe.hip hands to its wave 0
#pragma unroll
            for (int rb = 0; rb < kRB; ++rb)
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb) {
                    if (slices == 0) {
                        total[rb][cb] = slice[rb][cb];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) total[rb][cb][i] += slice[rb][cb][i];
                    }
                    slice[rb][cb] = float4_t{0.f, 0.f, 0.f, 0.f};
                }
            in_slice = 0;
            ++slices;
        }
        if (kb + 1 < nkb) land((kb + 1) & 1);  // (stage (kb + 1) & 1 was last read before the barrier that ended k-block kb - 1)
        __syncthreads();
    }
    for (; slices < kMoeWaves; ++slices) {  // the slices K leaves empty: +0 each, as the waves without a k-block add
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb)
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb)
#pragma unroll
                for (int i = 0; i < 4; ++i) total[rb][cb][i] += 0.f;
    }

    // ---- x 1 / 16 and the epilogue of w4a16_moe.hip, every wave on its own blocks ----
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb) {
        const int col = first + (wc * kCB + cb) * 16 + r16;
        if (col >= cnt) continue;
        int p = mylist[col];
        p = p < 0 ? 0 : (p >= a.P ? a.P - 1 : p);
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb) {
            const float4_t acc = total[rb][cb];
            const int nb = n0 + row16[rb] + 4 * kq;
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
}

}  // namespace

size_t moe_tiled_lds_bytes() { return (size_t)kStages * kStage; }

// the tiled form of launch_moe_stage (w4a16_moe.hip): the same arguments, another grid
int launch_moe_stage_tiled(bool up, const void *x, int ldx, const void *qweight, const void *scales, const void *zeros, int rows, int k, int E, int N, int K, int scales_stride,
                           int zeros_stride, bool z8, int n_max, void *workspace, hipStream_t stream, hipError_t *hip_err) {
    const MoeArgs a = moe_stage_args(up, x, ldx, qweight, scales, zeros, rows, k, E, N, K, scales_stride, zeros_stride, n_max, workspace);
    auto kfn = up ? (z8 ? w4a16_moe_tiled_kernel<true, true> : w4a16_moe_tiled_kernel<true, false>)
                  : (z8 ? w4a16_moe_tiled_kernel<false, true> : w4a16_moe_tiled_kernel<false, false>);
    // two stages are more than the 64 KiB a kernel gets by default: the limit is raised ONCE per instantiation (the size does not depend on K)
    static hipError_t raised[4] = {hipErrorNotReady, hipErrorNotReady, hipErrorNotReady, hipErrorNotReady};
    hipError_t &r = raised[(up ? 2 : 0) + (z8 ? 1 : 0)];
    if (r != hipSuccess) r = hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)moe_tiled_lds_bytes());
    if (r != hipSuccess) {
        if (hip_err) *hip_err = r;
        return TCE_ERR_HIP;
    }
    const int P = rows * k;
    // sum_e ceil(count[e] / kTM) <= floor(P / kTM) + (experts with a remainder) <= P / kTM + min(E, P), since sum_e count[e] <= P
    hipLaunchKernelGGL(kfn, dim3((N + kTN - 1) / kTN, P / kTM + (E < P ? E : P)), dim3(kThreads), moe_tiled_lds_bytes(), stream, a, E);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        if (hip_err) *hip_err = err;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace tce
