// attention_prefill.hip -- the reference's Llama attention block between the fused q/k/v linear and o_proj for m > 1 new rows
// (a prompt, or a chunk of one on top of an existing context): the prefill form of attention_fast.hip's decode step.
//
// What it replaces (llm/src/nn_modules/cuda/Int4llamaAttention.cu:116-229, the same code path as decode, sqlen > 1):
//     shape_qkv_cuda (:41-64, 130-136)          the fused projection's rows [m][(heads + 2 kv_heads) * hd] are read where they lie
//     RotaryPosEmb_cuda_forward (:157-159)      the reference's binary16 arithmetic hfma(x, cos, hmul(rot, sin)) (RotaryPosEmb.cu:4-34) on q and
//                                               the new keys: the keys that enter the cache are bit-identical to the reference's (and to what m
//                                               decode steps would append)
//     the KV append (:161-181)                  rows pos .. pos + m - 1 of the fixed-capacity caches [kv_heads][max_keys][hd] are written; nothing is copied
//     qk_bmm -> batch_Add -> check_inf_half -> softmax -> transpose_1_2idx -> pv_bmm -> unshape (:184-217)
//                                               one pass over the keys per (query head, 64 query rows): scores on the matrix pipe
//                                               (v_mfma_f32_16x16x32_f16, fp32 accumulate), online softmax in fp32, probabilities x values on the
//                                               matrix pipe, the output rows [m][heads * hd] are o_proj's input
// Two launches: `prepare` (element-wise: rotation + append + the rotated queries into a workspace) and the attention kernel.
//
// This is NOT the reference's arithmetic (binary16 accumulation chains, one thread per output: tce_bmm_f16t + tce_softmax_half reproduce those bit for
// bit and stay the compat path); it computes the same function with fp32 accumulation and is held to a float64 evaluation with a stated tolerance
// (tests/test_gpu_attention.py), like the decode step.
//
// Attention kernel: workgroup = (block of 64 or 128 query rows, query head), 4 or 8 waves x 16 query rows.  Per tile of 64 keys:
//   * the K tile [64 keys][128] is staged in LDS as it lies (row stride 272 bytes: the MFMA B fragments -- key = lane % 16, 8 consecutive head
//     dimensions -- are conflict-free 16-byte reads); S = Q K^T: 4 key tiles x 4 k-steps of 32 head dimensions, the Q fragments stay in registers;
//   * scale, additive mask, causal cut, online softmax in fp32 in registers (log2 units: one v_exp_f32 per probability; the validity tests only on tiles
//     that hold keys past the context or on the causal diagonal);
//   * everything is computed transposed (see the kernel): S^T = K Q^T leaves ONE query row per lane, so P never touches LDS -- the S^T accumulator
//     layout is the B-operand layout of v_mfma_f32_16x16x16_f16 -- and O^T += V^T P^T;
//   * the V tile is staged as it lies too (row stride 288 bytes); the P V product contracts over keys and an MFMA operand wants its contraction index
//     contiguous per lane, which a row-major V does not give: gfx950's LDS transpose read (ds_read_b64_tr_b16) hands each lane 4 keys of one head dimension
//     out of a [4 keys][16 dims] block.  (The first version transposed V while staging it -- eight 2-byte LDS writes per 16 bytes, the global loads one
//     row per lane -- and ran 158 us at 2048 rows; this one 130.)
// Grouped-query attention: query head i reads key / value head i / (heads / kv_heads); the workgroups of a group stage the same tiles (L2).
// Rows of the caches at and beyond pos + m may hold anything (uninitialised memory): staged as zeros, and their scores are cut.
//
// The PAGED form of both launches (tce_attention_prefill_paged_f16): the caches are the paged step's pools [num_pages][kv_heads][page_keys][hd] behind a block table
// (attention_fast.hip), and one launch serves up to kMaxSegments sequences -- a segment is {slot, pos, m, row0}: m new rows, rows row0 .. row0 + m - 1 of qkv / out, on
// top of pos cached keys of table row `slot`.  Only a row's ADDRESS changes: what is appended and what comes out is bit-identical to the contiguous launch of each
// segment alone.  Trust, as for the paged step: of a segment's table row only words 0 .. (pos + m - 1) / page_keys become addresses, no page number is validated, and no
// pool row other than rows pos .. pos + m - 1 of each segment is written.
#include <algorithm>

#include "tce_common.hpp"
#include "w4a16_kernels.hpp"
#include "fp8_kv.hpp"
#include "attn_dispatch.hpp"

namespace tce {

namespace {

constexpr int kHD = 128;
constexpr int kBK = 64;
constexpr int kKStride = 272;  // bytes per key row of the K tile in LDS
constexpr int kVStride = 288;  // bytes per key row of the V tile (72 dwords = 8 mod 64: the 8 key rows a 32-lane half reads with the transpose read hit 64 different banks)
constexpr float kNegBig = -1.0e30f;

struct PrepareArgs {
    const half_t *qkv;  // [m][ld_qkv]: per row the query heads, the key heads, the value heads
    int ld_qkv;
    half_t *qrot;       // [heads][m][hd]
    half_t *kc, *vc;    // [kv_heads][max_keys][hd]
    const half_t *cosv, *sinv;
    int heads, kv_heads, max_keys, pos, m;
};

// tce_prefill_segment's layout (include/tce_matmul.h)
struct PrefillSegment {
    int slot, pos, m, row0;
};
constexpr int kMaxSegments = 16;          // TCE_PREFILL_MAX_SEGMENTS
constexpr int kMaxListedBlocks = 1024;    // query blocks of one paged launch (their order travels in the kernel arguments)

// the paged prepare's arguments: the rows of every segment in one launch
struct PagedPrepareArgs {
    const half_t *qkv;  // [total_rows][ld_qkv]
    int ld_qkv;
    half_t *qrot;       // [heads][total_rows][hd]
    half_t *kc, *vc;    // the pools [num_pages][kv_heads][page_keys][hd]
    const half_t *cosv, *sinv;
    const int *table;   // int32 [table_rows][table_stride]
    int table_stride, page_shift;
    int heads, kv_heads, total_rows, nseg;
    PrefillSegment seg[kMaxSegments];
};

// the e4m3 form's (tce_attention_prefill_paged_fp8): kc / vc are pools of bytes; what a rotated key / a value row is multiplied by before it is rounded to bytes
struct PagedPrepareFp8Args : PagedPrepareArgs {
    float k_inv, v_inv;  // 2^-k_scale_log2, 2^-v_scale_log2
};

// one thread per 16-byte piece of a (row, head slot): rotation as RotaryPosEmb_cuda_forward (hd = 128: the partner half is piece ^ 8)
// PAGED: row r belongs to the segment whose row range holds it (a row in none is skipped), its position is that segment's pos + (r - row0), and the appended row goes
// to the page the segment's table row names for that position.
// FP8 (with PAGED): the rotation is the same binary16 statement; rows of query heads go to the fp16 workspace unchanged, rows of key and value heads are rounded to
// e4m3 (fp8_kv.hpp) and stored as 8-byte pieces of their page's 128-byte row.
template <bool PAGED = false, bool FP8 = false>
__global__ __launch_bounds__(256) void attn_prefill_prepare_kernel(const std::conditional_t<FP8, PagedPrepareFp8Args, std::conditional_t<PAGED, PagedPrepareArgs, PrepareArgs>> a) {
    static_assert(!FP8 || PAGED, "e4m3 caches exist as pages only");
    const int slots = a.heads + 2 * a.kv_heads;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    int rows;
    if constexpr (PAGED) rows = a.total_rows;
    else rows = a.m;
    if (idx >= (long long)rows * slots * 16) return;
    const int piece = (int)(idx & 15);
    const int hs = (int)((idx >> 4) % slots), r = (int)((idx >> 4) / slots);
    int key;            // the row's position: its key index in the cache
    int slot = 0;
    if constexpr (PAGED) {
        key = -1;
        for (int s = 0; s < a.nseg; ++s) {
            const int d = r - a.seg[s].row0;
            if (d >= 0 && d < a.seg[s].m) {
                key = a.seg[s].pos + d;
                slot = a.seg[s].slot;
            }
        }
        if (key < 0) return;
    } else {
        key = a.pos + r;
    }
    const half_t *src = a.qkv + (size_t)r * a.ld_qkv + (size_t)hs * kHD;
    half8_t v = *reinterpret_cast<const half8_t *>(src + piece * 8);
    if (hs < a.heads + a.kv_heads && a.cosv) {
        const half8_t p = *reinterpret_cast<const half8_t *>(src + (piece ^ 8) * 8);
        const half8_t c = *reinterpret_cast<const half8_t *>(a.cosv + (size_t)key * kHD + piece * 8);
        const half8_t s = *reinterpret_cast<const half8_t *>(a.sinv + (size_t)key * kHD + piece * 8);
        half8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const half_t rot = piece < 8 ? (half_t)(-p[e]) : p[e];
            const half_t t = rot * s[e];             // hmul
            o[e] = __builtin_fmaf16(v[e], c[e], t);  // hfma, one rounding (the same statement as the decode step's and tce_rope_half's)
        }
        v = o;
    }
    half_t *dst;
    if constexpr (PAGED) {
        if (hs < a.heads) {
            dst = a.qrot + ((size_t)hs * a.total_rows + r) * kHD;
        } else {
            const int page = a.table[(size_t)slot * a.table_stride + (key >> a.page_shift)];
            const int h = hs < a.heads + a.kv_heads ? hs - a.heads : hs - a.heads - a.kv_heads;
            const size_t off = ((((size_t)page * a.kv_heads + h) << a.page_shift) + (key & ((1 << a.page_shift) - 1))) * kHD;
            if constexpr (FP8) {  // (an element is a byte: the same offset counts bytes)
                const bool is_k = hs < a.heads + a.kv_heads;
                unsigned char *row = reinterpret_cast<unsigned char *>(is_k ? a.kc : a.vc) + off;
                *reinterpret_cast<uint2_t *>(row + piece * 8) = fp8_quant8(v, is_k ? a.k_inv : a.v_inv);
                return;
            }
            dst = (hs < a.heads + a.kv_heads ? a.kc : a.vc) + off;
        }
    } else {
        if (hs < a.heads) dst = a.qrot + ((size_t)hs * a.m + r) * kHD;
        else if (hs < a.heads + a.kv_heads) dst = a.kc + ((size_t)(hs - a.heads) * a.max_keys + a.pos + r) * kHD;
        else dst = a.vc + ((size_t)(hs - a.heads - a.kv_heads) * a.max_keys + a.pos + r) * kHD;
    }
    *reinterpret_cast<half8_t *>(dst + piece * 8) = v;
}

struct PrefillArgs {
    const half_t *qrot;      // [heads][m][hd]
    const half_t *kc, *vc;   // [kv_heads][max_keys][hd]
    const half_t *mask;      // [m][ld_mask] additive, or null
    half_t *out;             // [m][ld_out]: row r, columns head * hd ..
    int ld_mask, ld_out;
    int heads, rep, max_keys, pos, m, causal;
    int pair;  // a workgroup takes two query blocks (see attn_prefill_kernel)
    float alpha;
};

// the paged attention launch's arguments.  `order` lists the launch's query blocks, heaviest (most key tiles) first: entry i = segment << 12 | query block, two
// entries per word; workgroup i takes entry i and, paired, entry nblocks - 1 - i after it.
struct PagedPrefillArgs {
    const half_t *qrot;      // [heads][total_rows][hd]
    const half_t *kc, *vc;   // the pools
    half_t *out;             // [total_rows][ld_out]
    const int *table;        // int32 [table_rows][table_stride]
    int ld_out;
    int heads, rep, kv_heads, total_rows, causal;
    int pair;
    int table_stride, page_shift, nblocks;
    float alpha;
    PrefillSegment seg[kMaxSegments];
    unsigned order[kMaxListedBlocks / 2];
};
// the e4m3, windowed (fp16 and e4m3 pools: the two scales are unused on fp16 pools) and sink launches': each the one before and its own fields, so that a launcher
// fills the last and hands any form its base.  paged_prefill_args_t names a form's
struct PagedPrefillFp8Args : PagedPrefillArgs {
    float k_scale, v_scale;
};
struct PagedPrefillWindowArgs : PagedPrefillFp8Args {
    int window;
};
struct PagedPrefillSinkArgs : PagedPrefillWindowArgs {
    int sinks;
    const half_t *qkv;
    int ld_qkv;
    const half_t *cos_s, *sin_s;
};
template <bool FP8, bool WINDOW, bool SINK>
using paged_prefill_args_t = std::conditional_t<SINK, PagedPrefillSinkArgs, std::conditional_t<WINDOW, PagedPrefillWindowArgs, std::conditional_t<FP8, PagedPrefillFp8Args, PagedPrefillArgs>>>;

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum(float v) {  // over the 16 lanes of a DPP row, result in every lane of the row
    v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_f<0x141>(v);  // row_half_mirror
    v += dpp_f<0x140>(v);  // row_mirror
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_f<0xB1>(v));
    v = fmaxf(v, dpp_f<0x4E>(v));
    v = fmaxf(v, dpp_f<0x141>(v));
    v = fmaxf(v, dpp_f<0x140>(v));
    return v;
}

// NW: waves per workgroup; RT: 16-row MFMA tiles per wave (2: a K / V fragment feeds two MFMAs; kept for the sweep that ruled it out: > 200 registers,
// half the occupancy).  A block is 16 * RT * NW query rows: a staged K / V tile serves all of them.
//
// Everything is computed TRANSPOSED so that nothing but the operands' tiles touches LDS:
//   S^T = K Q^T    A = a K fragment (row = key, 8 head dimensions), B = the Q fragment (column = query row): the accumulator lane (n16, quad) holds
//                  query row n16, keys 16 j + 4 quad + r -- ONE query row per lane, so the online-softmax state is one (m, l) per lane and row tile,
//                  the row maximum is a register maximum over (j, r) plus two cross-quad exchanges, and the row sum stays a per-lane partial until the end
//                  (the rescale factor is the same in the four quads);
//   O^T += V^T P^T  on v_mfma_f32_16x16x16_f16 (contraction = 16 keys, 4 per lane): the B operand -- column = query row n16, keys 4 quad .. 4 quad + 3 -- IS
//                  the S^T accumulator layout of key tile j: the probabilities go from fp32 to packed fp16 in registers and never see LDS; A = a V^T
//                  fragment (row = head dimension, 4 keys: an 8-byte LDS read); the accumulator holds head dimensions 16 c + 4 quad + r of query row n16.
// The validity tests (keys past the context, the causal diagonal) run only on tiles that contain such keys.
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) fp16x4_t lds_fp16x4_t;

__device__ __forceinline__ float quad_max(float v) {  // over the four lanes n16, n16 + 16, n16 + 32, n16 + 48
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// PAGED: query block qb of one segment of a paged launch (PagedBlockArgs).  The rows of qrot / out are the segment's (row0 + ...), and a key row's address comes
// from the segment's table row: a tile of 64 keys is four runs of 16 keys, each inside one page (page_keys is a power of two >= 16), so a tile needs four table
// words -- one load per tile and wave, requested a whole tile ahead of the row requests that use them (TileWords), so that no row request ever waits for a table
// word.  Everything behind the fetch is the contiguous kernel's.
// (The paged kernel hands the block a PagedBlockArgs: the launch's arguments with one segment's pos / m / row0 / table row filled in, so that the statements both forms
// share read a.pos and a.m as they always did -- the contiguous instantiations compile to the instructions they compiled to before the flag existed.)
struct PagedBlockArgs {
    const half_t *qrot, *kc, *vc;
    half_t *out;
    const int *trow;  // the segment's table row
    int ld_out, rep, kv_heads, total_rows, row0, pos, m, causal, page_shift;
    float alpha;
    // FP8: the pools hold bytes, a tile's rows are dequantised on their way into LDS
    float k_scale, v_scale;  // 2^k_scale_log2, 2^v_scale_log2
    // WINDOW (causal only): row i of the segment sits at p = pos + i and weighs keys max(0, p - window + 1) .. p
    int window;  // >= 1
    // SINK (attention sinks beside the window): row i at p = pos + i BINDS iff p >= sinks + window and then weighs keys 0 .. sinks - 1, scored with its raw q rotated
    // by cos / sin row sinks + window - 1, beside keys p - window + 1 .. p; a row that does not bind weighs keys 0 .. p
    int sinks;                    // 1 .. 16
    const half_t *qkv;            // the launch's raw rows [total_rows][ld_qkv]: the second rotation is made from them in registers
    int ld_qkv;
    const half_t *cos_s, *sin_s;  // row sinks + window - 1 of the tables, or null (no rotation: the second query is the first)
};

// what differs between the forms in the statements they share: the row count and first row of the segment inside qrot / out, and a key / value head's base
__device__ __forceinline__ int qrows(const PrefillArgs &a) { return a.m; }
__device__ __forceinline__ int qrows(const PagedBlockArgs &a) { return a.total_rows; }
__device__ __forceinline__ int qrow0(const PrefillArgs &) { return 0; }
__device__ __forceinline__ int qrow0(const PagedBlockArgs &a) { return a.row0; }
__device__ __forceinline__ int head_keys(const PrefillArgs &a) { return a.max_keys; }
__device__ __forceinline__ int head_keys(const PagedBlockArgs &) { return 0; }  // (the head is part of a page's address: both bases are the pools')

// The table words of the four 16-key runs of one tile: lane l holds the word of run l % 4, fetched with ONE vector load whose request follows the row requests
// of the tile before -- vector loads return in order, so the word is there when those rows are (the wait in front of the LDS writes).  latch() moves the four words
// to scalars right behind that wait, unconditionally and outside the row requests' branches: no wait of its own, ever, and the compiler can see that the register is
// free again when the next request is issued.  (Measured first: scalar loads in front of the tile's first barrier -- the barrier's s_waitcnt lgkmcnt(0) waited for
// them at every tile, 6-16 % of the launch; then v_readlane inside the `key < kend` branches -- the compiler waited for ALL outstanding rows before each one.)
// Word indices are clamped to the last word the block may follow, (kend - 1) / page_keys: a run wholly at or beyond kend requests no row.
template <bool PAGED>
struct TileWords {};
template <>
struct TileWords<true> {
    int v, w[4];
    __device__ __forceinline__ void request(const PagedBlockArgs &a, int kt, int kend, int lane) {
        const int lastw = (kend - 1) >> a.page_shift;
        const int e = (kt * kBK + 16 * (lane & 3)) >> a.page_shift;
        v = a.trow[e < lastw ? e : lastw];
    }
    // SINK: the sink pass's tile -- keys 0 .. sinks - 1 <= 15, all in word 0's page
    __device__ __forceinline__ void request_word0(const PagedBlockArgs &a) { v = a.trow[0]; }
    // WINDOW: additionally clamped from below to the word of the block's first visible key, `firstw`: words under it may name pages that were given back
    __device__ __forceinline__ void request_from(const PagedBlockArgs &a, int kt, int kend, int lane, int firstw) {
        const int lastw = (kend - 1) >> a.page_shift;
        const int e = (kt * kBK + 16 * (lane & 3)) >> a.page_shift;
        v = a.trow[e < firstw ? firstw : (e < lastw ? e : lastw)];
    }
    __device__ __forceinline__ void latch() {
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = __builtin_amdgcn_readlane(v, r);
    }
};

// FP8 (with PAGED): a row of the pools is 128 e4m3 bytes; fetch_tile requests 8-byte pieces and the write into LDS dequantises them (exactly: fp8_kv.hpp), so the K
// and V tiles in LDS are the same fp16 images at the same strides and everything behind them is shared text.
// WINDOW (with PAGED, causal launches only): sliding-window attention.  The block walks key tiles from the tile of klo = lo(its first row) to the
// tile of its last row's position; tiles wholly below are neither requested nor computed, and keys below klo -- which may lie in pages that were given back -- are staged
// as zeros like the keys at and beyond kend.  The lower bound is tested on the tiles that hold a key below the lo of one of the wave's rows: the causal diagonal's `edge`.
// SINK (with WINDOW): the window pass is the windowed block's with lo_r = 0 for a row that does not bind (klo: the lo of the block's FIRST row, 0 if that
// row does not bind).  A block whose last row binds then makes one SINK PASS, the loop's last iteration (index ntiles): key tile 0 with keys >= sinks staged as zeros, scored
// against Q_s -- the rows' raw q rotated with row sinks + window - 1, made in registers from qkv at the head of that iteration with the prepare kernel's binary16 statement
// (a fragment's partner half qf[t][s ^ 2] is in the same lane) and put where Q was: no register is held for it through the window pass.  Keys >= sinks and rows that do not
// bind are cut; a fully cut tile leaves a row's state as it was.  A block none of whose rows binds walks exactly the windowed block's tiles.
template <bool MASK, int NW, int RT, bool PAGED = false, bool FP8 = false, bool WINDOW = false, bool SINK = false>
__device__ __forceinline__ void attn_prefill_block(const std::conditional_t<PAGED, PagedBlockArgs, PrefillArgs> &a, const int qb, const int head, unsigned char *ks, unsigned char *vs) {
    static_assert(!SINK || WINDOW, "sinks exist beside a window");
    static_assert(!PAGED || !MASK, "the paged form takes no additive mask");
    static_assert(!WINDOW || PAGED, "a window exists on pages only");
    static_assert(!FP8 || PAGED, "e4m3 caches exist as pages only");
    constexpr int kBQ = 16 * RT * NW, NT = 64 * NW, KI = 1024 / NT;
    constexpr float kLog2e = 1.4426950408889634f;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, quad = lane >> 4;
    const int kvh = head / a.rep;
    const int tgz = a.pos + a.m;
    const int r0 = qb * kBQ + wave * 16 * RT;
    // keys this block needs: all of them, or (causal) up to the block's last row's own position
    const int last_row = (qb * kBQ + kBQ < a.m ? qb * kBQ + kBQ : a.m) - 1;
    const int kend = a.causal ? a.pos + last_row + 1 : tgz;
    const int ntiles = (kend + kBK - 1) / kBK;
    // WINDOW: the first key the block's first row weighs -- no row of the block weighs an earlier one -- and its tile; else 0
    [[maybe_unused]] const int klo = [&]() -> int {
        if constexpr (SINK) return a.pos + qb * kBQ - a.window >= a.sinks ? a.pos + qb * kBQ - a.window + 1 : 0;
        else if constexpr (WINDOW) return a.pos + qb * kBQ - a.window + 1 > 0 ? a.pos + qb * kBQ - a.window + 1 : 0;
        else return 0;
    }();
    const int kt0 = WINDOW ? klo / kBK : 0;
    // SINK: the tiles of the loop, the sink pass (index ntiles) included when the block's last row binds
    int nt_all = ntiles;
    if constexpr (SINK) nt_all += a.pos + last_row - a.window >= a.sinks ? 1 : 0;
    const float scale2 = a.alpha * kLog2e;  // scores in units of log2: exp(x) = exp2(x * log2 e), one v_exp_f32 per probability

    // Q fragments of row tile t: row r0 + 16 t + n16 (clamped), head dimensions 32 s + 8 quad ..; that row is also the lane's softmax row
    half8_t qf[RT][4];
    int rowc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int row = r0 + 16 * t + n16;
        rowc[t] = row < a.m ? row : a.m - 1;
        const half_t *qrow = a.qrot + ((size_t)head * qrows(a) + qrow0(a) + rowc[t]) * kHD;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[t][s] = *reinterpret_cast<const half8_t *>(qrow + 32 * s + 8 * quad);
    }
    float4_t o[RT][8];     // O^T: head dimensions 16 c + 4 quad + r of query row n16
    float m_i[RT], l_i[RT];  // the row's running maximum (log2 units; the same in the four quads) and this lane's share of its sum
#pragma unroll
    for (int t = 0; t < RT; ++t) {
#pragma unroll
        for (int c = 0; c < 8; ++c) o[t][c] = float4_t{0.f, 0.f, 0.f, 0.f};
        m_i[t] = kNegBig;
        l_i[t] = 0.f;
    }
    const half_t *kbase = a.kc + (size_t)kvh * head_keys(a) * kHD, *vbase = a.vc + (size_t)kvh * head_keys(a) * kHD;
    TileWords<PAGED> tw;  // PAGED: the table words of the tile that is fetched next

    // a tile's global loads, K and V alike: piece idx = tid + NT i -> key idx / 16, piece idx % 16 (coalesced rows).  The loads of tile kt + 1 are requested
    // before tile kt is multiplied (registers) and written to LDS once every wave is done with tile kt.  (A ring of 3-4 register sets, tiles requested that
    // far ahead, measured SLOWER -- 151 -> 202 us at 2048 rows: the registers cost occupancy and the rows were not what the waves waited for.)
    using piece_t = std::conditional_t<FP8, uint2_t, half8_t>;  // a lane's 8 elements of a row between request and LDS write
    piece_t kreg[KI], vreg[KI];
    auto fetch_tile = [&](int kt) {
        const bool sink_tile = [&]() -> bool {  // (SINK: the sink pass reads tile 0, keys 0 .. sinks - 1 of it)
            if constexpr (SINK) return kt == ntiles;
            else return false;
        }();
        const int key0 = [&]() -> int {
            if constexpr (SINK) return sink_tile ? 0 : kt * kBK;
            else return kt * kBK;
        }();
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const int idx = tid + NT * i, gk = key0 + (idx >> 4);
            if constexpr (FP8) {  // (byte 0 is +0)
                kreg[i] = uint2_t{0u, 0u};
                vreg[i] = uint2_t{0u, 0u};
            } else {
                kreg[i] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
                vreg[i] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
            }
            const bool wanted = [&]() -> bool {
                if constexpr (SINK) return sink_tile ? gk < a.sinks : (gk < kend && gk >= klo);
                else return gk < kend && (!WINDOW || gk >= klo);
            }();
            if (wanted) {
                if constexpr (PAGED) {
                    // the piece's run of the tile: i with 4 waves (a pass of 256 pieces is 16 keys), 2 i + wave / 4 with 8 -- wave-uniform, so the page is a scalar
                    const int page = NT == 256 ? tw.w[i] : (wave >= 4 ? tw.w[(2 * i + 1) & 3] : tw.w[(2 * i) & 3]);
                    const int run0 = key0 + 16 * (NT == 256 ? i : 2 * i + (wave >> 2));
                    const size_t off = ((((size_t)page * a.kv_heads + kvh) << a.page_shift) + (run0 & ((1 << a.page_shift) - 1))) * kHD;
                    // (the lane's offset inside a 16-key run: row (tid / 16) % 16, its 16-byte piece -- the same for every tile)
                    const unsigned lane_off = (unsigned)(((tid >> 4) & 15) * kHD + (tid & 15) * 8);
                    if constexpr (FP8) {  // (an element is a byte: the same offsets count bytes)
                        kreg[i] = *reinterpret_cast<const uint2_t *>(reinterpret_cast<const unsigned char *>(a.kc) + off + lane_off);
                        vreg[i] = *reinterpret_cast<const uint2_t *>(reinterpret_cast<const unsigned char *>(a.vc) + off + lane_off);
                    } else {
                        kreg[i] = *reinterpret_cast<const half8_t *>(kbase + off + lane_off);
                        vreg[i] = *reinterpret_cast<const half8_t *>(vbase + off + lane_off);
                    }
                } else if constexpr (!FP8) {
                    kreg[i] = *reinterpret_cast<const half8_t *>(kbase + (size_t)gk * kHD + (idx & 15) * 8);
                    vreg[i] = *reinterpret_cast<const half8_t *>(vbase + (size_t)gk * kHD + (idx & 15) * 8);
                }
            }
        }
    };
    [[maybe_unused]] auto request_words = [&](int kt) {
        if constexpr (SINK) {
            if (kt == ntiles) tw.request_word0(a);
            else tw.request_from(a, kt, kend, lane, klo >> a.page_shift);
        } else if constexpr (WINDOW) tw.request_from(a, kt, kend, lane, klo >> a.page_shift);
        else if constexpr (PAGED) tw.request(a, kt, kend, lane);
    };
    if constexpr (PAGED) {
        request_words(kt0);  // (the one table round trip a block waits for)
        tw.latch();
    }
    fetch_tile(kt0);
    if constexpr (PAGED) request_words(kt0 + 1);
    // this lane's piece of a [4 keys][16 head dimensions] block for the transpose read: key 4 quad + n16 / 4, head dimensions 4 (n16 % 4) ..
    const unsigned char *vfrag = vs + (4 * quad + (n16 >> 2)) * kVStride + (n16 & 3) * 8;
    for (int kt = kt0; kt < nt_all; ++kt) {
        [[maybe_unused]] const bool sink_pass = SINK && kt == ntiles;
        const int key0 = sink_pass ? 0 : kt * kBK;
        if constexpr (SINK) {
            if (sink_pass && a.cos_s) {  // Q becomes Q_s
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const half_t *qraw = a.qkv + (size_t)(qrow0(a) + rowc[t]) * a.ld_qkv + (size_t)head * kHD;
                    half8_t raw[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) raw[s] = *reinterpret_cast<const half8_t *>(qraw + 32 * s + 8 * quad);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const half8_t c = *reinterpret_cast<const half8_t *>(a.cos_s + 32 * s + 8 * quad), sn = *reinterpret_cast<const half8_t *>(a.sin_s + 32 * s + 8 * quad);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const half_t rot = s < 2 ? (half_t)(-raw[s ^ 2][e]) : raw[s ^ 2][e];
                            const half_t tt = rot * sn[e];                         // hmul
                            qf[t][s][e] = __builtin_fmaf16(raw[s][e], c[e], tt);   // hfma, one rounding (the prepare kernel's statement)
                        }
                    }
                }
            }
        }
        __syncthreads();  // everybody has read the previous tiles
        // ---- both tiles as they lie ----
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const int idx = tid + NT * i;
            if constexpr (FP8) {
                *reinterpret_cast<half8_t *>(ks + (idx >> 4) * kKStride + (idx & 15) * 16) = fp8_dequant8(kreg[i], a.k_scale);
                *reinterpret_cast<half8_t *>(vs + (idx >> 4) * kVStride + (idx & 15) * 16) = fp8_dequant8(vreg[i], a.v_scale);
            } else {
                *reinterpret_cast<half8_t *>(ks + (idx >> 4) * kKStride + (idx & 15) * 16) = kreg[i];
                *reinterpret_cast<half8_t *>(vs + (idx >> 4) * kVStride + (idx & 15) * 16) = vreg[i];
            }
        }
        if constexpr (PAGED) tw.latch();  // tile kt + 1's words arrived with tile kt's rows
        __syncthreads();
        if (kt + 1 < nt_all) fetch_tile(kt + 1);
        if constexpr (PAGED) request_words(kt + 2);  // behind tile kt + 1's row requests, for the fetch a tile from now
        // ---- S^T = K Q^T (64 keys x this wave's 16 RT rows): a K fragment feeds the RT row tiles ----
        float4_t sacc[RT][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int t = 0; t < RT; ++t) sacc[t][j] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const half8_t kf = *reinterpret_cast<const half8_t *>(ks + (16 * j + n16) * kKStride + (32 * s + 8 * quad) * 2);
#pragma unroll
                for (int t = 0; t < RT; ++t) sacc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[t][s], sacc[t][j], 0, 0, 0);
            }
        }
        // does this tile hold keys some row of the wave must not see?  (wave-uniform; the last tile, and the tiles on the wave's causal diagonal)
        const bool edge = [&]() -> bool {
            const bool e = key0 + kBK > tgz || (a.causal && key0 + kBK - 1 > a.pos + r0);
            if constexpr (SINK) return sink_pass || e || (a.pos + r0 + 16 * RT - 1 - a.window >= a.sinks && key0 < a.pos + r0 + 16 * RT - 1 - a.window + 1);  // (if it binds)
            else if constexpr (WINDOW) return e || key0 < a.pos + r0 + 16 * RT - 1 - a.window + 1;  // (the lo of the wave's last row)
            else return e;
        }();
        // ---- scale, mask, cut; online softmax: the lane's row is rowc[t], its keys key0 + 16 j + 4 quad + r ----
        half4_t pb[RT][4];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            float best = kNegBig;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float4_t mk4 = float4_t{0.f, 0.f, 0.f, 0.f};
                if constexpr (MASK) {
                    const int kb = key0 + 16 * j + 4 * quad;
                    const half_t *mrow = a.mask + (size_t)rowc[t] * a.ld_mask;
#pragma unroll
                    for (int r = 0; r < 4; ++r) mk4[r] = kb + r < tgz ? (float)mrow[kb + r] * kLog2e : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = sacc[t][j][r] * scale2;
                    if constexpr (MASK) s += mk4[r];
                    // check_inf_half (Int4llamaAttention.cu:105-115, applied by the decode step as well, attention_fast.hip): inf / NaN / a score beyond
                    // binary16 weighs nothing -- in EVERY tile, interior and unmasked ones included (a NaN from an overflowed q.k used to poison
                    // the row here and not in the decode step).  !(|s| <= bound) is true for NaN.
                    // (round 5, ADVICE r4: such a score becomes -65504 and still takes part in the softmax -- what the reference and the decode step do; a row of
                    //  nothing but such scores then weighs its keys equally in prefill as in decode -- while a key that is CUT, past the context or the causal
                    //  bound, weighs nothing)
                    const bool in_range = __builtin_fabsf(s) <= 65504.0f * kLog2e;
                    bool cut = false;
                    if (MASK || edge) {
                        const int key = key0 + 16 * j + 4 * quad + r;
                        cut = edge && !(key < tgz && !(a.causal && key > a.pos + rowc[t]));
                        if constexpr (SINK) {
                            const bool binds = a.pos + rowc[t] - a.window >= a.sinks;
                            cut = sink_pass ? !(binds && key < a.sinks) : (cut || (binds && key < a.pos + rowc[t] - a.window + 1));
                        } else if constexpr (WINDOW) cut = cut || key < a.pos + rowc[t] - a.window + 1;
                    }
                    s = cut ? kNegBig : (in_range ? s : -65504.0f * kLog2e);
                    sacc[t][j][r] = s;
                    best = fmaxf(best, s);
                }
            }
            const float m_new = fmaxf(m_i[t], quad_max(best));
            const float corr = __builtin_amdgcn_exp2f(m_i[t] - m_new);
            float rs = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float4_t p;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // a key that is cut weighs nothing even when the whole row so far is cut (m_new == kNegBig: exp2(0) would be 1)
                    p[r] = __builtin_amdgcn_exp2f(sacc[t][j][r] - m_new);
                    if (MASK || edge) p[r] = sacc[t][j][r] > kNegBig ? p[r] : 0.f;
                    rs += p[r];
                }
                pb[t][j] = half4_t{(half_t)p[0], (half_t)p[1], (half_t)p[2], (half_t)p[3]};
            }
            l_i[t] = l_i[t] * corr + rs;
            m_i[t] = m_new;
#pragma unroll
            for (int c = 0; c < 8; ++c) o[t][c] *= corr;
        }
        // ---- O^T += V^T P^T: 8 head-dimension tiles x 4 sub-tiles of 16 keys; a V^T fragment (4 keys: 8 bytes) feeds the RT row tiles ----
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // V[key 16 j + 4 quad + r][head dimension 16 c + n16], r = 0 .. 3: the 16 lanes of a quad read a [4 keys][16 dims] block of the row-major
                // tile, 8 bytes each, and ds_read_b64_tr_b16 hands lane n16 the block's column n16 (gfx950's LDS transpose read)
                const half4_t vf = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                    (lds_fp16x4_t *)(vfrag + (16 * j) * kVStride + (16 * c) * 2)));
#pragma unroll
                for (int t = 0; t < RT; ++t) o[t][c] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pb[t][j], o[t][c], 0, 0, 0);
            }
    }
    // ---- out[row n16][head * hd + 16 c + 4 quad + r]: four consecutive halves per lane and column tile ----
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const float l = quad_sum(l_i[t]);
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        const int row = r0 + 16 * t + n16;
        if (row >= a.m) continue;
        half_t *orow = a.out + (size_t)(qrow0(a) + row) * a.ld_out + (size_t)head * kHD;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const half4_t v = half4_t{(half_t)(o[t][c][0] * inv), (half_t)(o[t][c][1] * inv), (half_t)(o[t][c][2] * inv), (half_t)(o[t][c][3] * inv)};
            *reinterpret_cast<half4_t *>(orow + 16 * c + 4 * quad) = v;
        }
    }
}

// The launch: a workgroup takes query block nb - 1 - blockIdx.x (causal launches dispatch the blocks with the most key tiles first) and, when `pair` is set,
// block blockIdx.x after it: block b of a causal prompt walks b + 1 (x 2 for 128-row blocks) key tiles, so the pair (nb - 1 - i, i) is the same work for every
// i -- unpaired, all workgroups are resident at once and the launch lasts as long as its heaviest block while the CUs of the light ones idle.
template <bool MASK, int NW, int RT, bool PAIR>
__global__ __launch_bounds__(64 * NW) void attn_prefill_kernel(const PrefillArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char ks[kBK * kKStride];  // K tile
    __shared__ __attribute__((aligned(16))) unsigned char vs[kBK * kVStride];  // V tile
    constexpr int kBQ = 16 * RT * NW;
    const int nb = (a.m + kBQ - 1) / kBQ;
    const int first = nb - 1 - (int)blockIdx.x;
    if constexpr (PAIR) {
        // (two inlined copies, not a loop around one: 35 registers more -- the paired launch is one 8-wave workgroup per CU anyway -- and 107 against 118 us
        //  at 2048 rows; the unpaired kernel is its own instantiation because those registers would cost it its second workgroup per CU)
        attn_prefill_block<MASK, NW, RT>(a, first, blockIdx.y, ks, vs);
        if ((int)blockIdx.x < first) attn_prefill_block<MASK, NW, RT>(a, blockIdx.x, blockIdx.y, ks, vs);
    } else {
        attn_prefill_block<MASK, NW, RT>(a, first, blockIdx.y, ks, vs);
    }
}

// The paged launch, every form -- fp16 and e4m3 pools, windowed, with sinks --: workgroup i takes entry i of the launch's block list (heaviest first) and, when `pair` is
// set, entry nblocks - 1 - i after it.  With one segment the list is that segment's blocks nb - 1 .. 0: the contiguous launch's order and pairs.
template <bool FP8, bool WINDOW, bool SINK>
__device__ __forceinline__ PagedBlockArgs paged_block_args(const paged_prefill_args_t<FP8, WINDOW, SINK> &a, const PrefillSegment sg) {
    PagedBlockArgs b{};
    b.qrot = a.qrot;
    b.kc = a.kc;
    b.vc = a.vc;
    b.out = a.out;
    b.trow = a.table + (size_t)sg.slot * a.table_stride;
    b.ld_out = a.ld_out;
    b.rep = a.rep;
    b.kv_heads = a.kv_heads;
    b.total_rows = a.total_rows;
    b.row0 = sg.row0;
    b.pos = sg.pos;
    b.m = sg.m;
    b.causal = a.causal;
    b.page_shift = a.page_shift;
    b.alpha = a.alpha;
    if constexpr (FP8) {
        b.k_scale = a.k_scale;
        b.v_scale = a.v_scale;
    }
    if constexpr (WINDOW) b.window = a.window;
    if constexpr (SINK) {
        b.sinks = a.sinks;
        b.qkv = a.qkv;
        b.ld_qkv = a.ld_qkv;
        b.cos_s = a.cos_s;
        b.sin_s = a.sin_s;
    }
    return b;
}

// Waves per SIMD, the two bounds of amdgpu_waves_per_eu.
// (fp16 pools, no window: the paired 8-wave form is pinned to the 3 its contiguous counterpart has.  Left alone it fits 126 registers, the compiler then keeps the schedule
//  it made for a fourth wave -- two K fragments read ahead of the MFMAs instead of six -- and the launch at 2048 rows took 108 us against the contiguous 93, though a
//  paired launch is one such workgroup per CU whatever its registers.  Every other form lands on its counterpart's occupancy by itself: 1 .. 8 leaves it alone.)
// (e4m3 pools, and every windowed and sink form: pinned to what the fp16 counterpart has, from profiles/fp8_kv/kernel_resources.txt: a tile's pieces are 8 registers fewer
//  per lane and pass, which by itself would let some forms fit one more wave and take the schedule the compiler makes for it, the effect the note above describes.  The
//  fp16 forms' registers -> waves per SIMD: 4 waves x 1 row tile 196 / 209 -> 2; 8 x 1 120 -> 4, paired 156 -> 3 (pinned); 8 x 2 221 / 232 -> 2; 4 x 2 301 / 314 -> 1)
struct WavesPerSimd {
    int lo, hi;
};
constexpr WavesPerSimd paged_prefill_waves(int NW, int RT, bool PAIR, bool FP8, bool WINDOW, bool SINK) {
    if (!FP8 && !WINDOW && !SINK) return PAIR && NW == 8 && RT == 1 ? WavesPerSimd{3, 3} : WavesPerSimd{1, 8};
    const int w = RT == 2 ? (NW == 8 ? 2 : 1) : (NW == 8 ? (PAIR ? 3 : 4) : 2);
    return {w, w};
}

template <int NW, int RT, bool PAIR, bool FP8, bool WINDOW, bool SINK>
__global__ __launch_bounds__(64 * NW)
__attribute__((amdgpu_waves_per_eu(paged_prefill_waves(NW, RT, PAIR, FP8, WINDOW, SINK).lo, paged_prefill_waves(NW, RT, PAIR, FP8, WINDOW, SINK).hi)))
void attn_prefill_paged_kernel(const paged_prefill_args_t<FP8, WINDOW, SINK> a) {
    __shared__ __attribute__((aligned(16))) unsigned char ks[kBK * kKStride];  // K tile (e4m3 pools: dequantised on the way in)
    __shared__ __attribute__((aligned(16))) unsigned char vs[kBK * kVStride];  // V tile
    const int i = (int)blockIdx.x;
    const unsigned e = (a.order[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
    attn_prefill_block<false, NW, RT, true, FP8, WINDOW, SINK>(paged_block_args<FP8, WINDOW, SINK>(a, a.seg[e >> 12]), (int)(e & 4095u), blockIdx.y, ks, vs);
    if constexpr (PAIR) {
        const int j = a.nblocks - 1 - i;
        if (i < j) {
            const unsigned f = (a.order[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
            attn_prefill_block<false, NW, RT, true, FP8, WINDOW, SINK>(paged_block_args<FP8, WINDOW, SINK>(a, a.seg[f >> 12]), (int)(f & 4095u), blockIdx.y, ks, vs);
        }
    }
}

thread_local int g_prefill_pair = 0;   // 0: by the rule; 1 / 2: pairing forced on / off
thread_local int g_prefill_waves = 0;  // 0: by the rule in launch_attention_prefill; forced (tests, sweeps): 4 / 8 waves with one row tile per wave, 14 / 18: with two

}  // namespace

void set_attention_prefill_waves(int w) {
    g_prefill_pair = w / 100;  // + 100: pairs forced on, + 200: off
    w %= 100;
    g_prefill_waves = (w == 4 || w == 8 || w == 14 || w == 18) ? w : 0;
}

size_t attention_prefill_workspace_bytes(int heads, int m, int hd) {
    if (hd != kHD || heads <= 0 || m <= 0) return 0;
    return (size_t)heads * m * kHD * sizeof(half_t);
}

namespace {

// The block form (4 / 8 waves x 1 row tile; 14 / 18: x 2, forced only) and the pairing of a launch whose query blocks number blocks(rows) at `rows` rows per block
// (all heads counted) -- ONE rule for the contiguous and the paged launch.
template <class F>
void prefill_form_rule(F blocks, int causal, int *form_out, int *pair_out) {
    // the block: 128 rows (8 waves) while that leaves two workgroups per CU, else 64 rows (forced: g_prefill_waves)
    int form = g_prefill_waves;
    if (form == 0) form = blocks(128) >= 512 ? 8 : 4;
    // causal prompts: pair a heavy block with a light one while the pairs still fill the chip
    *pair_out = g_prefill_pair == 1 || (g_prefill_pair == 0 && causal && blocks(form == 8 || form == 18 ? (form == 18 ? 256 : 128) : (form == 14 ? 128 : 64)) >= 512) ? 1 : 0;  // (two row tiles per wave -- forms 14 / 18 -- cost more in occupancy than the shared fragments give: 147 vs 130 us at 2048 rows)
    *form_out = form;
}

int form_rows(int form) { return form == 18 ? 256 : (form == 8 || form == 14 ? 128 : 64); }

// f(NW, RT) of a block form, as integral constants
template <class F>
void with_block_form(int form, F &&f) {
    using std::integral_constant;
    if (form == 18) f(integral_constant<int, 8>{}, integral_constant<int, 2>{});
    else if (form == 14) f(integral_constant<int, 4>{}, integral_constant<int, 2>{});
    else if (form == 8) f(integral_constant<int, 8>{}, integral_constant<int, 1>{});
    else f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
}

}  // namespace

int launch_attention_prefill(const void *qkv, int ld_qkv, void *kc, void *vc, const void *cosv, const void *sinv, const void *mask, int ld_mask, int causal,
                             void *out, int ld_out, void *workspace, int heads, int kv_heads, int max_keys, int pos, int m, float alpha, hipStream_t stream,
                             hipError_t *hip_err) {
    PrepareArgs p{};
    p.qkv = static_cast<const half_t *>(qkv);
    p.ld_qkv = ld_qkv;
    p.qrot = static_cast<half_t *>(workspace);
    p.kc = static_cast<half_t *>(kc);
    p.vc = static_cast<half_t *>(vc);
    p.cosv = static_cast<const half_t *>(cosv);
    p.sinv = static_cast<const half_t *>(sinv);
    p.heads = heads;
    p.kv_heads = kv_heads;
    p.max_keys = max_keys;
    p.pos = pos;
    p.m = m;
    const long long pieces = (long long)m * (heads + 2 * kv_heads) * 16;
    hipLaunchKernelGGL(attn_prefill_prepare_kernel<false>, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, stream, p);
    PrefillArgs a{};
    a.qrot = p.qrot;
    a.kc = p.kc;
    a.vc = p.vc;
    a.mask = static_cast<const half_t *>(mask);
    a.out = static_cast<half_t *>(out);
    a.ld_mask = ld_mask;
    a.ld_out = ld_out;
    a.heads = heads;
    a.rep = heads / kv_heads;
    a.max_keys = max_keys;
    a.pos = pos;
    a.m = m;
    a.causal = causal;
    a.alpha = alpha;
    auto blocks = [&](int rows) { return (long long)((m + rows - 1) / rows) * heads; };
    int form = 0;
    prefill_form_rule(blocks, causal, &form, &a.pair);
    with_block_form(form, [&](auto nw_c, auto rt_c) {
        with_bools([&](auto mask_c, auto pair_c) {
            constexpr int NW = decltype(nw_c)::value, RT = decltype(rt_c)::value;
            const int nb = (m + 16 * RT * NW - 1) / (16 * RT * NW);
            hipLaunchKernelGGL((attn_prefill_kernel<decltype(mask_c)::value, NW, RT, decltype(pair_c)::value>), dim3(a.pair ? (nb + 1) / 2 : nb, heads), dim3(64 * NW), 0, stream, a);
        }, mask != nullptr, a.pair != 0);
    });
    return launch_status(hip_err);
}

// ---- the paged launch ----
namespace {

// form, pairing and the block list (heaviest first; ties: in segment order, a segment's later blocks first) of a paged launch; false: more blocks than the list holds
// window >= 1 (causal): a block walks the tiles from the one of its first row's first visible key on -- those are what it is weighed by
// sinks >= 1 (with a window): a row binds from position sinks + window on -- a block whose first row does not bind walks from tile 0, one whose last row binds walks the
// sink pass's tile besides
bool plan_paged_prefill(int heads, int causal, const PrefillSegment *seg, int nseg, int *form_out, int *pair_out, int *nblocks_out, unsigned short *order, int window = 0,
                        int sinks = 0) {
    auto blocks = [&](int rows) {
        long long n = 0;
        for (int s = 0; s < nseg; ++s) n += (seg[s].m + rows - 1) / rows;
        return n * heads;
    };
    int form = 0, pair = 0;
    prefill_form_rule(blocks, causal, &form, &pair);
    const int rows = form_rows(form);
    const long long nb = blocks(rows) / heads;
    *form_out = form;
    *pair_out = pair;
    *nblocks_out = (int)(nb < 0x7fffffff ? nb : 0x7fffffff);
    if (nb > kMaxListedBlocks) return false;
    if (!order) return true;
    int tiles[kMaxListedBlocks];
    int n = 0;
    for (int s = 0; s < nseg; ++s) {
        const int nbs = (seg[s].m + rows - 1) / rows;
        for (int qb = nbs - 1; qb >= 0; --qb) {
            const int last_row = (qb * rows + rows < seg[s].m ? qb * rows + rows : seg[s].m) - 1;
            const int kend = causal ? seg[s].pos + last_row + 1 : seg[s].pos + seg[s].m;
            tiles[n] = (kend + kBK - 1) / kBK;
            if (window > 0) {
                const long long klo = (long long)seg[s].pos + (long long)qb * rows - window + 1;
                tiles[n] -= klo > sinks ? (int)(klo / kBK) : 0;  // (sinks = 0: klo > 0; else the first row binds iff its lo >= sinks + 1)
                if (sinks > 0 && (long long)seg[s].pos + last_row - window >= sinks) ++tiles[n];
            }
            order[n++] = (unsigned short)(s << 12 | qb);
        }
    }
    int idx[kMaxListedBlocks];
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::stable_sort(idx, idx + n, [&](int x, int y) { return tiles[x] > tiles[y]; });
    unsigned short sorted[kMaxListedBlocks];
    for (int i = 0; i < n; ++i) sorted[i] = order[idx[i]];
    for (int i = 0; i < n; ++i) order[i] = sorted[i];
    return true;
}

}  // namespace

size_t attention_prefill_paged_workspace_bytes(int heads, int total_rows, int hd) { return attention_prefill_workspace_bytes(heads, total_rows, hd); }

int describe_attention_prefill_paged(int heads, int causal, const int *segments, int nseg, int *form, int *pair, int *nblocks, int *workgroups, int window, int sinks) {
    PrefillSegment seg[kMaxSegments];
    if (nseg < 1 || nseg > kMaxSegments || heads < 1) return TCE_ERR_BAD_ARG;
    __builtin_memcpy(seg, segments, sizeof(PrefillSegment) * nseg);
    if (!plan_paged_prefill(heads, causal, seg, nseg, form, pair, nblocks, nullptr, window, sinks)) return TCE_ERR_UNSUPPORTED_SHAPE;
    *workgroups = (*pair ? (*nblocks + 1) / 2 : *nblocks) * heads;
    return TCE_OK;
}

// pages.fp8: the pools are e4m3 bytes and the two exponents apply; the plan and both launches' shapes are one text
int launch_attention_prefill_paged(const KvPages &pg, const AttnStepArgs &s, const PrefillRows &r, hipStream_t stream, hipError_t *hip_err) {
    const int heads = s.heads, kv_heads = s.kv_heads, nseg = r.nseg, total_rows = r.total_rows, causal = r.causal, table_stride = pg.table_stride;
    const int k_log2 = pg.k_scale_log2, v_log2 = pg.v_scale_log2;
    const bool fp8 = pg.fp8;
    const int *const table = pg.table;
    const int shift = page_shift_of(pg.page_keys);
    if (shift < 0 || nseg < 1 || nseg > kMaxSegments || !table || table_stride < 1 || kv_heads <= 0 || heads % kv_heads != 0 || total_rows < 1) return TCE_ERR_UNSUPPORTED_SHAPE;
    if (fp8 && !(fp8_log2_ok(k_log2) && fp8_log2_ok(v_log2))) return TCE_ERR_UNSUPPORTED_SHAPE;
    const int window = s.window;
    const int sinks = s.sinks;
    if (window < 0 || (window && !causal) || sinks < 0 || sinks > 16 || (sinks && !window)) return TCE_ERR_UNSUPPORTED_SHAPE;
    PagedPrefillSinkArgs a{};
    a.window = window;
    a.sinks = sinks;
    __builtin_memcpy(a.seg, r.segments, sizeof(PrefillSegment) * nseg);
    int form = 0;
    unsigned short order[kMaxListedBlocks] = {};
    if (!plan_paged_prefill(heads, causal, a.seg, nseg, &form, &a.pair, &a.nblocks, order, window, sinks)) return TCE_ERR_UNSUPPORTED_SHAPE;
    for (int i = 0; i < a.nblocks; ++i) a.order[i >> 1] |= (unsigned)order[i] << ((i & 1) * 16);
    PagedPrepareFp8Args p{};
    p.qkv = static_cast<const half_t *>(s.qkv);
    p.ld_qkv = r.ld_qkv;
    p.qrot = static_cast<half_t *>(s.workspace);
    p.kc = static_cast<half_t *>(pg.k_pool);
    p.vc = static_cast<half_t *>(pg.v_pool);
    p.cosv = static_cast<const half_t *>(s.cosv);
    p.sinv = static_cast<const half_t *>(s.sinv);
    p.table = table;
    p.table_stride = table_stride;
    p.page_shift = shift;
    p.heads = heads;
    p.kv_heads = kv_heads;
    p.total_rows = total_rows;
    p.nseg = nseg;
    __builtin_memcpy(p.seg, a.seg, sizeof(p.seg));
    const long long pieces = (long long)total_rows * (heads + 2 * kv_heads) * 16;
    if (fp8) {
        p.k_inv = host_pow2(-k_log2);
        p.v_inv = host_pow2(-v_log2);
        a.k_scale = host_pow2(k_log2);
        a.v_scale = host_pow2(v_log2);
        hipLaunchKernelGGL((attn_prefill_prepare_kernel<true, true>), dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(attn_prefill_prepare_kernel<true>, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, stream, static_cast<const PagedPrepareArgs &>(p));
    }
    a.qrot = p.qrot;
    a.kc = p.kc;
    a.vc = p.vc;
    a.out = static_cast<half_t *>(s.out);
    if (sinks) {  // (a row binds only at a position >= sinks + window: the tables then hold row sinks + window - 1; the pointers are followed by binding blocks alone)
        a.qkv = p.qkv;
        a.ld_qkv = p.ld_qkv;
        a.cos_s = p.cosv ? p.cosv + ((size_t)sinks + window - 1) * kHD : nullptr;
        a.sin_s = p.sinv ? p.sinv + ((size_t)sinks + window - 1) * kHD : nullptr;
    }
    a.table = table;
    a.ld_out = r.ld_out;
    a.heads = heads;
    a.rep = heads / kv_heads;
    a.kv_heads = kv_heads;
    a.total_rows = total_rows;
    a.causal = causal;
    a.table_stride = table_stride;
    a.page_shift = shift;
    half_t ah;
    __builtin_memcpy(&ah, &s.alpha_bits, 2);
    a.alpha = (float)ah;
    const dim3 grid(a.pair ? (a.nblocks + 1) / 2 : a.nblocks, heads);
    with_block_form(form, [&](auto nw_c, auto rt_c) {
        with_bools([&](auto pair_c, auto fp8_c, auto window_c, auto sink_c) {
            constexpr int NW = decltype(nw_c)::value, RT = decltype(rt_c)::value;
            constexpr bool PAIR = decltype(pair_c)::value, FP8 = decltype(fp8_c)::value, WINDOW = decltype(window_c)::value, SINK = decltype(sink_c)::value;
            if constexpr (!SINK || WINDOW)  // (sinks exist beside a window: refused above)
                hipLaunchKernelGGL((attn_prefill_paged_kernel<NW, RT, PAIR, FP8, WINDOW, SINK>), grid, dim3(64 * NW), 0, stream, static_cast<const paged_prefill_args_t<FP8, WINDOW, SINK> &>(a));
        }, a.pair != 0, fp8, window != 0, sinks != 0);
    });
    return launch_status(hip_err);
}

}  // namespace tce
