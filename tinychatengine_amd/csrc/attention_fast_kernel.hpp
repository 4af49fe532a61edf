// attention_fast_kernel.hpp -- the device text of the decode attention step (attention_fast.hip's head comment says what the step is): the argument structs, the
// helpers and attn_decode_fast_kernel, every form.  Two translation units instantiate it: attention_fast.hip -- every form but one, and the host side: the cuts, the
// launchers, the page copies -- and attention_rows_sink.hip: ROWS && WINDOW && SINK, the multi-row sink step.  Everything here has internal linkage, so each object
// holds the forms its unit launches and no other (tests/test_attn_forms_isa.py holds attention_fast.o to its kernels).
#pragma once
#include "tce_common.hpp"
#include "w4a16_kernels.hpp"
#include "fp8_kv.hpp"
#include "attn_dispatch.hpp"

namespace tce {

namespace {

struct FastAttnArgs {
    const half_t *qkv;    // [q_heads + 2 * kv_heads][hd]: q heads, then k heads, then v heads (the fused projection's row)
    half_t *kc, *vc;      // [kv_heads][max_keys][hd]
    const half_t *cosv, *sinv;  // [positions][hd] or null (no RoPE: q / k used as they are)
    const half_t *mask;   // [keys] additive or null
    half_t *out;          // [q_heads][hd]
    float *part;          // [q_heads][chunks][2 + hd]
    unsigned *cnt;        // [kv_heads], zero between launches
    int heads, kv_heads, rep, hd, max_keys, pos, keys, chunk, chunks;  // heads = query heads, rep = heads / kv_heads; chunks = chunk slots of the grid
    const int *pos_dev;   // non-null: the position is read from this device word (a captured launch replayed token after token); pos / keys above
                          // then only bound it (the grid and the chunk length were cut for them)
    float alpha;
    int defer;             // round 5: with several chunk slots the launch ENDS at its partial states -- plain stores of (M, L, -, -, O[hd]) per (query head, chunk slot),
                           // stride kDeferStride floats -- and the consumer (the o_proj launch: w4a16_gemv_i8.hip's COMB prologue) combines them while it stages its
                           // activations.  No acknowledged stores, no counter, no last workgroup: the kernel boundary orders the two launches
    int probe_no_combine;  // timing experiment (tce_w4a16_set_debug_mode(2931)): the partial states are stored plainly and the launch ends -- `out` is NOT written
};

// the paged step's arguments: the batched step's, with the caches replaced by two pools of pages and a block table (kc / vc = the pools, max_keys =
// table_stride << page_shift: the bound of a sequence's logical key index, what the workspace slices are sized for)
struct PagedAttnArgs : FastAttnArgs {
    const int *table;  // int32 [batch][table_stride]: logical key j of sequence b lives in page table[b][j >> page_shift], row j & (page_keys - 1)
    int table_stride, page_shift;  // page_keys = 1 << page_shift (16 .. 256)
};

// the e4m3 paged step's: kc / vc are pools of BYTES [num_pages][kv_heads][page_keys][hd] (include/tce_matmul.h, "FP8 pages"); the two powers of two and their inverses
struct PagedFp8AttnArgs : PagedAttnArgs {
    float k_scale, v_scale;  // 2^k_scale_log2, 2^v_scale_log2: a byte's value times this is the cache row's binary16 element, exactly
    float k_inv, v_inv;      // 2^-k_scale_log2, 2^-v_scale_log2: what the token's own row is multiplied by before it is rounded to a byte
};

// the multi-row paged step's (speculative decoding): the e4m3 step's arguments -- the two scales are unused on fp16 pools -- and T = rows per sequence.  The grid is
// (heads x chunk slots, T, batch): virtual row y = b * T + t has q/k/v row, output row, workspace slice and position word y, and table row b
struct PagedRowsAttnArgs : PagedFp8AttnArgs {
    int rows_per_seq;  // 1 .. TCE_SPEC_MAX_ROWS
};

// the windowed paged step's (sliding-window attention): the e4m3 step's arguments -- the two scales are unused on fp16 pools -- and W = window: a row at position p
// weighs keys max(0, p - W + 1) .. p.  chunk / chunks were cut for min(pos_bound + 1, W + 3) keys
struct PagedWindowAttnArgs : PagedFp8AttnArgs {
    int window;  // >= 1
};

// the windowed multi-row paged step's (speculative decoding on a sliding-window layer): both of the above -- T rows per sequence, each weighing the last W keys of ITS
// position.  chunk / chunks were cut for min(pos_bound + 1, W + 3) keys, the same for every row
struct PagedRowsWindowAttnArgs : PagedRowsAttnArgs {
    int window;  // >= 1
};

// the windowed paged step with attention sinks: the windowed step's arguments and S = sinks, 1 .. 16.  A row at position p BINDS iff p >= S + W: it then weighs keys
// 0 .. S - 1, scored with q rotated by cos / sin row S + W - 1, and keys p - W + 1 .. p, scored with q rotated by row p; a row that does not bind weighs keys 0 .. p
// (include/tce_matmul.h, "Attention sinks").  chunk / chunks were cut by attention_sink_cut_keys
struct PagedSinkAttnArgs : PagedWindowAttnArgs {
    int sinks;     // 1 .. 16
    int sink_row;  // min(S + W - 1, pos_bound): the cos / sin row of the second rotation (beyond pos_bound no row binds and the rotation is not used)
};

// the multi-row paged step with attention sinks (speculative decoding on a sink layer): the windowed multi-row step's arguments and the sink step's two.  Each virtual
// row binds or not by ITS position; chunk / chunks were cut by attention_sink_cut_keys, the same for every row.  The host guarantees window >= rows_per_seq
struct PagedRowsSinkAttnArgs : PagedRowsWindowAttnArgs {
    int sinks;     // 1 .. 16
    int sink_row;  // min(S + W - 1, pos_bound)
};

// a form's arguments (the kernel's static_asserts say which forms exist)
template <bool PAGED, bool FP8, bool ROWS, bool WINDOW, bool SINK>
using step_args_t = std::conditional_t<SINK, std::conditional_t<ROWS, PagedRowsSinkAttnArgs, PagedSinkAttnArgs>, std::conditional_t<WINDOW, std::conditional_t<ROWS, PagedRowsWindowAttnArgs, PagedWindowAttnArgs>,
                                       std::conditional_t<ROWS, PagedRowsAttnArgs, std::conditional_t<FP8, PagedFp8AttnArgs, std::conditional_t<PAGED, PagedAttnArgs, FastAttnArgs>>>>>;

__device__ __forceinline__ float row16_sum(float v) {  // sum over the 16 lanes of a DPP row, result in every lane of the row
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, false));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0x141>{});  // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});  // row_mirror
    return v;
}

// acc + p * (the low / high binary16 half of `pair`, widened exactly): one v_fma_mix_f32, no separate conversion
__device__ __forceinline__ float fma_mix_lo(float p, unsigned pair, float acc) {
    float d;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(p), "v"(pair), "v"(acc));
    return d;
}
__device__ __forceinline__ float fma_mix_hi(float p, unsigned pair, float acc) {
    float d;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(p), "v"(pair), "v"(acc));
    return d;
}

// RotaryPosEmb_cuda_forward on the 8 elements of `piece` (hd = 128: the partner half is piece ^ 8):
//   out[j] = hfma(x[j], cos[j], hmul(rot[j], sin[j])),  rot[j] = j < hd/2 ? -x[j + hd/2] : x[j - hd/2]
// v = the piece, p = the partner piece, c / s = the cos / sin pieces (all loaded by the caller, in one batch)
__device__ __forceinline__ half8_t rope_apply(const half8_t v, const half8_t p, const half8_t c, const half8_t s, int piece) {
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const half_t rot = piece < 8 ? (half_t)(-p[e]) : p[e];
        const half_t t = rot * s[e];                       // hmul
        o[e] = __builtin_fmaf16(v[e], c[e], t);            // hfma: v_fma_f16, one rounding (as tce_rope_half, attention_ops.hip)
    }
    return o;
}

constexpr int kHD = 128;
constexpr float kNegBig = -1.0e30f;
constexpr int kDeferStride = 4 + kHD;  // floats per deferred partial state: M, L, two unused, O[128] (16-byte aligned rows of O)

// one step's workspace in 4-byte words: the arrival counters (a 256-byte multiple), then the partial states for the smallest chunk (64 keys)
__host__ __device__ inline size_t attn_workspace_words(int heads, int max_keys) {
    return (((size_t)heads * 4 + 255) & ~(size_t)255) / 4 + (size_t)heads * ((max_keys + 63) / 64) * kDeferStride;
}

// MASK: the caller gave a mask row (a compile-time form: a branch inside the fetch block makes hipcc drain the load queue at the loop head)
// NW: waves per workgroup (4; 8 and 16 exist for the sweep that ruled them out, see pick_chunk).
// R: query heads per key / value head (grouped-query attention, llm/src/nn_modules/non_cuda/Int4llamaAttention.cc:166-185: query head i reads
//    key / value head i / R; Llama-3-8B: 32 / 8, llm/include/model.h:83).  A workgroup is (key / value head, chunk of keys): it streams the
//    chunk's cache rows ONCE and keeps R online-softmax states per lane, so the R query heads cost one pass over the cache, not R.
// BATCH: the batched step (launch_attention_decode_batch): grid.y = sequences, sequence blockIdx.y's q/k/v row, cache slot, output row, workspace slice and
// position word; a position outside [0, a.pos] marks the row inactive.  Every offset below is a constant 0 in the single step's form (BATCH == false).
// PAGED (with BATCH): the caches are pools of pages [num_pages][kv_heads][page_keys][hd] addressed through a block table (PagedAttnArgs).  Only the base of a
// cache row changes: a wave-instruction of the cache stream covers four consecutive keys from a multiple of four, which never cross a page, so the request stays
// 1 KiB contiguous.  Which table words a wave can need depends on the grid alone (its keys kw0 .. kw0 + per_wave - 1), so they are requested BEFORE the position
// word is waited for -- one word per lane, plain ints inside the table -- and a cache request picks its page with v_readlane: no round trip is added to the
// chain position word -> cache rows.  Only words 0 .. pos / page_keys of an active row become addresses (see page_of below); of an inactive row, none.
// FP8 (with PAGED): the pools hold OCP e4m3 bytes, a row is 128 bytes and a lane's cache load 8 of them: a wave instruction still covers four whole consecutive keys
// (512 contiguous bytes).  The bytes stay as they are in the double buffer -- a conversion at the request would wait for the rows there -- and become the binary16
// registers consume() has always read at its head: every instruction behind that, and its order, is the fp16 paged step's, so on pools whose fp16 image holds
// dequant(byte) the two steps agree bit for bit.  The token's own row is rounded to bytes (fp8_kv.hpp: the format's rule), stored as bytes, and enters `newrow`
// DEQUANTISED: the step weighs its own key and value as the cache will hold them.
// ROWS (with PAGED): T = rows_per_seq rows per sequence in one launch (PagedRowsAttnArgs): row t of sequence b sits at position pos_device[b * T + t] = p + t and must
// weigh keys p .. p + t - 1, which OTHER workgroups of this launch are appending -- so it never takes them from the pool.  The `newrow` idea, t + 1 times: the
// workgroup loads the k / v pieces of q/k/v rows y - t .. y, rotates each with the cos / sin row of ITS position (the same binary16 rope_apply; e4m3: quantised and
// dequantised as the appending wave does), keeps them in LDS and consume() takes every key in [pos - t, pos] from there.  Only the own row is appended: one writer per
// pool row, nobody waits for anybody.  The caller guarantees that a sequence's active rows are a prefix with consecutive positions (include/tce_matmul.h); all the kernel
// does about it is to clamp t to pos, so that no address is formed from a negative position.  The key loop is the paged step's: the wave-uniform rare-block test is a
// range overlap instead of a membership, and the work it guards is the only per-key addition.
// WINDOW (with PAGED): the row weighs keys lo .. pos only, lo = max(0, pos - W + 1) (PagedWindowAttnArgs).  The workgroup's key range starts at
// base = lo & ~3 instead of 0 -- chunk slot c covers keys base + c * chunk .. --, so the span pos - base + 1 <= W + 3 is what the grid was cut for, whatever pos is.
// Keys base .. lo - 1 of the first group of four are loaded -- they lie in the page of key lo, a group of four never crosses a page -- and weigh nothing, exactly as
// keys at and beyond kw1 do: excluded from the maximum and the sum by the same rare-block text.  TABLE WORDS: kw0 now depends on the position, so a wave's words
// cannot be requested in front of the position word's wait: the request follows it, ONE MORE DEPENDENT ROUND TRIP in the chain position word -> table word -> cache
// rows (DESIGN.md 3.4 says why the alternatives were not taken).  Lane i asks for word kw0 / page_keys + i clamped into [lo / page_keys, pos / page_keys] -- the only
// words of the row that become addresses; everything below may name a page that was given back --, lane 63 for word pos / page_keys: the page wholly invalid groups
// are read from (word 0's page may be gone).  The appending wave, newrow, RoPE, the e4m3 round trip of the own row, both merges, the counters and the inactive rows
// are the paged step's text.
// ROWS && WINDOW (PagedRowsWindowAttnArgs): both texts, each as it stands -- nothing is written for the pair.  Virtual row y = b * T + t at pos = p + t has its own
// lo_t = max(0, pos - W + 1) and base_t = lo_t & ~3, so its workgroups cover exactly the keys, chunk slots, waves and blocks of the windowed step at that position, and
// every key in [pos - tprev, pos] comes from `newrow` whether it weighs or not: an in-call key below lo_t (possible only with W <= tprev) is taken from LDS and then
// weighs nothing, like any key below lo.  When the window lies wholly inside the call's rows (lo_t >= pos - tprev) the pool range [lo_t, pos - tprev - 1] is empty: the
// rows the fetch reads at and beyond position p -- other workgroups of this launch are writing them -- are all replaced from LDS or invalid, none is weighted.  The
// table words follow the position word as in WINDOW, words lo_t / page_keys .. pos / page_keys of table row b; the workgroup order is WINDOW's (blockIdx.x alone).
// SINK (with WINDOW, PAGED; PagedSinkAttnArgs): a binding row weighs keys 0 .. S - 1 (the sinks) beside its window, the sinks scored with a SECOND rotation of q (cos /
// sin row S + W - 1, a launch constant requested with the prologue batch: R * 4 registers and two 16-byte loads).  The workgroups walk a VIRTUAL key sequence: with
// S4 = (S + 3) & ~3 and base2 = lo & ~3, virtual index v < S4 is key v (valid iff v < S) and v >= S4 is key base2 + (v - S4) (valid iff >= lo); for a row that does not
// bind S4 = lo = base2 = 0 and virtual equals actual: the unwindowed row.  Chunk slots, waves, blocks, both merges and the counters are the text above applied to v; only
// the fetch turns v into a key.  A group of four is wholly sink or wholly window (S4 is a multiple of 4), and S4 <= 16 = a block, so sink groups lie in the FIRST block of
// the waves whose run starts below S4 (wave 0 of chunk slot 0 when a wave's run is 16 keys or more): every wave's first block takes consume()'s sink form, which picks the
// query per step, wave-uniformly; every other block is the windowed text.  TABLE WORDS: word 0 (lane 62: S <= 16 <= page_keys, the sinks lie in its page) and lo / page_keys .. pos /
// page_keys, indices clamped into that set.  Rows S .. S4 - 1 of word 0's page and rows base2 .. lo - 1 are loaded and weigh nothing (value rows zeroed: the rare-block text).
// ROWS && WINDOW && SINK (PagedRowsSinkAttnArgs; instantiated by attention_rows_sink.hip alone): the two texts again, with ONE re-expression -- the key loop counts
// virtual indices, so the rows of this launch, keys pos - tprev .. pos, are the virtual indices kpos - tprev .. kpos (kpos = pos - vshift): the rare-block overlap test and
// the replacement from `newrow` are written in kpos, which IS pos wherever SINK is not set.  One shift serves all of them because the host guarantees W >= T: every
// in-call key then lies inside its row's window (pos - tprev >= pos - W + 1 = lo, virtual >= S4), and a sequence with a binding row starts at p >= S + 1, so no in-call
// key is a sink key.  Each virtual row binds or not by its own position: rows that do not bind may stand in front of rows that do in one launch (a row that does not
// bind: S4 = vshift = 0, the unwindowed rows text).  A wave's first block -- consume()'s sink form -- can hold in-call rows when W is small: the replacement sits in the
// rare-block text, which both forms of consume() share.  The appending workgroup, the e4m3 round trip of every in-call row, lanes 62 / 63 of the table-word request (of
// table row b) and the workgroup order are the texts above.
template <bool MASK, int NW, int R, bool BATCH = false, bool PAGED = false, bool FP8 = false, bool ROWS = false, bool WINDOW = false, bool SINK = false>
// (waves per SIMD: the sink forms are pinned to the windowed step's 4 -- left alone the fp16 one takes 141 registers for the second copy of consume() and runs 3; 1 .. 8
//  leaves every other form alone)
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(SINK ? 4 : 1, SINK ? 4 : 8))) void attn_decode_fast_kernel(const step_args_t<PAGED, FP8, ROWS, WINDOW, SINK> a) {
    static_assert(!SINK || WINDOW, "sinks exist beside a window");
    static_assert(!WINDOW || (PAGED && NW == 4), "a window exists on the paged steps only");
    static_assert(!PAGED || (BATCH && !MASK && R == 1), "the paged form is a form of the batched step");
    static_assert(!FP8 || PAGED, "e4m3 caches exist as pages only");
    static_assert(!ROWS || (PAGED && NW == 4), "several rows per sequence exist on pages only");
    constexpr int NT = 64 * NW, NS = 4 * NW;
    constexpr int NEW = ROWS ? TCE_SPEC_MAX_ROWS : 1;  // rows kept in LDS: the token's own, and (ROWS) the up to 7 in front of it
    static_assert(NEW <= NS, "one (wave, key slot) per new row");
    __shared__ __attribute__((aligned(16))) float st[NS][R][2 + kHD];  // the (wave, slot) states per query head: m, l, o[hd]
    __shared__ __attribute__((aligned(16))) half_t newrow[NEW][2][kHD];  // the token's own (rotated) key and value (ROWS: row j is position pos - tprev + j)
    __shared__ unsigned last_flag;
    // the sequence's offsets into the batched arrays, in elements / words (BATCH == false: 0)
    const unsigned seq = [&]() -> unsigned {
        if constexpr (ROWS) return blockIdx.z * (unsigned)a.rows_per_seq + blockIdx.y;  // the virtual row
        else return BATCH ? blockIdx.y : 0u;
    }();
    const unsigned tseq = ROWS ? blockIdx.z : seq;  // the block table's row
    const size_t seq_qkv = (size_t)seq * (a.heads + 2 * a.kv_heads) * kHD, seq_cache = PAGED ? 0 : (size_t)seq * a.kv_heads * a.max_keys * kHD;
    const size_t seq_out = (size_t)seq * a.heads * kHD, seq_ws = BATCH ? seq * attn_workspace_words(a.heads, a.max_keys) : 0;
    // grp: this workgroup's group of R consecutive query heads (R == rep: all the query heads of a key / value head, its cache rows streamed
    // once for all of them; R < rep: rep / R workgroups read the same cache rows -- from HBM once, the others from the memory-side cache)
    // WINDOW: the same (query head, chunk slot) pairs in another order.  The cut for W + 3 keys is rarely a power of two of slots (W = 4096: nine), and with
    // blockIdx.x = grp * 9 + c the rep query heads that stream the SAME cache rows land on rep different XCDs -- workgroups are dealt round-robin over the eight of
    // them, each with an L2 of its own (MI355X_MICROARCH.md; observed, not promised: only the speed depends on it) -- so every row came from beyond the L2 rep times:
    // 1.9 x the time of the unwindowed step over as many keys (profiles/window/).  Here pair p = key / value head * chunks + c takes the blockIdx.x that are
    // congruent to p modulo 8, its rep query heads 8 apart; the grid is padded to whole groups of 8 pairs and the padding returns at once.
    const unsigned bx = [&]() -> unsigned {
        if constexpr (WINDOW) {
            const int p = (int)(blockIdx.x / (8u * a.rep)) * 8 + (int)(blockIdx.x & 7u);
            if (p >= a.kv_heads * a.chunks) return ~0u;
            return (unsigned)(((p / a.chunks) * a.rep + (int)((blockIdx.x >> 3) % (unsigned)a.rep)) * a.chunks + p % a.chunks);  // query head * chunks + c, as below
        } else {
            return blockIdx.x;
        }
    }();
    if constexpr (WINDOW) {
        if (bx == ~0u) return;
    }
    const int grp = bx / a.chunks, c = bx - grp * a.chunks;
    // PAGED: lane i's table word kw0 / page_keys + i of this sequence's row (clamped into the row; lane 63: word 0, which every active row owns -- the page that
    // wholly invalid groups of four are read from).  Requested here, in front of the position word's wait: a load of an int inside the table, whatever it holds.
    int tabw = 0, tab_e0 = 0;
    if constexpr (PAGED && !WINDOW) {
        const int w_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l_ = threadIdx.x & 63;
        tab_e0 = (c * a.chunk + w_ * (a.chunk / NW)) >> a.page_shift;
        const int e = l_ == 63 ? 0 : (tab_e0 + l_ < a.table_stride ? tab_e0 + l_ : a.table_stride - 1);
        tabw = a.table[(size_t)tseq * a.table_stride + e];
    }
    // the position: by value, or from a device word (wave-uniform scalar load) -- then chunks past the context have nothing to do and the
    // head's combine expects only the chunks that exist
    const int pos = a.pos_dev ? __builtin_amdgcn_readfirstlane(*(a.pos_dev + seq)) : a.pos;
    if constexpr (BATCH) {
        // an inactive row (a retired slot: -1; or any word outside the bound the grid was cut for): zeros for o_proj, and nothing else -- no cache row, no
        // partial state, no counter.  The first chunk slot of each query-head group writes them.
        if (pos < 0 || pos > a.pos) {
            if (c == 0 && threadIdx.x < kHD) {
#pragma unroll
                for (int r = 0; r < R; ++r) a.out[seq_out + (size_t)grp * R * kHD + r * kHD + threadIdx.x] = (half_t)0;
            }
            return;
        }
    }
    int keys = pos + 1;  // (SINK: the virtual keys, below)
    // WINDOW: the first key that weighs, and the first key of the workgroups' range (a multiple of four: the groups of four stay aligned); else 0
    // SINK: of a binding row; a row that does not bind is the unwindowed row
    [[maybe_unused]] const int lo = [&]() -> int {
        if constexpr (SINK) return pos - a.window >= a.sinks ? pos - a.window + 1 : 0;
        else if constexpr (WINDOW) return pos - a.window + 1 > 0 ? pos - a.window + 1 : 0;
        else return 0;
    }();
    const int base = WINDOW && !SINK ? lo & ~3 : 0;
    // SINK: S and S4 of a binding row (else 0); what turns a virtual index at or beyond S4 into its key; the virtual index of key lo.  The range below (keys, key0, kw0,
    // kw1 ..) is virtual, kpos the row's own virtual index
    [[maybe_unused]] const int snk = [&]() -> int {
        if constexpr (SINK) return pos - a.window >= a.sinks ? a.sinks : 0;
        else return 0;
    }();
    [[maybe_unused]] const int s4 = (snk + 3) & ~3;
    [[maybe_unused]] const int vshift = SINK ? (lo & ~3) - s4 : 0;
    [[maybe_unused]] const int vlo = SINK ? lo - vshift : lo;
    int kpos = pos;
    if constexpr (SINK) {
        kpos = pos - vshift;
        keys = kpos + 1;
    }
    // ROWS: the rows of this sequence in front of this one, all in flight in this launch (keys pos - tprev .. pos - 1)
    [[maybe_unused]] const int tprev = ROWS ? ((int)blockIdx.y < pos ? (int)blockIdx.y : pos) : 0;
    const int chunks = a.pos_dev ? (keys - base + a.chunk - 1) / a.chunk : a.chunks;  // active chunks (<= the grid's chunk slots)
    if (c >= chunks) return;
    if constexpr (WINDOW) {
        // the table words, behind the position (see above): of an active row, words lo / page_keys .. pos / page_keys and no other
        const int w_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l_ = threadIdx.x & 63;
        const int e_lo = lo >> a.page_shift, e_hi = pos >> a.page_shift;
        if constexpr (SINK) {  // (the wave's first window key; lane 62: word 0, the sinks' page -- a wave's run spans at most 17 words)
            const int v0 = c * a.chunk + w_ * (a.chunk / NW);
            tab_e0 = ((v0 < s4 ? s4 : v0) + vshift) >> a.page_shift;
        } else {
            tab_e0 = (base + c * a.chunk + w_ * (a.chunk / NW)) >> a.page_shift;
        }
        int e = l_ == 63 ? e_hi : tab_e0 + l_;
        e = e < e_lo ? e_lo : (e > e_hi ? e_hi : e);
        if constexpr (SINK) e = l_ == 62 ? 0 : e;
        tabw = a.table[(size_t)tseq * a.table_stride + e];
    }
    const int head = (grp * R) / a.rep;  // the key / value head
    const bool appends = (grp * R) % a.rep == 0;  // one workgroup group per key / value head writes the token's row into the caches
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slot = lane >> 4, piece = lane & 15;
    const int key0 = base + c * a.chunk, key1 = key0 + a.chunk < keys ? key0 + a.chunk : keys;
    const half_t *cosr = a.cosv ? a.cosv + (size_t)pos * kHD : nullptr, *sinr = a.sinv ? a.sinv + (size_t)pos * kHD : nullptr;
    const size_t hoff = (size_t)head * kHD;
    // ---- this wave's keys: chunk / 4 consecutive ones, 4 per step.  Their addresses depend on nothing but the arguments, so the
    //      first block of cache rows is requested in the same batch as q / cos / sin: one memory round trip per launch instead of
    //      two -- and BEHIND them (round 4): loads return in order, the prologue's pieces are L2 hits, and with the cache rows in
    //      front of them the rotation waited for HBM (4.95 -> 4.5 us at 128 keys, 7.8 -> 7.5 at 512, 10.2 -> 9.8 at 2048) ----
    const int per_wave = a.chunk / NW;  // (the host made the chunk a multiple of 4 * NW)
    const int kw0 = key0 + wave * per_wave;
    const int kw1 = kw0 + per_wave < key1 ? kw0 + per_wave : key1;  // a block is 16 keys, a wave's run any multiple of 4: the rest weighs nothing
    const half_t *kbase = a.kc + seq_cache + (size_t)head * a.max_keys * kHD, *vbase = a.vc + seq_cache + (size_t)head * a.max_keys * kHD;
    // PAGED: the element offset of (page, this key / value head, row) in either pool
    [[maybe_unused]] auto page_row = [&](int page, int row) -> size_t {
        if constexpr (PAGED) return ((((size_t)page * a.kv_heads + head) << a.page_shift) + row) * kHD;
        else return 0;
    };
    // blocks of 4 steps (16 keys per wave): the 8 loads of the next block are in flight while this block's scores and
    // exponentials are computed (the online-softmax state is the only loop-carried dependence; without the explicit double
    // buffer every step paid a full memory round trip: 20 us at 2048 keys, profiles/r2/attention_decode_step.jsonl)
    constexpr int BLK = 4;
    using row_t = std::conditional_t<FP8, uint2_t, half8_t>;  // what a lane holds of a cache row between request and use: 8 elements
    row_t kbuf[2][BLK], vbuf[2][BLK];
    half_t mbuf[2][BLK];  // the keys' mask values travel with their rows (a load per step inside consume() drained the queue)
    auto fetch = [&](row_t (&kd)[BLK], row_t (&vd)[BLK], half_t (&md)[BLK], int it0) {
#pragma unroll
        for (int u = 0; u < BLK; ++u) {
            const int key = kw0 + it0 + u * 4 + slot;
            const int kk = key < kw1 ? key : (keys - 1);  // clamped: rows past the range are read (harmlessly) and weigh nothing
            if constexpr (PAGED) {
                // the group of four keys g .. g + 3 (g a multiple of 4, wave-uniform).  g < kw1: at least key g is in the range, so g <= pos, its table word
                // g / page_keys <= pos / page_keys is one the row owns and one of this wave's (lane g / page_keys - tab_e0 < 63 holds it); a slot past the range
                // is clamped to keys - 1, which then lies in the same group (kw1 is a multiple of 4 or keys itself) and so in the same page.  g >= kw1: nothing of
                // the group is weighted; it is read from rows 0 .. 3 of word 0's page (lane 63) -- never from a word past pos / page_keys.
                // WINDOW: g >= base, so g / page_keys >= lo / page_keys too (base and lo share a group of four, hence a page); lane 63 holds word pos / page_keys.
                // SINK: g is virtual.  A sink group (g < s4 <= kw1's group: never clamped) is keys g .. g + 3 of word 0's page (lane 62); a window group is keys
                // g + vshift .., and a slot clamped to keys - 1 = kpos stays in its group as above
                const int g = kw0 + it0 + u * 4;
                const bool live = g < kw1;
                const int page = [&]() -> int {
                    if constexpr (SINK)
                        return __builtin_amdgcn_readlane(tabw, __builtin_amdgcn_readfirstlane(live ? (g < s4 ? 62 : ((g + vshift) >> a.page_shift) - tab_e0) : 63));
                    else return __builtin_amdgcn_readlane(tabw, __builtin_amdgcn_readfirstlane(live ? (g >> a.page_shift) - tab_e0 : 63));
                }();
                const int krow = SINK ? (g < s4 ? kk : kk + vshift) : kk;
                const size_t off = page_row(page, live ? (krow & ((1 << a.page_shift) - 1)) : slot) + piece * 8;
                if constexpr (FP8) {  // (an element is a byte: the same offset counts bytes)
                    kd[u] = *reinterpret_cast<const uint2_t *>(reinterpret_cast<const unsigned char *>(a.kc) + off);
                    vd[u] = *reinterpret_cast<const uint2_t *>(reinterpret_cast<const unsigned char *>(a.vc) + off);
                } else {
                    kd[u] = *reinterpret_cast<const half8_t *>(a.kc + off);
                    vd[u] = *reinterpret_cast<const half8_t *>(a.vc + off);
                }
                md[u] = (half_t)0;
                continue;
            }
            if constexpr (!FP8) {
                kd[u] = *reinterpret_cast<const half8_t *>(kbase + (size_t)kk * kHD + piece * 8);
                vd[u] = *reinterpret_cast<const half8_t *>(vbase + (size_t)kk * kHD + piece * 8);
            }
            if constexpr (MASK) md[u] = a.mask[kk];
            else md[u] = (half_t)0;
        }
    };
    // ---- every piece the prologue needs, requested together: q, k (with their partner halves), v, cos, sin.  All four
    //      waves fetch the k / v pieces (L2 hits, 3 instructions) so that nobody waits for a second batch; wave 0 uses them ----
    const bool rope = cosr != nullptr;
    const half_t *xq = a.qkv + seq_qkv + (size_t)grp * R * kHD, *xk = a.qkv + seq_qkv + (size_t)a.heads * kHD + hoff,
                 *xv = a.qkv + seq_qkv + (size_t)(a.heads + a.kv_heads) * kHD + hoff;
    const half_t *cp = rope ? cosr : xq, *sp = rope ? sinr : xq;  // no rotation: harmless repeats of the q piece, not used
    auto ld8 = [](const half_t *ptr) { return *reinterpret_cast<const half8_t *>(ptr); };
    half8_t q_v[R], q_p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        q_v[r] = ld8(xq + r * kHD + piece * 8);
        q_p[r] = ld8(xq + r * kHD + (piece ^ 8) * 8);
    }
    const half8_t cc = ld8(cp + piece * 8), ss = ld8(sp + piece * 8);
    // ROWS: (wave, slot) j <= tprev takes new row j -- q/k/v row y - tprev + j at position pos - tprev + j, with that position's cos / sin pieces (j > tprev: the own
    // row's addresses again, not used)
    [[maybe_unused]] const int nj = ROWS ? (wave * 4 + slot <= tprev ? wave * 4 + slot : tprev) : 0;
    if constexpr (ROWS) {
        const ptrdiff_t back = (ptrdiff_t)(tprev - nj);
        xk -= back * (a.heads + 2 * a.kv_heads) * kHD;
        xv -= back * (a.heads + 2 * a.kv_heads) * kHD;
    }
    [[maybe_unused]] const half_t *cpk = ROWS && rope ? cp - (ptrdiff_t)(tprev - nj) * kHD : cp, *spk = ROWS && rope ? sp - (ptrdiff_t)(tprev - nj) * kHD : sp;
    const half8_t k_v = ld8(xk + piece * 8), k_p = ld8(xk + (piece ^ 8) * 8), v_v = ld8(xv + piece * 8);
    [[maybe_unused]] half8_t cck, ssk;
    if constexpr (ROWS) {
        cck = ld8(cpk + piece * 8);
        ssk = ld8(spk + piece * 8);
    }
    [[maybe_unused]] half8_t ccs, sss;  // SINK: the pieces of cos / sin row S + W - 1
    if constexpr (SINK) {
        ccs = ld8((rope ? a.cosv + (size_t)a.sink_row * kHD : xq) + piece * 8);
        sss = ld8((rope ? a.sinv + (size_t)a.sink_row * kHD : xq) + piece * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
    fetch(kbuf[0], vbuf[0], mbuf[0], 0);  // (the row at index pos may not be in the cache yet: consume() takes it from LDS)
    // (Round 4, tried: the SECOND block requested here too, so that a wave's first 32 keys cost one memory round trip instead of two.  Slower at every context, in
    // front of the prologue's loads or behind them -- 7.2 -> 7.7 us at 512 keys, 9.05 -> 9.6 at 1024; and again after consume() was made cheaper, as a ring of three
    // buffers with two blocks in flight: 4.35 -> 4.67 us at 128 keys, 7.2 -> 7.55 at 512, a tie on 256-key-per-wave runs.  Same-session A/Bs with
    // scripts/probes/attn_quick.py, profiles/r4/attention_block_softmax_ab.jsonl.)
    __builtin_amdgcn_sched_barrier(0);
    // ---- the R query heads (rotated), this lane's 8 dimensions of each ----
    half8_t qh[R];
#pragma unroll
    for (int r = 0; r < R; ++r) qh[r] = rope ? rope_apply(q_v[r], q_p[r], cc, ss, piece) : q_v[r];
    [[maybe_unused]] half8_t qs[R];  // SINK: the same raw q rotated with row S + W - 1, for the sink keys
    if constexpr (SINK) {
#pragma unroll
        for (int r = 0; r < R; ++r) qs[r] = rope ? rope_apply(q_v[r], q_p[r], ccs, sss, piece) : q_v[r];
    }
    // ---- the new key / value of this head: into LDS for this workgroup's use, into the cache by the workgroup that owns index pos ----
    if (ROWS ? wave * 4 + slot <= tprev : wave == 0) {
        half8_t kh;
        if constexpr (ROWS) kh = rope ? rope_apply(k_v, k_p, cck, ssk, piece) : k_v;
        else kh = rope ? rope_apply(k_v, k_p, cc, ss, piece) : k_v;
        half8_t vh = v_v;
        [[maybe_unused]] uint2_t kq, vq;  // FP8: the row's bytes, and the row as the cache will hold it
        if constexpr (FP8) {
            kq = fp8_quant8(kh, a.k_inv);
            vq = fp8_quant8(vh, a.v_inv);
            kh = fp8_dequant8(kq, a.k_scale);
            vh = fp8_dequant8(vq, a.v_scale);
        }
        if (ROWS || slot == 0) {
            *reinterpret_cast<half8_t *>(&newrow[nj][0][piece * 8]) = kh;
            *reinterpret_cast<half8_t *>(&newrow[nj][1][piece * 8]) = vh;
            if ((!ROWS || nj == tprev) && appends && kpos >= key0 && kpos < key1) {
                if constexpr (PAGED) {
                    // the page that holds index pos: word pos / page_keys, the last one the row owns (a wave-uniform load that depends on the position word, beside
                    // the cos / sin pieces which do too: it delays this store, not the cache requests)
                    const int page = __builtin_amdgcn_readfirstlane(a.table[(size_t)tseq * a.table_stride + (pos >> a.page_shift)]);
                    const size_t off = page_row(page, pos & ((1 << a.page_shift) - 1)) + piece * 8;
                    if constexpr (FP8) {
                        *reinterpret_cast<uint2_t *>(reinterpret_cast<unsigned char *>(a.kc) + off) = kq;
                        *reinterpret_cast<uint2_t *>(reinterpret_cast<unsigned char *>(a.vc) + off) = vq;
                    } else {
                        *reinterpret_cast<half8_t *>(a.kc + off) = kh;
                        *reinterpret_cast<half8_t *>(a.vc + off) = vh;
                    }
                } else {
                    *reinterpret_cast<half8_t *>(a.kc + seq_cache + ((size_t)head * a.max_keys + pos) * kHD + piece * 8) = kh;
                    *reinterpret_cast<half8_t *>(a.vc + seq_cache + ((size_t)head * a.max_keys + pos) * kHD + piece * 8) = vh;
                }
            }
        }
    }
    __syncthreads();
    float m[R], l[R], acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = kNegBig;
        l[r] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
    }
    // One block = 4 steps = 16 keys of the wave.  The online-softmax state moves ONCE per block (round 4): the block's scores first, one new maximum, one rescale
    // of the accumulators, then the four weighted value rows as fused multiply-adds that take the binary16 value straight from its register (v_fma_mix_f32).  The
    // step-by-step form this replaces -- a rescale, two exponentials and 8 conversions per step -- was bound by exactly that arithmetic: 58 vector instructions per
    // step, one wave per SIMD, 0.62 us per block against a memory round trip of about the same length (profiles/r4/attention_block_softmax_ab.jsonl).
    // sink_blk (SINK; a constant at each call: true for a wave's first block alone): step u takes the second query when its group is a sink group -- the scores' text
    // twice, everything else once
    auto consume = [&](const bool sink_blk, const row_t (&kd)[BLK], const row_t (&vd)[BLK], const half_t (&md)[BLK], int it0) {
        half8_t kk[BLK], vv[BLK];
        float sco[R][BLK];
        bool valid[BLK];
#pragma unroll
        for (int u = 0; u < BLK; ++u) {
            if constexpr (FP8) {
                kk[u] = fp8_dequant8(kd[u], a.k_scale);
                vv[u] = fp8_dequant8(vd[u], a.v_scale);
            } else {
                kk[u] = kd[u];
                vv[u] = vd[u];
            }
            valid[u] = true;
        }
        // the rare blocks -- the one that runs past the wave's range, the one that holds the token's own row -- are told apart by a wave-uniform test, so the
        // others carry no per-slot validity arithmetic at all
        const int b0 = kw0 + it0;
        if (b0 + BLK * 4 > kw1 || (ROWS ? (kpos >= b0 && kpos - tprev < b0 + BLK * 4) : (kpos >= b0 && kpos < b0 + BLK * 4)) || (WINDOW && b0 < vlo)) {  // (tprev: 0 unless ROWS; kpos: pos unless SINK; WINDOW: the block of keys base .. lo - 1; SINK: and of the sinks)
#pragma unroll
            for (int u = 0; u < BLK; ++u) {
                const int key = b0 + u * 4 + slot;
                valid[u] = key < kw1;
                if constexpr (SINK) valid[u] = valid[u] && (key >= vlo || key < snk);
                else if constexpr (WINDOW) valid[u] = valid[u] && key >= lo;
                if constexpr (ROWS) {
                    if (key >= kpos - tprev && key <= kpos) {  // this launch's rows of the sequence: in LDS, in the pool only once their workgroups have run (SINK: their virtual indices)
                        kk[u] = *reinterpret_cast<const half8_t *>(&newrow[key - (kpos - tprev)][0][piece * 8]);
                        vv[u] = *reinterpret_cast<const half8_t *>(&newrow[key - (kpos - tprev)][1][piece * 8]);
                    }
                } else if (key == kpos) {  // the token's own row: not necessarily visible in the cache yet
                    kk[u] = *reinterpret_cast<const half8_t *>(&newrow[0][0][piece * 8]);
                    vv[u] = *reinterpret_cast<const half8_t *>(&newrow[0][1][piece * 8]);
                }
                // a slot past the range was loaded from a row that may hold anything (the row at `pos` before this launch wrote it, an
                // uninitialised cache): its weight is 0, and 0 * inf would still be NaN -- the value row is zeroed, not just weighted
                if (!valid[u]) vv[u] = half8_t{(half_t)0, (half_t)0, (half_t)0, (half_t)0, (half_t)0, (half_t)0, (half_t)0, (half_t)0};
            }
        }
        if (SINK && sink_blk) {  // (the loop below with the step's query picked; SINK only)
            if constexpr (SINK) {
#pragma unroll
                for (int u = 0; u < BLK; ++u) {
                    const bool sg = b0 + u * 4 < s4;  // (wave-uniform)
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const half8_t qq = sg ? qs[r] : qh[r];
                        float d = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; e += 2) d = __builtin_amdgcn_fdot2(half2_t{qq[e], qq[e + 1]}, half2_t{kk[u][e], kk[u][e + 1]}, d, false);
                        d = row16_sum(d);
                        float sv = a.alpha * d;
                        if constexpr (MASK) sv += (float)md[u];
                        if (!(__builtin_fabsf(sv) <= 65504.0f)) sv = -65504.0f;  // check_inf_half (Int4llamaAttention.cu:105-115): inf / nan / beyond binary16 -> -65504
                        if (!valid[u]) sv = kNegBig;
                        sco[r][u] = sv;
                    }
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < BLK; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; e += 2) d = __builtin_amdgcn_fdot2(half2_t{qh[r][e], qh[r][e + 1]}, half2_t{kk[u][e], kk[u][e + 1]}, d, false);
                    d = row16_sum(d);
                    float sv = a.alpha * d;
                    if constexpr (MASK) sv += (float)md[u];
                    if (!(__builtin_fabsf(sv) <= 65504.0f)) sv = -65504.0f;  // check_inf_half (Int4llamaAttention.cu:105-115): inf / nan / beyond binary16 -> -65504
                    if (!valid[u]) sv = kNegBig;
                    sco[r][u] = sv;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float bm = __builtin_fmaxf(__builtin_fmaxf(sco[r][0], sco[r][1]), __builtin_fmaxf(sco[r][2], sco[r][3]));
            const float mn = __builtin_fmaxf(m[r], bm);
            const float sc = __expf(m[r] - mn);
            float p[BLK];
#pragma unroll
            for (int u = 0; u < BLK; ++u) p[u] = valid[u] ? __expf(sco[r][u] - mn) : 0.f;  // (a block of nothing but invalid slots on a fresh state: mn == kNegBig, the difference is 0)
            m[r] = mn;
            l[r] = l[r] * sc + ((p[0] + p[1]) + (p[2] + p[3]));
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[r][e] *= sc;
#pragma unroll
            for (int u = 0; u < BLK; ++u) {
                const uint4_t vw = __builtin_bit_cast(uint4_t, vv[u]);
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    acc[r][e] = fma_mix_lo(p[u], vw[e >> 1], acc[r][e]);
                    acc[r][e + 1] = fma_mix_hi(p[u], vw[e >> 1], acc[r][e + 1]);
                }
            }
        }
    };
    // per_wave is a multiple of 4 (steps); blocks of 4 steps, the last one possibly past the range (clamped loads, zero weights)
    // SINK: sink groups lie in a wave's FIRST block only (s4 <= 16), so that block is peeled off the loop and takes the sink form in every wave -- a wave-uniform select
    // of the query per step; the loop behind it carries nothing for the sinks.  (Measured against a wave-uniform branch on the first block inside the loop: the same
    // time, 7 registers fewer -- profiles/sink/sink_time.jsonl and DESIGN.md section 5 say what the sink step costs over the windowed one, and that the cause is not found.)
    if constexpr (SINK) {
        fetch(kbuf[1], vbuf[1], mbuf[1], BLK * 4);
        consume(true, kbuf[0], vbuf[0], mbuf[0], 0);
        for (int it = BLK * 4; it < per_wave; it += 2 * BLK * 4) {  // (the loop below, one block on: the buffers have changed places)
            fetch(kbuf[0], vbuf[0], mbuf[0], it + BLK * 4);
            consume(false, kbuf[1], vbuf[1], mbuf[1], it);
            if (it + BLK * 4 >= per_wave) break;
            fetch(kbuf[1], vbuf[1], mbuf[1], it + 2 * BLK * 4);
            consume(false, kbuf[0], vbuf[0], mbuf[0], it + BLK * 4);
        }
    } else {
        for (int it = 0; it < per_wave; it += 2 * BLK * 4) {
            fetch(kbuf[1], vbuf[1], mbuf[1], it + BLK * 4);
            consume(false, kbuf[0], vbuf[0], mbuf[0], it);
            if (it + BLK * 4 >= per_wave) break;
            fetch(kbuf[0], vbuf[0], mbuf[0], it + 2 * BLK * 4);
            consume(false, kbuf[1], vbuf[1], mbuf[1], it + BLK * 4);
        }
    }
    // ---- merge the workgroup's 4 * NW states, per query head ----
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float *s_ = st[wave * 4 + slot][r];
        if (piece == 0) {
            s_[0] = m[r];
            s_[1] = l[r];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s_[2 + piece * 8 + e] = acc[r][e];
    }
    __syncthreads();
    float M[R], Lq[R], O[R];  // thread d < 128 owns output dimension d of every query head
    if (tid < kHD) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float Mx = kNegBig;
#pragma unroll
            for (int i = 0; i < NS; ++i) Mx = __builtin_fmaxf(Mx, st[i][r][0]);
            float Lx = 0.f, Ox = 0.f;
#pragma unroll 16
            for (int i = 0; i < NS; ++i) {
                const float w = __expf(st[i][r][0] - Mx);
                Lx += st[i][r][1] * w;
                Ox += st[i][r][2 + tid] * w;
            }
            M[r] = Mx;
            Lq[r] = Lx;
            O[r] = Ox;
        }
    }
    const size_t qoff = (size_t)grp * R * kHD;  // the first of this workgroup's query heads in `out`
    if (chunks == 1) {
        if (tid < kHD) {
#pragma unroll
            for (int r = 0; r < R; ++r) a.out[seq_out + qoff + r * kHD + tid] = (half_t)(O[r] / Lq[r]);
        }
        return;
    }
    if (a.defer) {  // the combine happens in the next launch's prologue (same arithmetic, same order: tce_w4a16_forward_deferred_attention)
        if (tid < kHD) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float *mine = a.part + ((size_t)(grp * R + r) * a.chunks + c) * kDeferStride;
                mine[4 + tid] = O[r];
                if (tid == 0) {
                    mine[0] = M[r];
                    mine[1] = Lq[r];
                }
            }
        }
        return;
    }
    if (a.probe_no_combine) {  // (round 5 probe: what the launch costs without its combine -- the upper bound of moving the combine into the next launch's prologue)
        if (tid < kHD) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float *mine = a.part + ((size_t)(grp * R + r) * chunks + c) * (2 + kHD);
                mine[2 + tid] = O[r];
                if (tid == 0) {
                    mine[0] = M[r];
                    mine[1] = Lq[r];
                }
            }
        }
        return;
    }
    // ---- several chunks per head: partial (M, L, O) to the workspace, the last workgroup to arrive combines ----
    if (tid < kHD) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float *mine = a.part + seq_ws + ((size_t)(grp * R + r) * chunks + c) * (2 + kHD);
            __hip_atomic_store(mine + 2 + tid, O[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // write-through (sc1) stores
            if (tid == 0) {
                __hip_atomic_store(mine, M[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(mine + 1, Lq[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores are acknowledged before the workgroup arrives
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.cnt + seq_ws + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = old == (unsigned)chunks - 1 ? 1u : 0u;
        if (last_flag) __hip_atomic_store(a.cnt + seq_ws + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    }
    __syncthreads();
    if (!last_flag) return;
    // The partials were stored write-through; they are read back with device-coherent (sc0 sc1) buffer loads -- plain loads as
    // far as the compiler is concerned, so all of a thread's loads are in flight together (a loop of relaxed atomic loads is a
    // chain of round trips: 1 us per chunk, measured).  Thread i < chunks fetches (M_i, L_i), every thread d < hd its O_i[d].
    constexpr int kMaxChunksUnrolled = 16;
    float *ml = &st[0][0][0];  // [R][chunks][2], reuses the state area
    const int stride = (2 + kHD) * 4;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.part + seq_ws + (size_t)grp * R * chunks * (2 + kHD), 0, (int)((size_t)R * chunks * stride), 0x00020000);
    for (int i = tid; i < R * chunks; i += NT) {
        ml[2 * i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, i * stride, 0, /*sc0|sc1*/ 17));
        ml[2 * i + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, i * stride + 4, 0, 17));
    }
    float oi[R][kMaxChunksUnrolled];
    if (tid < kHD) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < kMaxChunksUnrolled; ++i)
                oi[r][i] = i < chunks ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (r * chunks + i) * stride + (2 + tid) * 4, 0, 17)) : 0.f;
    }
    __syncthreads();
    if (tid < kHD) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float *mlr = ml + 2 * r * chunks;
            float Mx = kNegBig;
            for (int i = 0; i < chunks; ++i) Mx = __builtin_fmaxf(Mx, mlr[2 * i]);
            float Lx = 0.f, Ox = 0.f;
#pragma unroll
            for (int i = 0; i < kMaxChunksUnrolled; ++i) {
                if (i < chunks) {
                    const float w = __expf(mlr[2 * i] - Mx);
                    Lx += mlr[2 * i + 1] * w;
                    Ox += oi[r][i] * w;
                }
            }
            for (int i = kMaxChunksUnrolled; i < chunks; ++i) {  // many chunks: the rest one by one
                const float w = __expf(mlr[2 * i] - Mx);
                Lx += mlr[2 * i + 1] * w;
                Ox += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (r * chunks + i) * stride + (2 + tid) * 4, 0, 17)) * w;
            }
            a.out[seq_out + qoff + r * kHD + tid] = (half_t)(Ox / Lx);
        }
    }
}

}  // namespace

}  // namespace tce
