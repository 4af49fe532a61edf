// attention_fast.hip -- one decode step of the reference's Llama attention block between the fused q/k/v linear and o_proj, as
// ONE launch, bandwidth-bound in the KV cache ("flash-decoding").
//
// What it replaces per token and layer (llm/src/nn_modules/cuda/Int4llamaAttention.cu:116-229):
//     shape_qkv_cuda (:41-64, 130-136)          the fused projection's row [3 * heads * hd] is read in place (q | k | v, head-major)
//     RotaryPosEmb_cuda_forward (:157-159)      applied to q and the new k while they are loaded -- the reference's binary16
//                                               arithmetic hfma(x, cos, hmul(rot, sin)) (llm/src/ops/cuda/RotaryPosEmb.cu:4-34): the
//                                               key that enters the cache is bit-identical to the reference's
//     the KV append (:161-181)                  the reference copies the WHOLE past into the layer's other cache buffer every token
//                                               (4 cudaMemcpyAsync per head, O(t)); here the cache is one fixed-capacity array
//                                               [heads][max_keys][hd] per K and V and the new row is written at index `pos`
//     qk_bmm -> batch_Add -> check_inf_half -> softmax -> transpose_1_2idx -> pv_bmm -> unshape (:184-217)
//                                               scores, online softmax and the weighted sum of V rows in fp32, the key range cut into
//                                               chunks over workgroups (heads x chunks fills the chip); V is read in the layout it was
//                                               appended in (no transposed copy); the output row [heads * hd] is o_proj's input
// The bit-exact form of the same block -- binary16 accumulation chains in the reference's order -- stays available as
// tce_attention_decode_f16 (attention_ops.hip); that one is what parity is claimed with.  THIS kernel computes the same function
// in fp32 and is checked against it with a stated tolerance (tests/test_gpu_attention.py): |out - ref| <= 2e-3 * max|ref| per head
// + one binary16 ulp, i.e. the difference between fp32 and binary16 accumulation, not a different algorithm.
//
// Work decomposition: workgroup = (head, chunk of keys), 4 waves; a wave takes 4 keys per step -- lane = (key slot = lane / 16,
// piece = lane % 16): one 16-byte load per lane covers 4 consecutive cache rows completely (1 KiB contiguous), the dot product is 4
// v_dot2_f32_f16 per lane plus a 4-step DPP sum over the 16 lanes of a row, every lane of the row then holds the score and
// rescales its own 8 output dimensions (online softmax state per (wave, key slot)).  The 16 states of a workgroup are merged
// through LDS, the chunks of a head through a small fp32 workspace by the last workgroup to arrive (write-through stores +
// device-scope loads: MI355X_MICROARCH.md, inter-workgroup visibility; no cache-wide fence).
#include "attention_fast_kernel.hpp"

namespace tce {

// chunk of keys per workgroup: heads x chunks should cover the chip a couple of times; a multiple of 16 (4 waves x 4 keys per step)
static thread_local int g_attn_target_wgs = 0;  // 0: the fitted rule below; tuning: tce_w4a16_set_debug_mode(3000 + workgroups) -- five rows of tuning_modes.hpp: other families' modes lie inside 3000 .. 11192; every count: tce_attention_set_tuning
void set_attention_fast_target(int wgs) { g_attn_target_wgs = wgs >= 32 && wgs <= 8192 ? wgs : 0; }

// Measured (scripts/attention_step_sweep.py, profiles/r2/attention_step_sweep.jsonl; 32 heads, caches rotating through > 256 MB so the
// keys come from HBM).  Two costs pull against each other: a workgroup streams its keys at ~60 GB/s (2.2 us per 256 keys), and
// combining the chunks of a head costs ~2 us whatever their number (the acknowledged-store -> counter -> coherent-read chain):
//   128 keys: one chunk 4.5 us, two 6.0          256: one chunk 6.5, two or four 7.0        512: 8.9 / 8.6 / 7.6 / 8.5 for 1 / 2 / 4 / 8 chunks
//   1024: 9.0 with 4 chunks, 9.3 with 8, 12.5 with 16      2048: 12.0 / 11.8 / 13.7 with 4 / 8 / 16      4096: 18.6 / 16.7 / 18.3
//   8192: 30.0 / 28.9 / 33.4 with 8 / 16 / 32
// Rule: up to 320 keys one chunk per head and no combine; four chunks up to 1024 keys (up to 640 with 4+ query heads per key / value head: round 4); beyond, eight chunks of at most 512 keys.
// A combine without the acknowledged-store -> counter -> coherent-read chain (the head's last workgroup polling (value, tag) pairs)
// was tried and was SLOWER (13.2 us at 2048 keys): a poll is a full memory round trip, and the chain it replaces is three of them
// only on the LAST workgroup.  So was the hybrid -- (value, tag) pairs stored without waiting for acknowledgements, the counter only
// electing who combines, the elected workgroup re-reading the pairs whose tag is not there yet: 7.1-8.0 / 10.5-11.4 / 13.7-14.6 us at
// 128 / 512 / 2048 keys against 6.0 / 8.6 / 11.8 (profiles/r2/attention_merge_variants.jsonl): a write-through store takes longer to
// become visible to another XCD than the counter's round trip, so the first read pass misses and every further pass is a round
// trip of its own.
static thread_local int g_attn_waves = 0;  // 0: by the chunk's length; tuning: tce_w4a16_set_debug_mode(2900 + 4 / 8 / 16)
void set_attention_fast_waves(int nw) { g_attn_waves = (nw == 4 || nw == 8 || nw == 16) ? nw : 0; }

static thread_local int g_attn_probe_no_combine = 0;
void set_attention_fast_probe_no_combine(int on) { g_attn_probe_no_combine = on ? 1 : 0; }
static thread_local int g_attn_fuse = 0;  // tuning: query heads per workgroup for grouped-query attention (0: the rule; 1, 2, 4)
void set_attention_fast_fuse(int r) { g_attn_fuse = (r == 1 || r == 2 || r == 4) ? r : 0; }

// `heads` here = workgroup groups (query heads / heads per workgroup)
// tuned = false: the fitted rule alone, whatever the calling thread's tuning settings (the batched step)
static void pick_chunk(int heads, int keys, int rep, int *chunk_out, int *waves_out, bool tuned = true) {
    int chunk;
    if (tuned && g_attn_target_wgs > 0) {
        const int target_chunks = heads >= g_attn_target_wgs ? 1 : g_attn_target_wgs / heads;
        chunk = (keys + target_chunks - 1) / target_chunks;
        if (chunk < 64) chunk = 64;
    } else if (keys <= 320) {
        chunk = keys;
    } else if (keys <= (rep >= 4 ? 640 : 1024)) {  // (round 4, after the block softmax, 4 query heads per key / value head: 1024 keys 8.7 us with four chunks, 8.2 with eight; 512 keys 7.25 / 7.45.
                                                   //  One query head per key / value head -- four times the cache bytes per query head --: 768 / 1024 keys 8.4 / 8.75 with four, 8.9 / 9.2 with eight)
        chunk = (keys + 3) >> 2;
    } else {
        chunk = (keys + 7) >> 3;
        if (chunk > 512) chunk = 512;
    }
    if (chunk > 1024) chunk = 1024;
    // Waves per workgroup: 4.  More waves on the same chunk (a shorter chain of 16-key blocks per wave, no extra partials) measured
    // SLOWER at every context -- 128 keys 4.5 / 5.2 / 7.4 us with 4 / 8 / 16 waves, 2048 keys 11.7 / 12.1 / 14.4
    // (profiles/r2/attention_step_waves_sweep.jsonl): the launch is at the floor of a dependent load -> compute -> store launch
    // (4.5 us; the 8 MiB GEMV's is 4.1) plus ~2 us for the combine plus the keys at 6.4 TB/s, and wider workgroups only add to the
    // fixed part (prologue loads per wave, barriers, the workgroup's own merge over 4 x waves states).
    int nw = tuned && g_attn_waves ? g_attn_waves : 4;
    chunk = (chunk + 4 * nw - 1) / (4 * nw) * (4 * nw);
    *chunk_out = chunk;
    *waves_out = nw;
}

// the cut launch_attention_decode_fast would use for `keys` keys (no HIP call)
// Query heads per workgroup for `rep` query heads per key / value head.  Measured (scripts/attention_gqa_sweep.py, 32 over 8 heads): the step is
// bound by latency and by the softmax / weighted-sum arithmetic per (query head, key), not by the cache bytes, so fusing the four query
// heads of a key / value head into one workgroup (a quarter of the bytes, a quarter of the workgroups, four times the arithmetic each) is
// SLOWER than one query head per workgroup reading the shared rows: 8.3 / 13.9 / 20.0 us against 4.6 / 7.9 / 11.9 at 128 / 512 / 2048 keys.
static int pick_fuse(int rep) {
    if (g_attn_fuse && rep % g_attn_fuse == 0) return g_attn_fuse;
    return 1;
}

void describe_attention_decode_fast(int heads, int keys, int *chunk, int *chunks, int *waves, int kv_heads) {
    const int rep = kv_heads > 0 ? heads / kv_heads : 1;
    pick_chunk(heads / pick_fuse(rep), keys, rep, chunk, waves);
    *chunks = (keys + *chunk - 1) / *chunk;
}

size_t attention_decode_workspace_bytes(int heads, int max_keys, int hd) {
    if (heads <= 0 || max_keys <= 0 || hd != kHD) return 0;
    return attn_workspace_words(heads, max_keys) * 4;  // (the deferred layout's stride; the combined form's 2 + hd fits inside)
}

int launch_attention_decode_fast(const void *qkv, void *kc, void *vc, const void *cosv, const void *sinv, const void *mask, void *out, void *workspace,
                                 int heads, int kv_heads, int hd, int max_keys, int pos, unsigned short alpha_bits, hipStream_t stream, hipError_t *hip_err,
                                 const int *pos_dev, AttnDeferred *deferred) {
    if (hd != kHD || kv_heads <= 0 || heads % kv_heads != 0) return TCE_ERR_UNSUPPORTED_SHAPE;
    const int rep = heads / kv_heads;

    FastAttnArgs a{};
    a.qkv = static_cast<const half_t *>(qkv);
    a.kc = static_cast<half_t *>(kc);
    a.vc = static_cast<half_t *>(vc);
    a.cosv = static_cast<const half_t *>(cosv);
    a.sinv = static_cast<const half_t *>(sinv);
    a.mask = static_cast<const half_t *>(mask);
    a.out = static_cast<half_t *>(out);
    const size_t cnt_bytes = ((size_t)heads * 4 + 255) & ~(size_t)255;
    a.cnt = static_cast<unsigned *>(workspace);
    a.part = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + cnt_bytes);
    a.heads = heads;
    a.kv_heads = kv_heads;
    a.rep = rep;
    const int fuse = pick_fuse(rep);
    a.hd = hd;
    a.max_keys = max_keys;
    a.pos = pos;
    a.keys = pos + 1;
    a.pos_dev = pos_dev;
    int nw = 4;
    pick_chunk(heads / fuse, a.keys, rep, &a.chunk, &nw);
    a.chunks = (a.keys + a.chunk - 1) / a.chunk;
    if (a.chunks > 1024) return TCE_ERR_UNSUPPORTED_SHAPE;  // (the combine's LDS image; unreachable with the fitted rule below 500k keys)
    half_t ah;
    __builtin_memcpy(&ah, &alpha_bits, 2);
    a.alpha = (float)ah;
    a.probe_no_combine = g_attn_probe_no_combine;
    if (deferred) {
        // deferred combine: 2 .. kDeferMaxSlots chunk slots (one slot: the launch writes `out` itself, as it does whenever only one chunk of the bound is live)
        a.defer = a.chunks >= 2 && a.chunks <= kAttnDeferMaxSlots ? 1 : 0;
        deferred->slots = a.defer ? a.chunks : 1;
        deferred->chunk = a.chunk;
        deferred->heads = heads;
        deferred->stride = kDeferStride;
        deferred->part = a.part;
    }
    const dim3 grid((heads / fuse) * a.chunks);
    auto go = [&](auto has_mask) {
        constexpr bool MK = decltype(has_mask)::value;
        if (fuse == 4) hipLaunchKernelGGL((attn_decode_fast_kernel<MK, 4, 4>), grid, dim3(256), 0, stream, a);
        else if (fuse == 2) hipLaunchKernelGGL((attn_decode_fast_kernel<MK, 4, 2>), grid, dim3(256), 0, stream, a);
        else if (nw == 16) hipLaunchKernelGGL((attn_decode_fast_kernel<MK, 16, 1>), grid, dim3(1024), 0, stream, a);
        else if (nw == 8) hipLaunchKernelGGL((attn_decode_fast_kernel<MK, 8, 1>), grid, dim3(512), 0, stream, a);
        else hipLaunchKernelGGL((attn_decode_fast_kernel<MK, 4, 1>), grid, dim3(256), 0, stream, a);
    };
    if (a.mask) go(std::true_type{});
    else go(std::false_type{});
    return launch_status(hip_err);
}

// the batched step's cut: the single step's fitted rule for pos_bound + 1 keys, one query head per workgroup (no HIP call)
void describe_attention_decode_batch(int heads, int kv_heads, int pos_bound, int *chunk, int *chunks, int *waves) {
    pick_chunk(heads, pos_bound + 1, heads / kv_heads, chunk, waves, false);
    *chunks = (pos_bound + 1 + *chunk - 1) / *chunk;
}

// the windowed paged step's cut: the same rule for the keys a workgroup group can span, min(pos_bound + 1, window + 3) -- base = lo & ~3 puts up to three keys in front
// of the window's first (no HIP call)
int attention_window_cut_keys(int pos_bound, int window) { return (long long)window + 3 < (long long)pos_bound + 1 ? window + 3 : pos_bound + 1; }
void describe_attention_decode_window(int heads, int kv_heads, int pos_bound, int window, int *chunk, int *chunks, int *waves) {
    describe_attention_decode_batch(heads, kv_heads, attention_window_cut_keys(pos_bound, window) - 1, chunk, chunks, waves);
}

// the sink step's cut: the same rule for the VIRTUAL keys a workgroup group can span (no HIP call).  A binding row's are S4 + (pos - base2 + 1) <= S4 + window + 3; a row
// that does not bind has its pos + 1 <= pos_bound + 1 keys.  While no row of the launch can bind (sinks + window > pos_bound) that is the unwindowed step's cut, chunk for
// chunk.  Else min(pos_bound + 1, S4 + window + 3) -- plus the S4 - ((S + 1) & ~3) keys (0 or 4) by which a binding row's virtual sequence can be LONGER than pos + 1: its
// first window group may start below S4 (S = 5, lo = 6: sinks in groups 0 and 4, the window's first group is 4 again)
int attention_sink_cut_keys(int pos_bound, int window, int sinks) {
    const long long s4 = (sinks + 3) & ~3, all = (long long)pos_bound + 1;
    if ((long long)sinks + window > pos_bound) return (int)all;
    const long long bound = all + (s4 - ((sinks + 1) & ~3)), span = s4 + window + 3;
    const long long cut = span < bound ? span : bound;
    return (int)(cut < 0x7fffffffLL ? cut : 0x7fffffffLL);
}
void describe_attention_decode_sink(int heads, int kv_heads, int pos_bound, int window, int sinks, int *chunk, int *chunks, int *waves) {
    describe_attention_decode_batch(heads, kv_heads, attention_sink_cut_keys(pos_bound, window, sinks) - 1, chunk, chunks, waves);
}

size_t attention_decode_batch_workspace_bytes(int batch, int heads, int max_keys, int hd) {
    if (batch <= 0) return 0;
    return (size_t)batch * attention_decode_workspace_bytes(heads, max_keys, hd);
}

int launch_attention_decode_batch(const AttnStepArgs &s, void *kc, void *vc, int max_keys, hipStream_t stream, hipError_t *hip_err) {
    const int batch = s.batch, heads = s.heads, kv_heads = s.kv_heads, hd = s.hd, pos_bound = s.pos_bound;
    if (hd != kHD || kv_heads <= 0 || heads % kv_heads != 0 || batch <= 0 || batch > 65535 || !s.pos_device) return TCE_ERR_UNSUPPORTED_SHAPE;
    FastAttnArgs a{};
    a.qkv = static_cast<const half_t *>(s.qkv);
    a.kc = static_cast<half_t *>(kc);
    a.vc = static_cast<half_t *>(vc);
    a.cosv = static_cast<const half_t *>(s.cosv);
    a.sinv = static_cast<const half_t *>(s.sinv);
    a.out = static_cast<half_t *>(s.out);
    const size_t cnt_bytes = ((size_t)heads * 4 + 255) & ~(size_t)255;  // (one sequence's slice: the single step's layout)
    a.cnt = static_cast<unsigned *>(s.workspace);
    a.part = reinterpret_cast<float *>(static_cast<unsigned char *>(s.workspace) + cnt_bytes);
    a.heads = heads;
    a.kv_heads = kv_heads;
    a.rep = heads / kv_heads;
    a.hd = hd;
    a.max_keys = max_keys;
    a.pos = pos_bound;
    a.keys = pos_bound + 1;
    a.pos_dev = s.pos_device;
    int nw = 4;
    describe_attention_decode_batch(heads, kv_heads, pos_bound, &a.chunk, &a.chunks, &nw);
    if (a.chunks > 1024 || nw != 4) return TCE_ERR_UNSUPPORTED_SHAPE;
    half_t ah;
    __builtin_memcpy(&ah, &s.alpha_bits, 2);
    a.alpha = (float)ah;
    hipLaunchKernelGGL((attn_decode_fast_kernel<false, 4, 1, true>), dim3(heads * a.chunks, batch), dim3(256), 0, stream, a);
    return launch_status(hip_err);
}

// ---- pages <-> a contiguous single-sequence cache pair, and the block-table check (the paged step's companions) ----
namespace {

// Rows [key0, key0 + nkeys) of every key / value head between a contiguous pair [kv_heads][lin_max_keys][hd] and the pages one table row names; GATHER: pages ->
// contiguous, else contiguous -> pages.  One thread per 16 bytes, grid.y: K / V.  A table word outside [0, num_pages) copies nothing (no address is formed from it).
template <bool GATHER>
__global__ __launch_bounds__(256) void kv_pages_copy_kernel(half_t *k_lin, half_t *v_lin, half_t *k_pool, half_t *v_pool, const int *table_row, int page_shift,
                                                            int num_pages, int kv_heads, int lin_max_keys, int key0, int nkeys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int piece = (int)(i & 15);
    const long long r = i >> 4;  // (head, key of the range)
    if (r >= (long long)kv_heads * nkeys) return;
    const int head = (int)(r / nkeys), key = key0 + (int)(r % nkeys);
    const int page = table_row[key >> page_shift];
    if (page < 0 || page >= num_pages) return;
    const size_t po = ((((size_t)page * kv_heads + head) << page_shift) + (key & ((1 << page_shift) - 1))) * kHD + piece * 8;
    const size_t lo = ((size_t)head * lin_max_keys + key) * kHD + piece * 8;
    half_t *lin = blockIdx.y ? v_lin : k_lin, *pool = blockIdx.y ? v_pool : k_pool;
    if constexpr (GATHER) *reinterpret_cast<half8_t *>(lin + lo) = *reinterpret_cast<const half8_t *>(pool + po);
    else *reinterpret_cast<half8_t *>(pool + po) = *reinterpret_cast<const half8_t *>(lin + lo);
}

// The same pair of copies with an e4m3 pool side and a contiguous fp16 side: scatter quantises (fp8_kv.hpp: the format's rule), gather dequantises.  One thread per 8
// elements -- 16 bytes of the contiguous row, 8 of the pool row; grid.y: K / V, each with its own power of two.
template <bool GATHER>
__global__ __launch_bounds__(256) void kv_pages_copy_fp8_kernel(half_t *k_lin, half_t *v_lin, unsigned char *k_pool, unsigned char *v_pool, const int *table_row, int page_shift,
                                                                int num_pages, int kv_heads, int lin_max_keys, int key0, int nkeys, int k_log2, int v_log2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int piece = (int)(i & 15);
    const long long r = i >> 4;  // (head, key of the range)
    if (r >= (long long)kv_heads * nkeys) return;
    const int head = (int)(r / nkeys), key = key0 + (int)(r % nkeys);
    const int page = table_row[key >> page_shift];
    if (page < 0 || page >= num_pages) return;
    const size_t po = ((((size_t)page * kv_heads + head) << page_shift) + (key & ((1 << page_shift) - 1))) * kHD + piece * 8;
    const size_t lo = ((size_t)head * lin_max_keys + key) * kHD + piece * 8;
    half_t *lin = blockIdx.y ? v_lin : k_lin;
    unsigned char *pool = blockIdx.y ? v_pool : k_pool;
    const int e = blockIdx.y ? v_log2 : k_log2;
    if constexpr (GATHER) *reinterpret_cast<half8_t *>(lin + lo) = fp8_dequant8(*reinterpret_cast<const uint2_t *>(pool + po), fp8_pow2(e));
    else *reinterpret_cast<uint2_t *>(pool + po) = fp8_quant8(*reinterpret_cast<const half8_t *>(lin + lo), fp8_pow2(-e));
}

// *violations = the number of table words an active row would follow that are not page numbers, plus the active rows whose position needs a word past the row
// (one workgroup: the tables are a few thousand words)
// WINDOW: of the words a WINDOWED row would follow, lo / page_keys .. pos / page_keys (lo = max(0, pos - window + 1)); else from word 0 (`window` unused)
// SINK (with WINDOW): of the words a sink row would follow -- one that binds (pos >= sinks + window) word 0 and lo / page_keys .. pos / page_keys, one that does not
// words 0 .. pos / page_keys
template <bool WINDOW, bool SINK = false>
__global__ __launch_bounds__(1024) void kv_block_table_check_kernel(const int *table, int table_stride, int page_shift, int num_pages, int batch, const int *pos_dev,
                                                                    int pos_bound, unsigned *violations, int window, int sinks = 0) {
    __shared__ unsigned bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int b = 0; b < batch; ++b) {
        const int pos = pos_dev[b];
        if (pos < 0 || pos > pos_bound) continue;
        int last = pos >> page_shift;
        if (last >= table_stride) {
            if (threadIdx.x == 0) ++mine;
            last = table_stride - 1;
        }
        const int first = WINDOW && (SINK ? pos - window >= sinks : pos - window + 1 > 0) ? (pos - window + 1) >> page_shift : 0;
        if constexpr (SINK) {
            if (first > 0 && threadIdx.x == 0) {
                const int page = table[(size_t)b * table_stride];
                if (page < 0 || page >= num_pages) ++mine;
            }
        }
        for (int e = first + threadIdx.x; e <= last; e += 1024) {
            const int page = table[(size_t)b * table_stride + e];
            if (page < 0 || page >= num_pages) ++mine;
        }
    }
    if (mine) atomicAdd(&bad, mine);
    __syncthreads();
    if (threadIdx.x == 0) *violations = bad;
}

}  // namespace

// ---- the paged step: the batched step on pools of pages.  The cut, the grid, the workspace layout and every row's arithmetic are the batched step's ----
size_t kv_pages_pool_bytes(int num_pages, int kv_heads, int page_keys, int hd) {
    if (num_pages <= 0 || kv_heads <= 0 || hd != kHD || page_shift_of(page_keys) < 0) return 0;
    return (size_t)num_pages * kv_heads * page_keys * kHD * sizeof(half_t);
}

size_t kv_pages_pool_bytes_fp8(int num_pages, int kv_heads, int page_keys, int hd) {
    if (num_pages <= 0 || kv_heads <= 0 || hd != kHD || page_shift_of(page_keys) < 0) return 0;
    return (size_t)num_pages * kv_heads * page_keys * kHD;
}

// pages.fp8: the pools are e4m3 bytes and the two exponents apply; everything else is one text for both
// rows = 0: the step; rows >= 1: the multi-row step with rows_per_seq = rows -- the same cut (pos_bound alone decides it), grid (heads x chunk slots, rows, batch)
// s.window >= 1 (with either): the windowed step -- the cut and the grid are made for min(pos_bound + 1, window + 3) keys.  The workspace slices stay where every
// other launch on the same workspace has them (one per table row's keys): the arrival counters at their heads are zero between launches only there
// s.window and rows: the windowed multi-row step -- the windowed cut and workgroup order, grid (padded pairs x rep, rows, batch), one workspace slice per virtual row
int launch_attention_decode_paged(const KvPages &pg, const AttnStepArgs &s, int rows, hipStream_t stream, hipError_t *hip_err) {
    const int batch = s.batch, heads = s.heads, kv_heads = s.kv_heads, hd = s.hd, pos_bound = s.pos_bound, table_stride = pg.table_stride;
    const bool fp8 = pg.fp8;
    const int shift = page_shift_of(pg.page_keys);
    if (hd != kHD || kv_heads <= 0 || heads % kv_heads != 0 || batch <= 0 || batch > 65535 || !s.pos_device || !pg.table || shift < 0 || table_stride < 1 ||
        (long long)pos_bound >= ((long long)table_stride << shift))
        return TCE_ERR_UNSUPPORTED_SHAPE;
    if (fp8 && !(fp8_log2_ok(pg.k_scale_log2) && fp8_log2_ok(pg.v_scale_log2))) return TCE_ERR_UNSUPPORTED_SHAPE;
    if (rows < 0 || rows > TCE_SPEC_MAX_ROWS || s.window < 0) return TCE_ERR_UNSUPPORTED_SHAPE;
    PagedFp8AttnArgs a{};
    a.qkv = static_cast<const half_t *>(s.qkv);
    a.kc = static_cast<half_t *>(pg.k_pool);
    a.vc = static_cast<half_t *>(pg.v_pool);
    a.cosv = static_cast<const half_t *>(s.cosv);
    a.sinv = static_cast<const half_t *>(s.sinv);
    a.out = static_cast<half_t *>(s.out);
    const size_t cnt_bytes = ((size_t)heads * 4 + 255) & ~(size_t)255;
    a.cnt = static_cast<unsigned *>(s.workspace);
    a.part = reinterpret_cast<float *>(static_cast<unsigned char *>(s.workspace) + cnt_bytes);
    a.heads = heads;
    a.kv_heads = kv_heads;
    a.rep = heads / kv_heads;
    a.hd = hd;
    a.max_keys = table_stride << shift;  // (the workspace slices' size; no cache address is formed from it)
    a.pos = pos_bound;
    a.keys = pos_bound + 1;
    a.pos_dev = s.pos_device;
    a.table = pg.table;
    a.table_stride = table_stride;
    a.page_shift = shift;
    if (s.sinks && (!s.window || rows || s.sinks < 1 || s.sinks > 16)) return TCE_ERR_UNSUPPORTED_SHAPE;
    int nw = 4;
    if (s.sinks) describe_attention_decode_sink(heads, kv_heads, pos_bound, s.window, s.sinks, &a.chunk, &a.chunks, &nw);
    else if (s.window) describe_attention_decode_window(heads, kv_heads, pos_bound, s.window, &a.chunk, &a.chunks, &nw);
    else describe_attention_decode_batch(heads, kv_heads, pos_bound, &a.chunk, &a.chunks, &nw);
    if (a.chunks > 1024 || nw != 4) return TCE_ERR_UNSUPPORTED_SHAPE;
    half_t ah;
    __builtin_memcpy(&ah, &s.alpha_bits, 2);
    a.alpha = (float)ah;
    if (fp8) {
        a.k_scale = host_pow2(pg.k_scale_log2);
        a.v_scale = host_pow2(pg.v_scale_log2);
        a.k_inv = host_pow2(-pg.k_scale_log2);
        a.v_inv = host_pow2(-pg.v_scale_log2);
    }
    // the grid: x -- (query head, chunk slot) pairs; windowed: whole groups of 8 (key / value head, chunk slot) pairs x rep query heads (see the kernel) --, then the
    // sequences, or (rows) the rows and the sequences
    const dim3 grid(s.window ? (kv_heads * a.chunks + 7) / 8 * 8 * a.rep : heads * a.chunks, rows ? rows : batch, rows ? batch : 1);
    with_bools([&](auto fp8_c, auto rows_c, auto window_c, auto sink_c) {
        constexpr bool FP8 = decltype(fp8_c)::value, ROWS = decltype(rows_c)::value, WINDOW = decltype(window_c)::value, SINK = decltype(sink_c)::value;
        if constexpr (!SINK || (WINDOW && !ROWS)) {  // (sinks exist beside a window; here on the one-row step -- refused above -- the rows form is attention_rows_sink.hip's)
            using args_t = step_args_t<true, FP8, ROWS, WINDOW, SINK>;  // the form's arguments: `a` (the fp16 step: its PagedAttnArgs) and the form's own fields
            args_t w{};
            static_cast<std::conditional_t<std::is_base_of_v<PagedFp8AttnArgs, args_t>, PagedFp8AttnArgs, PagedAttnArgs> &>(w) = a;
            if constexpr (ROWS) w.rows_per_seq = rows;
            if constexpr (WINDOW) w.window = s.window;
            if constexpr (SINK) {
                w.sinks = s.sinks;
                w.sink_row = (long long)s.sinks + s.window - 1 < (long long)pos_bound ? s.sinks + s.window - 1 : pos_bound;
            }
            hipLaunchKernelGGL((attn_decode_fast_kernel<false, 4, 1, true, true, FP8, ROWS, WINDOW, SINK>), grid, dim3(256), 0, stream, w);
        }
    }, fp8, rows != 0, s.window != 0, s.sinks != 0);
    return launch_status(hip_err);
}

// rows [key0, key0 + nkeys) between the contiguous pair and the pages of the table row pages.table; pages.fp8: scatter quantises, gather dequantises
int launch_kv_pages_copy(const KvPages &pg, const KvLinear &lin, bool gather, int key0, int nkeys, hipStream_t stream, hipError_t *hip_err) {
    const int shift = page_shift_of(pg.page_keys), kv_heads = lin.kv_heads, k_log2 = pg.k_scale_log2, v_log2 = pg.v_scale_log2;
    if (shift < 0 || kv_heads <= 0 || nkeys <= 0 || key0 < 0 || (long long)key0 + nkeys > lin.max_keys) return TCE_ERR_UNSUPPORTED_SHAPE;
    if (pg.fp8 && !(fp8_log2_ok(k_log2) && fp8_log2_ok(v_log2))) return TCE_ERR_UNSUPPORTED_SHAPE;
    const dim3 grid((unsigned)(((long long)kv_heads * nkeys * 16 + 255) / 256), 2);
    auto h = [](void *p) { return static_cast<half_t *>(p); };
    auto b = [](void *p) { return static_cast<unsigned char *>(p); };
    auto go = [&](auto kernel, auto pool, auto... exponents) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, h(lin.k), h(lin.v), pool(pg.k_pool), pool(pg.v_pool), pg.table, shift, pg.num_pages, kv_heads, lin.max_keys, key0, nkeys,
                           exponents...);
    };
    if (!pg.fp8) gather ? go(kv_pages_copy_kernel<true>, h) : go(kv_pages_copy_kernel<false>, h);
    else gather ? go(kv_pages_copy_fp8_kernel<true>, b, k_log2, v_log2) : go(kv_pages_copy_fp8_kernel<false>, b, k_log2, v_log2);
    return launch_status(hip_err);
}

int launch_kv_block_table_check(const KvPages &pg, int batch, const int *pos_dev, int pos_bound, unsigned *violations, hipStream_t stream, hipError_t *hip_err, int window,
                                int sinks) {
    const int shift = page_shift_of(pg.page_keys);
    if (shift < 0 || pg.table_stride < 1 || batch < 1 || (sinks && window < 1)) return TCE_ERR_UNSUPPORTED_SHAPE;
    if (sinks > 0) hipLaunchKernelGGL((kv_block_table_check_kernel<true, true>), dim3(1), dim3(1024), 0, stream, pg.table, pg.table_stride, shift, pg.num_pages, batch, pos_dev, pos_bound, violations, window, sinks);
    else if (window > 0) hipLaunchKernelGGL(kv_block_table_check_kernel<true>, dim3(1), dim3(1024), 0, stream, pg.table, pg.table_stride, shift, pg.num_pages, batch, pos_dev, pos_bound, violations, window);
    else hipLaunchKernelGGL(kv_block_table_check_kernel<false>, dim3(1), dim3(1024), 0, stream, pg.table, pg.table_stride, shift, pg.num_pages, batch, pos_dev, pos_bound, violations, 0);
    return launch_status(hip_err);
}

}  // namespace tce
