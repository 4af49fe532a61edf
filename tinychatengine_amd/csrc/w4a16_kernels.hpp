// w4a16_kernels.hpp -- host-visible declarations shared by the W4A16 translation units.
#pragma once
#include "tce_common.hpp"
#include "tuning_setters.hpp"  // the set_* tuning setters of the units below

namespace tce {

// One linear of a (possibly grouped) GEMV launch.
struct GemvSeg {
    const uint4_t *qweight;  // u32 [N][K/8] viewed as 16-byte chunks: [N][K/32]
    const half_t *scales;    // fp16 [N][scales_stride]
    const unsigned *zeros;   // u32 [N][zeros_stride]
    half_t *C;               // fp16 [M][ldc]
    int N, ldc, scales_stride, zeros_stride;
    int bytes_w, bytes_s, bytes_z;  // extents for the buffer descriptors (each < 2 GiB)
    int block_begin;         // first blockIdx.x of this linear
    int epilogue;            // TCE_W4_SILU_MUL_PAIRS / TCE_W4_ADD_TO_C bits of the descriptor
};

struct GemvArgs {
    const half_t *A;  // fp16 [M][lda]
    int lda, M, K, log2g;
    int nseg;
    unsigned long long *dbg;  // MODE 2 (timestamps) only
    int zeros_are_8;          // every linear of the launch carries TCE_W4_ZERO_POINT_IS_8
    const float *gamma;       // non-null: stage RMSNorm(A) * gamma instead of A (fused prologue, M = 1)
    float eps;
    GemvSeg seg[TCE_MAX_GROUP];
};

// (rows per wave, waves along N, waves splitting K, pipeline depth in steps) -- every tuple listed here is compiled
// for MB in {1,2,4}; tce_w4a16_set_gemv_config() can force any of them, the dispatcher picks by shape otherwise.
#define TCE_GEMV_VARIANTS(X) \
    X(1, 4, 1, 1)            \
    X(2, 4, 1, 1)            \
    X(4, 4, 1, 1)            \
    X(1, 4, 1, 2)            \
    X(2, 4, 1, 2)            \
    X(4, 4, 1, 2)            \
    X(2, 4, 1, 3)            \
    X(3, 4, 1, 1)            \
    X(3, 4, 1, 2)            \
    X(2, 8, 1, 2)            \
    X(4, 8, 1, 1)            \
    X(1, 2, 2, 1)            \
    X(2, 2, 2, 1)            \
    X(2, 2, 2, 2)            \
    X(1, 2, 4, 1)

bool gemv_variant_exists(int rows, int wn, int wk, int depth);

// persistent form, w4a16_gemv_stream.hip
// One GEMV launch (up to TCE_MAX_GROUP linears sharing the activation) as the persistent kernels read it.
struct StreamLaunch {
    const half_t *A;  // fp16 [K]
    int K, log2g;
    int nseg;
    int n_rg;                    // row groups over all linears of the launch
    GemvSeg seg[TCE_MAX_GROUP];  // block_begin = first row group of the linear
    const float *gamma;          // non-null: stage RMSNorm(A) * gamma instead of A (generalT5LayerNorm arithmetic)
    float eps;
    // tagged token plans only (w4a16_gemv_stream.hip): the activation as (tag << 16 | fp16 bits) words written by the launch of
    // the same plan that produces it (null: A comes from outside the plan, read at once), and where this launch's outputs go in
    // that form (per linear; null: nobody inside the plan reads them)
    const unsigned *A_tag;
    unsigned *C_tag[TCE_MAX_GROUP];
};
bool gemv_stream_supports(const tce_w4a16_desc *descs, int count);
int launch_w4a16_gemv_stream(const tce_w4a16_desc *descs, int count, hipStream_t stream, hipError_t *hip_err,
                             const float *gamma = nullptr, float eps = 0.f);
// token plans: a list of launches walked by ONE persistent kernel, the data flow between them ordered by tagged output words
struct TokenPlan;
// mode 0: the token kernel (one persistent kernel walks the list); mode 1: one kernel per launch on alternating graph branches, ordered
// by the same tagged words (w4a16_gemv_ovl.hip)
int token_plan_create(const tce_w4a16_desc *descs, const int32_t *groups, int n_launches, TokenPlan **out, hipError_t *hip_err, int mode = 0);
int token_plan_mode(const TokenPlan *tp);
// w4a16_gemv_ovl.hip: the per-launch kernel of overlapped plans
struct OvlGeom {
    int wn, xb, depth, rows_per_block, grid, per_cu;
    bool z8;
    size_t lds;
};
int ovl_chains();
int ovl_geometry(const tce_w4a16_desc *descs, int count, int cus, int chains, OvlGeom *g, hipError_t *hip_err);
hipError_t ovl_enqueue(const StreamLaunch *L, const OvlGeom &g, const unsigned *epoch, unsigned *status, int launch_index, hipStream_t stream);
int token_plan_enqueue(TokenPlan *tp, hipStream_t stream, hipError_t *hip_err);
int token_plan_status(TokenPlan *tp, unsigned *status, hipError_t *hip_err);
void token_plan_geometry(const TokenPlan *tp, int *rows, int *depth, int *waves, int *blocks);
void token_plan_destroy(TokenPlan *tp);
int launch_w4a16_gemv(const tce_w4a16_desc *descs, int count, int forced_rows, int forced_wn, int forced_wk,
                      int forced_depth, hipStream_t stream, hipError_t *hip_err, const float *gamma = nullptr, float eps = 0.f);

// w4a16_gemv_i8.hip: the decode GEMV (M <= 4) as an int8 contraction on the pre-packed copy
bool gemv_i8_supports(const tce_w4a16_desc *descs, int count, bool with_norm = false);
int gemv_i8_group_copy_members(const tce_w4a16_desc *descs, int count);  // > 0: the group is launched as ONE linear on its shared copy
int gemv_i8_rows_per_pass(int M, int K, int group_size);
struct I8ResidualNorm {  // tce_w4a16_forward_residual_rmsnorm: the RMSNorm that follows the residual add, produced by the same launch
    const float *gamma;
    float eps;
    void *xn_out;
    void *workspace;  // float [2048] + unsigned counter (zero between launches)
};
struct AttnDeferred;
int launch_w4a16_gemv_i8(const tce_w4a16_desc *descs, int count, hipStream_t stream, hipError_t *hip_err, const float *gamma = nullptr, float eps = 0.f, const I8ResidualNorm *rn = nullptr,
                         const AttnDeferred *comb = nullptr, const int *comb_pos_dev = nullptr, int comb_pos = 0);

// the mixed launch (round 6): up to TCE_MAX_INDEPENDENT decode linears with their own activations and K, one launch; bit-identical to the linears issued one by one
struct PeerGatherEpi;  // (below, with the communicator)
bool gemv_i8_mixed_supports(const tce_w4a16_desc *descs, int count);
void gemv_i8_mixed_geometry(const tce_w4a16_desc *descs, int count, int *waves, int *workgroups);
int launch_w4a16_gemv_i8_mixed(const tce_w4a16_desc *descs, int count, hipStream_t stream, hipError_t *hip_err, const PeerGatherEpi *gather = nullptr, int gathered = -1);
// w4a16_gemv_i8_token.hip (round 6): a prefix of a launch list as ONE persistent kernel on the int8-contraction body, the data flow ordered by tagged output words
struct I8TokenPlan;
int i8_token_plan_create(const tce_w4a16_desc *descs, const int32_t *groups, int n_launches, I8TokenPlan **out, int *n_taken, hipError_t *hip_err);
int i8_token_plan_enqueue(I8TokenPlan *tp, hipStream_t stream, hipError_t *hip_err);
int i8_token_plan_status(I8TokenPlan *tp, unsigned *status, hipError_t *hip_err);
int i8_token_plan_stages(const I8TokenPlan *tp);
int i8_token_plan_blocks(const I8TokenPlan *tp);
void i8_token_plan_destroy(I8TokenPlan *tp);

// MFMA GEMM on the q4_6 layout (prefill).  m_tiles x n_tiles 16x16 MFMA tiles per wave, 4 waves along N.
#define TCE_GEMM_VARIANTS(X) \
    X(8, 1)                  \
    X(8, 2)                  \
    X(4, 2)                  \
    X(4, 1)                  \
    X(2, 2)                  \
    X(4, 4)                  \
    X(2, 4)
bool gemm_variant_exists(int m_tiles, int n_tiles);
float gemm_dma_estimate_us(int M, int N, int K);
void gemm_dma_describe(int M, int N, bool g128, int *mt, int *nt, int *ks);  // the tile and form launch_w4a16_gemm_dma would pick  // the GEMM dispatcher's cost model (rounds x k-blocks x us per k-block)
// w4a16_gemm_dma.hip: same contract as launch_w4a16_gemm with an explicit tile; TCE_ERR_UNSUPPORTED_SHAPE when the shape
// (alignment, table size) does not fit, so the caller can fall back
int launch_w4a16_gemm_dma(const tce_w4a16_desc &d, int m_tiles, int n_tiles, hipStream_t stream, hipError_t *hip_err);  // tuning: XCD grid of xm x (8 / xm) over (row blocks x column blocks)
int launch_w4a16_gemm(const tce_w4a16_desc &d, int forced_mt, int forced_nt, hipStream_t stream, hipError_t *hip_err);

// w4a16_gemm_pk.hip: the 128-row GEMM on pre-packed weights (q4_mfma, w4a16_mfma_layout.hpp)
size_t prepack_bytes(int N, int K, int G);
int launch_w4a16_prepack(const tce_w4a16_desc &d, void *out, hipStream_t stream, hipError_t *hip_err, int tile0 = 0, int rows_total = 0);
// group copies (w4a16_mfma_layout.hpp): 0 bytes = the members cannot share a copy (N % 16, differing K / group size)
size_t prepack_group_bytes(const tce_w4a16_desc *descs, int count);
int launch_w4a16_prepack_group(const tce_w4a16_desc *descs, int count, void *out, hipStream_t stream, hipError_t *hip_err);
int launch_w4a16_gemm_pk(const tce_w4a16_desc &d, const void *packed, hipStream_t stream, hipError_t *hip_err);
float gemm_pk_estimate_us(int M, int N, int K, int *form_out, bool has_scratch = false, int *split_out = nullptr, int group_size = 128, bool zero_point_8 = false);
size_t gemm_pk_scratch_bytes();

int check_zero_point_8(const void *zeros, long long n_words, hipError_t *hip_err);
int check_zero_point_8_async(const void *zeros, long long n_words, int *verdict, hipStream_t stream, hipError_t *hip_err);  // one launch, no synchronisation: *verdict (host-mapped) = 1 / 2

// AWQ (q4_5) helpers
int launch_awq_fp16acc(int M, int N, int K, int G, const void *A, const void *qweight, const void *scales, void *C,
                       hipStream_t stream, hipError_t *hip_err);
int launch_awq_repack(int N, int K, int G, const void *qweight, const void *scales, void *workspace, hipStream_t stream,
                      hipError_t *hip_err);

// small batches, 2 <= M <= 16 (w4a16_skinny.hip)
bool skinny_supports(const tce_w4a16_desc &d);
int launch_w4a16_skinny(const tce_w4a16_desc &d, hipStream_t stream, hipError_t *hip_err);

// element-wise glue of the decoder layer (glue.hip)
int launch_layernorm_q(const float *x, const float *w, const float *b, void *out, int m, int n, hipStream_t stream, hipError_t *hip_err);
// w8a8_lnq_fused.hip
int launch_lnq_w8a8_group(const float *x, const float *ln_w, const float *ln_b, int m, int k, const tce_w8a8_desc *lin, int count, void *ln_out,
                          hipStream_t stream, hipError_t *hip_err);
int launch_opt_softmax_q(const float *scores, const float *mask, void *probs, int heads, int sq, int tgz, int ldp, hipStream_t stream, hipError_t *hip_err);
int launch_opt_kv_append(const void *k, const void *v, void *kc, void *vt, int heads, int hd, int sq, int pos, int max_keys, hipStream_t stream, hipError_t *hip_err);
int launch_rmsnorm_half(const void *x, const float *gamma, void *out, int m, int n, float eps, hipStream_t stream, hipError_t *hip_err);
// attention_ops.hip
int launch_bmm_f16t(const void *A, const void *B, void *C, int batch, int M, int N, int K, unsigned short alpha_bits, hipStream_t stream, hipError_t *hip_err);
int launch_attention_decode(const void *q, const void *K, const void *Vt, const void *mask, void *out, int heads, int t, int hd, unsigned short alpha_bits,
                            hipStream_t stream, hipError_t *hip_err);
// comm.hip
struct Comm;
int comm_create(int rank, int world, int max_vector_elems, int slots, Comm **out, hipError_t *he);
int comm_export(Comm *c, void *handle64, hipError_t *he);
int comm_connect_ipc(Comm *c, const void *handles, hipError_t *he);
int comm_connect_local(Comm *c, Comm *const *all, hipError_t *he);
int comm_set_timeout_ms(Comm *c, int ms);
int comm_reset(Comm *c, hipError_t *he);
int comm_device(const Comm *c);
int comm_status(Comm *c, hipError_t *he);
void comm_destroy(Comm *c);
int launch_allgather_f16(Comm *c, int slot, const void *src_slice, void *dst_full, int n_total, hipStream_t stream, hipError_t *he);
int comm_world_of(const Comm *c);
// the peer-write exchange of ONE linear's output slice inside the launch that computes it (w4a16_gemv_i8.hip, the mixed launch; round 6): what that kernel's epilogue
// needs of the communicator -- same window, buffers, flags and epochs as allgather_peer_kernel, so the two forms can alternate on one slot
constexpr int kCommMaxRanks = 8, kCommFlagStride = 16;  // the flag table of a window: [slots][2 parities][kCommMaxRanks] words, kCommFlagStride words apart (comm.hip)
struct PeerGatherEpi {
    unsigned char *peer[8];  // every rank's window as mapped here
    unsigned *epochs;        // [slots] exchanges completed per slot, the status word at [slots], the arrival counters at [slots + 1 + slot]
    void *dst;               // the complete vector on this rank
    int rank, world, slot, slots;
    unsigned slice_elems;    // halves per rank
    size_t vec_bytes, flags_off;
    unsigned long long timeout_ticks;
};
int comm_peer_gather_epi(Comm *c, int slot, void *dst_full, int n_total, PeerGatherEpi *out);  // the checks of launch_allgather_f16, no launch
int comm_rccl_unique_id(void *id128);
int comm_rccl_init(Comm *c, const void *id128);
bool comm_has_rccl(const Comm *c);
const char *comm_rccl_last_error();  // text of this thread's last failed RCCL call
bool comm_peer_regime(const Comm *c, int n_total);
int launch_allgather_rccl(Comm *c, const void *src_slice, void *dst_full, size_t n_per_rank, hipStream_t stream);
size_t allgather_rows_workspace_bytes(int M, int n_total);
int launch_allgather_rows_f16(Comm *c, int slot, const void *src, void *dst, int M, int n_total, int ldd, void *workspace, hipStream_t stream, hipError_t *he);
// attention_fast.hip
void describe_attention_decode_fast(int heads, int keys, int *chunk, int *chunks, int *waves, int kv_heads = 0);
size_t attention_decode_workspace_bytes(int heads, int max_keys, int hd);
// attention_prefill.hip: m > 1 new rows (rotation + append + causal / masked attention over pos + m keys), two launches
// opt_attention.hip: KV append + qk + mask / softmax / int8 + pv of the SmoothQuant OPT attention for m <= 8 new rows, one launch
int launch_opt_attention_decode(const void *q, const void *kn, const void *vn, void *kc, void *vtc, const float *mask, void *out, int heads, int hd, int m, int pos,
                                int max_keys, int ld, float a_qk, float a_pv, hipStream_t stream, hipError_t *hip_err);
size_t attention_prefill_workspace_bytes(int heads, int m, int hd);
int launch_attention_prefill(const void *qkv, int ld_qkv, void *kc, void *vc, const void *cosv, const void *sinv, const void *mask, int ld_mask, int causal,
                             void *out, int ld_out, void *workspace, int heads, int kv_heads, int max_keys, int pos, int m, float alpha, hipStream_t stream,
                             hipError_t *hip_err);
// ---- the paged family's arguments, from the C ABI (tce_capi.hip: the refusal rules) to the launchers ----
struct KvPages {  // the pools [num_pages][kv_heads][page_keys][hd] and the block table int32 [table_rows][table_stride] that names their pages
    void *k_pool, *v_pool;
    const int *table;
    int table_rows;  // the prefill's segments name their row (slot); 0: not checked -- the steps use rows 0 .. batch - 1, the copies see one row
    int table_stride, page_keys, num_pages;
    bool fp8;  // e4m3 bytes with one power-of-two exponent in [-8, 7] per pool (fp8_kv.hpp), else fp16
    int k_scale_log2, v_scale_log2;
};
struct AttnStepArgs {  // what every batched step (contiguous, paged, multi-row) and the paged prefill take besides the cache
    const void *qkv, *cosv, *sinv;
    void *out, *workspace;
    int batch, heads, kv_heads, hd;
    const int *pos_device;
    int pos_bound;
    unsigned short alpha_bits;
    int window = 0;  // the paged step and the paged prefill: >= 1 = sliding-window attention, a row at position p weighs keys max(0, p - window + 1) .. p; 0: every key
    int sinks = 0;   // with a window, 1 .. 16 = attention sinks: a row at p >= sinks + window also weighs keys 0 .. sinks - 1, scored with q rotated by row sinks + window - 1;
                     // a row below that weighs keys 0 .. p
};
struct PrefillRows {  // the paged prefill's rows: up to 16 segments {slot, pos, m, row0} (int32 x 4 each: tce_prefill_segment) of total_rows rows
    int ld_qkv, ld_out, causal;
    const int *segments;
    int nseg, total_rows;
};
struct KvLinear {  // a contiguous single-sequence cache pair fp16 [kv_heads][max_keys][hd]: the other side of the page copies
    void *k, *v;
    int kv_heads, max_keys;
};
// the paged prefill: both launches on the pools and block table; UNSUPPORTED_SHAPE: more query blocks than one launch lists (1024), or an exponent outside [-8, 7].
// describe: the form (4 / 8 / 14 / 18), pairing, query blocks and workgroups; no HIP call.
size_t attention_prefill_paged_workspace_bytes(int heads, int total_rows, int hd);
int describe_attention_prefill_paged(int heads, int causal, const int *segments, int nseg, int *form, int *pair, int *nblocks, int *workgroups, int window = 0, int sinks = 0);
int launch_attention_prefill_paged(const KvPages &pages, const AttnStepArgs &step, const PrefillRows &rows, hipStream_t stream, hipError_t *hip_err);
// what a deferred attention step leaves for its consumer (tce_attention_deferred of the C ABI, field for field)
struct AttnDeferred {
    int slots;   // chunk slots of the launch's grid: 1 = nothing deferred (`out` is final); 2 .. kAttnDeferMaxSlots = partial states per (query head, slot)
    int chunk;   // keys per chunk: slot i of a head is live when i * chunk < position + 1
    int heads;   // query heads
    int stride;  // floats per partial state: M, L, -, -, O[128]
    const float *part;
};
constexpr int kAttnDeferMaxSlots = 8;
int launch_attention_decode_fast(const void *qkv, void *kc, void *vc, const void *cosv, const void *sinv, const void *mask, void *out, void *workspace,
                                 int heads, int kv_heads, int hd, int max_keys, int pos, unsigned short alpha_bits, hipStream_t stream, hipError_t *hip_err,
                                 const int *pos_dev = nullptr, AttnDeferred *deferred = nullptr);
// the batched step: `batch` sequences in one launch, each with its own position word, cache slot, q/k/v and output rows and workspace slice
void describe_attention_decode_batch(int heads, int kv_heads, int pos_bound, int *chunk, int *chunks, int *waves);
size_t attention_decode_batch_workspace_bytes(int batch, int heads, int max_keys, int hd);
int launch_attention_decode_batch(const AttnStepArgs &step, void *kc, void *vc, int max_keys, hipStream_t stream, hipError_t *hip_err);
// the paged step: the batched step with the caches in pools of pages behind a block table int32 [batch][table_stride].  rows_per_seq 0: the step; 1 ..
// TCE_SPEC_MAX_ROWS: that many query rows per sequence.  Its companions: rows [key0, key0 + nkeys) of a contiguous pair <-> the pages of one table row (gather:
// pages -> contiguous; e4m3 pools: scatter quantises, gather dequantises), and the table check (*violations = count)
size_t kv_pages_pool_bytes(int num_pages, int kv_heads, int page_keys, int hd);
size_t kv_pages_pool_bytes_fp8(int num_pages, int kv_heads, int page_keys, int hd);
int launch_attention_decode_paged(const KvPages &pages, const AttnStepArgs &step, int rows_per_seq, hipStream_t stream, hipError_t *hip_err);
// the multi-row step with attention sinks (step.window >= rows_per_seq >= 1, step.sinks 1 .. 16): a unit of its own, attention_rows_sink.hip -- the one-row sink
// step's cut, the windowed rows step's grid, the multi-row step's workspace
int launch_attention_decode_paged_rows_sink(const KvPages &pages, const AttnStepArgs &step, int rows_per_seq, hipStream_t stream, hipError_t *hip_err);
int launch_kv_pages_copy(const KvPages &pages, const KvLinear &lin, bool gather, int key0, int nkeys, hipStream_t stream, hipError_t *hip_err);
int launch_kv_block_table_check(const KvPages &pages, int batch, const int *pos_dev, int pos_bound, unsigned *violations, hipStream_t stream, hipError_t *hip_err,
                                int window = 0, int sinks = 0);  // window >= 1: only the words a windowed row follows; sinks >= 1: a sink row
// the sink step's cut (AttnStepArgs::sinks >= 1): the batched rule for the virtual keys a workgroup group can span (attention_fast.hip)
int attention_sink_cut_keys(int pos_bound, int window, int sinks);
void describe_attention_decode_sink(int heads, int kv_heads, int pos_bound, int window, int sinks, int *chunk, int *chunks, int *waves);
// the windowed paged step's cut (AttnStepArgs::window >= 1): the batched rule for min(pos_bound + 1, window + 3) keys
void describe_attention_decode_window(int heads, int kv_heads, int pos_bound, int window, int *chunk, int *chunks, int *waves);
int launch_rope_half(void *q, void *k, const void *cosv, const void *sinv, int heads, int len, int hd, int start_idx, hipStream_t stream, hipError_t *hip_err);
int launch_softmax_half(const void *x, void *out, long long rows, int n, hipStream_t stream, hipError_t *hip_err);
int launch_prefetch(const void *ptr, long long bytes, int workgroups, hipStream_t stream, hipError_t *hip_err);
int launch_add_half(const void *a, const void *b, void *c, long long n, hipStream_t stream, hipError_t *hip_err);
int launch_silu_mul_half(void *a, const void *b, long long n, hipStream_t stream, hipError_t *hip_err);

}  // namespace tce
