/*
 * tce_matmul.h -- C ABI of libtce_hip.so: the MI355X (gfx950 / CDNA4) implementation of
 * TinyChatEngine's quantized-matmul hot path (reference: kernels/matmul.h @ 2024_08_07).
 *
 * This is the drop-in boundary.  Every entry point takes plain pointers and sizes (no C++
 * or torch types), is ASYNCHRONOUS (returns after enqueueing on `stream`; NULL = the HIP
 * null stream, which is what the reference uses -- kernels/cuda/gemv_cuda.cu:237), never
 * allocates, frees or retains caller memory, and returns 0 or a negative TCE_ERR_* code
 * (it never throws or exits; the C++ adapter in tinychatengine_amd/adapter/ maps failures to
 * the reference's printf+exit(1) behaviour -- kernels/cuda/gemv_cuda.cu:254-256).
 *
 * All data pointers must be device-accessible (hipMalloc or hipMallocManaged memory).
 *
 * Which reference symbol each entry point replaces:
 *
 *   tce_w4a16_forward          <- matmul::MatmulOperator::gemv_forward_cuda
 *                                 (kernels/cuda/gemv_cuda.cu:213-260; kernels gemv_kernel_g128 :140-194,
 *                                  gemv_kernel_g64 :68-123).  Serves every M like the reference does
 *                                 (grid.z = M there); here M <= 2 runs the bandwidth-bound GEMV kernels,
 *                                 3 <= M <= 16 (group 128) the small-batch kernel that streams the weights once for
 *                                 all rows -- also 17 <= M <= 128 in 16-row slices while N is too small to fill the
 *                                 chip with GEMM tiles --, larger M the MFMA GEMM kernels (groups of 128, and from
 *                                 M = 17 also 64 and 32 when K % 128 == 0); smaller M with another group size stays
 *                                 on the GEMV kernels.
 *   tce_w4a16_forward_group    <- several gemv_forward_cuda calls that read the same activation
 *                                 (fused q/k/v: llm/src/nn_modules/cuda/Int4llamaAttention.cu:125;
 *                                  gate+up: Int4llamaDecoderLayer.cu:96-99) issued as ONE launch.
 *   tce_w4a16_awq_fp16acc      <- MatmulOperator::naive_mat_mul_fp16_int4 (kernels/cuda/matmul_int4.cu:8-48)
 *   tce_w4a16_gemm_awq         <- MatmulOperator::gemm_forward_cuda* (declared kernels/matmul.h:140-145,
 *                                 never defined in the reference; AWQ q4_5 layout, fp32 accumulate here)
 *   tce_w8a8_matmul            <- the eight int8 methods of kernels/ref/matmul_ref_int8.cc:161-192
 *                                 (int8_ref_matmul{,_nobias,_nobias_batch,_bfp32_ofp32,_nobias_ofp32,
 *                                  _nobias_ofp32_batch}), selected by the descriptor's bias/out kinds.
 *   tce_plan_*                 <- the host loop that issues one decode token's linears
 *                                 (llm/src/nn_modules/cuda/Int4llamaDecoder.cu:84-103) captured once into a
 *                                 hipGraph and replayed; new on MI355X (launch latency ~ kernel time).
 */
#ifndef TCE_MATMUL_H
#define TCE_MATMUL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCE_API __attribute__((visibility("default")))

#define TCE_VERSION 113 /* additive, unversioned: tce_lora_shrink_f16, tce_lora_expand_add_f16 (per-row fp16 LoRA adapters beside a W4A16 linear: the rows of one launch pick their adapter by a word on the device), tce_lora_expand_silu_mul_f16 (the gate/up form: the delta in front of SiLU * mul); tce_w4a16_prepack_group_bytes, tce_w4a16_prepack_group (one packed copy for linears that are always launched together; a member's descriptor names the copy, its first tile and the copy's rows in `prepacked`, `reserved`, `reserved2` -- fields that were zero before, and zero still means an individual copy.  BEHAVIOUR CHANGE under the unchanged number: the two reserved fields are now READ, so a caller that left them uninitialised -- non-zero, with no packed copy or not describing N rows of one -- gets TCE_ERR_BAD_ARG from every W4A16 entry point where it ran before; zero them); tce_sample_workspace_bytes, tce_sample_f16, tce_embed_rows_f16 (device-side sampling and the embedding lookup: one graph replay is one token); tce_kv_pages_pool_bytes, tce_attention_decode_step_paged_f16, tce_attention_decode_describe_paged, tce_kv_pages_scatter_f16, tce_kv_pages_gather_f16, tce_kv_block_table_check (the batched step on a paged KV cache); tce_attention_decode_batch_workspace_bytes, tce_attention_decode_describe_batch, tce_attention_decode_step_batch_f16 (B sequences per attention launch); 0.1.13: tce_w8a8_describe_dispatch; 0.1.12: tce_w4a16_forward_independent (up to TCE_MAX_INDEPENDENT decode linears with their own activations and K as one launch: the sharded block); 0.1.11: tce_w4a16_gemm_scratch_faults (a k-cut exchange that gives up stores NaN and poisons its counter: loud, sticky), TCE_PLAN_TAGGED on packed copies runs the int8-contraction token kernel (tce_plan_is_chained = 4), TCE_DESC_V2_MAX_BYTES; 0.1.10: tce_attention_decode_step_deferred_f16 + tce_w4a16_forward_deferred_attention (the attention combine in o_proj's prologue); size-prefixed descriptors (tce_w4a16_desc_v2 / tce_w8a8_desc_v2 + the *_v2 entry points; the plain ones stay), TCE_ERR_RCCL, the tuning setters act on the CALLING THREAD only; 0.1.9: tce_w4a16_check_zero_point_8_async, tce_host_alloc / tce_host_free (the adapter no longer synchronises); 0.1.8: per-family tuning setters (tce_attention_set_tuning, tce_w8a8_set_tuning); 0.1.7: decode on the pre-packed copy (int8 contraction), tce_w4a16_set_gemv_i8; 0.1.6: TCE_PLAN_TUNED; 0.1.5: tce_opt_attention_decode; 0.1.4: tce_attention_prefill_f16 (0.1.3: tce_attention_decode_step_gqa_f16, TCE_PLAN_OVERLAPPED; 0.1.2: tce_w4a16_desc.scratch; 0.1.1: .prepacked, tce_w4a16_prepack*) */

/* error codes (return values) */
#define TCE_OK 0
#define TCE_ERR_BAD_ARG (-1)           /* null pointer / non-positive size */
#define TCE_ERR_UNSUPPORTED_GROUP (-2) /* group size not in {32,64,128}: reference prints "Unsupported group size" and exits */
#define TCE_ERR_UNSUPPORTED_SHAPE (-3) /* K % 32 != 0, N % 8 != 0 for the AWQ layout, ... */
#define TCE_ERR_HIP (-4)               /* a HIP runtime call failed; see tce_last_error() */
#define TCE_ERR_UNSUPPORTED_KIND (-5)  /* bias/out kind combination that has no reference counterpart */
#define TCE_ERR_RCCL (-6)              /* an RCCL call failed (ncclAllGather ...): tce_last_error() carries ncclGetErrorString's text -- NOT a HIP error */

/* M at or below which tce_w4a16_forward never uses the prefill GEMM (GEMV or small-batch kernels) */
#define TCE_W4A16_GEMV_MAX_M 8

/*
 * W4A16 on the reference's q4_6 ("CUDA GEMV") layout -- llm/tools/quantize_methods.py:370-442:
 *   A        fp16  [M][lda]           activations, row-major           (matmul_params.A.half_data_ptr)
 *   qweight  u32   [N][K/8]           nibble i of word j = code[n][8j+i] (matmul_params.B.int32_data_ptr)
 *   scales   fp16  [N][scales_stride] first K/G entries valid           (matmul_params.half_scales)
 *   zeros    u32   [N][zeros_stride]  nibble g%8 of word g/8            (matmul_params.int32_zero_point)
 *   C        fp16  [M][ldc]                                            (matmul_params.C.half_data_ptr)
 *   C[m][n] = fp16( sum_k fp32(s[n][k/G]) * (q[n][k] - z[n][k/G]) * fp32(A[m][k]) ), fp32 accumulate.
 * Strides of 0 select the reference's defaults: lda = K, ldc = N,
 * zeros_stride = calculate_zeros_width(K,G) (llm/src/nn_modules/cuda/utils.cu:162-178), scales_stride = 8x that.
 * Like the reference, B.row / B.column are NOT part of the contract (gemv_cuda.cu:217-221 ignores them).
 */
typedef struct tce_w4a16_desc {
    int32_t M, N, K;
    int32_t group_size; /* QK: 128 (reference CUDA default, llm/include/common.h:18), 64 or 32 */
    const void *A;
    const void *qweight;
    const void *scales;
    const void *zeros;
    void *C;
    int32_t lda, ldc;                     /* elements; 0 = dense */
    int32_t scales_stride, zeros_stride;  /* elements / words; 0 = reference default */
    int32_t flags;                        /* TCE_W4_* */
    int32_t reserved;                     /* 0, or -- a member of a group copy (tce_w4a16_prepack_group) -- its first 16-row tile inside the copy */
    const void *rmsnorm_gamma;            /* NULL = none.  fp32 [K]: A is the UN-normalised hidden state and the kernel stages
                                             RMSNorm(A) * gamma (generalT5LayerNorm arithmetic, see tce_rmsnorm_half); M = 1 */
    float rmsnorm_eps;
    int32_t reserved2;                    /* 0 = `prepacked` is this linear's own copy; > 0: `prepacked` is a group copy of this many rows */
    const void *prepacked;                /* NULL = none.  The q4_mfma copy of this linear's weights built by tce_w4a16_prepack
                                             (same N, K, group size): the prefill GEMM for large M AND the decode kernel for M <= 4
                                             (round 4: csrc/w4a16_gemv_i8.hip) read it instead of qweight / scales / zeros (which must
                                             still be valid: every other M, and the fused RMSNorm prologue, use them) */
    void *scratch;                        /* NULL = none.  tce_w4a16_gemm_scratch_bytes() bytes of device memory, 256-byte aligned, its first 4096
                                             bytes ZEROED once by the caller (every call leaves them zero): lets the pre-packed GEMM cut the k range of
                                             a launch with few tiles (M = 512 at N = 4096 is 128 tiles for 256 CUs) across workgroups
                                             and add the partial tiles in a fixed order.  One scratch area per stream that runs such
                                             calls concurrently; calls on one stream may share it.  (0.1.10: a range cut in TWO runs is a
                                             directed hand-off -- run 1 waits, for a bounded number of polls, for the tile of run 0, which is
                                             dispatched before it on the same XCD's queue.  A wait that runs out -- never seen -- is LOUD since
                                             0.1.11: the tile is stored as NaN, the tile's counter word is poisoned so that every later call
                                             meeting it stores NaN too, and the last word of the first 4096 bytes counts the faults:
                                             tce_w4a16_gemm_scratch_faults() reads it; zeroing the first 4096 bytes recovers the area.) */
} tce_w4a16_desc;

/* flags */
#define TCE_W4_FORCE_GEMV 1  /* use the GEMV kernel even when M > TCE_W4A16_GEMV_MAX_M (weights re-streamed per 4 rows) */
#define TCE_W4_FORCE_GEMM 2  /* use the MFMA GEMM kernel even for small M */
#define TCE_W4_ZERO_POINT_IS_8 4 /* the caller vouches that every 4-bit zero point of this linear is 8 (`zeros` all
                                    0x88888888 -- what the reference quantizer always writes, quantize_methods.py:436-440):
                                    the GEMV then does not stream the zeros.  Results are identical when the promise holds. */

/* Fused decode epilogues: the element-wise kernels the reference launches right behind these linears,
 * with the same fp16 arithmetic, applied while the result is still in registers.
 *   TCE_W4_SILU_MUL_PAIRS  replaces gate_proj + up_proj + SiLuMul_half (Int4llamaDecoderLayer.cu:20-30, 96-102): the
 *       linear holds the two projections' rows INTERLEAVED (row 2n = gate row n, row 2n+1 = up row n; a load-time row
 *       permutation, like the reference's offline qkv merge), N is even, and
 *           C[m][n] = hmul( hmul(g, hdiv(1, hadd(1, hexp(hneg(g))))), u ),  g = fp16(y[m][2n]), u = fp16(y[m][2n+1])
 *       with every operation rounded to fp16 as in the reference kernel.  C is [M][N/2] (ldc 0 = N/2).  Decode batches (M <= 8) run it in the GEMV
 *       kernels' epilogue; a batch of M > 128 rows with a `prepacked` copy in the 128-row GEMM's (the prompt path); anything else on the GEMV kernel,
 *       four rows per pass.
 *   TCE_W4_ADD_TO_C        replaces o_proj / down_proj + add_half (Int4llamaDecoderLayer.cu:12-18, 86-88, 107-108):
 *           C[m][n] = hadd(C[m][n], fp16(y[m][n]))   (C holds the residual on entry, like residual_add there). */
#define TCE_W4_SILU_MUL_PAIRS 8
#define TCE_W4_ADD_TO_C 16

TCE_API int tce_w4a16_forward(const tce_w4a16_desc *d, void *stream);

/* Size-prefixed form (0.1.10): a host compiled against THIS header keeps working when a later library appends fields to the descriptor, and a later host talks to
 * this library as long as it leaves the fields this library does not know at zero.  `struct_size` = sizeof(tce_w4a16_desc_v2) as the CALLER compiled it; the library
 * copies min(struct_size, its own size) bytes into a zeroed descriptor of its own and refuses a size below the 0.1.10 layout (TCE_ERR_BAD_ARG) or non-zero bytes
 * beyond what it knows.  `struct_size` above TCE_DESC_V2_MAX_BYTES (an uninitialised descriptor) and a non-zero `reserved0` are refused too (TCE_ERR_BAD_ARG).
 * Same semantics as tce_w4a16_forward(&v2->desc, stream). */
#define TCE_DESC_V2_MAX_BYTES 4096
typedef struct tce_w4a16_desc_v2 {
    uint32_t struct_size;
    uint32_t reserved0;
    tce_w4a16_desc desc;
    /* fields of later versions are appended here */
} tce_w4a16_desc_v2;
TCE_API int tce_w4a16_forward_v2(const tce_w4a16_desc_v2 *d, void *stream);

/* Round 4: o_proj / down_proj + residual add + the RMSNorm that FOLLOWS, one launch (decode, M = 1) -- replaces `linear; add_half; LlamaRMSNorm` of
 * Int4llamaDecoderLayer.cu:86-99 (post_attention_layernorm) and :107-108 + :78 of the next layer (input_layernorm):
 *   C[n]  = hadd(C[n], fp16(y[n]))                                           as TCE_W4_ADD_TO_C (which `d` must carry; C is the whole residual row: ldc 0 or N)
 *   xn[n] = half( clamp( (float(C[n]) * rs) * gamma[n] ) ),  rs = 1 / sqrt(mean_n C[n]^2 + eps)   generalT5LayerNorm on the UPDATED row: the bits of tce_rmsnorm_half
 * so that the next linears (q/k/v, gate/up) are plain launches on xn instead of carrying the prologue -- which every one of their workgroups repeats.  Every workgroup
 * writes its 16 values and their sums of squares through to memory and counts itself in; the one that arrives last normalises the row.  Needs `d->prepacked` (the
 * int8-contraction kernel), group 128, N % 8 == 0, N <= 16384.  `workspace`: tce_w4a16_residual_rmsnorm_workspace_bytes() bytes, 16-byte aligned, ZEROED once by the
 * caller (every launch leaves its counter zero); one per stream that runs such launches concurrently.
 * Measured (round 4): bit-exact and SLOWER than what it replaces on this part -- +3.8 us per launch (write-through acknowledgements, the last workgroup's
 * serial pass) against the +1.7 / +5.5 us the fused prologues cost q/k/v and gate/up: a whole token 1.65 against 1.41 ms.  Offered for hosts that must count launches. */
TCE_API size_t tce_w4a16_residual_rmsnorm_workspace_bytes(void);
TCE_API int tce_w4a16_forward_residual_rmsnorm(const tce_w4a16_desc *d, const float *gamma, float eps, void *xn_out, void *workspace, void *stream);

/* The same two element-wise operations as stand-alone kernels (for hosts that keep the reference's launch structure):
 *   tce_add_half:       c[i] = hadd(a[i], b[i])                                   (add_half, Int4llamaDecoderLayer.cu:12-18)
 *   tce_silu_mul_half:  a[i] = hmul(hmul(a[i], hdiv(1, hadd(1, hexp(-a[i])))), b[i])  (SiLuMul_half, :20-30)
 * n halves; pointers 16-byte aligned; c may alias a or b. */
/* The two fp16 operators between the q/k/v and the o linears of the reference's Llama attention, with its
 * arithmetic (see csrc/attention_ops.hip):
 *   tce_bmm_f16t     <- BMM_F16T::forward / mat_mul_transposed_cuda (llm/src/ops/cuda/BMM_F16T.cu:28-76):
 *                       A fp16 [batch][M][K], B fp16 [batch][N][K], C fp16 [batch][M][N];
 *                       C = hmul(alpha, acc), acc = hfma(A[i][k], B[j][k], acc) for k ascending (binary16 accumulation);
 *                       alpha as binary16 bits (what alpha_half.bin holds)
 *   tce_softmax_half <- softmax_cuda (llm/src/ops/cuda/softmax.cu:4-40): rows of n binary16 values */
TCE_API int tce_bmm_f16t(const void *A, const void *B, void *C, int batch, int M, int N, int K, unsigned short alpha_half_bits, void *stream);
TCE_API int tce_softmax_half(const void *x, void *out, long long rows, int n, void *stream);
/* RotaryPosEmb_cuda_forward (llm/src/ops/cuda/RotaryPosEmb.cu:4-34), in place on q and / or k fp16 [heads][len][head_dim] (NULL skips one);
 * cos / sin tables fp16 [positions][head_dim]; row i uses position i + start_idx:  x'[j] = hfma(x[j], cos[j], hmul(rot[j], sin[j])),
 * rot = (-x[head_dim/2:], x[:head_dim/2]). */
TCE_API int tce_rope_half(void *q, void *k, const void *cos_table, const void *sin_table, int heads, int len, int head_dim, int start_idx, void *stream);
/* One decode step (one query row per head) of Int4llamaAttention's qk_bmm -> batch_Add(mask) -> check_inf_half -> softmax ->
 * pv_bmm (llm/src/nn_modules/cuda/Int4llamaAttention.cu:184-211) as ONE launch, every operation and every order kept (bit-identical
 * to tce_bmm_f16t + hadd + tce_softmax_half + tce_bmm_f16t): q fp16 [heads][head_dim], K [heads][keys][head_dim],
 * Vt [heads][head_dim][keys] (the transposed values the reference also keeps), mask fp16 [keys] or NULL, out [heads][head_dim]. */
TCE_API int tce_attention_decode_f16(const void *q, const void *K, const void *Vt, const void *mask, void *out, int heads, int keys, int head_dim,
                                     unsigned short alpha_half_bits, void *stream);
/* One decode step of the reference's Llama attention block between the fused q/k/v linear and o_proj as ONE bandwidth-bound launch
 * (csrc/attention_fast.hip): replaces shape_qkv, RotaryPosEmb_cuda_forward, the KV append, qk_bmm, batch_Add, check_inf_half, softmax,
 * transpose_1_2idx, pv_bmm and unshape (llm/src/nn_modules/cuda/Int4llamaAttention.cu:130-217).
 *   qkv        fp16 [3][heads][head_dim]   the fused projection's output row (q | k | v, head-major: what qkv_proj.forward writes)
 *   k_cache, v_cache  fp16 [heads][max_keys][head_dim]   fixed-capacity caches; rows [0, pos) hold the past, row `pos` is WRITTEN by this
 *              call (the rotated key -- bit-identical to what the reference appends -- and the value)
 *   cos_table / sin_table  fp16 [positions][head_dim] (RotaryPosEmb's tables) or both NULL: no rotation
 *   mask       fp16 [pos + 1] additive, or NULL;  alpha as binary16 bits;  out fp16 [heads][head_dim] (= o_proj's input row)
 *   workspace  tce_attention_decode_workspace_bytes(heads, max_keys, head_dim) bytes, ZEROED once by the caller before the first use
 * Scores, softmax and the weighted sum run in fp32 over key chunks spread across the chip (the bit-exact binary16-chain form of the
 * same block is tce_attention_decode_f16): results agree with that form within 2e-3 * max|out| per head.  head_dim == 128. */
TCE_API size_t tce_attention_decode_workspace_bytes(int heads, int max_keys, int head_dim);
/* How tce_attention_decode_step_f16 would cut a context of `keys` keys (= pos + 1), as text: "chunks=C keys-per-chunk=K waves=W workgroups=G
 * combine=yes|no" -- one chunk per head and no combine up to 320 keys, four chunks up to 1024, then eight chunks of at most 512 keys.
 * Launches nothing, makes no HIP call. */
TCE_API int tce_attention_decode_describe(int heads, int keys, char *buf, int buf_len);
TCE_API int tce_attention_decode_step_f16(const void *qkv, void *k_cache, void *v_cache, const void *cos_table, const void *sin_table, const void *mask,
                                          void *out, void *workspace, int heads, int head_dim, int max_keys, int pos, unsigned short alpha_half_bits,
                                          void *stream);
/* The same step for grouped-query attention (Llama-3-8B: 32 query heads over 8 key / value heads, llm/include/model.h:83): query head i reads
 * key / value head i / (heads / kv_heads), the reference's `repeat` (llm/src/nn_modules/non_cuda/Int4llamaAttention.cc:166-185) without the copy.
 *   qkv  fp16 [heads + 2 * kv_heads][head_dim]: the query heads, then the key heads, then the value heads (the fused projection's row)
 *   k_cache, v_cache  fp16 [kv_heads][max_keys][head_dim];  out fp16 [heads][head_dim]
 *   workspace  tce_attention_decode_workspace_bytes(heads, max_keys, head_dim) bytes, zeroed once
 * Any heads % kv_heads == 0 (kv_heads == heads is tce_attention_decode_step_f16).  A workgroup owns (query head, chunk of keys) and the
 * heads / kv_heads workgroups of a key / value head read the same cache rows (from HBM once; the fused form -- one workgroup streaming a
 * chunk once for 2 or 4 query heads -- exists behind tce_w4a16_set_debug_mode(2922 / 2924) and measured slower, see csrc/attention_fast.hip).  Rows of the caches at and beyond `pos` may hold anything on entry (uninitialised
 * memory included): they are never weighted into the result. */
TCE_API int tce_attention_decode_step_gqa_f16(const void *qkv, void *k_cache, void *v_cache, const void *cos_table, const void *sin_table, const void *mask,
                                              void *out, void *workspace, int heads, int kv_heads, int head_dim, int max_keys, int pos,
                                              unsigned short alpha_half_bits, void *stream);
TCE_API int tce_attention_decode_describe_gqa(int heads, int kv_heads, int keys, char *buf, int buf_len);
/* The same step with the position read ON THE DEVICE: `pos_device` (int32, device memory) holds the token's position when the kernel runs, `pos_bound` >= every
 * value it will hold while this launch is replayed (the grid and the chunk length are cut for pos_bound; workgroups of chunks past the actual context leave at
 * once).  A launch captured into a hipGraph is then replayable token after token -- the host (or a one-thread kernel in the same graph) advances the word -- where
 * the by-value entry points bake the position into the graph node.  pos_device == NULL: pos_bound is the position (the by-value form).  `mask`, if given, must
 * cover pos_bound + 1 keys. */
TCE_API int tce_attention_decode_step_pos_f16(const void *qkv, void *k_cache, void *v_cache, const void *cos_table, const void *sin_table, const void *mask,
                                              void *out, void *workspace, int heads, int kv_heads, int head_dim, int max_keys, const int32_t *pos_device,
                                              int pos_bound, unsigned short alpha_half_bits, void *stream);
/* The same step for `batch` independent sequences in ONE launch (grid: query heads x chunk slots, batch).  Sequence b has
 *   qkv        fp16 [batch][heads + 2 * kv_heads][head_dim]: row b is sequence b's fused projection row (what tce_w4a16_forward writes for M = batch)
 *   k_cache, v_cache  fp16 [batch][kv_heads][max_keys][head_dim]: slot b is exactly a single-sequence cache
 *   out        fp16 [batch][heads][head_dim]: row b is o_proj's input row b
 *   pos_device int32 [batch], device memory: sequence b's position, read by the kernel (a captured launch is replayable token after token)
 *   workspace  tce_attention_decode_batch_workspace_bytes(batch, heads, max_keys, head_dim) bytes -- `batch` single-step workspaces back to back --, zeroed once
 * The RoPE tables (both or neither; row pos_device[b] for sequence b) and alpha are shared.  The cut is the fitted rule of the single step for pos_bound + 1 keys,
 * one query head per workgroup, whatever the calling thread's attention tuning settings: every active row's `out` and appended cache rows are BIT-IDENTICAL to
 * tce_attention_decode_step_pos_f16 on slot b with pos_device + b and the same pos_bound.  A row whose position is < 0 or > pos_bound is inactive: its `out` row is
 * written with zeros (o_proj then adds exactly 0 to its residual) and its caches and workspace slice are not touched -- a fixed-batch captured graph is a slot pool,
 * and a finished sequence is retired by writing -1.  No mask.  head_dim == 128, batch <= 65535, pointers 16-byte aligned.  New; the reference decodes one sequence.
 * tce_attention_decode_batch_workspace_bytes returns 0 for an unsupported shape (head_dim != 128, batch <= 0).  tce_attention_decode_describe_batch is
 * tce_attention_decode_describe_gqa(heads, kv_heads, pos_bound + 1) for the untuned rule with " batch=B" appended and workgroups B times the single step's; it makes no
 * HIP call. */
TCE_API size_t tce_attention_decode_batch_workspace_bytes(int batch, int heads, int max_keys, int head_dim);
TCE_API int tce_attention_decode_describe_batch(int batch, int heads, int kv_heads, int pos_bound, char *buf, int buf_len);
TCE_API int tce_attention_decode_step_batch_f16(const void *qkv, void *k_cache, void *v_cache, const void *cos_table, const void *sin_table,
                                                void *out, void *workspace, int batch, int heads, int kv_heads, int head_dim, int max_keys,
                                                const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, void *stream);

/* The batched step on a PAGED cache: keys and values live in fixed-size pages drawn from one pool, a per-sequence block table maps logical key index to page.
 *   k_pool, v_pool  fp16 [num_pages][kv_heads][page_keys][head_dim] each; page_keys a power of two from 16 to 256; one page number addresses both pools
 *   block_table     int32 [batch][table_stride], device memory, read when the kernel runs: logical key j of sequence b, key / value head h is row j % page_keys of
 *                   page p = block_table[b][j / page_keys], at element ((p * kv_heads + h) * page_keys + j % page_keys) * head_dim of either pool
 *   workspace       tce_attention_decode_batch_workspace_bytes(batch, heads, table_stride * page_keys, head_dim) bytes, zeroed once (the batched step's layout)
 * Everything else is tce_attention_decode_step_batch_f16: the grid, the untuned fitted cut for pos_bound + 1 keys, one query head per workgroup, pos_device, inactive
 * rows (position < 0 or > pos_bound: a zero `out` row, nothing else of theirs written), the new key / value rows appended -- to the page that holds index pos.  Every
 * active row's `out` and appended rows are BIT-IDENTICAL to the batched step on contiguous caches with the same contents; the arithmetic is the same instructions.
 * TRUST: for an active row only words 0 .. pos / page_keys of its table row become addresses (rows read past the range and not weighted stay inside those pages);
 * words beyond them and every word of an inactive row may hold anything.  The step does NOT validate page numbers -- a word it follows must lie in [0, num_pages) --;
 * tce_kv_block_table_check is the check to run first where a table is not known to be sound.  pos_bound < table_stride * page_keys.
 * tce_kv_pages_pool_bytes: the bytes of ONE pool, 0 for an unsupported shape (head_dim != 128, page_keys outside the rule, a count <= 0).
 * tce_attention_decode_describe_paged: tce_attention_decode_describe_batch's text with " page-keys=P" appended; no HIP call.
 * tce_kv_pages_scatter_f16: rows [key0, key0 + nkeys) of every head of a contiguous single-sequence pair [kv_heads][src_max_keys][head_dim] (what
 * tce_attention_prefill_f16 and the single steps write) into the pages ONE table row names (`table_row` = block_table + b * table_stride); tce_kv_pages_gather_f16 is
 * the reverse.  One launch of 16-byte copies each; key0 and nkeys need not be page-aligned; no other row of either side is written; a table word outside
 * [0, num_pages) copies nothing.  Admission: prefill on a contiguous staging pair (after a gather, on top of cached keys), then scatter the new rows.
 * tce_kv_block_table_check (asynchronous, one small launch): *violations (a device-visible word) = the number of words an active row (0 <= pos_device[b] <= pos_bound)
 * would follow -- 0 .. pos / page_keys -- that lie outside [0, num_pages), plus the active rows with pos / page_keys >= table_stride.  Words past the needed range and
 * inactive rows are not looked at.  The word is written, not accumulated. */
TCE_API size_t tce_kv_pages_pool_bytes(int num_pages, int kv_heads, int page_keys, int head_dim);
TCE_API int tce_attention_decode_describe_paged(int batch, int heads, int kv_heads, int pos_bound, int page_keys, char *buf, int buf_len);
TCE_API int tce_attention_decode_step_paged_f16(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int heads, int kv_heads,
                                                int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, void *stream);
TCE_API int tce_kv_pages_scatter_f16(const void *k_src, const void *v_src, void *k_pool, void *v_pool, const int32_t *table_row, int table_stride, int page_keys,
                                     int num_pages, int kv_heads, int head_dim, int src_max_keys, int key0, int nkeys, void *stream);
TCE_API int tce_kv_pages_gather_f16(const void *k_pool, const void *v_pool, void *k_dst, void *v_dst, const int32_t *table_row, int table_stride, int page_keys,
                                    int num_pages, int kv_heads, int head_dim, int dst_max_keys, int key0, int nkeys, void *stream);
TCE_API int tce_kv_block_table_check(const int32_t *block_table, int table_stride, int page_keys, int num_pages, int batch, const int32_t *pos_device, int pos_bound,
                                     uint32_t *violations, void *stream);

/* Round 5: the attention step WITHOUT its cross-workgroup combine, and the linear that consumes it (o_proj) doing the combine in its prologue.
 * A decode step over more than ~320 keys cuts every head's keys into 4 or 8 chunks; each chunk's workgroup ends with a partial online-softmax state (M, L, O[128]) and
 * the LAST one to arrive combines them -- acknowledged write-through stores, a counter, coherent re-reads: 2.3 - 3.2 us of a 7 - 10 us launch.
 * tce_attention_decode_step_deferred_f16 is tce_attention_decode_step_pos_f16 that stops at plain stores of the partial states and describes them in *info;
 * tce_w4a16_forward_deferred_attention is tce_w4a16_forward for the linear that reads the step's output row (d->A = the step's `out`; M = 1, d->prepacked, groups of
 * 128, K = heads * 128 a multiple of 1024, no RMSNorm prologue; TCE_W4_ADD_TO_C allowed): every workgroup forms the row from the partial states with the operations, and in
 * the order, of the step's own combine and rounds it to binary16 -- the SAME row, bit for bit -- while its weights are in flight.  The kernel boundary between the two launches
 * is the only ordering needed.  info->slots == 1 (a short context, or a cut beyond 8 slots): nothing was deferred, `out` is final, and the second call is the plain
 * tce_w4a16_forward.  With the position on the device the number of LIVE slots is recomputed by the consumer from the same word (when one is live the step wrote `out`
 * itself).  Both calls must see the same pos_device / pos_bound.  `workspace` as for the other entry points (tce_attention_decode_workspace_bytes). */
typedef struct tce_attention_deferred {
    int32_t slots;   /* chunk slots per query head: 1 = nothing deferred */
    int32_t chunk;   /* keys per chunk */
    int32_t heads;   /* query heads */
    int32_t stride;  /* floats per partial state: M, L, two unused, O[128] */
    const float *part; /* [heads][slots][stride], inside `workspace` */
} tce_attention_deferred;
TCE_API int tce_attention_decode_step_deferred_f16(const void *qkv, void *k_cache, void *v_cache, const void *cos_table, const void *sin_table, const void *mask,
                                                   void *out, void *workspace, int heads, int kv_heads, int head_dim, int max_keys, const int32_t *pos_device, int pos_bound,
                                                   unsigned short alpha_half_bits, tce_attention_deferred *info, void *stream);
TCE_API int tce_w4a16_forward_deferred_attention(const tce_w4a16_desc *d, const tce_attention_deferred *info, const int32_t *pos_device, int pos_bound, void *stream);
/* The same block for m > 1 NEW rows -- a prompt, or a chunk of one on top of pos cached keys (Int4llamaAttention.cu:116-229 with sqlen > 1) -- as two
 * launches (csrc/attention_prefill.hip): rotation of q and the new keys with the reference's binary16 arithmetic + the KV append (rows pos .. pos + m - 1;
 * bit-identical to what m decode steps append), then one pass over the keys per (query head, 64 query rows): scores and the weighted sum of V on the
 * matrix pipe with fp32 accumulation, online softmax in fp32.
 *   qkv        fp16 [m][ld_qkv]: per row the query heads, the key heads, the value heads (what the fused projection writes for M = m);
 *              ld_qkv = 0: (heads + 2 kv_heads) * head_dim
 *   k_cache, v_cache  fp16 [kv_heads][max_keys][head_dim] as for the decode step (pos + m <= max_keys); cos / sin tables [positions][head_dim] or both NULL
 *   mask       fp16 [m][ld_mask] additive (the reference's attention_mask: 0 / the lowest half), or NULL;  ld_mask = 0: pos + m
 *   causal     non-zero: row r sees keys 0 .. pos + r (in addition to the mask, if any) -- key tiles behind a block's diagonal are skipped
 *   out        fp16 [m][ld_out]: row r, columns head * head_dim .. (= o_proj's input rows; ld_out = 0: heads * head_dim)
 *   workspace  tce_attention_prefill_workspace_bytes(heads, m, head_dim) bytes (the rotated queries; no zeroing needed)
 * Not the reference's binary16 accumulation chains (tce_bmm_f16t + tce_softmax_half are those, bit for bit): agrees with a float64 evaluation within
 * 2e-3 * max|out| per head and row.  head_dim == 128.  Cache rows at and beyond pos + m may hold anything. */
TCE_API size_t tce_attention_prefill_workspace_bytes(int heads, int m, int head_dim);
TCE_API int tce_attention_prefill_f16(const void *qkv, int ld_qkv, void *k_cache, void *v_cache, const void *cos_table, const void *sin_table, const void *mask,
                                      int ld_mask, int causal, void *out, int ld_out, void *workspace, int heads, int kv_heads, int head_dim, int max_keys,
                                      int pos, int m, unsigned short alpha_half_bits, void *stream);
/* The PAGED prefill: the two launches above on the paged step's pools and block table (k_pool / v_pool [num_pages][kv_heads][page_keys][head_dim], block_table int32
 * [table_rows][table_stride], as for tce_attention_decode_step_paged_f16), for up to TCE_PREFILL_MAX_SEGMENTS sequences at once.  No staging cache, no gather, no
 * scatter: appended rows go straight into their pages, key tiles are read through the table.
 *   segments   a HOST array, read at the call: segment i is m new rows -- rows row0 .. row0 + m - 1 of qkv and out -- on top of pos cached keys of table row `slot`.
 *              Distinct slots, disjoint row ranges inside [0, total_rows); rows of qkv that belong to no segment are skipped.
 *   qkv, out   fp16 [total_rows][ld_qkv] / [total_rows][ld_out] as for tce_attention_prefill_f16; workspace: tce_attention_prefill_paged_workspace_bytes(heads,
 *              total_rows, head_dim) bytes (the rotated queries [heads][total_rows][head_dim])
 *   causal     0 or non-zero, as above; the paged form takes no additive mask
 * Every segment's output rows and appended cache rows are bit-identical to tce_attention_prefill_f16 (mask NULL) for that sequence alone on a contiguous cache with the
 * same contents.  Trust, as for the paged step: of a segment's table row only words 0 .. (pos + m - 1) / page_keys ever become addresses; rows of the last page at and
 * beyond pos + m may hold anything; no pool row other than rows pos .. pos + m - 1 of each segment is written; page numbers are NOT validated
 * (tce_kv_block_table_check).  A launch lists at most 1024 query blocks (of 64 rows, or 128 once the launch has 512 of those over all heads):
 * TCE_ERR_UNSUPPORTED_SHAPE beyond -- several calls.  Every other refusal happens before any HIP call and tce_last_error() names the segment.
 * tce_attention_prefill_describe_paged: "form=F rows-per-block=R pair=yes|no blocks=B workgroups=W segments=S" for such a launch (a thread-local buffer; NULL and
 * tce_last_error() for a refused list; no HIP call).  With one segment, form and pairing are what tce_attention_prefill_f16 chooses for the same heads, m, causal. */
#define TCE_PREFILL_MAX_SEGMENTS 16
typedef struct tce_prefill_segment {
    int32_t slot, pos, m, row0;
} tce_prefill_segment;
TCE_API size_t tce_attention_prefill_paged_workspace_bytes(int heads, int total_rows, int head_dim);
TCE_API int tce_attention_prefill_paged_f16(const void *qkv, int ld_qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_rows, int table_stride,
                                            int page_keys, int num_pages, const void *cos_table, const void *sin_table, int causal, void *out, int ld_out, void *workspace,
                                            int heads, int kv_heads, int head_dim, const tce_prefill_segment *segments, int num_segments, int total_rows,
                                            unsigned short alpha_half_bits, void *stream);
TCE_API const char *tce_attention_prefill_describe_paged(int heads, int kv_heads, int causal, const tce_prefill_segment *segments, int num_segments);

/* FP8 pages: the paged cache with OCP e4m3 elements -- half the bytes held and half the bytes streamed per token -- for the paged step, the paged prefill and the copies.
 *   k_pool, v_pool  uint8 [num_pages][kv_heads][page_keys][128] each.  Page sizes, block table, trust rule and "one page number addresses both pools" are
 *                   tce_attention_decode_step_paged_f16's.  A row is 128 bytes; a group of four consecutive keys is 512 contiguous bytes and never crosses a page.
 *   encoding        a byte is OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; subnormals m * 2^-9; 0x7f / 0xff are NaN; no infinities; the largest finite
 *                   value is 448.  (Not the fnuz encoding.)
 *   scales          two per call and layer, k_scale_log2 and v_scale_log2, integers in [-8, 7] passed by value: a floating-point format needs a scale for range
 *                   only, and a power of two keeps dequantisation exact.
 *   dequant(b, e)   = e4m3(b) * 2^e as binary16, EXACT for every finite byte and every e in the range (448 * 2^7 = 57344 <= 65504; 2^-9 * 2^-8 = 2^-17 is a multiple
 *                   of 2^-24); a NaN byte gives a NaN.
 *   quant(x, e)     = e4m3_rne(clamp(float(x) * 2^-e, -448, 448)) for a binary16 x: the product is exact in fp32, rounding is to nearest with ties to the even
 *                   mantissa, the clamp saturates (+-inf included), -0 stays -0 (0x80), NaN becomes a NaN byte.
 * tce_attention_decode_step_paged_fp8 is tce_attention_decode_step_paged_f16 with the two exponents: workspace, grid, cut, pos_device, inactive rows and
 * tce_attention_decode_describe_paged's text are that step's.  Rows are dequantised as they are read and every arithmetic instruction behind that is the fp16 paged
 * step's: on pools whose fp16 image holds dequant(byte) the two steps' `out` rows are bit-identical.  The token's own key (rotated in binary16 as always) and value are
 * quantised, stored as BYTES, and weighed DEQUANTISED: the step's result is a function of the pools' contents, and a token that arrived by prefill and one that arrived by
 * a decode step are indistinguishable.
 * tce_attention_prefill_paged_fp8 is tce_attention_prefill_paged_f16 with the two exponents: the same segment list, block forms, pairing rule, 1024-block limit and
 * workspace function (tce_attention_prefill_describe_paged serves both).  Rotated keys and values are quantised into their pages; key / value tiles are dequantised into
 * the fp16 images the fp16 launch stages, so `out` is bit-identical to that launch on pools holding dequant(byte) when the new rows are on the e4m3 grid.
 * tce_kv_pages_scatter_fp8 / tce_kv_pages_gather_fp8: the f16 pair with an e4m3 pool side and a contiguous fp16 side; scatter quantises, gather dequantises; one
 * exponent per pool.  tce_kv_pages_pool_bytes_fp8: the bytes of ONE pool (half of tce_kv_pages_pool_bytes), 0 for an unsupported shape.
 * Every refusal happens before any HIP call and tce_last_error() names the argument; beyond the fp16 entry points' refusals: an exponent outside [-8, 7]
 * (TCE_ERR_BAD_ARG) and a pointer that is not 16-byte aligned (TCE_ERR_UNSUPPORTED_SHAPE, named). */
TCE_API size_t tce_kv_pages_pool_bytes_fp8(int num_pages, int kv_heads, int page_keys, int head_dim);
TCE_API int tce_attention_decode_step_paged_fp8(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int heads, int kv_heads,
                                                int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, int k_scale_log2,
                                                int v_scale_log2, void *stream);
TCE_API int tce_attention_prefill_paged_fp8(const void *qkv, int ld_qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_rows, int table_stride,
                                            int page_keys, int num_pages, const void *cos_table, const void *sin_table, int causal, void *out, int ld_out, void *workspace,
                                            int heads, int kv_heads, int head_dim, const tce_prefill_segment *segments, int num_segments, int total_rows,
                                            unsigned short alpha_half_bits, int k_scale_log2, int v_scale_log2, void *stream);
TCE_API int tce_kv_pages_scatter_fp8(const void *k_src, const void *v_src, void *k_pool, void *v_pool, const int32_t *table_row, int table_stride, int page_keys,
                                     int num_pages, int kv_heads, int head_dim, int src_max_keys, int key0, int nkeys, int k_scale_log2, int v_scale_log2, void *stream);
TCE_API int tce_kv_pages_gather_fp8(const void *k_pool, const void *v_pool, void *k_dst, void *v_dst, const int32_t *table_row, int table_stride, int page_keys,
                                    int num_pages, int kv_heads, int head_dim, int dst_max_keys, int key0, int nkeys, int k_scale_log2, int v_scale_log2, void *stream);

/* The paged step with T = rows_per_seq QUERY ROWS PER SEQUENCE (1 .. TCE_SPEC_MAX_ROWS): the attention launch of speculative decoding, where a sequence's next token
 * and up to T - 1 guessed continuations go through the layers together.  The arguments are tce_attention_decode_step_paged_f16 / _fp8's plus rows_per_seq:
 *   qkv, out, pos_device   batch * T rows / words: virtual row y = b * T + t belongs to sequence b -- row b of block_table -- and sits at position pos_device[y]
 *   workspace              tce_attention_decode_batch_workspace_bytes(batch * rows_per_seq, heads, table_stride * page_keys, head_dim) bytes, zeroed once: one slice
 *                          per virtual row
 * A row is active under the project's rule, 0 <= pos_device[y] <= pos_bound; an inactive row gets a zero `out` row and nothing else.  THE CALLER GUARANTEES that the
 * active rows of a sequence are a prefix t < n_b and that their positions are p, p + 1, ..., p + n_b - 1.  The kernel TRUSTS this as it trusts page numbers: row t
 * takes keys p .. p + t from the q/k/v rows y - t .. y of this call (rotated with the cos / sin row of each one's position; on e4m3 pools quantised and dequantised as
 * the append does) and never from the pool, where other workgroups of the same launch are writing them; all it does on its own is never to reach below position 0.
 * Each row appends only its own key / value row, at its own position: every pool row has one writer.
 * CONTRACT (no tolerance): row (b, t)'s `out` and the pool rows one call appends are bit-identical to what t + 1 successive calls of
 * tce_attention_decode_step_paged_f16 / _fp8 with the same pos_bound (hence the same cut) produce for sequence b; no other pool byte changes; rows_per_seq = 1 is
 * that step.  batch <= 65535; refusals as for the steps, plus rows_per_seq outside 1 .. TCE_SPEC_MAX_ROWS (TCE_ERR_UNSUPPORTED_SHAPE). */
#define TCE_SPEC_MAX_ROWS 8
TCE_API int tce_attention_decode_step_paged_rows_f16(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                     const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int rows_per_seq, int heads,
                                                     int kv_heads, int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, void *stream);
TCE_API int tce_attention_decode_step_paged_rows_fp8(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                     const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int rows_per_seq, int heads,
                                                     int kv_heads, int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, int k_scale_log2,
                                                     int v_scale_log2, void *stream);

/* SLIDING-WINDOW attention on the paged cache (Mistral-7B v0.1, the local layers of Gemma-2/3, Phi-3): window = W >= 1, a query at position p weighs keys lo(p) .. p,
 * lo(p) = max(0, p - W + 1) -- the last W keys, its own included.  A per-layer property: each entry point below is its unwindowed namesake with `int window` in front
 * of `stream`, and everything not said here (arguments, workspace, inactive rows, appended rows, e4m3 rules, refusals) is the namesake's.
 *   key range   the step's workgroups cover keys from base = lo & ~3 on, not from 0: the keys base .. lo - 1 of the first group of four are loaded -- they lie in the
 *               page of key lo -- and weigh NOTHING (excluded from the maximum and the sum, like keys beyond the position).  The prefill's query blocks walk key tiles
 *               from the tile of lo(their first row) on; tiles wholly below are neither requested nor computed.
 *   cut         the batched step's fitted rule for min(pos_bound + 1, W + 3) keys: the grid follows the window, not pos_bound
 *               (tce_attention_decode_describe_paged_window; text as tce_attention_decode_describe_paged).  The workspace and its per-sequence slices are the unwindowed
 *               step's, so one workspace serves both.
 *   trust       of an active row only table words lo / page_keys .. pos / page_keys become addresses (prefill: from lo(first row of the block) / page_keys); the words
 *               below may hold anything -- the pages they named can be handed to another sequence (PageAllocator.release_behind).  Page numbers are NOT validated:
 *               tce_kv_block_table_check_window is tce_kv_block_table_check restricted to the words a windowed row follows.
 *   identities  (no tolerance) 1. NEVER BINDING: with W >= pos_bound + 1 (prefill: W >= pos + m of every segment) `out` and every pool byte equal the unwindowed entry
 *               point's.  2. RE-BASED: where lo is a multiple of page_keys, the windowed step at pos = lo + W - 1 equals the unwindowed step at position W - 1 with
 *               pos_bound W + 2, a table row that starts at word lo / page_keys and cos / sin tables advanced by lo rows -- both launches use the same cut.
 *               Elsewhere: a float64 evaluation over keys lo .. p within the steps' stated bound.
 *   refusals    window < 1: TCE_ERR_BAD_ARG; the prefill with causal == 0: TCE_ERR_BAD_ARG (a row's window ends at its own key).  Before any HIP call, BAD_ARG rules
 *               before UNSUPPORTED_SHAPE rules, as everywhere in the paged family.
 *   rows        tce_attention_decode_step_paged_rows_window_f16 / _fp8: the multi-row step with a window (speculative decoding on a windowed layer) -- the arguments
 *               of tce_attention_decode_step_paged_rows_f16 / _fp8 with `int window` in front of `stream`.  Virtual row y = b * T + t at position pos = p + t weighs
 *               keys lo_t .. pos, lo_t = max(0, pos - W + 1); its workgroups start at base_t = lo_t & ~3; the cut, the grid's chunk slots and the workgroup order are
 *               the windowed step's (min(pos_bound + 1, W + 3) keys, the same for every row), the workspace the multi-row step's (one slice per virtual row).  Keys
 *               in [pos - t, pos] come from the call's own q/k/v rows, never from the pool (the multi-row rule); one of them below lo_t -- possible only with W <= t,
 *               so W < 8 -- weighs nothing.  Where the window lies wholly inside the call's rows no pool row at or beyond position p is weighted.  Of table row b
 *               only words lo_t / page_keys .. pos / page_keys become addresses: a sequence's active rows p .. p + n - 1 follow exactly the words that
 *               tce_kv_block_table_check_window follows for position p + n - 1 with window W + n - 1 (there is no further check entry point).
 *               CONTRACT (no tolerance): row (b, t)'s `out` and the pool rows one call appends are bit-identical to t + 1 successive calls of
 *               tce_attention_decode_step_paged_window_f16 / _fp8 with the same pos_bound and window; no other pool byte changes; rows_per_seq = 1 is that step;
 *               window >= pos_bound + 1 is the unwindowed multi-row step.  Refusals: window < 1 TCE_ERR_BAD_ARG, rows_per_seq outside 1 .. TCE_SPEC_MAX_ROWS
 *               TCE_ERR_UNSUPPORTED_SHAPE, everything else the two parents' rules.
 * NOT BUILT: windows on contiguous caches and on the single-sequence step (attention sinks, below, exist wherever windows do: step, multi-row step, prefill); a
 * ring table for unbounded streams -- positions stay bounded by table_stride * page_keys. */
TCE_API int tce_attention_decode_describe_paged_window(int batch, int heads, int kv_heads, int pos_bound, int page_keys, int window, char *buf, int buf_len);
TCE_API int tce_attention_decode_step_paged_window_f16(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                       const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int heads, int kv_heads,
                                                       int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, int window, void *stream);
TCE_API int tce_attention_decode_step_paged_window_fp8(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                       const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int heads, int kv_heads,
                                                       int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, int k_scale_log2,
                                                       int v_scale_log2, int window, void *stream);
TCE_API int tce_attention_decode_step_paged_rows_window_f16(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys,
                                                            int num_pages, const void *cos_table, const void *sin_table, void *out, void *workspace, int batch,
                                                            int rows_per_seq, int heads, int kv_heads, int head_dim, const int32_t *pos_device, int pos_bound,
                                                            unsigned short alpha_half_bits, int window, void *stream);
TCE_API int tce_attention_decode_step_paged_rows_window_fp8(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys,
                                                            int num_pages, const void *cos_table, const void *sin_table, void *out, void *workspace, int batch,
                                                            int rows_per_seq, int heads, int kv_heads, int head_dim, const int32_t *pos_device, int pos_bound,
                                                            unsigned short alpha_half_bits, int k_scale_log2, int v_scale_log2, int window, void *stream);
TCE_API int tce_attention_prefill_paged_window_f16(const void *qkv, int ld_qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_rows, int table_stride,
                                                   int page_keys, int num_pages, const void *cos_table, const void *sin_table, int causal, void *out, int ld_out,
                                                   void *workspace, int heads, int kv_heads, int head_dim, const tce_prefill_segment *segments, int num_segments,
                                                   int total_rows, unsigned short alpha_half_bits, int window, void *stream);
TCE_API int tce_attention_prefill_paged_window_fp8(const void *qkv, int ld_qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_rows, int table_stride,
                                                   int page_keys, int num_pages, const void *cos_table, const void *sin_table, int causal, void *out, int ld_out,
                                                   void *workspace, int heads, int kv_heads, int head_dim, const tce_prefill_segment *segments, int num_segments,
                                                   int total_rows, unsigned short alpha_half_bits, int k_scale_log2, int v_scale_log2, int window, void *stream);
TCE_API int tce_kv_block_table_check_window(const int32_t *block_table, int table_stride, int page_keys, int num_pages, int batch, const int32_t *pos_device, int pos_bound,
                                            uint32_t *violations, int window, void *stream);

/* ATTENTION SINKS beside the sliding window (StreamingLLM: a model that was not trained with a window fails once the first keys of the sequence leave it; keeping them
 * beside the window is the remedy).  window = W >= 1, sinks = S, 1 <= S <= 16: the smallest page holds 16 keys, so the sinks always lie in table word 0's page.  Each entry
 * point below is its *_window namesake with `int sinks` behind `window`; everything not said here is the namesake's.
 * A row at position p BINDS iff p >= S + W.
 *   not binding  the row is the unwindowed row: it weighs keys 0 .. p, every score with q rotated with cos / sin row p.
 *   binding      lo = p - W + 1.  Keys 0 .. S - 1 are scored with q rotated by cos / sin row S + W - 1, keys lo .. p with q rotated by row p; ONE softmax runs over these
 *                S + W scores; keys S .. lo - 1 weigh nothing.  check_inf_half, alpha and the value handling are the step's.
 *   appended key rotated with row p, as always: the pools after any sequence of sink calls equal the pools after the unwindowed calls on the same inputs -- no pool byte
 *                depends on window or sinks, so forks, prefill and decode stay interchangeable.
 *   no RoPE      with cos = sin = NULL both queries are the raw q.
 * Why a second rotation of q is all it takes: StreamingLLM scores with positions INSIDE the cache, and a RoPE score depends on the position difference alone.  For a window
 * key j the difference is p - j in both numberings; for a sink key i < S it is (S + W - 1) - i, which is what q rotated with row S + W - 1 gives against the key as the
 * pool holds it (rotated with row i).  The definition is in terms of table ROWS, not angles: any cos / sin table is valid input.
 *   key range   the step's workgroups walk a virtual key sequence: S4 = (S + 3) & ~3 keys for the sinks (virtual v < S4 is key v, valid iff v < S), then the windowed
 *               step's keys from base2 = lo & ~3 on (valid iff >= lo); a row that does not bind walks keys 0 .. p.  Rows S .. S4 - 1 of word 0's page and rows base2 ..
 *               lo - 1 are loaded and weigh nothing.  The prefill: a query block's window pass is the windowed block's (a row that does not bind has lo = 0; the block
 *               starts at the lo of its first row, 0 if that row does not bind), and a block whose last row binds makes one more pass over keys 0 .. S - 1.
 *   cut         the batched step's fitted rule for the virtual keys: pos_bound + 1 while S + W > pos_bound (no row can bind: the unwindowed step's cut), else
 *               min(pos_bound + 1 + d, S4 + W + 3) with d = S4 - ((S + 1) & ~3), 0 or 4: the keys by which a binding row's virtual sequence can exceed pos + 1
 *               (tce_attention_decode_describe_paged_sink).  Workspace: the unwindowed step's.
 *   trust       of an active binding row only table word 0 and words lo / page_keys .. pos / page_keys become addresses (prefill, per block: word 0 if a row of the block
 *               binds, and the words from klo / page_keys on); of a row that does not bind words 0 .. pos / page_keys.  tce_kv_block_table_check_sink checks those words.
 *               The caller keeps the first ceil(S / page_keys) = 1 page of a sequence alive (PageAllocator.release_behind(..., keep_pages=1)).
 *   identities  (no tolerance) 1. NEVER BINDING: with S + W >= pos_bound + 1 (prefill: >= pos + m of every segment) `out` and every pool byte equal the unwindowed entry
 *               point's.  2. COMPACTION: with cos = sin = NULL, S a multiple of 4 and lo % 4 == 0 the step at a binding pos equals the unwindowed step at position
 *               S + W - 1 under pos_bound S + W + 2 on a pool that holds keys [0, S) ++ [lo, pos) -- both launches use the same cut.  Elsewhere: the float64 evaluation
 *               of the definition (two binary16 rotations of q) within the steps' stated bound.
 *   refusals    the *_window entry point's, in its order, then sinks < 1 || sinks > 16: TCE_ERR_BAD_ARG.  Before any HIP call.  The prefill is causal only.
 *   rows        tce_attention_decode_step_paged_rows_sink_f16 / _fp8: the multi-row step with sinks (speculative decoding on a sink layer; csrc/attention_rows_sink.hip)
 *               -- the arguments of tce_attention_decode_step_paged_rows_window_f16 / _fp8 with `int sinks` behind `window`.  Virtual row y = b * T + t sits at
 *               pos = p + t and BINDS iff pos >= S + W, by itself: one call may hold rows that do not bind in front of rows that do.  A binding row weighs keys
 *               0 .. S - 1, scored with q rotated by cos / sin row min(S + W - 1, pos_bound), and keys pos - W + 1 .. pos, scored with q rotated by row pos, under one
 *               softmax; a row that does not bind is the unwindowed row.  Keys in [pos - t, pos] come from the call's own q/k/v rows, never from the pool (the
 *               multi-row rule); each row appends only its own key / value row, rotated with its own position: no pool byte depends on window or sinks.
 *               SHAPE RULE: window >= rows_per_seq.  With pos >= S + W it gives p >= S + 1 for every sequence that has a binding row, so no key the call itself
 *               appends is a sink key and every in-call key lies inside its row's window (the corner the windowed rows step carries for W <= t does not exist here;
 *               sinks beside a window of fewer than 8 keys are not a use case).  The cut and the chunk slots are the one-row sink step's
 *               (tce_attention_decode_describe_paged_sink describes them; there is no further describe entry point), the grid the windowed rows step's, the
 *               workspace the multi-row step's (one slice per virtual row).  Of table row b an active binding row turns only word 0 and words
 *               lo_t / page_keys .. pos / page_keys into addresses, a row that does not bind words 0 .. pos / page_keys: a sequence's rows p .. p + n - 1 are
 *               covered by tce_kv_block_table_check_sink for position p + n - 1 with window W + n - 1 and sinks S -- exactly their words when p >= S + W, else
 *               words 0 .. (p + n - 1) / page_keys, a superset (nothing behind page 0 can have been released before position S + W).
 *               CONTRACT (no tolerance): row (b, t)'s `out` and the pool rows one call appends are bit-identical to t + 1 successive calls of
 *               tce_attention_decode_step_paged_sink_f16 / _fp8 with the same pos_bound, window and sinks; no other pool byte changes; rows_per_seq = 1 is that step;
 *               sinks + window >= pos_bound + 1 is the unwindowed multi-row step, bit for bit.  Refusals, before any HIP call, BAD_ARG rules before
 *               UNSUPPORTED_SHAPE rules as everywhere in the paged family: the *_rows_window entry point's TCE_ERR_BAD_ARG rules in its order, then sinks < 1 ||
 *               sinks > 16: TCE_ERR_BAD_ARG; then the *_rows_window entry point's TCE_ERR_UNSUPPORTED_SHAPE rules in its order, then window < rows_per_seq:
 *               TCE_ERR_UNSUPPORTED_SHAPE (the message names both arguments). */
TCE_API int tce_attention_decode_step_paged_rows_sink_f16(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys,
                                                          int num_pages, const void *cos_table, const void *sin_table, void *out, void *workspace, int batch,
                                                          int rows_per_seq, int heads, int kv_heads, int head_dim, const int32_t *pos_device, int pos_bound,
                                                          unsigned short alpha_half_bits, int window, int sinks, void *stream);
TCE_API int tce_attention_decode_step_paged_rows_sink_fp8(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys,
                                                          int num_pages, const void *cos_table, const void *sin_table, void *out, void *workspace, int batch,
                                                          int rows_per_seq, int heads, int kv_heads, int head_dim, const int32_t *pos_device, int pos_bound,
                                                          unsigned short alpha_half_bits, int k_scale_log2, int v_scale_log2, int window, int sinks, void *stream);
TCE_API int tce_attention_decode_describe_paged_sink(int batch, int heads, int kv_heads, int pos_bound, int page_keys, int window, int sinks, char *buf, int buf_len);
TCE_API int tce_attention_decode_step_paged_sink_f16(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                     const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int heads, int kv_heads,
                                                     int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, int window, int sinks, void *stream);
TCE_API int tce_attention_decode_step_paged_sink_fp8(const void *qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_stride, int page_keys, int num_pages,
                                                     const void *cos_table, const void *sin_table, void *out, void *workspace, int batch, int heads, int kv_heads,
                                                     int head_dim, const int32_t *pos_device, int pos_bound, unsigned short alpha_half_bits, int k_scale_log2,
                                                     int v_scale_log2, int window, int sinks, void *stream);
TCE_API int tce_attention_prefill_paged_sink_f16(const void *qkv, int ld_qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_rows, int table_stride,
                                                 int page_keys, int num_pages, const void *cos_table, const void *sin_table, int causal, void *out, int ld_out,
                                                 void *workspace, int heads, int kv_heads, int head_dim, const tce_prefill_segment *segments, int num_segments,
                                                 int total_rows, unsigned short alpha_half_bits, int window, int sinks, void *stream);
TCE_API int tce_attention_prefill_paged_sink_fp8(const void *qkv, int ld_qkv, void *k_pool, void *v_pool, const int32_t *block_table, int table_rows, int table_stride,
                                                 int page_keys, int num_pages, const void *cos_table, const void *sin_table, int causal, void *out, int ld_out,
                                                 void *workspace, int heads, int kv_heads, int head_dim, const tce_prefill_segment *segments, int num_segments,
                                                 int total_rows, unsigned short alpha_half_bits, int k_scale_log2, int v_scale_log2, int window, int sinks, void *stream);
TCE_API int tce_kv_block_table_check_sink(const int32_t *block_table, int table_stride, int page_keys, int num_pages, int batch, const int32_t *pos_device, int pos_bound,
                                          uint32_t *violations, int window, int sinks, void *stream);

/* Device-side sampling: what the reference does on the host between Int4LlamaForCausalLM::forward and the next token's Embedding (llm/src/Generate.cc driven by
 * LLaMA3Generate.cc:127-198), for `batch` rows of fp16 logits [batch][ld] (lm_head's output at M = batch; vocab <= ld) in TWO launches (csrc/sampling.hip), so that a
 * captured decode graph yields one token per replay for every sequence with no host round trip.  Per ACTIVE row (0 <= pos_device[b] <= pos_bound, the project's rule;
 * an inactive row has nothing read and nothing written: token, log, ring, counters and position stay as they are), in fp32 on the exact value of each fp16 word:
 *   1. sample_repetition_penalty over the last repeat_last_n (<= 64) tokens of the row's ring (x <= 0 ? x * penalty : x / penalty, once per distinct id), then
 *      sample_frequency_and_presence_penalties (x -= float(count) * alpha_frequency + float(count > 0) * alpha_presence); IEEE operations, no contraction.
 *   2. temp <= 0: greedy -- the LOWEST id among the maxima (std::max_element returns the first maximum).
 *   3. otherwise top_k (1 .. top_k_bound <= 256) -> softmax over the k in descending order (subtract the maximum, expf, a SEQUENTIAL fp32 sum, divide) -> top_p
 *      (with cum the running sum of p, n = the first i >= 1 with cum_i > top_p; candidates [0, n) are kept: the one that crosses the threshold is dropped -- the
 *      reference's behaviour --, top_p >= 1 keeps all k) -> logit / temp -> softmax over the n -> inverse-CDF draw on a uniform u in [0, 1): the first i with u < cdf_i
 *      (the last candidate if rounding leaves none).
 *   ORDER (std::partial_sort leaves it open and fp16 logits tie constantly): descending penalised logit, ASCENDING token id among equals, inside the top-k and at
 *   its boundary.  -0 and +0 are one value and come back as +0.
 *   u = (Philox4x32-10(counter = (rows[b].generated, 0, 0, 0), key = (seed_lo, seed_hi)) word 0 >> 8) * 2^-24: keyed by the sequence's seed and the index of the token
 *   within its sequence, never by slot, batch or launch; uniform_override ([batch] fp32, may be NULL) replaces it (tests).
 *   The tail, same launch: next_token[b] = token; out_log[b][generated] = token; the token is pushed into the ring; generated += 1; then pos_device[b] += 1 -- or = -1
 *   (retired) when the token is one of the n_stop (<= 4) stop_ids or generated has reached rows[b].max_new (or log_stride).
 * rows: DEVICE array [batch] of tce_sample_row (304 bytes): the row's parameters and its state -- a slot changes hands by one copy of its row, a captured graph needs
 * no recapture.  A fresh row has generated = ring_pushed = 0 and ring = 64 zeros, as the reference's last_n_tokens starts (token 0 is penalised until 64 tokens have
 * passed); prompt tokens are pushed by the host at admission (ring[ring_pushed % 64], ring_pushed += 1).  A row's top_k outside [1, top_k_bound] is clamped (it lives
 * on the device: the host cannot refuse it at the call).
 * NOT BUILT: top_k <= 0 = "whole vocabulary", k > 256; and this entry point runs no tail-free or typical stage and no mirostat -- the CALL accepts only the disabled values
 * tfs_z 1.0, typical_p 1.0, mirostat 0 --: TCE_ERR_UNSUPPORTED_SHAPE before any launch.  (The two stages ARE built, per slot: tce_sample_stages_f16 below; so is mirostat,
 * per slot over the top-k candidates: tce_sample_mirostat_f16 below.  Token masks,
 * automata and logit_bias ARE built: tce_sample_constrained_f16 below; this entry point applies none.)  Also refused there: vocab > ld (TCE_ERR_BAD_ARG), vocab > 2^20, logits not 16-byte aligned or ld % 8 != 0, and ceil(vocab / 4096) * top_k_bound
 * > 8192 (the second launch holds the chunks' survivors in registers: 131072 entries at k = 256, 838k at k = 40).
 * workspace: tce_sample_workspace_bytes(batch, vocab) bytes (0 for a bad shape), zeroed once; word 0 counts the ids tce_embed_rows_f16 refused, the rest carries the
 * first launch's survivors to the second -- the kernel boundary is the only ordering, there is no counter to reset.  The logits are not modified.
 * debug (may be NULL): [batch] records of the row's sorted candidates for tests. */
typedef struct tce_sample_row {
    float temp;              /* <= 0: greedy */
    int32_t top_k;
    float top_p;
    float repeat_penalty;    /* 1.0: off */
    float alpha_frequency, alpha_presence;
    int32_t repeat_last_n;   /* 0 .. 64 */
    int32_t max_new;         /* the row retires when `generated` reaches it */
    uint32_t seed_lo, seed_hi;
    uint32_t generated;      /* tokens sampled for this sequence so far = the generator's counter */
    uint32_t ring_pushed;    /* tokens pushed into the ring (prompt + generated) */
    int32_t ring[64];
} tce_sample_row;
typedef struct tce_sample_debug {
    int32_t n, k;            /* candidates kept after top-p; candidates after top-k */
    float u;
    int32_t choice;          /* the index drawn */
    int32_t ids[256];
    float logit[256], p[256], final_p[256]; /* sorted penalised logits, p of the first softmax, p after temperature (n entries) */
} tce_sample_debug;
typedef struct tce_sample_call {
    const void *logits;
    int32_t ld, vocab, batch, top_k_bound;
    tce_sample_row *rows;
    int32_t *pos_device;
    int32_t pos_bound, log_stride;
    int32_t *next_token;     /* [batch] */
    int32_t *out_log;        /* [batch][log_stride] */
    const float *uniform_override;
    tce_sample_debug *debug;
    void *workspace;
    int32_t stop_ids[4];
    int32_t n_stop, mirostat;
    float tfs_z, typical_p;
} tce_sample_call;
TCE_API size_t tce_sample_workspace_bytes(int batch, int vocab);
TCE_API int tce_sample_f16(const tce_sample_call *call, void *stream);
/* Speculative decoding's two device-side pieces around the layers (csrc/sampling.hip): drafts from the sequence's own history, and the verifier.
 * tce_draft_ngram (one launch).  history: DEVICE int32 [batch][hist_stride], history[b][i] = the token processed at position i (the prompt, then every emitted token;
 * the token at index p is the one the next step feeds).  pos_device [batch]: the SEQUENCES' positions.  Written: row_token, row_pos [batch * rows_per_seq].
 *   inactive sequence (p < 0, p > pos_bound or p >= hist_stride): every row (0, -1)
 *   row 0: (history[b][p], p)
 *   drafts, n = ngram (1 .. 4): i* = the largest i with n - 1 <= i < p and history[i - n + 1 .. i] == history[p - n + 1 .. p]; none, or p < n: no drafts.  Row t >= 1 is
 *   (history[b][i* + t], p + t) while i* + t <= p and p + t <= pos_bound; every row behind that is inactive: (0, -1)
 *   script (may be NULL; a test hook, int32 [batch][hist_stride]): replaces the lookup -- row t >= 1 is (script[b][p + t], p + t) while p + t <= pos_bound, p + t <
 *   hist_stride and no script[b][p + 1 .. p + t] is negative.
 * tce_sample_verify_f16 (three launches; the kernel boundary is the only ordering, no counters).  s: a tce_sample_call in which batch = B SEQUENCES -- rows, pos_device,
 * next_token and out_log are per sequence --, logits is [B * T][ld] and uniform_override / debug are per VIRTUAL row y = b * T + t; workspace:
 * tce_sample_verify_workspace_bytes(batch, rows_per_seq, vocab) bytes, zeroed once (its word 0 is tce_embed_rows_f16's counter, as tce_sample_f16's).  row_token /
 * row_pos: what tce_draft_ngram wrote and the layers ran on.  Per ACTIVE sequence (0 <= pos_device[b] = p <= pos_bound) with n active rows and g = rows[b].generated,
 * for t = 0, 1, ...:
 *   1. y_t = the token tce_sample_f16 would choose from logits row (b, t) with the penalty window of the ring after y_0 .. y_{t-1} were pushed and the uniform keyed
 *      (seed, g + t)
 *   2. y_t is emitted with tce_sample_f16's tail: out_log[b][g + t], the ring push, generated += 1; and history[b][p + 1 + t] = y_t (where < hist_stride)
 *   3. a stop id, or generated reaching max_new / log_stride: the sequence retires (pos_device[b] = -1) and the chain ends
 *   4. t + 1 >= n or row_token[(b, t + 1)] != y_t: the chain ends with pos_device[b] = p + t + 1
 *   and next_token[b] = the last y_t; emitted[b] = the tokens emitted (0 for an inactive sequence, whose state is not touched).
 * LOSSLESS: the emitted tokens are those of tce_sample_f16 called once per token.  A row that is reached at all has had all its drafts accepted, so its window (the
 * ring plus drafts 1 .. t) is known in advance: the select launch runs for all B * T rows at once, the draw per row into a candidate array, and a last small launch
 * walks the chain and writes state.  Cache rows p + t + 1 .. of REJECTED drafts stay behind the position as garbage: the next step overwrites them or never weighs them.
 * Refusals: tce_sample_f16's (k > 256 and whole-vocabulary top-k stay unbuilt; tail-free and typical run behind tce_sample_verify_stages_f16, mirostat behind
 * tce_sample_verify_mirostat_f16), rows_per_seq outside 1 .. TCE_SPEC_MAX_ROWS, batch *
 * rows_per_seq > 65535, ngram outside 1 .. 4, hist_stride <= pos_bound. */
typedef struct tce_sample_verify_call {
    tce_sample_call s;
    int32_t rows_per_seq, hist_stride;
    const int32_t *row_token, *row_pos; /* [batch * rows_per_seq] */
    int32_t *history;                   /* [batch][hist_stride] */
    int32_t *emitted;                   /* [batch] */
} tce_sample_verify_call;
TCE_API size_t tce_sample_verify_workspace_bytes(int batch, int rows_per_seq, int vocab);
TCE_API int tce_sample_verify_f16(const tce_sample_verify_call *call, void *stream);
TCE_API int tce_draft_ngram(const int32_t *history, const int32_t *script, int hist_stride, const int32_t *pos_device, int pos_bound, int batch, int rows_per_seq, int ngram,
                            int32_t *row_token, int32_t *row_pos, void *stream);
/* Log-probabilities on the device (csrc/sampling.hip; additive within ABI 113, no existing struct or entry point changes): of the token just sampled, and of given
 * target tokens (scoring, perplexity).  ONE definition serves both:
 *   logprob(row, t) = x_t - LSE(x),  LSE(x) = M + logf(sum_i expf(x_i - M)),  M = max_i x_i,  i < vocab,
 * x = the row's RAW fp16 logits as lm_head wrote them, widened exactly to fp32; fp32 arithmetic.  It is the model's distribution: it does NOT depend on penalties,
 * top-k, top-p, temperature, seed or slot -- a sampled token's value and a scored prompt token's value are comparable.  The sums are taken in one fixed order in
 * every entry point (per 4096-logit chunk: 16 per thread in index order, a wave butterfly, waves 0 .. 3 in order; then the <= 256 chunk pairs (m_c, s_c) through a
 * fixed tree), so a value does not depend on batch size, slot, or eager versus captured launches either.  For rows with every |x_i| <= 64 the result lies within
 * 2^-16 of the float64 value.  Degenerate rows are defined: a NaN or +inf logit, or a row of -inf only, gives NaN; a chunk of -inf beside finite chunks takes no part.
 * tce_logprob_out: out_logprob fp32 [batch][log_stride], indexed as out_log (value g of sequence b beside token g, written under the same bound); last_lse fp32
 *   [batch], may be NULL: the LSE of the row the sequence's last token was drawn from; partials: tce_logprobs_workspace_bytes(rows, vocab) bytes, 8-byte aligned, need
 *   not be zeroed (every word read in a call was written by that call's first launch), rows = batch, for the verifier batch * rows_per_seq.
 * tce_sample_logprobs_f16: tce_sample_f16 -- token, log, ring, counters, position and debug record bit for bit -- plus the value; still two launches.
 * tce_sample_verify_logprobs_f16: tce_sample_verify_f16 plus out_logprob[b][g + t] for every EMITTED y_t (rejected rows write nothing); still three launches.
 * tce_logprobs_f16 (two launches; the kernel boundary is the only ordering): logits fp16 [rows][ld], target DEVICE int32 [rows]; out_logprob fp32 [rows]; out_lse fp32
 *   [rows], may be NULL.  target -1 = "no target": out_logprob 0.0, the LSE still written; any other target outside [0, vocab): NaN.  rows <= 65535.
 * Refusals, before any launch: tce_sample_f16's / tce_sample_verify_f16's own (alignment, ld % 8, vocab <= ld, vocab <= 2^20, ...), a NULL tce_logprob_out, out_logprob
 * or partials (TCE_ERR_BAD_ARG), partials not 8-byte or a float array not 4-byte aligned (TCE_ERR_UNSUPPORTED_SHAPE). */
typedef struct tce_logprob_out {
    float *out_logprob;
    float *last_lse;
    void *partials;
} tce_logprob_out;
TCE_API size_t tce_logprobs_workspace_bytes(int rows, int vocab);
TCE_API int tce_sample_logprobs_f16(const tce_sample_call *call, const tce_logprob_out *lp, void *stream);
TCE_API int tce_sample_verify_logprobs_f16(const tce_sample_verify_call *call, const tce_logprob_out *lp, void *stream);
TCE_API int tce_logprobs_f16(const void *logits, int ld, int vocab, int rows, const int32_t *target, float *out_logprob, float *out_lse, void *partials, void *stream);
/* Constrained decoding on the device (csrc/sampling.hip; additive within ABI 113, no existing struct or entry point changes): which tokens a row may draw is a TOKEN
 * AUTOMATON that lives on the device and advances in the sampler's tail, plus up to TCE_BIAS_MAX (id, value) logit-bias pairs per row -- the reference carries
 * logit_bias in its generation config (llm/include/Generate.h:59) and never applies it.  A captured replay stays one token per live slot with no host round trip.
 * tce_sample_constrained_f16 is tce_sample_f16 (with lp: tce_sample_logprobs_f16) with, per ACTIVE row, c->rows[b] = (fsm, state, bias):
 *   1. BIAS.  The row's first min(max(n_bias, 0), 16) pairs; for each pair with 0 <= id < vocab, x_id = float(fp16 logit) + bias_val: one fp32 add, BEFORE any penalty;
 *      an id that occurs twice has the later pair added on top of the earlier one, in index order.  tce_sample_f16's step 1 (the penalties) acts on the biased value.
 *   2. MASK.  fsm >= 0: token t is a candidate only if bit (t & 31) of word mask[state][t >> 5] is set (a word at or past mask_words counts as 0).  A masked token is
 *      "no element", like an entry past the vocabulary, whatever its logit; an allowed token whose logit is -inf IS a candidate.  fsm < 0: every token is allowed.
 *   3. THE CHAIN.  Greedy, top-k, softmax, top-p, temperature and the draw run unchanged over the candidates, in the same order (descending penalised logit, ascending id
 *      among equals); with fewer than k candidates, k becomes their number.
 *   4. TAIL.  next = edge_next[e] of the edge e in [edge_begin[state], edge_begin[state + 1]) with edge_token[e] == token (binary search: ascending), else
 *      default_next[state].  next == TCE_FSM_DONE: the token is emitted, then the row retires (pos_device[b] = -1) exactly as for a stop id; the state word stays.
 *      Otherwise state = next -- also when a stop id or max_new retires the row in the same call.
 *   5. LOG-PROBABILITIES (lp != NULL) stay what they are: x_t - LSE(x) on the RAW logits; neither the mask nor the bias enters.
 *   6. INVALID STATE (the row lives on the device: the host cannot refuse it at the call; ONE defined path).  A constrained row is invalid when fsm >= n_fsm, when state
 *      lies outside [0, states), when the chosen token's next lies outside [-1, states), or when its state leaves no candidate inside the vocabulary.  An invalid row
 *      emits NOTHING -- token, log, ring, generated, state and debug record stay untouched --, retires (pos_device[b] = -1) and adds 1 to *violations.  The state changes
 *      only in the tail.
 *   7. fsm < 0 and n_bias <= 0: everything tce_sample_f16 (tce_sample_logprobs_f16) writes comes out bit for bit.
 * tce_sample_verify_constrained_f16: c->rows is per SEQUENCE; virtual row t is sampled in the state delta*(state, row_token[(b, 1)] .. row_token[(b, t)]), known in advance
 *   for the reason the penalty window is (thread 0 of the select workgroup walks the <= TCE_SPEC_MAX_ROWS - 1 transitions).  A draft that is forbidden, or whose
 *   transition is DONE or invalid, makes its row and every row behind it unreachable -- the token sampled in front of it is allowed and so differs from the draft --:
 *   they are not sampled and their candidate word is -1.  The chain launch advances the state once per EMITTED token and applies 4's retirement and 6 (an invalid row t
 *   emits nothing and retires the sequence behind the t tokens already emitted).  LOSSLESS: the emitted tokens, the state words and *violations are those of
 *   tce_sample_constrained_f16 called once per token.
 * tce_fsm (56 bytes) and its arrays are DEVICE memory written by the host, stream-ordered; a captured graph keeps c->fsms, c->rows and c->violations.  The arrays'
 * contents are trusted as far as rule 6 does not name them (edge_begin ascending within [0, edges], mask [states][mask_words]).
 * Refusals, before any launch: tce_sample_f16's / tce_sample_verify_f16's own, the logprob forms' for a non-NULL lp; TCE_ERR_BAD_ARG for a NULL c, rows or violations,
 * n_fsm outside 0 .. TCE_FSM_MAX, n_fsm > 0 with NULL fsms; TCE_ERR_UNSUPPORTED_SHAPE for fsms not 8-byte or rows / violations not 4-byte aligned.
 * NOT BUILT: log-probabilities renormalised over the allowed set, constraints in scoring, cutting tce_draft_ngram's drafts at the first forbidden token. */
#define TCE_FSM_DONE      (-1)   /* a transition to it: the token is emitted, then the sequence retires */
#define TCE_FSM_MAX       64     /* automata resident at once */
#define TCE_BIAS_MAX      16     /* (id, value) pairs per row */
typedef struct tce_fsm {          /* one token automaton, all arrays on the DEVICE */
    const uint32_t *mask;         /* [states][mask_words]; bit (t & 31) of word t >> 5 set: token t allowed in the state; bits at t >= vocab are ignored */
    const int32_t *edge_begin;    /* [states + 1] */
    const int32_t *edge_token;    /* [edges], strictly ascending within a state */
    const int32_t *edge_next;     /* [edges] */
    const int32_t *default_next;  /* [states]: next state of an allowed token that has no edge */
    int32_t states, mask_words, start, reserved0;
} tce_fsm;
typedef struct tce_constraint_row { /* per slot (144 bytes); changes hands by one copy, like tce_sample_row */
    int32_t fsm;                  /* index into fsms, -1: unconstrained */
    int32_t state;
    int32_t n_bias, reserved0;
    int32_t bias_id[TCE_BIAS_MAX];
    float bias_val[TCE_BIAS_MAX];
} tce_constraint_row;
typedef struct tce_constraint {
    const tce_fsm *fsms; int32_t n_fsm, reserved0;   /* DEVICE array; a captured graph keeps the pointer, the host rewrites entries stream-ordered */
    tce_constraint_row *rows;                        /* DEVICE [batch] (per SEQUENCE in the verifier) */
    uint32_t *violations;                            /* DEVICE, one word, zeroed once */
} tce_constraint;
TCE_API int tce_sample_constrained_f16(const tce_sample_call *call, const tce_constraint *c, const tce_logprob_out *lp /* may be NULL */, void *stream);
TCE_API int tce_sample_verify_constrained_f16(const tce_sample_verify_call *call, const tce_constraint *c, const tce_logprob_out *lp /* may be NULL */, void *stream);
/* Tail-free and locally typical sampling per slot (csrc/sampling.hip; additive within ABI 113, no existing struct or entry point changes): the two stages the reference
 * runs between top-k and top-p in its temperature branch (LLaMA3Generate.cc:174-179: sample_top_k -> sample_tail_free(tfs_z) -> sample_typical(typical_p) -> sample_top_p
 * -> sample_temperature -> sample_token; Generate.cc:203-302), with their two values PER SLOT in st->rows[b] -- two requests of one batch may differ, and a slot changes
 * hands by one copy with no recapture.  tce_sample_stages_f16 is tce_sample_f16 (with lp: tce_sample_logprobs_f16; with c: tce_sample_constrained_f16) with, per ACTIVE
 * row with temp > 0, behind the penalties (bias, mask) and top-k, on the kk candidates in the project's order (descending penalised logit, ascending id among equals),
 * values l_i.  fp32, IEEE operations, no contraction; sums SEQUENTIAL in index order from 0.0f; expf and logf; comparisons as the reference writes them:
 *   1. SOFTMAX(m candidates in their current order): e_i = expf(l_i - l_first), s = sum e_i, p_i = e_i / s, l_first = the value of the candidate that stands FIRST --
 *      after rule 3 that need not be the maximum (the reference's `sorted` flag stays set and sample_softmax takes data[0].logit), so an argument may be positive.
 *   2. TAIL-FREE.  Runs iff !(tfs_z >= 1.0f) and kk > 2, on p = softmax(kk): d1_i = p_i - p_{i+1} (i < kk - 1), d2_i = fabsf(d1_i - d1_{i+1}) (i < kk - 2), S = sum d2_i,
 *      w_i = d2_i / S, cum the running sum of w; n1 = the first i >= 1 with cum_i > tfs_z, else kk.  S == 0 (equal candidates): NaN weights, no comparison holds, nothing
 *      is cut.  tfs_z <= 0 keeps one candidate; a NaN tfs_z runs the stage and cuts nothing.
 *   3. TYPICAL.  Runs iff !(typical_p >= 1.0f), on p = softmax(the first n1) (bit-identical to rule 2's when n1 == kk): H = sum (-p_i) * logf(p_i), one multiply and one
 *      add per term; s_i = fabsf(-logf(p_i) - H); the candidates are ordered by ASCENDING s, the EARLIER candidate first among equal scores (std::sort leaves ties open:
 *      the project's choice, like the id rule) -- rank_i = #{ j : s_j < s_i || (!(s_i < s_j) && j < i) }.  A p_i of 0 makes logf -inf, H NaN and every score NaN: the
 *      order stays as it is.  With cum the running sum of p in that order, n2 = i + 1 at the first i >= 0 with cum > typical_p, else n1.  The candidates BECOME
 *      order[0 .. n2) in that order.
 *   4. TOP-P.  Runs iff top_p < 1.0f, as tce_sample_f16's, over softmax(the n2 in their current order): n = the first i >= 1 with cum_i > top_p, else n2.
 *   5. l_i / temp, softmax(the n in their current order), the inverse-CDF draw in that order (the first i with u < cdf_i, else n - 1); the token is the id of the
 *      candidate at that position.  Greedy rows, the generator's counter, the tail, stop ids, retirement and inactive rows are tce_sample_f16's.
 *   6. IDENTITY.  A row whose two values are both >= 1.0f comes out bit for bit as the underlying entry point writes it: token, log, ring, counters, position, debug
 *      record, logprob and constraint state.
 * st->rows: DEVICE array [batch] of tce_stage_row; a captured graph keeps the pointer, the host rewrites a slot's pair stream-ordered.  st->debug (may be NULL): [batch]
 * records for tests.  With it, tce_sample_debug keeps the meaning of ids, logit, p (the softmax over kk) and k -- the SORTED top-k candidates --; n, final_p and choice
 * refer to the final order.
 * tce_sample_verify_stages_f16: tce_sample_verify_f16 (with lp / c: its logprob / constrained form); st->rows is per SEQUENCE -- every virtual row of a sequence is
 * sampled with its sequence's pair --, st->debug per VIRTUAL row.  LOSSLESS as the verifier is: the emitted tokens are those of tce_sample_stages_f16 called once per token.
 * Launches: 2 and 3 as before; the first (the vocabulary pass) is the underlying form's own kernel.
 * Refusals, before any launch: everything the underlying entry point refuses -- non-default tfs_z / typical_p / mirostat in the CALL included: the call's two fields stay
 * refused, the values live in st->rows --, the constrained / logprob forms' for a non-NULL c / lp; TCE_ERR_BAD_ARG for a NULL st or st->rows; TCE_ERR_UNSUPPORTED_SHAPE for
 * rows or debug not 4-byte aligned.
 * Mirostat is not run by these two entry points (mirostat != 0 in the CALL stays refused): it lives per slot behind tce_sample_mirostat_f16 below, over the row's top-k
 * candidates, and behind tce_sample_verify_mirostat_f16, which needs one more launch (a speculative row's cut depends on the draw of the row in front of it).  Also not built, as before: top_k <= 0 = "whole vocabulary", k > 256. */
typedef struct tce_stage_row { float tfs_z, typical_p; } tce_stage_row;   /* per slot (8 bytes); 1.0 = off; changes hands by one copy */
typedef struct tce_stage_debug {                                          /* tests; per row (per virtual row in the verifier); 2056 bytes.  A greedy row (temp <= 0) has ONE
                                                                             candidate: n_tfs = n_typ = 1, order = {0}, p_top = 0.  An inactive or rule-6 row writes nothing */
    int32_t n_tfs, n_typ;          /* candidates after tail-free, after typical */
    int32_t order[256];            /* position i of the final order -> index into the sorted top-k candidates, i < n_typ (-1 behind) */
    float p_top[256];              /* the softmax top-p walked (n_typ entries, final order) */
} tce_stage_debug;
typedef struct tce_sample_stages { tce_stage_row *rows; tce_stage_debug *debug /* may be NULL */; } tce_sample_stages;
TCE_API int tce_sample_stages_f16(const tce_sample_call *call, const tce_sample_stages *st, const tce_constraint *c /* may be NULL */, const tce_logprob_out *lp /* may be NULL */,
                                  void *stream);
TCE_API int tce_sample_verify_stages_f16(const tce_sample_verify_call *call, const tce_sample_stages *st, const tce_constraint *c /* may be NULL */,
                                         const tce_logprob_out *lp /* may be NULL */, void *stream);
/* Mirostat v1 and v2 per slot (csrc/sampling.hip; additive within ABI 113, no existing struct or entry point changes): the last branch of the reference's sampling
 * configuration (Generate.h:69-71; LLaMA3Generate.cc:162-171: penalties -> sample_temperature -> sample_token_mirostat[_v2], Generate.cc:138-201), and the sampler's
 * first STATEFUL rule: a running value mu per slot, read and written by the launch that emits the token, so a captured replay carries it with no host round trip.
 * tce_sample_mirostat_f16 is tce_sample_stages_f16 with, per ACTIVE row b whose mi->rows[b].mode is 1 or 2 and whose temp > 0, INSTEAD of tail-free -> typical -> top-p
 * -> temperature, on the row's kk candidates behind the penalties (bias, mask) and top-k in the project's order (descending penalised logit, ascending id among equals).
 * fp32, IEEE operations, no contraction; sums SEQUENTIAL in index order from 0.0f; expf, logf, log2f, powf:
 *   1. TEMPERATURE FIRST: l_i = logit_i / temp, a division per candidate (sample_temperature).  p = SOFTMAX(the kk) as rule 1 of the stages above.
 *   2. MODE 1.  nt = min(m - 1, kk - 1) terms (m - 1 < 0: kk - 1, as the reference's size_t(m - 1)); t_i = logf(float(i + 2) / float(i + 1)), b_i = logf(p_i / p_{i+1});
 *      A = sum t_i * b_i, B = sum t_i * t_i (one multiply and one add per term); s_hat = A / B; eps = s_hat - 1; N = float(call->vocab);
 *      k_f = powf((eps * powf(2, mu)) / (1 - powf(N, -eps)), 1 / s_hat).  The first k' candidates are kept, where C leaves int(k_f) open the project's rule:
 *      !(k_f >= 1) (NaN included) -> 1; k_f >= kk (+inf included) -> kk; otherwise int(k_f), truncated.  kk == 1 (or m == 1): no term, s_hat NaN, k' = 1.
 *   3. MODE 2.  k' = the first i with -log2f(p_i) > mu, or kk where there is none.
 *   4. final p = SOFTMAX(the first k'); the inverse-CDF draw on the row's uniform (Philox as tce_sample_f16's, or uniform_override): the first i with u < cdf_i, else k' - 1.
 *   5. UPDATE, in the tail that stores the token: mu = mu - eta * ((-log2f(final p of the candidate drawn)) - tau).  mu is written whenever a token is emitted, a stop token
 *      or the row's last token included; it is NOT touched where nothing is emitted: an inactive row, constraint rule 6.  A NaN mu stays NaN (mode 2 then keeps all kk).
 *   6. temp <= 0: greedy as everywhere, mu untouched.  mode 0 (and any value but 1 and 2: the row lives on the device, the host cannot refuse it at the call): the row is
 *      tce_sample_stages_f16's row bit for bit -- token, log, ring, counters, position, debug and stage records, logprob, constraint state --, mu untouched.  A mirostat
 *      row ignores its tce_stage_row and top_p; its stage record shows kk candidates in sorted order.
 * DEVIATIONS from the reference, all three deliberate:
 *   a. CANDIDATES.  The reference's mirostat sees the WHOLE vocabulary and ignores top_k; here it sees the row's top_k <= 256 candidates, like every rule of this sampler
 *      (N stays the vocabulary).  The two are the same chain whenever vocab <= top_k (tests/golden/mirostat_golden.npz holds such configurations).
 *   b. EMPTY CUT.  Mode 2 with -log2f(p_0) > mu keeps ONE candidate; the reference would set size 0 and read an empty array.
 *   c. mu IS PER SLOT and starts at 2 * tau, written by the host at admission; the reference's function-static mu, which leaks from one generate call into the next, is
 *      not reproduced.
 * mi->rows: DEVICE array [batch] of tce_mirostat_row (20 bytes): a slot changes hands by one stream-ordered copy, a captured graph keeps the pointer: no recapture.
 * mi->debug (may be NULL): [batch] records for tests, written for every row that emits (mode 0 for a row that ran no mirostat: kept = n, mu_in = mu_out, the rest 0).
 * With it, tce_sample_debug keeps its meaning: ids / logit the sorted penalised candidates (before the division), p the softmax of rule 1, n = k', final_p of rule 4.
 * Launches: two; the first is the underlying form's own kernel, the second the MIRO = true form of the draw kernel, whose branch is uniform per workgroup.
 * Refusals, before any launch: tce_sample_stages_f16's -- call->mirostat != 0 included: the mode lives per row --; TCE_ERR_BAD_ARG for a NULL mi or mi->rows;
 * TCE_ERR_UNSUPPORTED_SHAPE for rows or debug not 4-byte aligned.
 * powf: the device evaluates each of rule 2's three powers as the fp64 pow of the widened fp32 operands, rounded once to fp32 -- within one fp32 ulp of the exact
 * value, with pow's special cases (the device library's fp32 powf compiles to an instruction form this library's build refuses).
 * tce_sample_verify_mirostat_f16: tce_sample_verify_stages_f16 (with lp / c: its logprob / constrained form) with mi->rows per SEQUENCE and mi->debug per VIRTUAL row
 * (written for the rows of sequences that run mirostat only; tce_sample_debug and the stage record are NOT written for those rows).  mu at virtual row t depends on the
 * draws of rows < t, so the per-row draw launch cannot finish a mirostat sequence: it stops such a row behind the sort and leaves the sorted candidates in the
 * workspace; ONE ADDED LAUNCH, one workgroup per sequence, walks the sequence's active rows t = 0, 1, ... with mu carried -- the same device function the plain entry
 * point runs, on the uniform keyed (seed, generated + t) (uniform_override: per virtual row) -- and writes the row's token and the mu behind it; the chain launch emits
 * as the verifier does and stores the mu behind the LAST token it emits.  FOUR launches, no host round trip.  LOSSLESS: the emitted tokens, generated, ring, position,
 * constraint state, logprobs and the stored mu are those of tce_sample_mirostat_f16 called once per emitted token; a sequence that emits nothing keeps its mu.  Sequences
 * in mode 0 and greedy sequences are tce_sample_verify_stages_f16's.  workspace: tce_sample_verify_mirostat_workspace_bytes(batch, rows_per_seq, vocab) bytes (the
 * verifier's, then 2064 bytes per virtual row), zeroed once.  Refusals: tce_sample_verify_stages_f16's and tce_sample_mirostat_f16's.
 * NOT BUILT, as before: top_k <= 0 = "whole vocabulary", k > 256. */
typedef struct tce_mirostat_row { int32_t mode; int32_t m; float tau, eta, mu; } tce_mirostat_row;   /* per slot (20 bytes); the reference's defaults: m 100, tau 5, eta 0.1 */
typedef struct tce_mirostat_debug {   /* tests; per row; 40 bytes.  An inactive or rule-6 row writes nothing */
    int32_t mode, kk;                 /* the mode that RAN (0: none; a greedy row too); the candidates behind top-k */
    float s_hat, k_f;                 /* mode 1 only (else 0) */
    int32_t kept;                     /* k' */
    float mu_in, mu_out, surprise;    /* surprise = -log2f(final p of the candidate drawn) (0 where no mirostat ran) */
    int32_t choice;
    float final_p;                    /* of the candidate drawn (0 for a greedy row) */
} tce_mirostat_debug;
typedef struct tce_sample_mirostat { tce_mirostat_row *rows; tce_mirostat_debug *debug /* may be NULL */; } tce_sample_mirostat;
TCE_API int tce_sample_mirostat_f16(const tce_sample_call *call, const tce_sample_stages *st, const tce_sample_mirostat *mi, const tce_constraint *c /* may be NULL */,
                                    const tce_logprob_out *lp /* may be NULL */, void *stream);
TCE_API size_t tce_sample_verify_mirostat_workspace_bytes(int batch, int rows_per_seq, int vocab);
TCE_API int tce_sample_verify_mirostat_f16(const tce_sample_verify_call *call, const tce_sample_stages *st, const tce_sample_mirostat *mi,
                                           const tce_constraint *c /* may be NULL */, const tce_logprob_out *lp /* may be NULL */, void *stream);
/* The next step's input rows, one launch: row token[b] of an fp16 table [vocab][hidden] into out[b] ([batch][hidden]) for every active row (pos_device / pos_bound as
 * above; inactive rows are left as they are).  The reference looks an fp32 table up and rounds with float2half (Int4llamaDecoder: Embedding + float2half); a table
 * rounded once to fp16 gives the same bits.  A token outside [0, vocab) is not followed: the row is written as zeros and word 0 of `workspace` (tce_sample_f16's, or
 * any zeroed uint32) is incremented.  hidden % 8 == 0, 16-byte aligned table and out. */
TCE_API int tce_embed_rows_f16(const void *table, int vocab, int hidden, const int32_t *token, void *out, int batch, const int32_t *pos_device, int pos_bound,
                               void *workspace, void *stream);
/* Multi-LoRA: per-row fp16 adapters beside a W4A16 linear (csrc/lora.hip; additive within ABI 113, no existing struct or entry point changes).  The base weights are
 * packed int4, so a LoRA delta cannot be merged into them: an adapted linear y = W4A16(x) ([rows][K] -> [rows][N]) is the base launch plus these two.  A pool holds
 * n_adapters adapters of padded rank R (a smaller rank is zero-padded), all on the DEVICE:
 *     A      fp16 [n_adapters][R][K] row-major        B      fp16 [n_adapters][R][N] row-major        scale  fp32 [n_adapters] (alpha / r)
 *     row_adapter  int32 [rows]: the adapter of row i, READ WHEN THE KERNEL RUNS (a captured graph follows a word that the host rewrites, stream-ordered)
 * tce_lora_shrink_f16      t[i][j] = sum_k x[i][k] * A[a][j][k], a = row_adapter[i]; t fp32 [rows][R], never rounded to fp16.  Products and sums in fp32 (an
 *                          fp16 * fp16 product is exact there), one fmaf per element; the summation order is fixed by the kernel and depends on K ALONE: not on the
 *                          row, its index in the launch, `rows`, or the other rows' words.
 * tce_lora_expand_add_f16  C[i][n] = fp16(float(C[i][n]) + scale[a] * sum_j t[i][j] * B[a][j][n]), IN PLACE on what the base linear has just written (under
 *                          TCE_W4_ADD_TO_C: the residual stream it has just added into).  j ascends, one fmaf per step in fp32, then fmaf(scale, sum, float(C)) and ONE
 *                          rounding to fp16.
 * A row whose word lies outside [0, n_adapters) -- -1 is "no adapter" -- is left untouched: C[i] keeps its bits, nothing of the pool is read for it, t[i] is not written.
 * No floating-point atomics: a row's result bits depend only on that row's x, that row's C and its adapter's contents.  Rows that share an adapter share its read
 * within a block of 4 rows (across blocks it comes from the L2); nothing is sorted on the host.
 * Refusals, before any HIP call, arguments before shapes: TCE_ERR_BAD_ARG for a NULL pointer, rows / K / N / R / n_adapters < 1, ldx < K, ldc < N;
 * TCE_ERR_UNSUPPORTED_SHAPE for K, N, ldx or ldc not a multiple of 8, R not a multiple of 8 or above TCE_LORA_MAX_RANK, n_adapters above TCE_LORA_MAX_ADAPTERS, more than
 * 262140 rows, x / A / B / C not 16-byte aligned, t / scale / row_adapter not 4-byte aligned.
 * Gate / up.  The decode path runs gate, up and SiLU * mul as ONE launch (TCE_W4_SILU_MUL_PAIRS), and a delta has to land in front of the nonlinearity.  An adapted
 * gate/up is three launches: tce_lora_shrink_f16 on the shared input with gate's and up's A stacked (rows 0 .. R-1 gate's, R .. 2R-1 up's: t fp32 [rows][2R]); the
 * base gate_up linear WITHOUT the pair flag (y fp16 [rows][2N], column 2n = gate n, column 2n + 1 = up n); and
 * tce_lora_expand_silu_mul_f16   Bg, Bu fp16 [n_adapters][R][N]; y with row stride ldy, only read; C fp16 [rows][N] with row stride ldc.  For a row whose word a lies in
 *                          [0, n_adapters):  g = fp16(fmaf(scale[a], sum_{j<R} t[i][j] * Bg[a][j][n], float(y[i][2n]))),
 *                                            u = fp16(fmaf(scale[a], sum_{j<R} t[i][R + j] * Bu[a][j][n], float(y[i][2n+1])))
 *                          (j ascends, one fmaf per step in fp32 from +0: tce_lora_expand_add_f16's order); any other word: g = y[i][2n], u = y[i][2n+1], and nothing of
 *                          the pool or of t is read.  EVERY row below `rows` then gets C[i][n] = silu_mul_half(g, u), the pair epilogue's function.  The sums are
 *                          SEGMENTED (gate's walk gate's R rows, up's walk up's: no zero block is read) and bit-identical, for finite t, to tce_lora_expand_add_f16 on y
 *                          with the block-structured B' [2R][2N] followed by tce_silu_mul_half on the de-interleaved columns.  No atomics; a row's bits depend only on
 *                          that row's y and t and its adapter; rows of one 4-row block that share an adapter share one read of Bg and Bu.
 *                          Refusals as above: TCE_ERR_BAD_ARG for a NULL pointer, rows / N / R / n_adapters < 1, ldy < 2 N, ldc < N, C overlapping y;
 *                          TCE_ERR_UNSUPPORTED_SHAPE for N, ldy or ldc not a multiple of 8, R not a multiple of 8, 2 R above TCE_LORA_MAX_RANK, n_adapters above
 *                          TCE_LORA_MAX_ADAPTERS, more than 262140 rows, Bg / Bu / y / C not 16-byte aligned, t / scale / row_adapter not 4-byte aligned.
 * Speculative rows need nothing here: the T rows of a slot carry the slot's word (row_adapter int32 [batch * T], written by the host).
 * NOT BUILT: a segmented expand for a fused q/k/v (its B is block-structured with zeros off the blocks), an MFMA shrink for long prefills, quantised adapters, adapters on
 * lm_head and the embedding. */
#define TCE_LORA_MAX_RANK     192   /* padded rank R of a pool: 8 .. 192 in steps of 8 (a fused q/k/v at r = 64) */
#define TCE_LORA_MAX_ADAPTERS 64    /* adapters resident in one pool */
TCE_API int tce_lora_shrink_f16(const void *x, int ldx, const void *A, const int32_t *row_adapter, float *t, int rows, int K, int R, int n_adapters, void *stream);
TCE_API int tce_lora_expand_add_f16(const float *t, const void *B, const float *scale, const int32_t *row_adapter, void *C, int ldc, int rows, int N, int R, int n_adapters,
                                    void *stream);
TCE_API int tce_lora_expand_silu_mul_f16(const float *t, const void *Bg, const void *Bu, const float *scale, const int32_t *row_adapter, const void *y, int ldy, void *C,
                                         int ldc, int rows, int N, int R, int n_adapters, void *stream);
/* Reads [ptr, ptr + bytes) with at most `workgroups` workgroups (0 = as many as the range needs) and discards the data: the
 * range then sits in the memory-side cache (256 MiB) for the launch that needs it.  Meant for a side stream / graph branch
 * next to the launch BEFORE that one (no reference counterpart: cudaMallocManaged prefetching is the closest idea). */
TCE_API int tce_prefetch(const void *ptr, long long bytes, int workgroups, void *stream);
TCE_API int tce_add_half(const void *a, const void *b, void *c, long long n, void *stream);
/* RMSNorm as the reference's CUDA build computes it (generalT5LayerNorm, llm/src/ops/cuda/LlamaRMSNorm.cu:68-115):
 *   out[r][i] = half( clamp( (float(x[r][i]) * rs_r) * gamma[i] ) ),  rs_r = 1 / sqrt(mean_i x[r][i]^2 + eps), fp32,
 *   clamp to +-(65504 - 1000).  x, out fp16 [m][n]; gamma fp32 [n]; n % 8 == 0.
 * A descriptor with rmsnorm_gamma set has that normalisation applied to its (un-normalised) activation while it is staged
 * -- input_layernorm + q/k/v, post_attention_layernorm + gate/up (Int4llamaDecoderLayer.cu:78, 92-99) as one launch each;
 * M = 1 (decode) only; the linears of a group share gamma and eps like they share A.  Works in tce_w4a16_forward,
 * tce_w4a16_forward_group and plans.  tce_w4a16_forward_group_rmsnorm is the same call with gamma / eps passed separately
 * (the descriptors' own rmsnorm fields are ignored). */
TCE_API int tce_rmsnorm_half(const void *x, const float *gamma, void *out, int m, int n, float eps, void *stream);
TCE_API int tce_w4a16_forward_group_rmsnorm(const tce_w4a16_desc *descs, int count, const float *gamma, float eps, void *stream);
TCE_API int tce_silu_mul_half(void *a, const void *b, long long n, void *stream);

/* Load-time helper for TCE_W4_ZERO_POINT_IS_8: returns 1 if all `n_words` packed zero-point words are 0x88888888, 0 if
 * not, negative on error.  Synchronous; call it once per weight tensor (weights are immutable after loading). */
TCE_API int tce_w4a16_check_zero_point_8(const void *zeros, long long n_words);
/* The same check WITHOUT a synchronisation (round 5; what the C++ adapter uses inside gemv_forward_cuda, whose contract is "asynchronous, never syncs" --
 * kernels/cuda/gemv_cuda.cu:237-251): enqueues one kernel on `stream` that writes 1 (every word is 0x88888888) or 2 (not) to *verdict when it has run.
 * `verdict` must be a word the device can write and the host can read without a copy -- tce_host_alloc memory -- and should be 0 on entry; the caller polls it
 * with plain loads.  Returns after the launch. */
TCE_API int tce_w4a16_check_zero_point_8_async(const void *zeros, long long n_words, int *verdict, void *stream);

/* Load-time re-layout for the prefill GEMM ("offline pre-swizzle to an MFMA-friendly tile layout"; no reference
 * counterpart -- the reference re-runs its GEMV M times).  tce_w4a16_prepack reads qweight / scales / zeros (+ strides) of `d`
 * (q4_6 as loaded from weight_int4.bin / scaling_factor_int4.bin / zero_point_int4.bin; A, C, M are ignored) and writes the
 * q4_mfma copy (csrc/w4a16_mfma_layout.hpp: 16-row x 128-k tiles in MFMA fragment order, nibbles ordered for a 9-instruction
 * exact unpack, per-group effective scales and zero-point constants) into `packed`, which must hold
 * tce_w4a16_prepack_bytes(N, K, group_size) bytes of device memory (0 = shape not supported: K % 128 != 0).  Asynchronous on
 * `stream`; once per weight tensor.  A descriptor whose `prepacked` points at that copy lets tce_w4a16_forward run the 128-row
 * MFMA kernel (csrc/w4a16_gemm_pk.hip) for M > 128 (where its cost model beats the 64-row kernel's); results stay within the W4A16 tolerance of every other path. */
TCE_API size_t tce_w4a16_prepack_bytes(int N, int K, int group_size);
TCE_API size_t tce_w4a16_gemm_scratch_bytes(void); /* size of tce_w4a16_desc.scratch (32 MiB + 4 KiB) */
/* (0.1.11) Exchanges between workgroups on `scratch` that gave up waiting, counted since the area was last zeroed: synchronises `stream`, copies one word.  0 is the only
 * value ever observed; non-zero means some outputs computed with this area since hold NaN (never a plausible wrong number) and the area stays poisoned until its first
 * 4096 bytes are zeroed again.  A host that keeps a scratch area for a long time calls this where it synchronises anyway (the adapter: at teardown and on request). */
TCE_API int tce_w4a16_gemm_scratch_faults(const void *scratch, void *stream, uint32_t *faults);
TCE_API int tce_w4a16_prepack(const tce_w4a16_desc *d, void *packed, void *stream);

/* ONE packed copy for `count` (<= TCE_MAX_GROUP) linears that are always launched together (q/k/v; gate, up).  The copy is, byte for byte, what
 * tce_w4a16_prepack writes for the row-concatenated linear (rows of descs[0], then descs[1], ...): words, then scales, then zero points.  Valid when every member
 * shares K and the group size and every member's N is a multiple of 16 (so that no 16-row tile holds rows of two members); otherwise _bytes returns 0 and
 * tce_w4a16_prepack_group TCE_ERR_UNSUPPORTED_SHAPE, and the caller keeps individual copies.  `packed`: tce_w4a16_prepack_group_bytes(descs, count) bytes, 256-byte aligned.
 * A member's descriptor then carries `prepacked` = the copy's base, `reserved` = its first 16-row tile inside the copy (the rows in front of it / 16) and `reserved2` =
 * the copy's rows (the sum of the members' N).  Every entry point that reads `prepacked` takes such a descriptor: it addresses the member's slice, which holds the
 * bytes of the member's own copy -- same results, bit for bit.  tce_w4a16_forward_group / _group_rmsnorm (and plans) given the members of ONE copy in the copy's order,
 * without a gap, launch them as one linear on it: no per-linear addressing in front of the weight requests (csrc/w4a16_gemv_i8.hip).  Any other member list runs as
 * a group of individual linears. */
TCE_API size_t tce_w4a16_prepack_group_bytes(const tce_w4a16_desc *descs, int count);
TCE_API int tce_w4a16_prepack_group(const tce_w4a16_desc *descs, int count, void *packed, void *stream);

/* count (<= TCE_MAX_GROUP) linears with identical M, K, group_size and A/lda, one launch (GEMV path only). */
#define TCE_MAX_GROUP 4
TCE_API int tce_w4a16_forward_group(const tce_w4a16_desc *descs, int count, void *stream);
/* (0.1.12) count (<= TCE_MAX_INDEPENDENT) decode linears that share NOTHING -- each its own activation, K, N, epilogue flags -- as ONE launch.  For the column-sharded
 * model (the one-gather-per-block form): a rank's q / k / v / o / gate / up / down shards of a block read replicated inputs and do not depend on each
 * other; one by one they are launches of 1-6 MB at 8 ranks, each paying a full launch boundary.  No ordering among the linears of the call is implied or provided (a
 * linear that reads another one's output belongs in a later call).  Every output is bit-identical to the same descriptor through tce_w4a16_forward.
 * One launch when every linear has M = 1, group_size 128, K <= 16384, a packed copy (`prepacked`) and no RMSNorm prologue (csrc/w4a16_gemv_i8.hip, the mixed launch);
 * otherwise the linears are issued one after the other on `stream` -- same results.  *launches (may be null) receives the number of kernel launches made. */
#define TCE_MAX_INDEPENDENT 8
TCE_API int tce_w4a16_forward_independent(const tce_w4a16_desc *descs, int count, int *launches, void *stream);
/* How tce_w4a16_forward_independent would run `descs` (no launch, no HIP call): "gemv-i8-mixed waves=<per workgroup> workgroups=<n>" -- one launch -- or
 * "one-by-one launches=<count>". */
TCE_API int tce_w4a16_describe_independent(const tce_w4a16_desc *descs, int count, char *buf, int buf_len);

/*
 * AWQ "CUDA GEMM" (q4_5) layout -- quantize_methods.py:299-368, kernels/cuda/matmul_int4.cu:19-39:
 *   qweight u32 [K][N/8], nibbles 0..7 of word j hold n = 8j + {0,2,4,6,1,3,5,7}; scales fp16 [K/G][N];
 *   zero point fixed 8.  tce_w4a16_awq_fp16acc reproduces naive_mat_mul_fp16_int4 bit-for-bit
 *   (every operation rounded to binary16, sequential over k).  tce_w4a16_gemm_awq is the fast path
 *   (fp32 accumulate): `workspace` must hold tce_w4a16_awq_workspace_bytes(N,K,G) bytes and receives the
 *   q4_6 re-layout of the weights (pass the same workspace again with repack=0 to skip the re-layout).
 */
TCE_API int tce_w4a16_awq_fp16acc(int M, int N, int K, int group_size, const void *A, const void *qweight,
                                  const void *scales, void *C, void *stream);
TCE_API size_t tce_w4a16_awq_workspace_bytes(int N, int K, int group_size);
TCE_API int tce_w4a16_gemm_awq(int M, int N, int K, int group_size, const void *A, const void *qweight,
                               const void *scales, void *C, void *workspace, int repack, void *stream);

/*
 * W8A8 (SmoothQuant) -- kernels/ref/matmul_ref_int8.cc.  A int8 [M][K]; B int8 [N][K] (K contiguous;
 * matmul_params.B.row = K, B.column = N -- llm/src/ops/W8A8B8O8Linear.cc:47-50); acc int32 exact.
 *   out_kind TCE_OUT_INT8: C int8 [M][N] = clamp( (int32) round( (float)acc*alpha [+ (float)bias_i8[n]*beta] ), q_min, q_max )
 *            (round = half away from zero; multiply, multiply, add each rounded separately -- :29-32)
 *   out_kind TCE_OUT_FP32: C fp32 [M][N] = (float)acc*alpha [+ bias_f32[n]]          (:108, :132)
 *   b_per_row != 0: row i of A multiplies its own B_i, B laid out [M][N][K] (the *_batch variants, :79, :153); batch must be 1 (TCE_ERR_UNSUPPORTED_KIND otherwise)
 *   batch > 1: `batch` independent problems at element strides strideA/strideB/strideC (the per-head loop of
 *            llm/src/ops/BMM_S8T_S8N_F32T.cc:45-59 / BMM_S8T_S8N_S8T.cc:47-60 as one launch).
 */
#define TCE_BIAS_NONE 0
#define TCE_BIAS_INT8 1
#define TCE_BIAS_FP32 2
#define TCE_OUT_INT8 0
#define TCE_OUT_FP32 1

typedef struct tce_w8a8_desc {
    int32_t M, N, K;
    int32_t batch;        /* >= 1 */
    const void *A;
    const void *B;
    const void *bias;     /* int8 [N] or fp32 [N] or NULL */
    void *C;
    int64_t strideA, strideB, strideC; /* elements between consecutive batch entries (ignored when batch == 1) */
    float alpha, beta;
    int32_t q_min, q_max; /* C.qparams.q_min/q_max: -128..127, or 0..127 for the fused-ReLU linear (W8A8B8O8LinearReLU.cc:32) */
    int32_t bias_kind, out_kind;
    int32_t b_per_row;
    int32_t accumulate;   /* TCE_OUT_FP32 only: C[m][n] = C[m][n] + result, one more rounding -- the residual add the reference issues behind out_proj / fc2
                             (`add`, llm/src/nn_modules/Int8OPTDecoderLayer.cc:14-22, 39, 54) in the same launch; bit-exact against the two-step form */
    int32_t lda, ldb, ldc; /* row strides in elements, 0 = dense (K, K, N): a head's 64-column slice of a [rows][heads * 64] projection output is an
                             operand as it lies (strideA = 64, lda = heads * 64), a cache with room for max_keys keys likewise; b_per_row with
                             batch == 1 and strideB != 0: the per-row B_m are strideB elements apart */
    int32_t reserved2;
} tce_w8a8_desc;

TCE_API int tce_w8a8_matmul(const tce_w8a8_desc *d, void *stream);
/* size-prefixed form (0.1.10), as tce_w4a16_desc_v2 */
typedef struct tce_w8a8_desc_v2 {
    uint32_t struct_size;
    uint32_t reserved0;
    tce_w8a8_desc desc;
    void *scratch;  /* NULL = none.  tce_w8a8_scratch_bytes() bytes of device memory, 256-byte aligned, its first 4096 bytes ZEROED once by the caller (every call leaves
                       them zero): lets a launch with few 64 x 64 tiles and a long k chain (OPT's fc2 at prefill: 512 x 768 x 3072 is 96 tiles of 48 steps on 256 CUs) cut
                       the chain into runs on several workgroups; the int32 partial tiles are added exactly, in any order -- the result stays bit-exact.  One area per
                       stream that runs such calls concurrently */
} tce_w8a8_desc_v2;
TCE_API int tce_w8a8_matmul_v2(const tce_w8a8_desc_v2 *d, void *stream);
TCE_API size_t tce_w8a8_scratch_bytes(void);

/* The element-wise steps between the two int8 BMMs of the reference's OPT attention (llm/src/nn_modules/Int8OPTAttention.cc:254-268), as ONE launch:
 *   batch_Add (llm/src/ops/batch_add.cc:3-24): s[h][j][k] + mask[j][k];  softmax over k (llm/src/ops/softmax.cc:5-40: the running maximum starts
 *   from `m_data[0]` -- element [0][0][0] of the tensor the reference normalises IN PLACE, i.e. the masked score for row (0, 0) and that row's first
 *   probability for every later row --, exponentials summed in k order in fp32, the quotient formed in double: exp / (sum + 1e-10));
 *   attn_probs_int8 = (int8) std::round(p * 127)  (:266).
 * scores fp32 [heads][sq][tgz] (the qk BMM's output), mask fp32 [sq][tgz], probs int8 [heads][sq][ld_probs] (ld_probs 0 = tgz; a multiple of 16
 * lets the pv BMM take its vector path).  Same operations in the same order; the device's expf may differ from the host's in the last bit. */
TCE_API int tce_opt_softmax_q(const float *scores, const float *mask, void *probs, int heads, int sq, int tgz, int ld_probs, void *stream);
/* The KV append of Int8OPTAttention::forward (:205-236; the reference copies the whole past into the other cache buffer per token): the new
 * key / value rows k, v int8 [sq][heads * hd] (k_proj / v_proj outputs as they lie) go to rows [pos, pos + sq) of k_cache [heads][max_keys][hd]
 * and, TRANSPOSED (the pv BMM's operand, :271-273 without the per-token transpose of the whole cache), to columns [pos, pos + sq) of
 * vt_cache [heads][hd][max_keys]. */
TCE_API int tce_opt_kv_append(const void *k, const void *v, void *k_cache, void *vt_cache, int heads, int hd, int sq, int pos, int max_keys, void *stream);
/* The whole OPT attention of a DECODE step (m <= 8 new rows) between the q/k/v projections and out_proj as ONE launch (csrc/opt_attention.hip): the KV append
 * of tce_opt_kv_append, the qk BMM (BMM_S8T_S8N_F32T.cc:12-62), tce_opt_softmax_q and the pv BMM (BMM_S8T_S8N_S8T.cc:12-63, clamp -128 .. 127) -- int32 dot
 * products and the same floating-point operations in the same order, so `out` and both caches are bit-identical to the four separate launches.
 *   q, k_new, v_new  int8 [m][ld]: the projections' output rows (head h: columns h * hd ..; ld 0 = heads * hd)
 *   k_cache int8 [heads][max_keys][hd], vt_cache int8 [heads][hd][max_keys]: rows / columns pos .. pos + m - 1 are written
 *   mask fp32 [m][pos + m] additive;  out int8 [m][ld]: head h writes its hd columns (out_proj's input rows)
 * hd == 64 (OPT-125M / 1.3B) or 128 (OPT-6.7B), m <= 8, ld and max_keys multiples of 16. */
TCE_API int tce_opt_attention_decode(const void *q, const void *k_new, const void *v_new, void *k_cache, void *vt_cache, const float *mask, void *out, int heads,
                                     int head_dim, int m, int pos, int max_keys, int ld, float alpha_qk, float alpha_pv, void *stream);

/* LayerNormQ::forward (llm/src/ops/LayerNormQ.cc:12-52), the op in front of the W8A8 linears: x fp32 [m][n],
 * weight / bias fp32 [n], out int8 [m][n] = (int8) round((x - mean) / sqrt(var + 1e-5) * weight + bias), sums sequential
 * in fp32 exactly like the reference loop: BIT-EXACT.  n % 4 == 0, n <= 8192. */
TCE_API int tce_layernorm_q(const float *x, const float *weight, const float *bias, void *out, int m, int n, void *stream);

/* LayerNormQ and the int8 linears that read its output as ONE launch, for decode: replaces
 *   self_attn_layer_norm.forward + q_proj / k_proj / v_proj.forward   (llm/src/nn_modules/Int8OPTAttention.cc:186-201 behind LayerNormQ.cc:12-52)
 *   final_layer_norm.forward + fc1.forward                             (LayerNormQ + W8A8B8O8LinearReLU)
 * x fp32 [m][k] (m <= 8), ln_weight / ln_bias fp32 [k]; `linears[i]` (count <= TCE_MAX_GROUP) describe the consumers exactly as for
 * tce_w8a8_matmul with M = m, K = k, batch = 1, b_per_row = 0 -- their `A` is ignored (it is the normalised row, which never
 * leaves the chip unless ln_out, int8 [m][k], is given).  BIT-EXACT against tce_layernorm_q followed by tce_w8a8_matmul (and so
 * against the reference).  k % 16 == 0. */
TCE_API int tce_layernorm_q_w8a8_group(const float *x, const float *ln_weight, const float *ln_bias, int m, int k, const tce_w8a8_desc *linears,
                                       int count, void *ln_out, void *stream);

/* ---- replayable plan: a fixed sequence of W4A16 launches captured into one hipGraph ---- */
typedef struct tce_plan tce_plan;
/* group_sizes[i] consecutive descriptors form launch i (1 = tce_w4a16_forward, >1 = tce_w4a16_forward_group). */
TCE_API int tce_plan_create(const tce_w4a16_desc *descs, const int32_t *group_sizes, int n_launches, tce_plan **out);
/* TCE_PLAN_TAGGED (TCE_PLAN_CHAINED is accepted as a synonym): ONE persistent kernel walks the whole launch list -- no kernel
 * boundaries, no barriers.  Every output of a launch is ALSO written as one 32-bit word (token tag << 16 | fp16 bits,
 * device-scope store) into a shadow vector the plan owns, and a launch whose activation vector is (a 16-byte-aligned slice
 * of) an output of an earlier launch of the plan polls those words -- the poll is its activation read; its first weight
 * tiles are requested before it starts to wait.  A launch whose activations come from outside the plan reads them at once.
 * What is ordered is therefore the plan's DATA FLOW (and, transitively, everything in front of it), not the launch list as
 * such: launches that do not feed each other may overlap.  Outputs are bit-identical to the stream-ordered plan.
 * Round 6: when the linears carry packed copies (tce_w4a16_prepack) and TCE_W4_ZERO_POINT_IS_8, the walk runs on the int8-contraction body of the decode GEMV
 * (csrc/w4a16_gemv_i8_token.hip; tce_plan_is_chained = 4): the list's longest prefix of M = 1, group-128, K <= 15360 launches goes into ONE kernel, what is left (e.g. a
 * linear with general zero points) follows it as ordinary launches of the same graph.  Bit-identical to the stream-ordered plan; measured level with it (0.976 vs 0.962 ms
 * per Llama-3-8B token, profiles/r6/i8_token_kernel.md) -- opt-in.
 * Not taken (the plan is then built stream-ordered; tce_plan_is_chained tells: 0 stream-ordered, 2 token kernel on the fp16 body, 4 on the int8 body): a launch that
 * is not an M = 1 GEMV the persistent kernel takes; an activation vector that straddles two outputs or starts at an odd
 * 16-byte offset; a launch list in which a launch overwrites memory that an earlier launch reads un-tagged (activations from
 * outside the plan, the old value of TCE_W4_ADD_TO_C) or also writes WITHOUT being downstream of that launch in the data
 * flow -- stream order would protect such a hazard by position, polls do not.  tce_plan_status synchronises the device and returns TCE_ERR_HIP
 * if a wait ever timed out (~0.3 s; cannot happen unless the device is shared with a kernel that never ends).
 * tce_plan_geometry reports what the token kernel runs with (rows per row group, ring depth, waves per workgroup, workgroups).
 * Measured (MI355X, Llama-2-7B-shaped token): the primitive is cheap -- 1.8 us per bare hand-off against 2.0 us for a kernel
 * boundary and 5.0 us for round 1's arrival-counter barrier (scripts/probes/handoff_probe.hip) -- but the token is NOT faster
 * than the stream-ordered graph (1.40 vs 0.995 ms): opt-in, and bench.py picks whichever is faster. */
#define TCE_PLAN_CHAINED 1
#define TCE_PLAN_TAGGED 2
/* TCE_PLAN_OVERLAPPED: the same tagged data flow, but every launch stays a kernel of its own; the launches are issued on two (tunable)
 * alternating graph branches with NO edge between consecutive launches, so launch j+1's workgroups are dispatched, request their first
 * weight steps and poll their activation words while launch j is still running (csrc/w4a16_gemv_ovl.hip).  A launch's grid is capped at
 * 1 / branches of what the chip holds of that kernel, so waiting workgroups cannot keep their producers off the chip.  Same acceptance
 * rules as TCE_PLAN_TAGGED (plus: no fused RMSNorm prologue yet); tce_plan_is_chained returns 3.  Outputs bit-identical to the
 * stream-ordered plan. */
#define TCE_PLAN_OVERLAPPED 4
/* TCE_PLAN_TUNED (stream-ordered plans): the geometry of every decode (M = 1) launch is chosen at plan creation by timing the compiled candidates on this
 * device -- the WHOLE launch list is captured and replayed with one group of same-shaped launches at a time on each compiled candidate, a candidate stays
 * only if the whole plan gets 0.7 % faster; outputs are redirected to a scratch buffer (the caller's buffers are not written).  Costs a second or two, once; results are bit-identical to the
 * untuned plan's (only geometries that keep every row's summation order are candidates). */
#define TCE_PLAN_TUNED 8
/* (0.1.12) TCE_PLAN_INDEPENDENT: every group of the list is a set of linears that share NOTHING (tce_w4a16_forward_independent: group sizes up to
 * TCE_MAX_INDEPENDENT, own activation / K / N / flags per linear) -- a rank's shards of one transformer block in the one-gather-per-block form.  Stream-ordered plan;
 * not combinable with the other flags. */
#define TCE_PLAN_INDEPENDENT 16
TCE_API int tce_plan_create_ex(const tce_w4a16_desc *descs, const int32_t *group_sizes, int n_launches, int flags, tce_plan **out);
TCE_API int tce_plan_is_chained(const tce_plan *plan);
TCE_API int tce_plan_geometry(const tce_plan *plan, int *rows, int *depth, int *waves, int *workgroups);
/* TCE_PLAN_TUNED plans: the geometry that won the timing for launch `launch` -- (rows per wave, waves along N, waves splitting K, pipeline depth) of the
 * row-block GEMV -- or all zero where the dispatcher's own choice stayed (also for untuned plans); depth + 1000 / + 2000: its issue order was forced to
 * activations-first / weights-first (the other knob the timing tries).  The hundreds digit of `depth` is always 0 (it once encoded a knob the kernel no longer has). */
TCE_API int tce_plan_launch_geometry(const tce_plan *plan, int launch, int *rows, int *waves_n, int *waves_k, int *depth);
TCE_API int tce_plan_status(tce_plan *plan);
TCE_API int tce_plan_launch(tce_plan *plan, void *stream);
TCE_API int tce_plan_n_launches(const tce_plan *plan);
TCE_API void tce_plan_destroy(tce_plan *plan);

/* ---- multi-GPU: column shards + peer-write all-gather (no reference counterpart, the reference is single-device) ----
 * One process per GPU.  Every linear is sharded by OUTPUT ROWS: rank r of P computes rows [r*N/P, (r+1)*N/P) from the replicated
 * activation; tce_w4a16_shard fills the shard's descriptor (in q4_6 a row range is one contiguous byte range of qweight, scales and
 * zeros; N % P == 0 and (N / P) % 16 == 0, the reference wrapper's own divisibility rule, linear.cu:16-17); A, C, M, flags and the
 * strides are copied, C must then be pointed at the rank's slice buffer [M][N/P].
 * The slices are joined by tce_allgather_f16: at decode sizes (1-4 KB per rank) a latency-bound exchange, done as ONE small kernel
 * per call that writes the slice into every rank's window over xGMI, publishes an epoch flag, waits for the other ranks' flags
 * and copies the complete vector to `dst_full` (csrc/comm.hip).  The call is asynchronous, stream-ordered and capturable into a
 * hipGraph (epochs are counted on the device).  Every rank must issue the same sequence of calls per slot.
 *   tce_comm_create   rank's window for vectors of up to max_vector_elems halves, `slots` independent exchange slots
 *   tce_comm_export / tce_comm_connect   the host all-gathers the 64-byte handles (MPI, torch.distributed, a file ...) and hands every
 *                     rank the table [world][64]; tce_comm_connect_local instead when all ranks live in one process (tests)
 *                     (ONE host thread driving several devices, the reference's host shape -- Int4llamaForCausalLM.cu:40-44: create each rank's
 *                     communicator with that rank's device current; tce_comm_connect_local enables peer access between the devices, and
 *                     tce_allgather_f16 / tce_comm_status / tce_comm_reset make the communicator's device current for their own calls and restore
 *                     the caller's; the stream passed to tce_allgather_f16 must be a stream of the communicator's device)
 *   tce_comm_status   synchronous: 1 if a wait ever timed out (a rank never arrived within the bound: 2 s, tce_comm_set_timeout_ms), 0 if not,
 *                     negative on error; a flagged communicator's later exchanges do not wait any more (their outputs are void): one lost exchange
 *                     costs one bound, not one bound each.  A host that uses the outputs checks the status (per token, or per batch of tokens).
 *   tce_comm_reset    re-arms a flagged communicator.  Every rank calls it after the host made sure no exchange is in flight anywhere
 *                     (barrier + device synchronisation); the per-slot epochs are kept -- every rank's gather kernels ran to their end.
 *   tce_comm_export refuses a window that is not fine-grained memory (the flags are polled across the link; TCE_ERR_UNSUPPORTED_SHAPE).
 * Prefill (M >= 17) moves megabytes per exchange: use RCCL there (ncclAllGather; this repository's host code does, through
 * torch.distributed) -- the peer-write kernel is a single workgroup. */
typedef struct tce_comm tce_comm;
#define TCE_COMM_HANDLE_BYTES 64
#define TCE_COMM_MAX_RANKS 8
TCE_API int tce_w4a16_shard(const tce_w4a16_desc *full, int rank, int world, tce_w4a16_desc *shard);
TCE_API int tce_comm_create(int rank, int world, int max_vector_elems, int slots, tce_comm **out);
TCE_API int tce_comm_export(tce_comm *comm, void *handle_out /* 64 bytes */);
TCE_API int tce_comm_connect(tce_comm *comm, const void *handles /* [world][64], rank order */);
TCE_API int tce_comm_connect_local(tce_comm *comm, tce_comm *const *all_ranks /* [world] */);
TCE_API int tce_allgather_f16(tce_comm *comm, int slot, const void *src_slice, void *dst_full, int n_total, void *stream);
/* (0.1.12) tce_w4a16_forward_independent with the all-gather of ONE of its linears INSIDE the launch (the one-gather-per-block form as one launch per block:
 * layers + 1 launches per token).  Linear `gathered` of the call is this rank's slice (its N rows; M = 1) of a vector of N * world halves: besides storing the slice at
 * its own C, the tiles that compute it write their 16 values straight into every rank's window, the tile that arrives last publishes this rank's flag, waits for the
 * other ranks' flags and copies the complete vector to `dst_full` -- tce_allgather_f16's protocol, window, buffers, flags and epochs (the two calls may alternate on one
 * slot), without its launch.  Same contract: every rank issues the same sequence of exchanges per slot; a rank that never arrives flags the communicator after the bound
 * (tce_comm_status).  The other linears of the call are not delayed by the exchange (one wave of the launch waits).
 * One launch under tce_w4a16_forward_independent's conditions (+ the gathered linear has no SiLU-mul-pair epilogue, N * world % 8 == 0 and <= 16384, the vector fits the window);
 * otherwise tce_w4a16_forward_independent followed by tce_allgather_f16 -- same results.  *launches (may be null): kernel launches made. */
TCE_API int tce_w4a16_forward_independent_gather(const tce_w4a16_desc *descs, int count, int gathered, tce_comm *comm, int slot, void *dst_full, int *launches, void *stream);
/* Round 4: RCCL behind the same communicator, for exchanges beyond the latency regime (north star: "a single RCCL all-gather over xGMI per transformer block";
 * SURVEY 8e sizes a prompt's exchange at 0.65-1.97 MB per rank).  librccl is opened on first use (dlopen); the communicator is built from an opaque
 * TCE_RCCL_ID_BYTES blob that rank 0 obtains (tce_comm_rccl_unique_id) and the host hands to every rank exactly like the IPC handles (tce_comm_rccl_init is
 * collective: every rank calls it; one rank per device -- RCCL refuses two ranks on one GPU).  tce_allgather_f16 then dispatches by size: slices of at most
 * 64 KiB that fit the window -> the peer-write kernel (one launch, graph-capturable); larger -> ncclAllGather on `stream`.
 *   tce_allgather_rows_f16: the column-sharded outputs of M > 1 rows (a sharded prompt): src fp16 [M][n_total / world] (this rank's columns), dst fp16 [M][ldd]
 *   (ldd = 0: n_total) on every rank.  M = 1 is tce_allgather_f16.  M > 1: the ranks' whole blocks are gathered rank-major into `workspace`
 *   (tce_allgather_rows_workspace_bytes(M, n_total) bytes, 16-byte aligned; peer-write kernel or RCCL by size) and one kernel lays the rows side by side. */
#define TCE_RCCL_ID_BYTES 128
TCE_API int tce_comm_rccl_unique_id(void *id_out /* TCE_RCCL_ID_BYTES */);
TCE_API int tce_comm_rccl_init(tce_comm *comm, const void *id /* TCE_RCCL_ID_BYTES */);
TCE_API size_t tce_allgather_rows_workspace_bytes(int M, int n_total);
TCE_API int tce_allgather_rows_f16(tce_comm *comm, int slot, const void *src, void *dst, int M, int n_total, int ldd, void *workspace, void *stream);
TCE_API int tce_comm_status(tce_comm *comm);
TCE_API int tce_comm_set_timeout_ms(tce_comm *comm, int milliseconds); /* 1 .. 600000; takes effect for exchanges enqueued (or captured) afterwards */
TCE_API int tce_comm_reset(tce_comm *comm);
TCE_API int tce_comm_device(const tce_comm *comm);
TCE_API void tce_comm_destroy(tce_comm *comm);

/* ---- memory / sync helpers: what the L2 wrappers need from the runtime ----
 * tce_malloc(managed=1) / tce_free replace allocate_aligned_memory_gpu / free_aligned_memory_gpu
 * (llm/src/nn_modules/cuda/utils.cu:92-103, cudaMallocManaged there: model files are read straight into that memory,
 * llm/include/common.h:111-120).  managed=0 gives plain device memory (preferred on MI355X; fill it with tce_memcpy).
 * tce_synchronize(NULL) is the per-forward device sync (Int4llamaForCausalLM.cu:40-44 / tests' cudaDeviceSynchronize). */
#define TCE_MEMCPY_H2D 0
#define TCE_MEMCPY_D2H 1
#define TCE_MEMCPY_D2D 2
TCE_API int tce_malloc(void **ptr, size_t bytes, int managed);
TCE_API int tce_free(void *ptr);
/* Pinned, device-mapped, coherent host memory (hipHostMalloc): small words the device writes and the host polls (see tce_w4a16_check_zero_point_8_async). */
TCE_API int tce_host_alloc(void **ptr, size_t bytes);
TCE_API int tce_host_free(void *ptr);
TCE_API int tce_memcpy(void *dst, const void *src, size_t bytes, int kind, void *stream);
TCE_API int tce_synchronize(void *stream);
TCE_API int tce_device_count(void);

/* ---- introspection / tuning (not part of the reference surface) ---- */
TCE_API int tce_version(void);
TCE_API const char *tce_last_error(void);
TCE_API const char *tce_build_info(void);
/* Drops the HIP runtime's sticky last error (and this library's message).  For a host that recovers from a failure of
 * its own -- e.g. a stream capture that was invalidated: the runtime keeps reporting hipErrorStreamCaptureInvalidated as the
 * "last error", and the next launch's check here would return it as TCE_ERR_HIP.  Returns the HIP error code it dropped. */
TCE_API int tce_reset_last_error(void);
/* Which kernel family (and, for the GEMM, which tile and form) tce_w4a16_forward would run for this descriptor, as text:
 * "gemv passes=P kernel=row-block|persistent" | "gemv-i8 rows-per-pass=R group=G" | "small-batch slices=S" | "gemm-pk tile=128xC quartets=Q group=G" |
 * "gemm-dma tile=RxC quartets=Q group=G" | "gemm tile=RxC".  Launches nothing and
 * makes no HIP call (works without a GPU); a shape the chosen GEMM form cannot hold in LDS still falls back at launch time. */
TCE_API int tce_w4a16_describe_dispatch(const tce_w4a16_desc *d, char *buf, int buf_len);
/* (0.1.13) The same for tce_w8a8_matmul / tce_w8a8_matmul_v2 (with_scratch != 0: as if tce_w8a8_desc_v2.scratch were given): "w8a8 wave-per-column rows=M" |
 * "w8a8 wave-per-output (a B per row of A)" | "w8a8 tile=128xC quartets=Q" | "w8a8 k-slice tile=RxC waves=W workgroups=G" (the whole tile in every wave, the k-steps
 * dealt to the waves) | "w8a8 tile=64x64 deep-pipeline quartets=Q" | "w8a8 tile=64x64 quartets=Q [kcut=S]" | "w8a8 tile=32x64 quartets=Q" | "w8a8 generic ...".
 * Operand pointers enter through their 16-byte alignment only (null pointers: aligned).  Launches nothing, makes no HIP call. */
TCE_API int tce_w8a8_describe_dispatch(const tce_w8a8_desc *d, int with_scratch, char *buf, int buf_len);
/* Tuning and diagnostics entry points (forced kernel forms for parity tests and sweeps, per-family setters, the debug buffer): include/tce_tuning.h -- exported by
 * this library, never needed by a host, not part of the operator boundary. */
/* Algorithmic HBM bytes of one tce_w4a16_forward call: N*K/2 + 2*N*K/G + N*K/(2G) + 2*M*K + 2*M*N. */
TCE_API int64_t tce_w4a16_algorithmic_bytes(int M, int N, int K, int group_size);

#ifdef __cplusplus
}
#endif
#endif /* TCE_MATMUL_H */
