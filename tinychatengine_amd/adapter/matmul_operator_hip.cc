// matmul_operator_hip.cc -- matmul::MatmulOperator members for a QM_HIP build of TinyChatEngine, on top of the C ABI
// of libtce_hip.so (include/tce_matmul.h).  This is the only C++-mangled layer; it is plain host code (g++ or hipcc).
//
// Behavioural contract kept from the reference:
//   * each member reads ONLY the matmul_params fields the corresponding reference member reads (the L2 wrappers leave
//     the rest of the struct uninitialised -- llm/src/ops/cuda/linear.cu:19-33);
//   * work is enqueued on the null stream and the call returns without synchronising
//     (kernels/cuda/gemv_cuda.cu:237-251; the only sync is once per forward, Int4llamaForCausalLM.cu:40-44);
//   * failures print a message and exit(1), which is what the reference does for an unsupported group size
//     (gemv_cuda.cu:254-256); its asserts become the same exit path.
#include "tce_matmul_operator.h"

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "tce_matmul.h"

namespace {

[[noreturn]] void die(const char *who, int rc) {
    std::printf("%s: %s (tce error %d)\n", who, tce_last_error(), rc);
    std::exit(1);
}

// The descriptors are plain structs without a size field: an adapter compiled against one header revision and a libtce_hip.so built from another
// would hand structs of the wrong layout across the boundary.  Checked once, when the adapter library is loaded; the failure is loud.
const int g_abi_checked = [] {
    if (tce_version() != TCE_VERSION) {
        std::printf("libtce_matmul_operator: libtce_hip.so reports ABI version %d, this adapter was compiled against %d (include/tce_matmul.h): rebuild both\n", tce_version(), TCE_VERSION);
        std::exit(1);
    }
    return 1;
}();

// Per-tensor state the stateless reference operator does not have ("the HIP shim may keep an internal cache keyed
// by weight pointer").  Both caches are hash maps keyed by the tensor's identity AS THE CALL DESCRIBES IT -- pointer AND shape
// (a different N / K / group at a recycled address is a different key, never a stale hit) -- guarded by one mutex, with no
// capacity cliff.  A host that frees or overwrites model buffers tells the adapter: tce_adapter_forget(ptr) (called by the
// free_aligned_memory_gpu of INTEGRATION.md 2.4) or tce_adapter_forget_all().  Same pointer + same shape + different CONTENTS
// without that call is the one case the adapter cannot see; model weights are immutable after loading in the reference
// (Linear_half_int4's constructor is the only writer, llm/include/ops/linear.h:215-240).
struct TensorKey {
    const void *ptr;
    long long a, b, c;  // shape words (zeros: n_words, 0, 0; AWQ weights: N, K, G)
    bool operator==(const TensorKey &o) const { return ptr == o.ptr && a == o.a && b == o.b && c == o.c; }
};
struct TensorKeyHash {
    size_t operator()(const TensorKey &k) const {
        size_t h = std::hash<const void *>()(k.ptr);
        for (long long v : {k.a, k.b, k.c}) h ^= std::hash<long long>()(v) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
        return h;
    }
};
struct AwqEntry {
    void *workspace = nullptr;  // q4_6 re-layout of a q4_5 tensor (tce_w4a16_gemm_awq) / q4_mfma copy of a q4_6 linear
    size_t bytes = 0;
    const void *scales = nullptr, *zeros = nullptr;  // packed copies: the side tensors the copy was built from (it embeds them)
};
std::mutex g_mu;
std::unordered_map<TensorKey, AwqEntry, TensorKeyHash> g_awq;   // AWQ weight tensor -> re-laid-out copy
std::unordered_map<TensorKey, AwqEntry, TensorKeyHash> g_pack;  // q4_6 weight tensor -> q4_mfma copy (decode GEMV M <= 4, prefill GEMM M >= kPackMinM)
constexpr int kPackMinM = 129;
std::atomic<uint64_t> g_generation{1};  // bumped by tce_adapter_forget* and by a re-pack: un-publishes every entry of the lock-free front cache below

// The q4_mfma copy of a linear, built on first sight of a large batch (the reference's Linear_half_int4 has no load-time hook
// the adapter could use: its constructor only reads files, llm/include/ops/linear.h:215-240).  Enqueued on the null stream in
// front of the GEMM that needs it, so no synchronisation; costs one extra copy of the int4 weights in HBM.
const void *packed_copy(const tce_w4a16_desc &d) {
    const size_t need = tce_w4a16_prepack_bytes(d.N, d.K, d.group_size);
    if (need == 0) return nullptr;
    std::lock_guard<std::mutex> lk(g_mu);
    AwqEntry &e = g_pack[TensorKey{d.qweight, d.N, d.K, d.group_size}];
    const bool fresh = !e.workspace;
    if (fresh) {
        if (tce_malloc(&e.workspace, need, /*managed=*/0) != TCE_OK) {  // no memory for the copy: the other kernels take the call
            e.workspace = nullptr;
            return nullptr;
        }
        e.bytes = need;
    }
    // the copy embeds the scales and the zero points: the same weights with OTHER side tensors (a test harness; never a model) are packed again, into the same
    // buffer -- ordered behind every earlier reader by the null stream
    if (fresh || e.scales != d.scales || e.zeros != d.zeros) {
        if (!fresh) g_generation.fetch_add(1, std::memory_order_acq_rel);  // the buffer changes under front-cache entries that point at it: un-publish them all
        const int rc = tce_w4a16_prepack(&d, e.workspace, nullptr);
        if (rc != TCE_OK) die("gemv_forward_cuda (prepack)", rc);
        e.scales = d.scales;
        e.zeros = d.zeros;
    }
    return e.workspace;
}

// tce_w4a16_desc.scratch: one area for the process (the adapter launches on the null stream, so its calls are ordered), its counter
// words zeroed once
void *gemm_scratch() {
    static void *area = nullptr;
    static bool tried = false;
    std::lock_guard<std::mutex> lk(g_mu);
    if (!tried) {
        tried = true;
        const size_t need = tce_w4a16_gemm_scratch_bytes();
        void *p = nullptr;
        if (need && tce_malloc(&p, need, /*managed=*/0) == TCE_OK) {
            static const unsigned char zeros[4096] = {};
            if (tce_memcpy(p, zeros, sizeof(zeros), TCE_MEMCPY_H2D, nullptr) == TCE_OK) area = p;  // (null stream: ordered in front of every GEMM; the source is static -- no synchronisation)
            else tce_free(p);
        }
    }
    return area;
}

// TCE_W4_ZERO_POINT_IS_8 fast path, decided once per zero-point tensor WITHOUT a host synchronisation (round 5; the operator's contract is "asynchronous, never
// syncs"): first sight enqueues a check kernel on the null stream that writes its verdict into a word of pinned, device-mapped host memory; until that
// word is non-zero the calls simply do not make the promise (the kernels then READ the zero points -- same bits when they are all 8); a later call -- in practice
// the next token -- finds the verdict.  No hipMemcpy D2H, no hipDeviceSynchronize, on any call.
struct ZeroState {
    volatile int *verdict = nullptr;  // 0 pending, 1 every zero point is 8, 2 not
    int known = 0;                    // cached verdict once it arrived
};
std::unordered_map<TensorKey, ZeroState, TensorKeyHash> g_zero_state;
volatile int *g_verdict_pool = nullptr;  // pinned words, handed out one per zero-point tensor; chunks are never freed (a forgotten tensor's kernel may still be queued)
size_t g_verdict_used = 0, g_verdict_cap = 0;

volatile int *new_verdict_word() {  // g_mu held
    if (g_verdict_used == g_verdict_cap) {
        void *p = nullptr;
        constexpr size_t kChunk = 4096;
        if (tce_host_alloc(&p, kChunk * sizeof(int)) != TCE_OK) return nullptr;
        g_verdict_pool = static_cast<volatile int *>(p);
        g_verdict_used = 0;
        g_verdict_cap = kChunk;
    }
    volatile int *w = g_verdict_pool + g_verdict_used++;
    *w = 0;
    return w;
}

// 1: every zero point is 8 (verdict in); 0: not, or not known yet.  *final: the answer will not change.
int zeros_are_8(const void *zeros, long long words, bool *final) {
    const TensorKey key{zeros, words, 0, 0};
    std::lock_guard<std::mutex> lk(g_mu);
    ZeroState &z = g_zero_state[key];
    if (!z.known) {
        if (!z.verdict) {
            z.verdict = new_verdict_word();
            if (!z.verdict || tce_w4a16_check_zero_point_8_async(zeros, words, const_cast<int *>(z.verdict), nullptr) != TCE_OK) {
                z.known = 2;  // no pinned memory / launch refused: never make the promise for this tensor
            }
        }
        if (!z.known) z.known = *z.verdict;  // (a plain read of coherent host memory)
    }
    *final = z.known != 0;
    return z.known == 1;
}

// ---- the hot path: a lock-free front cache of fully resolved decode calls --------------------------------------------------------------------------------
// A steady-state token calls gemv_forward_cuda 161-225 times with tensors the adapter has seen; everything it needs per call -- the packed copy, the zero-point
// verdict, the scratch area -- is then a pure function of (qweight, scales, zeros, N, K, G).  Round 4 took g_mu two or three times per call for it; now one
// acquire load of a direct-mapped table entry.  Entries are immutable once published; tce_adapter_forget* bump the generation, which un-publishes all of them
// (they are rebuilt from the maps above on the next call).  An entry is only ever replaced when it is stale (or by a racing publication of another thread), and a
// replaced entry is retired, not freed -- a reader may still hold it: 72 bytes per weight tensor per generation, i.e. per tce_adapter_forget* or re-pack, never per
// token.  A tensor whose two probes both hold live entries of other tensors is not published and stays on the slow path (front_publish).
struct FrontEntry {
    const void *qweight, *scales, *zeros;
    int N, K, G;
    const void *prepacked;
    void *scratch;
    int flags;
    uint64_t generation;
};
constexpr size_t kFrontSize = 8192;  // direct-mapped, 2 probes; a 70B-class model has ~560 linears
std::atomic<FrontEntry *> g_front[kFrontSize];
std::vector<FrontEntry *> g_retired;  // g_mu

inline size_t front_slot(const void *p) {
    uint64_t x = reinterpret_cast<uintptr_t>(p) >> 6;
    x ^= x >> 17;
    x *= 0x9E3779B97F4A7C15ull;
    return (size_t)(x >> 40) & (kFrontSize - 1);
}
inline const FrontEntry *front_find(const tce_w4a16_desc &d) {
    const uint64_t gen = g_generation.load(std::memory_order_acquire);
    const size_t s0 = front_slot(d.qweight);
    for (size_t i = 0; i < 2; ++i) {
        const FrontEntry *e = g_front[(s0 + i) & (kFrontSize - 1)].load(std::memory_order_acquire);
        if (e && e->qweight == d.qweight && e->generation == gen && e->scales == d.scales && e->zeros == d.zeros && e->N == d.N && e->K == d.K && e->G == d.group_size) return e;
    }
    return nullptr;
}
void front_publish(const tce_w4a16_desc &d, uint64_t gen) {
    // `gen` was loaded before the call was resolved: a forget, or this call's own re-pack, since then makes the entry stale on arrival -- publish nothing, allocate
    // nothing; the next call publishes
    if (g_generation.load(std::memory_order_acquire) != gen) return;
    const size_t s0 = front_slot(d.qweight);
    size_t slot = kFrontSize;
    for (size_t i = 0; i < 2; ++i) {  // an empty or stale probe, else nothing: a live entry of another tensor is never evicted
        const FrontEntry *cur = g_front[(s0 + i) & (kFrontSize - 1)].load(std::memory_order_acquire);
        if (!cur || cur->generation != gen) {
            if (slot == kFrontSize) slot = (s0 + i) & (kFrontSize - 1);
        } else if (cur->qweight == d.qweight && cur->scales == d.scales && cur->zeros == d.zeros && cur->N == d.N && cur->K == d.K && cur->G == d.group_size) {
            return;  // another thread published this very call between our miss and now
        }
    }
    // Both probes hold live entries of other tensors (three or more weight addresses on one window): this tensor stays on the slow path -- the mutex and two map
    // lookups per call, no allocation.  Evicting instead ("newest wins") made the tensors of such a window evict each other on every token: two slow paths AND two
    // retired entries per token, for the life of the process.
    if (slot == kFrontSize) return;
    auto *e = new FrontEntry{d.qweight, d.scales, d.zeros, d.N, d.K, d.group_size, d.prepacked, d.scratch, d.flags, gen};
    FrontEntry *old = g_front[slot].exchange(e, std::memory_order_acq_rel);
    if (old) {
        std::lock_guard<std::mutex> lk(g_mu);
        g_retired.push_back(old);
    }
}

void int8_call(const char *who, const struct matmul_params *p, int bias_kind, int out_kind, int b_per_row) {
    const struct matrix *A = &p->A, *B = &p->B, *C = &p->C;
    if (A->column != B->row || C->row != A->row || C->column != B->column) {  // kernels/ref/matmul_ref_int8.cc:19-21
        std::printf("%s: assertion failed: A.column == B.row && C.row == A.row && C.column == B.column\n", who);
        std::exit(1);
    }
    tce_w8a8_desc d;
    std::memset(&d, 0, sizeof(d));
    d.M = A->row;
    d.N = B->column;
    d.K = A->column;
    d.batch = 1;
    d.A = A->int8_data_ptr;
    d.B = B->int8_data_ptr;
    d.bias = bias_kind == TCE_BIAS_INT8 ? static_cast<const void *>(p->bias.int8_data_ptr)
                                        : (bias_kind == TCE_BIAS_FP32 ? static_cast<const void *>(p->bias.data_ptr) : nullptr);
    d.C = out_kind == TCE_OUT_INT8 ? static_cast<void *>(C->int8_data_ptr) : static_cast<void *>(C->data_ptr);
    d.alpha = p->alpha;
    d.beta = p->beta;
    d.q_min = C->qparams.q_min;
    d.q_max = C->qparams.q_max;
    d.bias_kind = bias_kind;
    d.out_kind = out_kind;
    d.b_per_row = b_per_row;
    const int rc = tce_w8a8_matmul(&d, nullptr);
    if (rc != TCE_OK) die(who, rc);
}

}  // namespace

namespace matmul {

// kernels/cuda/gemv_cuda.cu:213-260.  IC = A.column, OC = C.column, M = C.row; B.row / B.column are not read.
void MatmulOperator::gemv_forward_cuda(const struct matmul_params *params) {
    tce_w4a16_desc d;
    std::memset(&d, 0, sizeof(d));
    d.M = params->C.row;
    d.N = params->C.column;
    d.K = params->A.column;
    d.group_size = params->block_size;  // QK
    d.A = params->A.half_data_ptr;
    d.qweight = params->B.int32_data_ptr;
    d.scales = params->half_scales;
    d.zeros = params->int32_zero_point;
    d.C = params->C.half_data_ptr;
    static const bool pack_on = [] { const char *e = std::getenv("TCE_ADAPTER_PACK"); return !(e && e[0] == '0'); }();
    // The packed copy serves both ends: decode batches (M <= 4: the int8-contraction GEMV reads it, round 4) and prompts (M > 128: the 128-row GEMM).
    // One extra copy of the int4 weights per linear in HBM (an 8B-class model: +3.9 GB of 288); TCE_ADAPTER_PACK=0 keeps the q4_6 arrays only;
    // tce_adapter_prepare() builds it at load time instead of inside the first call.
    const bool wants_pack = pack_on && (d.M <= 4 || d.M >= kPackMinM) && d.K % 128 == 0 && d.A && d.qweight && d.scales && d.zeros;
    if (const FrontEntry *fe = front_find(d)) {  // steady state: one table probe, no lock
        d.flags |= fe->flags;
        if (wants_pack) {
            d.prepacked = fe->prepacked;
            d.scratch = fe->scratch;
        }
    } else {
        const uint64_t gen = g_generation.load(std::memory_order_acquire);
        bool final = true;
        if (d.group_size == 128 || d.group_size == 64 || d.group_size == 32) {
            // rows of packed zero points: calculate_zeros_width (llm/src/nn_modules/cuda/utils.cu:162-178)
            const int mult = d.group_size >= 128 ? 1 : (d.group_size == 64 ? 2 : 4);
            const int zw = (((d.K / d.group_size + 7) / 8) + mult - 1) / mult * mult;
            if (d.zeros && zeros_are_8(d.zeros, (long long)d.N * zw, &final)) d.flags |= TCE_W4_ZERO_POINT_IS_8;
        }
        if (wants_pack) {
            d.prepacked = packed_copy(d);
            if (d.prepacked) d.scratch = gemm_scratch();
        }
        // published once nothing about the call can change any more (the zero-point verdict is in) and only from a call that resolved the packed copy
        const bool packable = pack_on && d.K % 128 == 0 && d.qweight && d.scales && d.zeros;
        if (final && (!packable || d.prepacked)) front_publish(d, gen);
    }
    const int rc = tce_w4a16_forward(&d, nullptr);
    if (rc == TCE_ERR_UNSUPPORTED_GROUP) {
        std::printf("Unsupported group size: %d\n", params->block_size);  // the reference's own message
        std::exit(1);
    }
    if (rc != TCE_OK) die("gemv_forward_cuda", rc);
}

// kernels/cuda/matmul_int4.cu:8-48: AWQ layout, binary16 arithmetic, B.row = K.
void MatmulOperator::naive_mat_mul_fp16_int4(const struct matmul_params *params) {
    const int rc = tce_w4a16_awq_fp16acc(params->C.row, params->C.column, params->B.row, params->block_size,
                                         params->A.fp16_data_ptr, params->B.int32_data_ptr, params->fp16_scales,
                                         params->C.fp16_data_ptr, nullptr);
    if (rc != TCE_OK) die("naive_mat_mul_fp16_int4", rc);
}

// Declared in kernels/matmul.h:142-145, never defined in the reference: AWQ (q4_5) layout GEMM.  split_k_iters is
// accepted for signature compatibility; the HIP kernels accumulate the whole K in fp32 and need no split-K merge.
void MatmulOperator::gemm_forward_cuda(const struct matmul_params *params, int /*split_k_iters*/) {
    const int M = params->C.row, N = params->C.column, K = params->B.row, G = params->block_size;
    const void *qw = params->B.int32_data_ptr;
    const size_t need = tce_w4a16_awq_workspace_bytes(N, K, G);
    if (need == 0) die("gemm_forward_cuda", TCE_ERR_UNSUPPORTED_GROUP);
    void *ws = nullptr;
    int repack = 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        AwqEntry &e = g_awq[TensorKey{qw, N, K, G}];
        if (!e.workspace || e.bytes < need) {  // first sight of this (pointer, N, K, G): allocate and re-lay-out
            if (e.workspace) tce_free(e.workspace);
            e.workspace = nullptr;
            e.bytes = 0;
            const int arc = tce_malloc(&e.workspace, need, /*managed=*/0);
            if (arc != TCE_OK) die("gemm_forward_cuda (workspace)", arc);
            e.bytes = need;
            repack = 1;
        }
        ws = e.workspace;
    }
    // Fields read: the CUDA-typed ones (A / C .half_data_ptr, half_scales) -- gemm_forward_cuda is a device entry point like
    // gemv_forward_cuda (kernels/matmul.h:140-145 sits in the QM_CUDA block); fp16_scales belongs to the software-half
    // reference naive_mat_mul_fp16_int4.  The Python mirror (tinychatengine_amd/matmul.py) reads the same fields.
    const void *scales = params->half_scales;
    const int rc = tce_w4a16_gemm_awq(M, N, K, G, params->A.half_data_ptr, qw, scales, params->C.half_data_ptr, ws, repack, nullptr);
    if (rc != TCE_OK) die("gemm_forward_cuda", rc);
}
void MatmulOperator::gemm_forward_cuda_8splits(const struct matmul_params *params, float16_t * /*split_8_buffer*/) {
    gemm_forward_cuda(params, 8);
}
void MatmulOperator::gemm_forward_cuda_half(const struct matmul_params *params, int split_k_iters) {
    gemm_forward_cuda(params, split_k_iters);
}
void MatmulOperator::gemm_forward_cuda_half_test(const struct matmul_params *params, int split_k_iters) {
    gemm_forward_cuda(params, split_k_iters);
}

// kernels/ref/matmul_ref_int8.cc:161-192
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll", p, TCE_BIAS_INT8, TCE_OUT_INT8, 0);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_32unroll_over_column(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_32unroll_over_column", p, TCE_BIAS_INT8, TCE_OUT_INT8, 0);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias", p, TCE_BIAS_NONE, TCE_OUT_INT8, 0);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_batch(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_batch", p, TCE_BIAS_NONE, TCE_OUT_INT8, 1);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32", p, TCE_BIAS_FP32, TCE_OUT_FP32, 0);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32_over_column(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32_over_column", p, TCE_BIAS_FP32, TCE_OUT_FP32, 0);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32", p, TCE_BIAS_NONE, TCE_OUT_FP32, 0);
}
void MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32_batch(const struct matmul_params *p) {
    int8_call("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32_batch", p, TCE_BIAS_NONE, TCE_OUT_FP32, 1);
}

// kernels/cuda/gemv_cuda.cu:262-268: empty in the GPU build
void MatmulOperator::mat_mul_accelerator_int4_fast(const struct matmul_params *) {}
void MatmulOperator::mat_mul_accelerator_int4_fast_no_offset(const struct matmul_params *) {}

}  // namespace matmul

// Drops what the adapter remembers about a buffer (any tensor whose data starts at ptr): call it before freeing or
// rewriting model memory.  tce_adapter_forget_all() drops everything (e.g. on model reload).
extern "C" void tce_adapter_forget(const void *ptr) {
    if (!ptr) return;  // names no buffer (and would match the null side-tensor fields of every AWQ entry below)
    std::lock_guard<std::mutex> lk(g_mu);
    g_generation.fetch_add(1, std::memory_order_acq_rel);  // every front-cache entry is stale from here on
    for (auto it = g_zero_state.begin(); it != g_zero_state.end();) it = it->first.ptr == ptr ? g_zero_state.erase(it) : std::next(it);
    for (auto *m : {&g_awq, &g_pack})
        for (auto it = m->begin(); it != m->end();) {
            if (it->first.ptr == ptr || it->second.scales == ptr || it->second.zeros == ptr) {
                if (it->second.workspace) tce_free(it->second.workspace);
                it = m->erase(it);
            } else {
                ++it;
            }
        }
}
extern "C" void tce_adapter_forget_all(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_generation.fetch_add(1, std::memory_order_acq_rel);
    g_zero_state.clear();
    for (auto *m : {&g_awq, &g_pack}) {
        for (auto &kv : *m)
            if (kv.second.workspace) tce_free(kv.second.workspace);
        m->clear();
    }
}
extern "C" long tce_adapter_cache_entries(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return (long)(g_zero_state.size() + g_awq.size() + g_pack.size());
}

// Load-time hook (optional): what the first gemv_forward_cuda on this linear would do lazily -- build the packed copy, start the zero-point
// check -- done when the host calls it, e.g. from Linear_half_int4's constructor behind the three file reads (llm/include/ops/linear.h:215-240), so that the first
// token pays neither the re-layout (3 prepack launches per linear) nor the allocation.  Asynchronous on the null stream like everything else.  Returns the bytes of
// device memory the adapter now holds for this linear (0: no packed form for this shape / TCE_ADAPTER_PACK=0).
extern "C" long long tce_adapter_prepare(const void *qweight, const void *scales, const void *zeros, int N, int K, int group_size) {
    static const bool pack_on = [] { const char *e = std::getenv("TCE_ADAPTER_PACK"); return !(e && e[0] == '0'); }();
    if (!qweight || !scales || !zeros || N <= 0 || K <= 0 || (group_size != 128 && group_size != 64 && group_size != 32)) return 0;
    tce_w4a16_desc d;
    std::memset(&d, 0, sizeof(d));
    d.M = 1;
    d.N = N;
    d.K = K;
    d.group_size = group_size;
    d.qweight = qweight;
    d.scales = scales;
    d.zeros = zeros;
    const int mult = group_size >= 128 ? 1 : (group_size == 64 ? 2 : 4);
    const int zw = (((K / group_size + 7) / 8) + mult - 1) / mult * mult;
    bool final = false;
    (void)zeros_are_8(zeros, (long long)N * zw, &final);
    if (!pack_on || K % 128 != 0) return 0;
    return packed_copy(d) ? (long long)tce_w4a16_prepack_bytes(N, K, group_size) : 0;
}

// Bytes of device memory the adapter holds beyond the model's own tensors (packed copies + AWQ re-layouts).
// Exchanges between workgroups on the adapter's GEMM scratch area that gave up waiting (tce_w4a16_gemm_scratch_faults: synchronises; 0 is the only value ever
// observed; non-zero = some prefill outputs since hold NaN and the area is poisoned until tce_adapter_forget_all() is followed by a new area -- a host checks where it
// synchronises anyway, e.g. once per generated sequence).  -1: the call failed; 0 also when no area was ever allocated.
extern "C" long tce_adapter_gemm_faults(void) {
    void *area = gemm_scratch();
    if (!area) return 0;
    uint32_t n = 0;
    return tce_w4a16_gemm_scratch_faults(area, nullptr, &n) == TCE_OK ? (long)n : -1;
}

extern "C" long long tce_adapter_device_bytes(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    long long n = 0;
    for (auto *m : {&g_awq, &g_pack})
        for (auto &kv : *m) n += (long long)kv.second.bytes;
    return n;
}

extern "C" long tce_adapter_layout(int idx) {
    switch (idx) {
        case 0: return (long)sizeof(matmul_params);
        case 1: return (long)sizeof(matrix);
        case 2: return (long)offsetof(matmul_params, B);
        case 3: return (long)offsetof(matmul_params, C);
        case 4: return (long)offsetof(matmul_params, bias);
        case 5: return (long)offsetof(matmul_params, opt_params);
        case 6: return (long)offsetof(matmul_params, alpha);
        case 7: return (long)offsetof(matmul_params, beta);
        case 8: return (long)offsetof(matmul_params, half_scales);
        case 9: return (long)offsetof(matmul_params, fp16_scales);
        case 10: return (long)offsetof(matmul_params, int32_zero_point);
        case 11: return (long)offsetof(matmul_params, block_size);
        case 12: return (long)offsetof(matrix, half_data_ptr);
        case 13: return (long)offsetof(matrix, int32_data_ptr);
        case 14: return (long)offsetof(matrix, int8_data_ptr);
        case 15: return (long)offsetof(matrix, qparams);
        case 16: return (long)(offsetof(matrix, qparams) + offsetof(quantization_params, q_min));
        case 17: return (long)offsetof(matmul_params, A_scales);
        default: return -1;
    }
}
