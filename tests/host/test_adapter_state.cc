// test_adapter_state.cc -- the adapter's host state (tinychatengine_amd/adapter/matmul_operator_hip.cc) on a MODEL of the C ABI.  CPU only; never links libtce_hip.so or HIP.
//
// The adapter's translation unit is #included, so front_slot(), front_find(), g_front, g_retired, g_generation, g_mu and the three maps are read directly: the product
// carries no test hook.  The tce_* functions the adapter calls are defined below ("the stand-in"; `nm -u` of the adapter's object is the list).  The stand-in is a model:
//   * device memory is host memory (malloc); tce_free poisons the block and -- in the AddressSanitizer build -- really frees it, so a use of a freed copy is a report
//     there and a "not a live allocation" violation in every build;
//   * tce_w4a16_prepack writes a digest of the BYTES of qweight, scales, zeros and of (N, K, G) into the copy;
//   * tce_w4a16_check_zero_point_8_async only queues the check; drain() -- a device synchronise -- writes 1 / 2 into the verdict word from the tensor's contents at
//     that moment: verdicts are pending exactly as on the device;
//   * every call is counted per function, and the last 64 are kept in a ring for the failure message;
//   * tce_w4a16_forward checks every call:
//       F1  the five pointers and four shape words are those of the caller's matmul_params, everything else in the descriptor is zero (the caller poisons every
//           field of matmul_params the reference's wrapper does not set: none of that may arrive);
//       F2  prepacked != NULL  <=>  (M <= 4 || M >= 129) && K % 128 == 0          (TCE_ADAPTER_PACK unset)
//       F3  a non-null prepacked is a live allocation that holds the digest of the tensors as they are NOW;
//       F4  scratch != NULL <=> prepacked != NULL, and it is the one zeroed area;
//       F5  TCE_W4_ZERO_POINT_IS_8 only if every zero-point word of this tensor is 0x88888888 now;
//       F6  TCE_W4_ZERO_POINT_IS_8 on every call made after the tensor's latest check was drained with verdict 1 (single-threaded scenarios).
//
// Two windows are the CALLER's contract, not defects, and no scenario enters them:
//   (a) one call uses a packed copy while another thread re-packs the same weights with other side tensors (the copy is rewritten in place, ordered only by the stream);
//   (b) two threads make concurrent FIRST calls of gemm_forward_cuda on one AWQ tensor (both may see repack = 1 / the second may launch before the first's re-layout).
// A third follows from "call tce_adapter_forget before freeing or rewriting": a forget of a tensor that another thread is calling at that moment frees the copy that
// call is about to launch on.  The threads scenario forgets tensors nobody rewrites; the stand-in counts (and tolerates, there only) calls that lost that race.
//
// Each scenario prints one line; any violation makes the process exit 1.  Built three times by tests/test_adapter_state_host.py: plain, address+undefined, thread.
#include "matmul_operator_hip.cc"

#include <sys/wait.h>
#include <unistd.h>

#include <cstdarg>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <utility>

// ---- every operator new of the process is counted: "a steady-state token allocates nothing" is measured, not inferred.  In the plain build only: a sanitiser's
// runtime, linked statically, defines these operators itself; there the count stays 0 and the conservation of retired + live entries carries the scenario -----------
static std::atomic<long> g_news{0};
#if !defined(__SANITIZE_ADDRESS__) && !defined(__SANITIZE_THREAD__)
__attribute__((noinline)) void *operator new(std::size_t n) {
    g_news.fetch_add(1, std::memory_order_relaxed);
    void *p = std::malloc(n ? n : 1);
    if (!p) std::abort();
    return p;
}
void *operator new[](std::size_t n) { return operator new(n); }
__attribute__((noinline)) void operator delete(void *p) noexcept { std::free(p); }
__attribute__((noinline)) void operator delete[](void *p) noexcept { std::free(p); }
__attribute__((noinline)) void operator delete(void *p, std::size_t) noexcept { std::free(p); }
__attribute__((noinline)) void operator delete[](void *p, std::size_t) noexcept { std::free(p); }
#endif

#if defined(__SANITIZE_ADDRESS__)
#define STANDIN_REALLY_FREES 1
// The adapter keeps its retired front-cache entries and its verdict chunks until the process ends, on purpose (a reader / a queued kernel may still hold them): at
// exit they are unreachable "leaks".  The leak report is off; every other report of the build (use after free, overflow, undefined behaviour) stays fatal.
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }
#else
#define STANDIN_REALLY_FREES 0
#endif

namespace standin {

enum Fn { kVersion, kLastError, kPrepackBytes, kMalloc, kFree, kPrepack, kScratchBytes, kMemcpy, kHostAlloc, kCheck, kForward, kAwqFp16acc, kAwqBytes, kGemmAwq, kW8a8, kScratchFaults, kFnCount };
const char *const kFnName[kFnCount] = {"version", "last_error", "prepack_bytes", "malloc", "free", "prepack", "gemm_scratch_bytes", "memcpy", "host_alloc", "check_zero_point_8_async", "forward",
                                       "awq_fp16acc", "awq_workspace_bytes", "gemm_awq", "w8a8_matmul", "gemm_scratch_faults"};
std::atomic<long> calls[kFnCount];
std::atomic<unsigned> ring_pos;
std::atomic<int> ring[64];
void log_call(Fn f) {
    calls[f].fetch_add(1, std::memory_order_relaxed);
    ring[ring_pos.fetch_add(1, std::memory_order_relaxed) & 63].store((int)f, std::memory_order_relaxed);
}

std::atomic<int> failures{0};
void violation(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void violation(const char *fmt, ...) {
    if (failures.fetch_add(1) >= 20) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    std::string tail;
    const unsigned pos = ring_pos.load();
    for (unsigned i = pos > 8 ? pos - 8 : 0; i < pos; ++i) tail += std::string(" ") + kFnName[ring[i & 63].load()];
    std::printf("VIOLATION: %s   (last calls:%s)\n", buf, tail.c_str());
    std::fflush(stdout);
}

std::mutex mu;  // the stand-in's own state; always taken after the adapter's g_mu where both are held
struct Block {
    size_t bytes;
};
std::map<const void *, Block> live;
std::vector<void *> quarantine;  // freed blocks of the builds that do not really free: poisoned, kept, never handed out again
void *scratch_area = nullptr;
struct Check {
    const void *zeros;
    long long words;
    int *verdict;
};
std::vector<Check> pending;
struct Latest {
    int *word = nullptr;
    int verdict = 0;  // 0: queued, not drained
};
std::map<std::pair<const void *, long long>, Latest> latest;
bool threaded = false;          // the threads scenario: F6 is off, and a prepacked that a concurrent forget freed is counted, not a violation
std::atomic<long> raced{0};
thread_local const matmul_params *cur_params = nullptr;  // the caller's struct of the call in progress
thread_local tce_w4a16_desc last_forward;
thread_local tce_w8a8_desc last_w8a8;
thread_local int last_repack = -1;

constexpr size_t kScratchSize = 8192;
constexpr uint64_t kMagic = 0x7463655f70616b64ull;

int zeros_width(int K, int G) {  // packed zero-point words per row, padded to the layout's multiple (the q4_6 layout)
    const int mult = G >= 128 ? 1 : (G == 64 ? 2 : 4);
    return (((K / G + 7) / 8) + mult - 1) / mult * mult;
}
bool group_ok(int G) { return G == 128 || G == 64 || G == 32; }
uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const uint32_t *w = static_cast<const uint32_t *>(p);  // (every tensor here is a whole number of 32-bit words)
    for (size_t i = 0; i < n / 4; ++i) h = (h ^ w[i]) * 0x100000001b3ull;
    return h;
}
uint64_t digest_q4_6(const void *qweight, const void *scales, const void *zeros, int N, int K, int G) {
    const int zw = zeros_width(K, G);
    uint64_t h = 0xcbf29ce484222325ull;
    h = fnv(h, qweight, (size_t)N * (K / 8) * 4);
    h = fnv(h, scales, (size_t)N * zw * 8 * 2);
    h = fnv(h, zeros, (size_t)N * zw * 4);
    const int shape[3] = {N, K, G};
    return fnv(h, shape, sizeof(shape));
}
uint64_t digest_awq(const void *qweight, int N, int K, int G) {
    uint64_t h = 0xcbf29ce484222325ull;
    h = fnv(h, qweight, (size_t)K * (N / 8) * 4);
    const int shape[3] = {N, K, G};
    return fnv(h, shape, sizeof(shape));
}
bool all_eight(const void *zeros, long long words) {
    const uint32_t *z = static_cast<const uint32_t *>(zeros);
    for (long long i = 0; i < words; ++i)
        if (z[i] != 0x88888888u) return false;
    return true;
}

// the device catches up: every queued zero-point check writes its verdict from the tensor as it is now
void drain() {
    std::lock_guard<std::mutex> lk(mu);
    for (const Check &c : pending) {
        const int v = all_eight(c.zeros, c.words) ? 1 : 2;
        *c.verdict = v;
        auto it = latest.find({c.zeros, c.words});
        if (it != latest.end() && it->second.word == c.verdict) it->second.verdict = v;
    }
    pending.clear();
}
// the threads scenario: the verdict words are plain memory the adapter reads under its mutex (on the device: coherent pinned memory written by a kernel), so the model's
// "device" writes them under that mutex too
void drain_threaded() {
    std::lock_guard<std::mutex> lk(g_mu);
    drain();
}

struct Snap {
    long c[kFnCount];
};
Snap snap() {
    Snap s;
    for (int i = 0; i < kFnCount; ++i) s.c[i] = calls[i].load();
    return s;
}
// calls since `s`, with the functions that answer a question and touch nothing (version, last_error) left out
std::string since(const Snap &s) {
    std::string r;
    for (int i = kPrepackBytes; i < kFnCount; ++i) {
        const long n = calls[i].load() - s.c[i];
        if (n) r += (r.empty() ? "" : " ") + std::string(kFnName[i]) + "=" + std::to_string(n);
    }
    return r.empty() ? "nothing" : r;
}

}  // namespace standin

// ---- the C ABI, modelled ----------------------------------------------------------------------------------------------------------------------------------------
using namespace standin;

extern "C" {
int tce_version(void) { return TCE_VERSION; }  // (not counted: runs from the adapter's static initialiser, before anything here is constructed)
const char *tce_last_error(void) {
    log_call(kLastError);
    return "stand-in error text";
}
size_t tce_w4a16_prepack_bytes(int N, int K, int G) {
    log_call(kPrepackBytes);
    return (N > 0 && K > 0 && group_ok(G) && K % 128 == 0) ? 256 + (size_t)N * K / 2 : 0;
}
size_t tce_w4a16_gemm_scratch_bytes(void) {
    log_call(kScratchBytes);
    return kScratchSize;
}
int tce_malloc(void **ptr, size_t bytes, int /*managed*/) {
    log_call(kMalloc);
    void *p = std::malloc(bytes);
    if (!p) return TCE_ERR_HIP;
    std::memset(p, 0xCD, bytes);
    std::lock_guard<std::mutex> lk(mu);
    live[p] = Block{bytes};
    *ptr = p;
    return TCE_OK;
}
int tce_free(void *p) {
    log_call(kFree);
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(p);
    if (it == live.end()) {
        violation("tce_free(%p): not a live allocation (double free?)", p);
        return TCE_ERR_BAD_ARG;
    }
    std::memset(p, 0xDD, it->second.bytes);
    live.erase(it);
    if (p == scratch_area) scratch_area = nullptr;
#if STANDIN_REALLY_FREES
    std::free(p);
#else
    quarantine.push_back(p);
#endif
    return TCE_OK;
}
int tce_host_alloc(void **ptr, size_t bytes) {
    log_call(kHostAlloc);
    void *p = std::calloc(1, bytes);
    if (!p) return TCE_ERR_HIP;
    std::lock_guard<std::mutex> lk(mu);
    quarantine.push_back(p);  // (kept reachable: the adapter never frees verdict chunks)
    *ptr = p;
    return TCE_OK;
}
int tce_memcpy(void *dst, const void *src, size_t bytes, int kind, void * /*stream*/) {
    log_call(kMemcpy);
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(dst);
    if (kind != TCE_MEMCPY_H2D || it == live.end() || it->second.bytes < bytes) {
        violation("tce_memcpy: kind %d into %p (%zu bytes) is not a copy into a live block that holds it", kind, dst, bytes);
        return TCE_ERR_BAD_ARG;
    }
    std::memcpy(dst, src, bytes);
    if (it->second.bytes == kScratchSize) scratch_area = dst;
    return TCE_OK;
}
int tce_w4a16_check_zero_point_8_async(const void *zeros, long long n_words, int *verdict, void * /*stream*/) {
    log_call(kCheck);
    std::lock_guard<std::mutex> lk(mu);
    if (!zeros || n_words <= 0 || !verdict || *verdict != 0) {
        violation("check_zero_point_8_async(%p, %lld, %p): bad argument or a verdict word that is not 0 on entry", zeros, n_words, (void *)verdict);
        return TCE_ERR_BAD_ARG;
    }
    pending.push_back(Check{zeros, n_words, verdict});
    Latest &l = latest[{zeros, n_words}];
    l.word = verdict;
    l.verdict = 0;
    return TCE_OK;
}
int tce_w4a16_prepack(const tce_w4a16_desc *d, void *packed, void * /*stream*/) {
    log_call(kPrepack);
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(packed);
    const size_t need = (group_ok(d->group_size) && d->K % 128 == 0) ? 256 + (size_t)d->N * d->K / 2 : 0;
    if (!need || it == live.end() || it->second.bytes < need || !d->qweight || !d->scales || !d->zeros) {
        violation("prepack N=%d K=%d G=%d into %p: no packed form, or not a live block of %zu bytes", d->N, d->K, d->group_size, packed, need);
        return TCE_ERR_BAD_ARG;
    }
    std::memset(packed, 0x5A, need);
    const uint64_t head[2] = {kMagic, digest_q4_6(d->qweight, d->scales, d->zeros, d->N, d->K, d->group_size)};
    std::memcpy(packed, head, sizeof(head));
    return TCE_OK;
}
int tce_w4a16_forward(const tce_w4a16_desc *d, void *stream) {
    log_call(kForward);
    last_forward = *d;
    const matmul_params *p = cur_params;
    if (!p) {
        violation("forward without a caller");
        return TCE_OK;
    }
    // F1
    if (d->M != p->C.row || d->N != p->C.column || d->K != p->A.column || d->group_size != p->block_size || d->A != p->A.half_data_ptr || d->qweight != p->B.int32_data_ptr ||
        d->scales != p->half_scales || d->zeros != p->int32_zero_point || d->C != p->C.half_data_ptr)
        violation("forward: M=%d N=%d K=%d G=%d or a pointer is not the caller's", d->M, d->N, d->K, d->group_size);
    if (d->lda || d->ldc || d->scales_stride || d->zeros_stride || d->reserved || d->reserved2 || d->rmsnorm_gamma || d->rmsnorm_eps != 0.0f || stream || (d->flags & ~TCE_W4_ZERO_POINT_IS_8))
        violation("forward: a field the adapter never sets is non-zero (flags 0x%x)", d->flags);
    if (!group_ok(d->group_size)) return TCE_ERR_UNSUPPORTED_GROUP;
    const int zw = zeros_width(d->K, d->group_size);
    const long long words = (long long)d->N * zw;
    std::lock_guard<std::mutex> lk(mu);
    // F2
    const bool want = (d->M <= 4 || d->M >= 129) && d->K % 128 == 0;
    if (want != (d->prepacked != nullptr)) violation("forward M=%d K=%d: prepacked is %s, the rule says %s", d->M, d->K, d->prepacked ? "set" : "null", want ? "set" : "null");
    // F3
    if (d->prepacked) {
        auto it = live.find(d->prepacked);
        if (it == live.end()) {
            if (threaded) raced.fetch_add(1);
            else violation("forward M=%d: prepacked %p is not a live allocation (a freed copy)", d->M, d->prepacked);
        } else {
            uint64_t head[2];
            std::memcpy(head, d->prepacked, sizeof(head));
            if (head[0] != kMagic || head[1] != digest_q4_6(d->qweight, d->scales, d->zeros, d->N, d->K, d->group_size))
                violation("forward M=%d N=%d K=%d G=%d: the packed copy is not built from the tensors as they are now (stale copy)", d->M, d->N, d->K, d->group_size);
        }
    }
    // F4
    if ((d->scratch != nullptr) != (d->prepacked != nullptr)) violation("forward M=%d: scratch %s with prepacked %s", d->M, d->scratch ? "set" : "null", d->prepacked ? "set" : "null");
    if (d->scratch) {
        static const unsigned char zero[4096] = {};
        if (d->scratch != scratch_area || std::memcmp(d->scratch, zero, sizeof(zero)) != 0) violation("forward: scratch %p is not the zeroed area %p", d->scratch, scratch_area);
    }
    // F5, F6
    const bool flag = (d->flags & TCE_W4_ZERO_POINT_IS_8) != 0;
    if (flag && !all_eight(d->zeros, words)) violation("forward M=%d N=%d K=%d G=%d: TCE_W4_ZERO_POINT_IS_8 on a tensor whose zero points are not all 8", d->M, d->N, d->K, d->group_size);
    if (!threaded) {
        auto it = latest.find({d->zeros, words});
        if (it == latest.end()) violation("forward: no zero-point check was ever queued for (%p, %lld words)", d->zeros, words);
        else if (it->second.verdict == 1 && !flag) violation("forward M=%d: the verdict 'all 8' is in and the call does not make the promise", d->M);
    }
    return TCE_OK;
}
int tce_w4a16_awq_fp16acc(int, int, int, int, const void *, const void *, const void *, void *, void *) {
    log_call(kAwqFp16acc);
    return TCE_OK;
}
size_t tce_w4a16_awq_workspace_bytes(int N, int K, int G) {
    log_call(kAwqBytes);
    return (N > 0 && K > 0 && group_ok(G) && N % 8 == 0 && K % G == 0) ? 128 + (size_t)N * K / 2 : 0;
}
int tce_w4a16_gemm_awq(int M, int N, int K, int G, const void *A, const void *qw, const void *scales, void *C, void *ws, int repack, void *stream) {
    log_call(kGemmAwq);
    last_repack = repack;
    const matmul_params *p = cur_params;
    if (!p || M != p->C.row || N != p->C.column || K != p->B.row || G != p->block_size || A != p->A.half_data_ptr || qw != p->B.int32_data_ptr || scales != p->half_scales ||
        C != p->C.half_data_ptr || stream)
        violation("gemm_awq: M=%d N=%d K=%d G=%d or a pointer is not the caller's", M, N, K, G);
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(ws);
    if (it == live.end() || it->second.bytes < 128 + (size_t)N * K / 2) {
        violation("gemm_awq: workspace %p is not a live block that holds the re-layout", ws);
        return TCE_ERR_BAD_ARG;
    }
    const uint64_t head[2] = {kMagic, digest_awq(qw, N, K, G)};
    if (repack) std::memcpy(ws, head, sizeof(head));
    else if (std::memcmp(ws, head, sizeof(head)) != 0) violation("gemm_awq repack=0: the workspace does not hold the re-layout of the weights as they are now");
    return TCE_OK;
}
int tce_w8a8_matmul(const tce_w8a8_desc *d, void *stream) {
    log_call(kW8a8);
    last_w8a8 = *d;
    if (stream) violation("w8a8_matmul: not the null stream");
    return TCE_OK;
}
int tce_w4a16_gemm_scratch_faults(const void *scratch, void *, uint32_t *faults) {
    log_call(kScratchFaults);
    std::lock_guard<std::mutex> lk(mu);
    if (scratch != scratch_area) violation("gemm_scratch_faults: %p is not the scratch area", scratch);
    *faults = 0;
    return TCE_OK;
}
}  // extern "C"

// ---- scenarios --------------------------------------------------------------------------------------------------------------------------------------------------
namespace {

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            char m_[400];                                         \
            std::snprintf(m_, sizeof(m_), __VA_ARGS__);           \
            violation("%s:%d: %s -- %s", __func__, __LINE__, #cond, m_); \
        }                                                         \
    } while (0)

uint32_t g_rng = 12345;
uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

struct Linear {
    int N = 0, K = 0, G = 0, zw = 0;
    int32_t *qw = nullptr;  // may point into an arena (the collision scenario)
    uint16_t *sc = nullptr;
    int32_t *zp = nullptr;
    size_t qw_bytes() const { return (size_t)N * (K / 8) * 4; }
    size_t sc_bytes() const { return (size_t)N * zw * 8 * 2; }
    size_t zp_bytes() const { return (size_t)N * zw * 4; }
    long long words() const { return (long long)N * zw; }
};
void fill(void *p, size_t bytes) {
    unsigned char *b = static_cast<unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) b[i] = (unsigned char)rnd();
}
void set_zeros(Linear &l, bool all8) {
    for (long long i = 0; i < l.words(); ++i) l.zp[i] = (int32_t)0x88888888u;
    if (!all8) l.zp[l.words() - 1] = (int32_t)0x88888887u;  // one zero point of 7 in the last word of the last row
}
Linear make_linear(int N, int K, int G, bool all8, void *qw_at = nullptr) {
    Linear l;
    l.N = N, l.K = K, l.G = G, l.zw = zeros_width(K, G);
    l.qw = static_cast<int32_t *>(qw_at ? qw_at : std::malloc(l.qw_bytes()));
    l.sc = static_cast<uint16_t *>(std::malloc(l.sc_bytes()));
    l.zp = static_cast<int32_t *>(std::malloc(l.zp_bytes()));
    fill(l.qw, l.qw_bytes());
    fill(l.sc, l.sc_bytes());
    set_zeros(l, all8);
    return l;
}
void drop_linear(Linear &l, bool own_qw = true) {
    if (own_qw) std::free(l.qw);
    std::free(l.sc);
    std::free(l.zp);
    l = Linear{};
}

// activations and outputs are never dereferenced by the stand-in: one pair of buffers per thread stands for them
struct Act {
    alignas(64) unsigned char x[64];
    alignas(64) unsigned char out[64];
};
thread_local Act t_act;

// the call as the reference's wrapper makes it (llm/src/ops/cuda/linear.cu in the reference tree): a struct whose other fields are garbage
void gemv(const Linear &l, int M, const uint16_t *scales = nullptr, const int32_t *zeros = nullptr, int n = 0, int k = 0) {
    matmul_params p;
    std::memset(static_cast<void *>(&p), 0xA5, sizeof(p));
    p.A.row = M;
    p.A.column = k ? k : l.K;
    p.A.half_data_ptr = reinterpret_cast<float16_t *>(t_act.x);
    p.B.int32_data_ptr = l.qw;
    p.C.row = M;
    p.C.column = n ? n : l.N;
    p.C.half_data_ptr = reinterpret_cast<float16_t *>(t_act.out);
    p.half_scales = reinterpret_cast<float16_t *>(const_cast<uint16_t *>(scales ? scales : l.sc));
    p.int32_zero_point = const_cast<int32_t *>(zeros ? zeros : l.zp);
    p.block_size = l.G;
    cur_params = &p;
    matmul::MatmulOperator op;
    op.gemv_forward_cuda(&p);
    cur_params = nullptr;
}
tce_w4a16_desc desc_of(const Linear &l) {
    tce_w4a16_desc d;
    std::memset(&d, 0, sizeof(d));
    d.N = l.N, d.K = l.K, d.group_size = l.G, d.qweight = l.qw, d.scales = l.sc, d.zeros = l.zp;
    return d;
}
bool published(const Linear &l) { return front_find(desc_of(l)) != nullptr; }
long front_live() {
    long n = 0;
    for (size_t i = 0; i < kFrontSize; ++i) n += g_front[i].load() != nullptr;
    return n;
}
long retired() {
    std::lock_guard<std::mutex> lk(g_mu);
    return (long)g_retired.size();
}
size_t pack_bytes(const Linear &l) { return l.K % 128 == 0 ? 256 + (size_t)l.N * l.K / 2 : 0; }

// runs f in a forked child with its stdout in a pipe; returns the exit status (-1: killed by a signal)
template <typename F>
int in_child(F f, std::string *out) {
    std::fflush(stdout);
    int fd[2];
    if (pipe(fd) != 0) return -2;
    const pid_t pid = fork();
    if (pid == 0) {
        close(fd[0]);
        dup2(fd[1], 1);
        f();
        std::fflush(stdout);
        _exit(0);
    }
    close(fd[1]);
    char buf[256];
    ssize_t n;
    while ((n = read(fd[0], buf, sizeof(buf))) > 0) out->append(buf, (size_t)n);
    close(fd[0]);
    int st = 0;
    waitpid(pid, &st, 0);
    return WIFEXITED(st) ? WEXITSTATUS(st) : -1;
}

void steady_state() {
    int cases = 0;
    for (int G : {128, 64, 32})
        for (int K : {512, 4096, 1472})
            for (bool all8 : {true, false}) {
                tce_adapter_forget_all();
                Linear l = make_linear(16, K, G, all8);
                const bool packs = K % 128 == 0;
                Snap s = snap();
                gemv(l, 1);  // first sight: the check is queued, the copy is built, no promise yet
                CHECK(calls[kCheck] - s.c[kCheck] == 1 && calls[kPrepack] - s.c[kPrepack] == (packs ? 1 : 0) && calls[kForward] - s.c[kForward] == 1, "G=%d K=%d first call: %s", G, K, since(s).c_str());
                CHECK(!(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "promise made while the verdict is pending");
                CHECK(!published(l), "published with the verdict pending");
                drain();
                s = snap();
                gemv(l, 1);  // reads the verdict, publishes
                CHECK(calls[kCheck] == s.c[kCheck] && calls[kPrepack] == s.c[kPrepack] && calls[kMalloc] == s.c[kMalloc], "G=%d K=%d second call: %s", G, K, since(s).c_str());
                CHECK(published(l), "G=%d K=%d: not published by the call that read the verdict", G, K);
                const tce_w4a16_desc second = last_forward;
                CHECK(((second.flags & TCE_W4_ZERO_POINT_IS_8) != 0) == all8, "flags 0x%x with all8=%d", second.flags, (int)all8);
                s = snap();
                const long news = g_news.load();
                for (int i = 0; i < 101; ++i) {  // the third call and 100 more: hits
                    gemv(l, 1);
                    CHECK(last_forward.flags == second.flags && last_forward.prepacked == second.prepacked && last_forward.scratch == second.scratch, "call %d differs from the second", i + 3);
                }
                CHECK(since(s) == "forward=101", "G=%d K=%d all8=%d hit path saw: %s", G, K, (int)all8, since(s).c_str());
                CHECK(g_news.load() == news, "%ld allocations on the hit path", g_news.load() - news);
                tce_adapter_forget_all();
                drop_linear(l);
                ++cases;
            }
    std::printf("steady state: %d linears (G x K x zero points), calls 3..103 reach the C ABI as forward only, same flags and copy: ok\n", cases);
}

void m_classes() {
    const int Ms[] = {1, 4, 5, 128, 129, 200, 1};
    for (int first : {1, 200, 64}) {
        for (int K : {512, 1472}) {
            tce_adapter_forget_all();
            Linear l = make_linear(24, K, 64, true);
            gemv(l, first);
            drain();
            gemv(l, first);
            const bool packable = K % 128 == 0;
            // M = 64 resolves no packed copy: publishing that call would leave every later decode call without one
            CHECK(published(l) == (first != 64 || !packable), "first M=%d K=%d: published=%d", first, K, (int)published(l));
            const void *copy = nullptr;
            Snap s = snap();
            for (int M : Ms) {
                gemv(l, M);  // (F2: the stand-in holds every call to the rule)
                CHECK(last_forward.flags & TCE_W4_ZERO_POINT_IS_8, "M=%d lost the promise", M);
                if (last_forward.prepacked) {
                    CHECK(!copy || copy == last_forward.prepacked, "M=%d runs on another copy", M);
                    copy = last_forward.prepacked;
                }
            }
            if (first != 64 || !packable) CHECK(since(s) == "forward=7", "first M=%d K=%d: the classes saw %s", first, K, since(s).c_str());
            else CHECK(published(l) && calls[kPrepack] - s.c[kPrepack] == 1 && calls[kCheck] == s.c[kCheck], "first M=64: %s", since(s).c_str());  // M = 1 built the copy and published
            CHECK(tce_adapter_cache_entries() == (packable ? 2 : 1), "entries %ld", tce_adapter_cache_entries());
            tce_adapter_forget_all();
            drop_linear(l);
        }
    }
    std::printf("M classes: 1 4 5 128 129 200 1 on a tensor first seen at M = 1, 200, 64 (K = 512, 1472): packed copy exactly for M <= 4 and M >= 129: ok\n");
}

void identity() {
    tce_adapter_forget_all();
    // the same qweight address described with another (N, K)
    Linear a = make_linear(32, 512, 128, true);
    Linear b = a;  // same buffers, read as 16 x 1024
    b.N = 16, b.K = 1024, b.zw = zeros_width(1024, 128);
    CHECK(b.qw_bytes() == a.qw_bytes() && b.zp_bytes() <= a.zp_bytes() && b.sc_bytes() <= a.sc_bytes(), "the second view must fit the buffers");
    gemv(a, 1);
    drain();
    gemv(a, 1);
    gemv(a, 1);
    const void *copy_a = last_forward.prepacked;
    Snap s = snap();
    gemv(b, 1);
    CHECK(calls[kPrepack] - s.c[kPrepack] == 1 && last_forward.prepacked && last_forward.prepacked != copy_a, "another (N, K) at the same address: %s", since(s).c_str());
    CHECK(calls[kCheck] - s.c[kCheck] == 1, "the same zeros pointer with another word count (%lld vs %lld) gets its own check: %s", b.words(), a.words(), since(s).c_str());
    drain();
    gemv(b, 1);
    gemv(b, 1);
    gemv(a, 1);
    CHECK(last_forward.prepacked == copy_a, "the first shape lost its copy");
    CHECK(tce_adapter_cache_entries() == 4 && tce_adapter_device_bytes() == (long long)(pack_bytes(a) + pack_bytes(b)), "entries %ld bytes %lld", tce_adapter_cache_entries(), tce_adapter_device_bytes());
    // the same zeros pointer, another word count: the first 16 rows are all 8, the rest is not -- two verdicts
    tce_adapter_forget_all();
    for (long long i = 16 * a.zw; i < a.words(); ++i) a.zp[i] = 0x77777777;
    Linear top = a;
    top.N = 16;
    gemv(top, 1);
    gemv(a, 1);
    drain();
    gemv(top, 1);
    CHECK(last_forward.flags & TCE_W4_ZERO_POINT_IS_8, "16 rows of 8s");
    gemv(a, 1);
    CHECK(!(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "32 rows, 16 of them 7s");
    gemv(top, 1);
    CHECK(last_forward.flags & TCE_W4_ZERO_POINT_IS_8, "16 rows of 8s, again");
    // the same weights with scales A, B, A, B, each change made while the entry of the OTHER pair is live in the front cache: front_find must miss on the side tensors
    // alone (same qweight, N, K, G, generation) -- a hit would launch on the copy that embeds the other scales, and F3 holds every forward to the digest
    tce_adapter_forget_all();
    set_zeros(a, true);
    uint16_t *sc_b = static_cast<uint16_t *>(std::malloc(a.sc_bytes()));
    fill(sc_b, a.sc_bytes());
    auto live_with = [&](const uint16_t *scales, const int32_t *zeros) {
        tce_w4a16_desc d = desc_of(a);
        d.scales = scales, d.zeros = zeros;
        return front_find(d) != nullptr;
    };
    gemv(a, 1);
    drain();
    gemv(a, 1);
    CHECK(live_with(a.sc, a.zp), "A is not live before the first B");
    s = snap();
    const uint64_t gen = g_generation.load();
    for (int i = 0; i < 4; ++i) {
        const uint16_t *now = i % 2 ? a.sc : sc_b, *before = i % 2 ? sc_b : a.sc;
        CHECK(live_with(before, a.zp) && !live_with(now, a.zp), "round %d: the other pair must be the live one", i);
        const long packs = calls[kPrepack];
        gemv(a, 1, now);  // the miss: re-pack, generation bump
        CHECK(calls[kPrepack] - packs == 1 && !live_with(before, a.zp), "round %d: other scales did not re-pack", i);
        gemv(a, 1, now);  // nothing changes any more: publishes
        CHECK(live_with(now, a.zp), "round %d: not published", i);
        const Snap h = snap();
        gemv(a, 1, now);
        CHECK(since(h) == "forward=1", "round %d: the third call is no hit: %s", i, since(h).c_str());
    }
    CHECK(calls[kPrepack] - s.c[kPrepack] == 4 && calls[kMalloc] == s.c[kMalloc] && g_generation.load() == gen + 4, "B A B A: %s", since(s).c_str());
    CHECK(tce_adapter_cache_entries() == 2, "entries %ld", tce_adapter_cache_entries());
    s = snap();
    for (int i = 0; i < 3; ++i) gemv(a, 200);  // the last pair stays: hits
    CHECK(since(s) == "forward=3", "same side tensors: %s", since(s).c_str());
    // the same with a second zeros buffer (one zero point of 7): a hit of the live entry would carry its promise onto zero points that are not 8 (F5) and its copy (F3)
    int32_t *zp_b = static_cast<int32_t *>(std::malloc(a.zp_bytes()));
    std::memcpy(zp_b, a.zp, a.zp_bytes());
    zp_b[a.words() - 1] = (int32_t)0x88888887u;
    s = snap();
    gemv(a, 1, nullptr, zp_b);
    CHECK(calls[kPrepack] - s.c[kPrepack] == 1 && calls[kCheck] - s.c[kCheck] == 1 && !(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "other zeros on a live entry: %s", since(s).c_str());
    drain();
    gemv(a, 1, nullptr, zp_b);
    CHECK(live_with(a.sc, zp_b) && !live_with(a.sc, a.zp) && !(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "the second zeros buffer is not the live one");
    gemv(a, 1, nullptr, zp_b);
    s = snap();
    gemv(a, 1);  // back to the first zeros while the second's entry is live
    CHECK(calls[kPrepack] - s.c[kPrepack] == 1 && calls[kCheck] == s.c[kCheck] && (last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "first zeros on the second's live entry: %s", since(s).c_str());
    gemv(a, 1);
    CHECK(live_with(a.sc, a.zp) && !live_with(a.sc, zp_b), "the first zeros buffer is not the live one");
    CHECK(tce_adapter_cache_entries() == 3, "entries %ld", tce_adapter_cache_entries());
    tce_adapter_forget_all();
    std::free(zp_b);
    std::free(sc_b);
    drop_linear(a);
    std::printf("identity: (pointer, N, K) keys the copy, (pointer, words) the verdict, other scales or zeros on a live entry miss and re-pack: ok\n");
}

void forget() {
    tce_adapter_forget_all();
    Linear l = make_linear(16, 512, 32, true), other = make_linear(16, 512, 32, true);
    auto warm = [&](const Linear &t) {
        gemv(t, 1);
        drain();
        gemv(t, 1);
        gemv(t, 1);
    };
    auto expect = [&](long entries, long long bytes, const char *when) {
        CHECK(tce_adapter_cache_entries() == entries && tce_adapter_device_bytes() == bytes, "%s: entries %ld (want %ld), bytes %lld (want %lld)", when, tce_adapter_cache_entries(), entries,
              tce_adapter_device_bytes(), bytes);
    };
    const long long pb = (long long)pack_bytes(l);
    warm(l);
    warm(other);
    expect(4, 2 * pb, "two linears");
    // forget(qweight): the copy goes, the zero-point verdict (keyed by the zeros pointer) stays
    Snap s = snap();
    tce_adapter_forget(l.qw);
    CHECK(calls[kFree] - s.c[kFree] == 1, "forget(qweight): %s", since(s).c_str());
    expect(3, pb, "forget(qweight)");
    fill(l.qw, l.qw_bytes());
    s = snap();
    gemv(l, 1);  // F3: a kept copy would carry the old digest; F3 also refuses the freed block
    CHECK(calls[kPrepack] - s.c[kPrepack] == 1 && calls[kCheck] == s.c[kCheck] && (last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "after forget(qweight): %s", since(s).c_str());
    expect(4, 2 * pb, "qweight called again");
    gemv(other, 1);
    CHECK(last_forward.flags & TCE_W4_ZERO_POINT_IS_8, "the other linear lost its promise");
    // forget(scales): the copy embeds them
    gemv(l, 1);
    tce_adapter_forget(l.sc);
    expect(3, pb, "forget(scales)");
    fill(l.sc, l.sc_bytes());
    s = snap();
    gemv(l, 4);
    CHECK(calls[kPrepack] - s.c[kPrepack] == 1 && calls[kCheck] == s.c[kCheck], "after forget(scales): %s", since(s).c_str());
    expect(4, 2 * pb, "scales called again");
    // forget(zeros): verdict and copy go; the zero points change 8 -> not 8 in place
    gemv(l, 1);
    tce_adapter_forget(l.zp);
    expect(2, pb, "forget(zeros)");
    set_zeros(l, false);
    s = snap();
    gemv(l, 1);  // F5: an old flag on the rewritten tensor is a violation
    CHECK(calls[kPrepack] - s.c[kPrepack] == 1 && calls[kCheck] - s.c[kCheck] == 1 && !(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "after forget(zeros): %s", since(s).c_str());
    drain();
    for (int M : {1, 1, 200, 5}) {
        gemv(l, M);
        CHECK(!(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "M=%d: promise on zero points that are not 8", M);
    }
    expect(4, 2 * pb, "zeros called again");
    // and back: not 8 -> 8 needs the same forget to get the promise
    tce_adapter_forget(l.zp);
    set_zeros(l, true);
    gemv(l, 1);
    drain();
    gemv(l, 1);
    CHECK(last_forward.flags & TCE_W4_ZERO_POINT_IS_8, "8s again");
    // forget_all: everything is rewritten
    s = snap();
    tce_adapter_forget_all();
    CHECK(calls[kFree] - s.c[kFree] == 2, "forget_all: %s", since(s).c_str());
    expect(0, 0, "forget_all");
    fill(l.qw, l.qw_bytes());
    fill(l.sc, l.sc_bytes());
    set_zeros(l, false);
    fill(other.qw, other.qw_bytes());
    gemv(l, 1);
    gemv(other, 200);
    drain();
    gemv(l, 1);
    gemv(other, 1);
    CHECK(last_forward.flags & TCE_W4_ZERO_POINT_IS_8, "other: 8s");
    gemv(l, 1);
    CHECK(!(last_forward.flags & TCE_W4_ZERO_POINT_IS_8), "l: not 8s");
    expect(4, 2 * pb, "after forget_all, both called");
    // a buffer the adapter never saw, and a null pointer
    tce_adapter_forget(&s);
    tce_adapter_forget(nullptr);
    expect(4, 2 * pb, "forget(unknown)");
    gemv(l, 1);
    tce_adapter_forget_all();
    drop_linear(l);
    drop_linear(other);
    std::printf("forget: qweight, scales, zeros, forget_all, each followed by a rewrite in place: no old flag, no old digest, no freed copy; entries and bytes exact at every step: ok\n");
}

void prepare() {
    tce_adapter_forget_all();
    Linear l = make_linear(16, 512, 64, true), odd = make_linear(16, 1472, 32, true);
    Snap s = snap();
    CHECK(tce_adapter_prepare(nullptr, l.sc, l.zp, l.N, l.K, l.G) == 0 && tce_adapter_prepare(l.qw, nullptr, l.zp, l.N, l.K, l.G) == 0 && tce_adapter_prepare(l.qw, l.sc, nullptr, l.N, l.K, l.G) == 0 &&
              tce_adapter_prepare(l.qw, l.sc, l.zp, 0, l.K, l.G) == 0 && tce_adapter_prepare(l.qw, l.sc, l.zp, l.N, -128, l.G) == 0 && tce_adapter_prepare(l.qw, l.sc, l.zp, l.N, l.K, 48) == 0 &&
              tce_adapter_prepare(l.qw, l.sc, l.zp, l.N, l.K, 0) == 0,
          "a refusal returned bytes");
    CHECK(since(s) == "nothing" && tce_adapter_cache_entries() == 0, "refusals reached the C ABI: %s", since(s).c_str());
    const long long got = tce_adapter_prepare(l.qw, l.sc, l.zp, l.N, l.K, l.G);
    CHECK(got == (long long)pack_bytes(l) && tce_adapter_device_bytes() == got && tce_adapter_cache_entries() == 2, "prepare returned %lld, holds %lld", got, tce_adapter_device_bytes());
    CHECK(calls[kCheck] - s.c[kCheck] == 1 && calls[kPrepack] - s.c[kPrepack] == 1, "prepare: %s", since(s).c_str());
    s = snap();
    CHECK(tce_adapter_prepare(l.qw, l.sc, l.zp, l.N, l.K, l.G) == got, "second prepare");
    CHECK(since(s) == "prepack_bytes=2" && tce_adapter_cache_entries() == 2 && tce_adapter_device_bytes() == got, "preparing twice: %s", since(s).c_str());
    // K % 128 != 0: no copy, but the zero-point check starts
    s = snap();
    CHECK(tce_adapter_prepare(odd.qw, odd.sc, odd.zp, odd.N, odd.K, odd.G) == 0, "K = 1472 has no packed form");
    CHECK(calls[kCheck] - s.c[kCheck] == 1 && calls[kMalloc] == s.c[kMalloc] && tce_adapter_cache_entries() == 3, "prepare K=1472: %s", since(s).c_str());
    drain();
    for (Linear *t : {&l, &odd}) {
        s = snap();
        const long scratch_mallocs = scratch_area ? 0 : 1;
        gemv(*t, 1);  // the first call after prepare + drain: nothing left to build, verdict in -> publishes
        CHECK(published(*t) && (last_forward.flags & TCE_W4_ZERO_POINT_IS_8) && calls[kCheck] == s.c[kCheck] && calls[kPrepack] == s.c[kPrepack] &&
                  calls[kMalloc] - s.c[kMalloc] == (t == &l ? scratch_mallocs : 0),
              "first call after prepare (K=%d): published=%d, %s", t->K, (int)published(*t), since(s).c_str());
        s = snap();
        gemv(*t, 1);
        CHECK(since(s) == "forward=1", "second call after prepare: %s", since(s).c_str());
    }
    tce_adapter_forget_all();
    drop_linear(l);
    drop_linear(odd);
    std::printf("prepare: 7 refusals return 0 and touch nothing, bytes = the copy's, twice = once, the first call after prepare + drain publishes: ok\n");
}

void awq_call(int which, const matmul_params *p) {
    matmul::MatmulOperator op;
    cur_params = p;
    switch (which) {
        case 0: op.gemm_forward_cuda(p, 8); break;
        case 1: op.gemm_forward_cuda_8splits(p, nullptr); break;
        case 2: op.gemm_forward_cuda_half(p, 4); break;
        default: op.gemm_forward_cuda_half_test(p, 1); break;
    }
    cur_params = nullptr;
}
void awq() {
    tce_adapter_forget_all();
    const int N = 24, K = 256, G = 64;
    std::vector<int32_t> qw((size_t)K * N / 8), qw2(qw.size());
    std::vector<uint16_t> sc((size_t)K / 32 * N);  // (room for the G = 32 call below)
    fill(qw.data(), qw.size() * 4);
    fill(qw2.data(), qw2.size() * 4);
    matmul_params p;
    auto set = [&](int32_t *w, int n, int k, int g) {
        std::memset(static_cast<void *>(&p), 0xA5, sizeof(p));
        p.A.half_data_ptr = reinterpret_cast<float16_t *>(t_act.x);
        p.B.row = k;
        p.B.int32_data_ptr = w;
        p.C.row = 3;
        p.C.column = n;
        p.C.half_data_ptr = reinterpret_cast<float16_t *>(t_act.out);
        p.half_scales = reinterpret_cast<float16_t *>(sc.data());
        p.block_size = g;
    };
    const long long ws = 128 + (long long)N * K / 2;
    set(qw.data(), N, K, G);
    for (int which = 0; which < 4; ++which) {
        awq_call(which, &p);
        CHECK(last_repack == (which == 0 ? 1 : 0), "call %d of one tensor: repack = %d", which, last_repack);
    }
    CHECK(tce_adapter_cache_entries() == 1 && tce_adapter_device_bytes() == ws, "entries %ld bytes %lld", tce_adapter_cache_entries(), tce_adapter_device_bytes());
    // another pointer, and the same pointer with another (N, K, G): one re-layout each
    set(qw2.data(), N, K, G);
    awq_call(1, &p);
    CHECK(last_repack == 1, "another pointer");
    awq_call(2, &p);
    CHECK(last_repack == 0, "another pointer, again");
    set(qw.data(), N, K, 32);
    awq_call(0, &p);
    CHECK(last_repack == 1, "another group size");
    set(qw.data(), N / 3, K * 3, G);
    awq_call(3, &p);
    CHECK(last_repack == 1, "another (N, K)");
    awq_call(3, &p);
    CHECK(last_repack == 0, "another (N, K), again");
    CHECK(tce_adapter_cache_entries() == 4 && tce_adapter_device_bytes() == 4 * ws, "entries %ld bytes %lld", tce_adapter_cache_entries(), tce_adapter_device_bytes());
    // a null pointer names no buffer (an AWQ entry has no side tensors: its scales / zeros fields are null, and a forget(NULL) that compared them dropped every re-layout)
    tce_adapter_forget(nullptr);
    CHECK(tce_adapter_cache_entries() == 4 && tce_adapter_device_bytes() == 4 * ws, "forget(NULL): entries %ld bytes %lld", tce_adapter_cache_entries(), tce_adapter_device_bytes());
    // forget + rewrite: the next call re-lays the weights out (the stand-in refuses repack = 0 on a workspace built from other bytes)
    Snap s = snap();
    tce_adapter_forget(qw.data());
    CHECK(calls[kFree] - s.c[kFree] == 3 && tce_adapter_cache_entries() == 1, "forget(qweight) of three shapes: %s, entries %ld", since(s).c_str(), tce_adapter_cache_entries());
    fill(qw.data(), qw.size() * 4);
    set(qw.data(), N, K, G);
    awq_call(0, &p);
    CHECK(last_repack == 1, "after forget");
    awq_call(1, &p);
    CHECK(last_repack == 0, "after forget, again");
    tce_adapter_forget_all();
    CHECK(tce_adapter_cache_entries() == 0 && tce_adapter_device_bytes() == 0, "forget_all");
    // an unsupported group: the message and exit(1), like the reference
    std::string out;
    set(qw.data(), N, K, 48);
    int rc = in_child([&] { awq_call(0, &p); }, &out);
    CHECK(rc == 1 && out.find("gemm_forward_cuda") != std::string::npos && out.find("tce error -2") != std::string::npos, "gemm_forward_cuda G=48: exit %d, output '%s'", rc, out.c_str());
    out.clear();
    Linear l = make_linear(16, 512, 128, true);
    l.G = 48;
    rc = in_child([&] { gemv(l, 1); }, &out);
    CHECK(rc == 1 && out.find("Unsupported group size: 48") != std::string::npos, "gemv_forward_cuda G=48: exit %d, output '%s'", rc, out.c_str());
    drop_linear(l);
    std::printf("awq: gemm_forward_cuda and its three aliases re-lay out once per (pointer, N, K, G) and again after forget; group 48 exits 1 with the message: ok\n");
}

void int8_members() {
    using Member = void (matmul::MatmulOperator::*)(const matmul_params *);
    const struct {
        Member fn;
        int bias_kind, out_kind, b_per_row;
        const char *name;
    } table[8] = {
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll, TCE_BIAS_INT8, TCE_OUT_INT8, 0, "2x2_32unroll"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_32unroll_over_column, TCE_BIAS_INT8, TCE_OUT_INT8, 0, "32unroll_over_column"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias, TCE_BIAS_NONE, TCE_OUT_INT8, 0, "nobias"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_batch, TCE_BIAS_NONE, TCE_OUT_INT8, 1, "nobias_batch"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32, TCE_BIAS_FP32, TCE_OUT_FP32, 0, "bfp32_ofp32"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32_over_column, TCE_BIAS_FP32, TCE_OUT_FP32, 0, "bfp32_ofp32_over_column"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32, TCE_BIAS_NONE, TCE_OUT_FP32, 0, "nobias_ofp32"},
        {&matmul::MatmulOperator::mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32_batch, TCE_BIAS_NONE, TCE_OUT_FP32, 1, "nobias_ofp32_batch"},
    };
    static int8_t a8[8], b8[8], c8[8], bias8[8];
    static float cf[8], biasf[8];
    matmul_params p;
    auto set = [&] {
        std::memset(static_cast<void *>(&p), 0xA5, sizeof(p));
        p.A.row = 3, p.A.column = 96, p.A.int8_data_ptr = a8;
        p.B.row = 96, p.B.column = 40, p.B.int8_data_ptr = b8;
        p.C.row = 3, p.C.column = 40, p.C.int8_data_ptr = c8, p.C.data_ptr = cf;
        p.C.qparams.q_min = -7, p.C.qparams.q_max = 99;
        p.bias.int8_data_ptr = bias8, p.bias.data_ptr = biasf;
        p.alpha = 0.375f, p.beta = -1.5f;
    };
    for (const auto &t : table) {
        set();
        std::memset(&last_w8a8, 0xEE, sizeof(last_w8a8));
        const long before = calls[kW8a8];
        matmul::MatmulOperator op;
        (op.*t.fn)(&p);
        const tce_w8a8_desc &d = last_w8a8;
        const void *bias = t.bias_kind == TCE_BIAS_INT8 ? (const void *)bias8 : (t.bias_kind == TCE_BIAS_FP32 ? (const void *)biasf : nullptr);
        const void *out = t.out_kind == TCE_OUT_INT8 ? (const void *)c8 : (const void *)cf;
        CHECK(calls[kW8a8] - before == 1 && d.M == 3 && d.N == 40 && d.K == 96 && d.batch == 1 && d.A == a8 && d.B == b8 && d.bias == bias && d.C == out && d.alpha == 0.375f && d.beta == -1.5f &&
                  d.q_min == -7 && d.q_max == 99 && d.bias_kind == t.bias_kind && d.out_kind == t.out_kind && d.b_per_row == t.b_per_row,
              "%s: bias_kind %d out_kind %d b_per_row %d q [%d, %d]", t.name, d.bias_kind, d.out_kind, d.b_per_row, d.q_min, d.q_max);
        CHECK(!d.strideA && !d.strideB && !d.strideC && !d.accumulate && !d.lda && !d.ldb && !d.ldc && !d.reserved2, "%s: a field the adapter never sets is non-zero", t.name);
    }
    int bad = 0;
    for (int which = 0; which < 3; ++which) {  // A.column != B.row; C.row != A.row; C.column != B.column
        set();
        if (which == 0) p.B.row = 95;
        if (which == 1) p.C.row = 4;
        if (which == 2) p.C.column = 48;
        std::string out;
        const int rc = in_child([&] { matmul::MatmulOperator op; (op.*table[which * 3].fn)(&p); }, &out);
        CHECK(rc == 1 && out.find("assertion failed") != std::string::npos, "shape assertion %d: exit %d, output '%s'", which, rc, out.c_str());
        bad += rc == 1;
    }
    std::printf("int8 members: 8 members pass their name's bias_kind / out_kind / b_per_row and C.qparams' clamp; %d of 3 shape mismatches exit 1: ok\n", bad);
}

// Tensors whose weight addresses share one front_slot(): up to two live in the window, the others stay on the slow path, and NO steady-state token allocates.
bool collisions() {
    const size_t arena_bytes = 64u << 20, stride = 1024;  // a tensor below is 1024 bytes of weights; only the pages of the chosen tensors are touched
    unsigned char *arena = static_cast<unsigned char *>(std::aligned_alloc(4096, arena_bytes));
    std::vector<std::vector<size_t>> by_slot(kFrontSize);
    size_t slot = kFrontSize;
    for (size_t off = 0; off + stride <= arena_bytes && slot == kFrontSize; off += stride) {
        auto &v = by_slot[front_slot(arena + off)];
        v.push_back(off);
        if (v.size() == 9) slot = front_slot(arena + off);
    }
    if (slot == kFrontSize) {
        violation("no 9 addresses of one front_slot() in a %zu MiB arena", arena_bytes >> 20);
        return false;
    }
    bool ok = true;
    for (int n : {2, 3, 4, 9}) {
        tce_adapter_forget_all();  // every entry the earlier scenarios published is stale: both probes of the window are free
        std::vector<Linear> ls;
        for (int i = 0; i < n; ++i) ls.push_back(make_linear(16, 128, 128, i % 2 == 0, arena + by_slot[slot][i]));
        for (auto &l : ls) gemv(l, 1);
        drain();
        long at10 = 0, news10 = 0;
        Snap s10{};
        const int before = failures.load();
        for (int token = 1; token <= 1000; ++token) {
            for (auto &l : ls) gemv(l, 1);  // (F1-F6 on every call)
            if (token == 10) at10 = retired() + front_live(), news10 = g_news.load(), s10 = snap();
        }
        const long at1000 = retired() + front_live(), news = g_news.load() - news10;
        int hits = 0;
        for (auto &l : ls) hits += published(l);
        const long forwards = calls[kForward] - s10.c[kForward], slow = calls[kPrepackBytes] - s10.c[kPrepackBytes];
        const bool good = at1000 == at10 && news == 0 && forwards == 990L * n && hits == (n < 2 ? n : 2) && slow == 990L * (n - hits) && failures.load() == before;
        std::printf("collisions: %d tensors on slot %zu, tokens 11..1000: forward %ld, slow-path calls %ld, published %d, retired + live entries %ld -> %ld, allocations %ld: %s\n", n, slot, forwards,
                    slow, hits, at10, at1000, news, good ? "ok" : "FAIL");
        if (!good) violation("collisions n=%d: a steady-state token allocates or a tensor within the window's two ways misses", n);
        ok &= good;
        tce_adapter_forget_all();
        for (auto &l : ls) drop_linear(l, /*own_qw=*/false);
    }
    std::free(arena);
    return ok;
}

void threads() {
    tce_adapter_forget_all();
    const int kLinears = 64, kThreads = 4, kTokens = 300;
    std::vector<Linear> ls;
    for (int i = 0; i < kLinears; ++i) ls.push_back(make_linear(16, 128 << (i % 3), i % 2 ? 64 : 128, i % 5 != 0));
    threaded = true;
    std::atomic<int> done{0}, progress{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreads; ++t)
        pool.emplace_back([&, t] {
            for (int token = 0; token < kTokens; ++token) {
                const int M = (token + t) % 2 ? 200 : 1;
                for (auto &l : ls) gemv(l, M);
                if (t == 0) progress.store(token);
            }
            done.fetch_add(1);
        });
    std::thread forgetter([&] {  // tensors nobody rewrites; stops 50 tokens before the end so that the survivors are all of them
        unsigned i = 0;
        long at = 0;
        while (progress.load() < kTokens - 50 && done.load() == 0) {
            if (calls[kForward].load() - at < 64) {  // one forget per 64 calls of the workers: ~900 in all
                std::this_thread::yield();
                continue;
            }
            at = calls[kForward].load();
            if (++i % 16 == 0) tce_adapter_forget_all();
            else tce_adapter_forget(ls[(i * 7) % kLinears].zp);
        }
    });
    for (long at = 0; done.load() < kThreads;) {  // the device runs alongside: it catches up every 16 calls
        if (calls[kForward].load() - at < 16) {
            std::this_thread::yield();
            continue;
        }
        at = calls[kForward].load();
        drain_threaded();
    }
    for (auto &th : pool) th.join();
    forgetter.join();
    drain_threaded();
    threaded = false;
    const long entries = tce_adapter_cache_entries();
    const long long bytes = tce_adapter_device_bytes();
    // every promise the threads left behind is still held to F5 / F6, single-threaded
    for (auto &l : ls) gemv(l, 1);
    drain();
    for (auto &l : ls) gemv(l, 1);
    // the replay: the same tensors, one thread, from nothing
    tce_adapter_forget_all();
    for (int M : {1, 200})
        for (auto &l : ls) gemv(l, M);
    drain();
    CHECK(entries == tce_adapter_cache_entries() && bytes == tce_adapter_device_bytes(), "threads left %ld entries / %lld bytes, the single-threaded replay %ld / %lld", entries, bytes,
          tce_adapter_cache_entries(), tce_adapter_device_bytes());
    CHECK(entries == 2L * kLinears, "entries %ld", entries);
    tce_adapter_forget_all();
    std::printf("threads: %d threads x %d tokens x %d linears, M = 1 / 200, beside forget(zeros) / forget_all: %ld entries = the single-threaded replay; %ld calls lost the race against a forget: ok\n",
                kThreads, kTokens, kLinears, entries, raced.load());
    for (auto &l : ls) drop_linear(l);
}

}  // namespace

int main() {
    if (std::getenv("TCE_ADAPTER_PACK")) {
        std::printf("TCE_ADAPTER_PACK is set: the rules above are those of the default\n");
        return 2;
    }
    steady_state();
    m_classes();
    identity();
    forget();
    prepare();
    awq();
    int8_members();
    collisions();
    threads();  // last: the scenarios above fork
    CHECK(tce_adapter_gemm_faults() == 0, "gemm faults");
    const int f = failures.load();
    std::printf("adapter state: %s (%d violations)\n", f ? "FAILED" : "ok", f);
    return f ? 1 : 0;
}
