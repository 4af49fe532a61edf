// sampling.hip -- the piece between lm_head's output and the next step's input, on the device (include/tce_matmul.h: tce_sample_f16, tce_embed_rows_f16).
//
// The reference samples on the host (llm/src/Generate.cc driven by LLaMA3Generate.cc:127-198): penalties over the recent-token window, then greedy, or
// top-k -> softmax -> top-p -> temperature -> softmax -> draw, all in fp32 on the half2float'ed logits.  Here the same chain runs for B rows in TWO launches, so that
// a captured decode graph produces a token per replay without a host round trip:
//
//   1  sample_select_kernel   grid (vocab chunks of 4096, B): 16-byte loads, 16 logits per thread in registers; the <= 64 penalised ids of the row are patched in
//                             through a per-thread bit mask (no membership test per vocabulary entry); every logit becomes an order-preserving 32-bit key and
//                             (key, 4095 - index) a 44-bit number that is DISTINCT per element, so "the chunk's k largest, lowest id first among equals" is one
//                             bitwise threshold search (44 counting rounds: ballots + one barrier each; no atomics on the data, no sort).  The k survivors of
//                             each chunk go to the workspace.
//   2  sample_draw_kernel     grid (B): the chunks' survivors (chunks x k <= 8192, in registers) through the same search with (key, ~id), a rank sort of the k
//                             winners, then the reference's arithmetic in the reference's order -- expf, SEQUENTIAL fp32 sums, IEEE divisions -- top-p with the
//                             reference's quirk, temperature, the second softmax, the inverse-CDF draw; and the tail that closes the loop: token, log, ring,
//                             counters, position (or retirement).
//
// The kernel boundary is the only ordering between the two: no counters, no flags, nothing to reset -- launch 200 of a workspace is launch 1.
// A row whose position word is < 0 or > pos_bound is skipped by both kernels before it reads anything of the row.
//
// LOG-PROBABILITIES (tce_sample_logprobs_f16, tce_sample_verify_logprobs_f16, tce_logprobs_f16): logprob = x_t - LSE(x) on the RAW fp16 logits widened to fp32 -- the
// model's distribution, whatever the penalties, top-k, top-p, temperature, seed or slot.  The LSE = true forms of the two kernels carry it along: the select launch
// already holds the chunk's 16 logits per thread and stores the chunk's pair (m_c, s_c = sum expf(x_i - m_c)) before it patches the penalties in; the draw launch
// merges the row's <= 256 pairs and subtracts.  The summation order is FIXED (chunk_lse_pair, merge_lse below), so a value does not depend on the batch, the slot or
// the entry point: scoring (logprobs_partials_kernel -> logprobs_merge_kernel) calls the same two device functions.  The LSE = false forms are the code they were.
//
// CONSTRAINED DECODING (tce_sample_constrained_f16, tce_sample_verify_constrained_f16; the rules are in include/tce_matmul.h): the CON = true forms of the three sampler
// kernels.  Select tests a bit of mask[state] before a logit becomes a key and patches the row's <= 16 bias pairs in beside the penalties; draw treats "no survivor" and
// an invalid transition as one path (nothing emitted, the row retires, *violations += 1) and stores the next state in the tail; the verifier walks the drafts' transitions
// to know each virtual row's state in advance.  fsm_next is the one edge lookup of all three.  The CON = false forms declare nothing new and compile to the instructions
// they were (profiles/constrained/).
//
// TAIL-FREE AND TYPICAL SAMPLING (tce_sample_stages_f16, tce_sample_verify_stages_f16; the rules are in include/tce_matmul.h): the STG = true forms of the draw kernel
// run the reference's sample_tail_free and sample_typical between the rank sort and top-p, on the candidates already in LDS, with the two values per slot in a
// tce_stage_row.  The select and chain kernels are the underlying form's own.  The STG = false forms declare nothing new -- not even a local variable -- and compile to
// the instructions they were (profiles/sampler_stages/).
//
// MIROSTAT (tce_sample_mirostat_f16; the rule and its three deviations from the reference are in include/tce_matmul.h): the MIRO = true forms of the draw kernel, on
// top of the plain STG = true forms.  A row whose tce_mirostat_row says mode 1 or 2 runs temperature -> softmax -> sample_token_mirostat[_v2]'s cut -> softmax -> draw
// on its sorted candidates and thread 0 stores the new mu beside the token; every other row takes the STG = true path.  The MIRO = false forms compile to the
// instructions they were (profiles/mirostat/).  The verifier (tce_sample_verify_mirostat_f16) takes a fourth launch, sample_miro_walk_kernel: see MiroRowWs below.
#include "tce_common.hpp"

#include <type_traits>

namespace tce {

namespace {

constexpr int kChunk = 4096;  // logits per workgroup of the select launch: 256 threads x 16
constexpr int kThreads = 256;
constexpr int kMaxK = 256;
constexpr int kMergePerThread = 32;  // the draw launch holds chunks x k <= 256 x 32 survivors in registers

typedef unsigned long long u64;
typedef float float2_t __attribute__((ext_vector_type(2)));  // a chunk's (m_c, s_c): one 8-byte store / load

// fp32 -> 32-bit integer with the same order (-0 and +0 are one value for the reference's comparisons: both map to +0's key).  0 is kept for "no element".
__device__ __forceinline__ unsigned order_key(float x) {
    x = x == 0.0f ? 0.0f : x;
    unsigned u = __builtin_bit_cast(unsigned, x);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return u ? u : 1u;
}
__device__ __forceinline__ float key_value(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}

__device__ __forceinline__ bool row_active(const int32_t *pos, int b, int pos_bound) {
    const int p = pos[b];
    return p >= 0 && p <= pos_bound;
}

__device__ __forceinline__ int row_k(const tce_sample_row &r, int kbound) {
    if (r.temp <= 0.0f) return 1;  // greedy: the first maximum = the largest (key, lowest id)
    const int k = r.top_k < 1 ? 1 : r.top_k;
    return k > kbound ? kbound : k;
}

// the number of threads of the workgroup (4 waves) whose `pred` holds, summed over `n` predicates per thread by the caller: per wave a ballot and a scalar
// population count per predicate, across waves two alternating LDS rows (one barrier per round)
__device__ __forceinline__ int block_total(int wave_count, int (*cnt)[4], int round, int wave, int lane) {
    if (lane == 0) cnt[round & 1][wave] = wave_count;
    __syncthreads();
    return cnt[round & 1][0] + cnt[round & 1][1] + cnt[round & 1][2] + cnt[round & 1][3];
}

// ---- log-sum-exp in two levels; every sum in one written-down order ----
// The chunk's pair for x[16] = the thread's logits (index i0 + e) BEFORE any penalty: m_c = the maximum of the chunk's in-vocabulary values, s_c = sum expf(x_i - m_c).
//   per thread   e = 0 .. 15 in index order, sequentially
//   per wave     a butterfly: s += s of lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32 (fp32 addition commutes, so all 64 lanes hold the same bits)
//   across waves ((w0 + w1) + w2) + w3
// An entry past `vocab` and a -inf logit contribute exactly 0 and do not move the maximum, so a chunk of -inf only gives (-inf, 0).  A NaN logit is not a maximum
// (fmaxf drops it) but its term is NaN; a +inf logit gives expf(inf - inf) = NaN: both make s_c, and with it the row's LSE, NaN.  Returned to every thread.
__device__ __forceinline__ float2_t chunk_lse_pair(const float (&x)[16], int i0, int vocab, int wave, int lane) {
    __shared__ float wave_max[4], wave_sum[4];
    const float ninf = -__builtin_inff();
    float m = ninf;
#pragma unroll
    for (int e = 0; e < 16; ++e) m = fmaxf(m, i0 + e < vocab ? x[e] : ninf);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) s += (i0 + e < vocab && x[e] != ninf) ? expf(x[e] - m) : 0.0f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
    if (lane == 0) wave_sum[wave] = s;
    __syncthreads();
    float2_t pair;
    pair.x = m;
    pair.y = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
    return pair;
}

// The row's LSE from its nchunks (<= 256 = kThreads) pairs: thread c < nchunks holds pair c; M = the workgroup's maximum of m_c; the term of pair c is
// s_c * expf(m_c - M), exactly 0 where s_c == 0 (a chunk of -inf; also where the whole row is -inf and m_c - M would be inf - inf); S = the terms through a FIXED tree --
// the wave butterfly above (6 levels), then (w0 + w1) + (w2 + w3) --, never a sequential sum over the chunks; lse = M + logf(S).  A row of -inf only: -inf + logf(0) =
// -inf, and x_t - lse = NaN.  Returned to every thread.
__device__ __forceinline__ float merge_lse(const float2_t *pairs, int nchunks, int tid, int wave, int lane) {
    __shared__ float merge_max[4], merge_sum[4];
    const float ninf = -__builtin_inff();
    float2_t p;
    p.x = ninf;
    p.y = 0.0f;
    if (tid < nchunks) p = pairs[tid];
    float M = p.x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) M = fmaxf(M, __shfl_xor(M, off));
    if (lane == 0) merge_max[wave] = M;
    __syncthreads();
    M = fmaxf(fmaxf(merge_max[0], merge_max[1]), fmaxf(merge_max[2], merge_max[3]));
    float S = p.y == 0.0f ? 0.0f : p.y * expf(p.x - M);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) S += __shfl_xor(S, off);
    if (lane == 0) merge_sum[wave] = S;
    __syncthreads();
    S = (merge_sum[0] + merge_sum[1]) + (merge_sum[2] + merge_sum[3]);
    return M + logf(S);
}

// ---- constrained decoding (tce_sample_constrained_f16, tce_sample_verify_constrained_f16): the CON = true forms ----
// The automaton's transition: the edge of state s that carries tok (binary search: edge_token ascends within a state), else the state's default.  The ONE lookup of
// the select launch's walk, the draw launch's tail and the chain launch.  The caller has checked s against [0, states) and checks the result against [-1, states).
__device__ __forceinline__ int fsm_next(const tce_fsm &f, int s, int tok) {
    int lo = f.edge_begin[s];
    const int end = f.edge_begin[s + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (f.edge_token[mid] < tok) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && f.edge_token[lo] == tok ? f.edge_next[lo] : f.default_next[s];
}
__device__ __forceinline__ bool fsm_state_ok(const tce_constraint &con, int fsm, int s) { return fsm < con.n_fsm && s >= 0 && s < con.fsms[fsm].states; }
__device__ __forceinline__ bool fsm_allows(const tce_fsm &f, int s, int tok, int vocab) {
    if (tok < 0 || tok >= vocab || (tok >> 5) >= f.mask_words) return false;
    return (f.mask[(size_t)s * f.mask_words + (tok >> 5)] >> (tok & 31)) & 1u;
}
// The state virtual row vt of a constrained sequence is sampled in: delta*(state, drafts 1 .. vt) (drafts[j] = draft j + 1), or -1 where the row cannot be reached (the
// base state is invalid -- row 0 then carries rule 6 --, or a draft is forbidden or its transition DONE or invalid).  At most TCE_SPEC_MAX_ROWS - 1 transitions.
__device__ __forceinline__ int fsm_walk(const tce_constraint &con, int fsm, int s, const int32_t *drafts, int vt, int vocab) {
    if (!fsm_state_ok(con, fsm, s)) return -1;
    const tce_fsm &f = con.fsms[fsm];
    for (int j = 0; j < vt; ++j) {
        const int d = drafts[j];
        if (!fsm_allows(f, s, d, vocab)) return -1;
        s = fsm_next(f, s, d);
        if (s < 0 || s >= f.states) return -1;
    }
    return s;
}
__device__ __forceinline__ int &con_next_word() {  // the draw launch's LDS word for thread 0's lookup (only the CON = true forms instantiate it)
    __shared__ int word;
    return word;
}
// the chain launch's state of a sequence's automaton; the CON = false forms hold an empty struct instead, so that they declare nothing new
struct ChainCon {
    int fsm = -1, state = 0, nx = 0;
    bool invalid = false;
};
struct NoCon {};
template <class Base>
struct ConArgs : Base {  // the CON = true forms' arguments: the base form's, then the constraint (the CON = false instantiations keep their argument layout)
    tce_constraint con;
};

// SPEC (tce_sample_verify_f16): blockIdx.y is a VIRTUAL row y = seq * RT + t -- logits row, position word (row_pos) and survivors are y's, the sampling row is seq's.
// Row t is only ever used when drafts 1 .. t were all accepted, so the window it must be sampled with is known now: the ring as it stands with row_token[(seq, 1)] ..
// row_token[(seq, t)] pushed behind it.
// LSE: the chunk's pair of the RAW logits goes to partials[row][chunk] (one 8-byte store) before the penalties are patched in.
// CON: the thread's 16 logits are one half of one word of mask[state]; a cleared bit gives key 0 ("no element").  The row -> descriptor -> mask word loads are issued
// in front of the logits loads (three dependent round trips that should hide under them; SPEC rows behind row 0 wait for thread 0's walk instead).  The row's bias ids
// join the patch path (<= 64 + 16 ids): an id both biased and penalised is patched by its window thread with penalty(raw + bias).  An invalid or unreachable row
// writes k "no element" entries per chunk and searches nothing: the draw launch finds no candidate and takes rule 6's path (SPEC: cand = -1).
template <bool SPEC, bool LSE, bool CON>
__global__ __launch_bounds__(kThreads) void sample_select_kernel(const half_t *logits, int ld, int vocab, const tce_sample_row *rows, const int32_t *pos, int pos_bound,
                                                                  int kbound, uint2_t *entries, int nchunks, int RT, const int32_t *row_token,
                                                                  [[maybe_unused]] float2_t *partials, [[maybe_unused]] tce_constraint con) {
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!row_active(pos, b, pos_bound)) return;
    [[maybe_unused]] const int seq = SPEC ? b / RT : b, vt = SPEC ? b - seq * RT : 0;
    constexpr int kPatch = CON ? 64 + TCE_BIAS_MAX : 64;
    __shared__ int win_id[64], pen_id[kPatch];
    __shared__ float pen_val[kPatch];
    __shared__ unsigned mask[kThreads];
    __shared__ int cnt[2][4];
    __shared__ int nsel;
    const tce_sample_row &r = rows[SPEC ? seq : b];
    const int k = row_k(r, kbound);
    const half_t *row = logits + (size_t)b * ld;
    const int base = c * kChunk, i0 = base + tid * 16;

    [[maybe_unused]] unsigned allow = 0xFFFFu;  // CON: bit e = entry i0 + e may be a candidate
    [[maybe_unused]] int nbias = 0;
    [[maybe_unused]] bool dead = false;          // CON: an invalid or unreachable row
    if constexpr (CON) {
        __shared__ int walked;
        const tce_constraint_row &cr = con.rows[seq];
        const int fsm = cr.fsm;
        int s = cr.state;
        nbias = cr.n_bias < 0 ? 0 : (cr.n_bias > TCE_BIAS_MAX ? TCE_BIAS_MAX : cr.n_bias);
        if (fsm >= 0) {
            if (SPEC && vt > 0) {  // (uniform) the state behind drafts 1 .. vt: one thread walks, the workgroup waits
                if (tid == 0) walked = fsm_walk(con, fsm, s, row_token + b - vt + 1, vt, vocab);
                __syncthreads();
                s = walked;
                dead = s < 0;
            } else {
                dead = !fsm_state_ok(con, fsm, s);
            }
            allow = 0u;
            if (!dead && i0 < vocab) {
                const tce_fsm &f = con.fsms[fsm];
                if ((i0 >> 5) < f.mask_words) allow = (f.mask[(size_t)s * f.mask_words + (i0 >> 5)] >> (i0 & 16)) & 0xFFFFu;
            }
        }
    }

    float x[16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        half8_t v = {};
        if (i0 + 8 * h < vocab) v = *reinterpret_cast<const half8_t *>(row + i0 + 8 * h);  // (a piece across `vocab` stays inside the row: vocab <= ld, ld % 8 == 0)
#pragma unroll
        for (int j = 0; j < 8; ++j) x[8 * h + j] = (float)v[j];
    }
    if constexpr (CON) {
        if (dead) {  // (uniform) k "no element" entries and nothing else
            if (tid < k) {
                uint2_t ent;
                ent.x = 0u;
                ent.y = 0u;
                entries[((size_t)b * nchunks + c) * kMaxK + tid] = ent;
            }
            return;
        }
    }
    if constexpr (LSE) {
        const float2_t pair = chunk_lse_pair(x, i0, vocab, wave, lane);
        if (tid == 0) partials[(size_t)b * nchunks + c] = pair;
    }

    // ---- penalties: window slot t < nwin is the t-th most recent token of the ring; the first occurrence of an id that lies in this chunk patches its logit ----
    const float rp = r.repeat_penalty, af = r.alpha_frequency, ap = r.alpha_presence;
    const bool freq_on = !(af == 0.0f && ap == 0.0f);
    const int nwin = r.repeat_last_n < 0 ? 0 : (r.repeat_last_n > 64 ? 64 : r.repeat_last_n);
    mask[tid] = 0;
    if (tid == 0) nsel = 0;
    if (tid < 64) {
        if constexpr (SPEC) win_id[tid] = tid >= nwin ? -1 : tid < vt ? row_token[b - tid] : r.ring[(r.ring_pushed - 1u - (unsigned)(tid - vt)) & 63u];
        else win_id[tid] = tid < nwin ? r.ring[(r.ring_pushed - 1u - (unsigned)tid) & 63u] : -1;
        pen_id[tid] = -1;
    }
    if constexpr (CON) {
        if (tid >= 64 && tid < kPatch) pen_id[tid] = -1;
    }
    __syncthreads();
    if constexpr (CON) {  // thread 64 + j: bias pair j, where its id lies in this chunk, is the id's first pair and no window thread patches the id
        const int j = tid - 64;
        if (j >= 0 && j < nbias) {
            const tce_constraint_row &cr = con.rows[seq];
            const int id = cr.bias_id[j];
            if (id >= base && id < base + kChunk && id < vocab) {
                bool mine = true;
                for (int i = 0; i < j; ++i) mine = mine && cr.bias_id[i] != id;
                if (rp != 1.0f || freq_on)
                    for (int i = 0; i < nwin; ++i) mine = mine && win_id[i] != id;
                if (mine) {
                    float v = (float)row[id];
                    for (int i = j; i < nbias; ++i)
                        if (cr.bias_id[i] == id) v = v + cr.bias_val[i];
                    pen_id[tid] = id;
                    pen_val[tid] = v;
                    atomicOr(&mask[(id - base) >> 4], 1u << ((id - base) & 15));
                }
            }
        }
    }
    if ((rp != 1.0f || freq_on) && tid < nwin) {
        const int id = win_id[tid];
        if (id >= base && id < base + kChunk && id < vocab) {
            int count = 0;
            bool first = true;
            for (int j = 0; j < nwin; ++j) {
                const bool same = win_id[j] == id;
                count += same ? 1 : 0;
                first = first && !(same && j < tid);
            }
            if (first) {
                float v = (float)row[id];
                if constexpr (CON) {
                    const tce_constraint_row &cr = con.rows[seq];
                    for (int i = 0; i < nbias; ++i)
                        if (cr.bias_id[i] == id) v = v + cr.bias_val[i];
                }
                if (rp != 1.0f) v = v <= 0.0f ? v * rp : v / rp;                   // sample_repetition_penalty (Generate.cc:26-30)
                if (freq_on) v = v - ((float)count * af + 1.0f * ap);             // sample_frequency_and_presence_penalties (:56)
                pen_id[tid] = id;
                pen_val[tid] = v;
                atomicOr(&mask[(id - base) >> 4], 1u << ((id - base) & 15));
            }
        }
    }
    __syncthreads();
    const unsigned m = mask[tid];
    if (m) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if ((m >> e) & 1u) {
                for (int j = 0; j < kPatch; ++j)
                    if (pen_id[j] == i0 + e) x[e] = pen_val[j];
            }
        }
    }

    // ---- the chunk's k largest (key, lowest index first): a bitwise search for the k-th largest of 4096 distinct 44-bit numbers ----
    u64 comp[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        unsigned key = i0 + e < vocab ? order_key(x[e]) : 0u;
        if constexpr (CON) key = (allow >> e) & 1u ? key : 0u;
        comp[e] = ((u64)key << 12) | (u64)(0xFFF - (tid * 16 + e));
    }
    u64 T = 0;
    for (int bit = 43; bit >= 0; --bit) {
        const u64 cand = T | (1ull << bit);
        int cw = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) cw += __builtin_popcountll(__ballot(comp[e] >= cand));
        if (block_total(cw, cnt, bit, wave, lane) >= k) T = cand;
    }
    // exactly k numbers are >= T (they are distinct and there are 4096 >= k of them); those past the vocabulary (key 0) are dropped
    uint2_t *out = entries + ((size_t)b * nchunks + c) * kMaxK;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const unsigned key = (unsigned)(comp[e] >> 12);
        if (comp[e] >= T && key != 0u) {
            const int slot = atomicAdd(&nsel, 1);
            if (slot < kMaxK) {
                uint2_t ent;
                ent.x = key;
                ent.y = (unsigned)(i0 + e);
                out[slot] = ent;
            }
        }
    }
    __syncthreads();
    if (tid >= nsel && tid < k) {
        uint2_t ent;
        ent.x = 0u;
        ent.y = 0u;
        out[tid] = ent;  // "no element": the draw launch reads k entries of every chunk
    }
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter (c0, 0, 0, 0), key (k0, k1); the first output word.
__device__ __forceinline__ unsigned philox4x32_10_first(unsigned c0, unsigned k0, unsigned k1) {
    unsigned c[4] = {c0, 0u, 0u, 0u};
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const u64 p0 = (u64)0xD2511F53u * c[0], p1 = (u64)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c[0];
}

struct DrawArgs {
    const uint2_t *entries;
    int nchunks, kbound, pos_bound, log_stride;
    tce_sample_row *rows;
    int32_t *pos, *next_token, *out_log;
    const float *uniform_override;
    tce_sample_debug *debug;
    int32_t stop_ids[4];
    int n_stop;
};

// the LSE = true forms' arguments: a struct of their own (DrawArgs first), so the LSE = false instantiations keep their argument layout
struct DrawLseArgs : DrawArgs {
    const half_t *logits;     // the rows the select launch read: [rows][ld]
    int ld, vocab;
    const float2_t *partials; // [rows][nchunks]
    float *out_logprob;       // [batch][log_stride] (the plain form; the chain launch writes it in the SPEC form)
    float *last_lse;          // [batch] or null (as out_logprob)
    float *cand_logprob, *cand_lse;  // SPEC: [batch * T] beside cand
};

// tce_sample_verify_f16's second and third launch: DrawArgs (pos = the SEQUENCES' position words) and the per-virtual-row arrays
struct VerifyArgs {
    DrawArgs d;
    int T, hist_stride, batch;
    const int32_t *row_token, *row_pos;
    int32_t *cand;  // [batch * T]: the token virtual row y would emit
    int32_t *history, *emitted;
};

// SPEC: blockIdx.x is a virtual row y = seq * RT + t (a.pos = row_pos): the draw of token generated + t of the sequence, into cand[y]; no state is written
// LSE: the row's log-sum-exp from the select launch's pairs (merge_lse); logprob = the RAW logit of the token drawn - lse, written beside the token.
// CON: no survivor at all (V == 0: an invalid or unreachable row, or a state that allows nothing inside the vocabulary) is rule 6 -- the row retires, *violations += 1,
// nothing else is written (SPEC: cand = -1, the chain launch applies the rule).  Otherwise thread 0 looks the drawn token's transition up (fsm_next) BEFORE anything
// is written: a next outside [-1, states) is rule 6 again; DONE retires the row behind the token like a stop id; any other next is stored as the state, in the tail.
// STG (tce_sample_stages_f16, tce_sample_verify_stages_f16; the rules are in include/tce_matmul.h): sample_tail_free and sample_typical (Generate.cc:203-302) between
// the rank sort and top-p, on the <= 256 sorted candidates in LDS and in the kernel's idiom -- per-element work on threads < kk, every thread walks the sequential sums
// itself.  Tail-free cuts the sorted candidates to n1; typical ranks the n1 by |-logf(p) - H| (the 256 x 256 count that sorted the winners; equal scores keep their
// order), cuts to n2 and PERMUTES lg / ids, so that top-p, temperature, the draw, the constraint lookup and the tail read the final order unchanged.  A row whose two
// values are both >= 1.0 takes neither branch and recomputes nothing: its arithmetic is the STG = false form's.  The STG = false forms declare nothing new.
struct StgLds {  // the STG = true forms' LDS (only they instantiate it): the sorted candidates, the softmax top-p walks, d2 / the scores, the order by score
    float sv_lg[kMaxK], pq[kMaxK + 8], sc[kMaxK + 8];
    int sv_id[kMaxK], ord[kMaxK];
    int n1, n2, permuted, recomputed;  // thread 0's, for the debug record: a local variable, even an unused one, changes the STG = false forms' code
};
__device__ __forceinline__ StgLds &stg_lds() {
    __shared__ StgLds s;
    return s;
}
template <class Base>
struct StgArgs : Base {  // the STG = true forms' arguments: the underlying form's, then the stage rows (the STG = false instantiations keep their argument layout)
    const tce_stage_row *srows;  // [batch] (SPEC: per sequence)
    tce_stage_debug *sdebug;     // [rows] or null
};
template <bool LSE, bool CON>
using DrawArgsBase = std::conditional_t<CON, ConArgs<std::conditional_t<LSE, DrawLseArgs, DrawArgs>>, std::conditional_t<LSE, DrawLseArgs, DrawArgs>>;
// MIRO (tce_sample_mirostat_f16; the rule is in include/tce_matmul.h): on top of STG = true only, plain rows only.  A row whose mode is 1 or 2 (and temp > 0) skips the
// whole top-p / stages / temperature block -- the branch is uniform per workgroup -- and runs sample_temperature, sample_softmax and sample_token_mirostat[_v2]
// (Generate.cc:138-201) on the sorted candidates in LDS, in the kernel's idiom: per-element work on threads < kk, every thread walks the sequential sums itself.  ex[]
// is computed ONCE: the reference's second softmax subtracts the same maximum from the same values, so only the sum over the kept and the divisions are redone.  The
// row's mu is read here and written by thread 0 in the tail, beside the token.  Any other row takes the STG = true form's path unchanged.  The MIRO = false forms
// declare nothing new: miro_mode folds to 0.
struct MiroLds {  // the MIRO = true forms' LDS (only they instantiate it): thread 0's words from the rule to the tail
    int mode, kept;
    float s_hat, k_f;
};
__device__ __forceinline__ MiroLds &miro_lds() {
    __shared__ MiroLds s;
    return s;
}
// powf through the fp64 pow, rounded once to fp32: within one fp32 ulp of the exact value, with pow's special cases.  The fp32 powf of the device library inlines into
// packed f32 multiplies whose low half picks a high register, the form the build refuses (isa_lint.py RULE 1); three calls per mode-1 row, uniform, off the mode-0 path.
__device__ __forceinline__ float pow_f32(float x, float y) { return (float)pow((double)x, (double)y); }
// SPEC + MIRO (tce_sample_verify_mirostat_f16): mu at virtual row t depends on the draws of rows < t, so the per-row draw launch cannot finish a mirostat sequence.  It
// stops such a row behind the sort and leaves the sorted candidates in a MiroRowWs; sample_miro_walk_kernel (one workgroup per sequence) then walks rows 0 .. n - 1
// with mu carried through miro_rule -- the SAME device function the plain form runs, so a row's arithmetic is the plain form's -- and writes cand[y] and mu_after;
// the chain kernel's MIRO form stores mu_after of the last token it emits.
struct MiroRowWs {  // per virtual row, behind the verifier's workspace
    int kk;          // the candidates behind top-k; 0: no candidate (constraint rule 6)
    float mu_after;  // mu behind this row's token, had rows 0 .. t all been emitted
    int pad[2];
    float lg[kMaxK];  // the sorted penalised logits (before the division)
    int ids[kMaxK];
};
template <class Base>
struct MiroArgs : Base {  // the MIRO = true forms' arguments: the STG = true form's, then the mirostat rows
    tce_mirostat_row *mrows;      // [batch] (SPEC: per sequence)
    tce_mirostat_debug *mdebug;   // [batch] or null (SPEC: written by the walk launch, per virtual row)
    int mvocab;                   // N of mode 1
    MiroRowWs *mws;               // SPEC: [batch * T]; else null
};
// The rule on the kk sorted candidates in lg[] (include/tce_matmul.h, rules 1 - 4), for the whole workgroup: lg is divided in place, pr holds the first softmax, fp the
// final p of the `n` kept, `choice` the position drawn on u.  tb / bb: kMaxK words each.  Every thread returns the same values.
__device__ __forceinline__ void miro_rule(int mode, int m, float mu, float temp, int vocab, int kk, float u, int tid, float *lg, float *ex, float *pr, float *fp, float *tb,
                                          float *bb, int &n, int &choice, float &s_hat, float &k_f) {
    if (tid < kk) lg[tid] = lg[tid] / temp;  // sample_temperature (:72-76)
    __syncthreads();
    const float l0 = lg[0];
    if (tid < kk) ex[tid] = expf(lg[tid] - l0);
    __syncthreads();
    float sum = 0.0f;
    for (int i = 0; i < kk; ++i) sum += ex[i];
    if (tid < kk) pr[tid] = ex[tid] / sum;
    __syncthreads();
    int keep = kk;
    s_hat = k_f = 0.0f;
    if (mode == 1) {  // sample_token_mirostat (:138-160)
        const int want = m - 1;
        const int nt = want < 0 || want > kk - 1 ? kk - 1 : want;  // size_t(m - 1) && candidates->size - 1
        if (tid < nt) {  // the products side by side (each rounded once, as the reference's uncontracted multiply): the walk below only adds
            const float t = logf((float)(tid + 2) / (float)(tid + 1));
            bb[tid] = t * logf(pr[tid] / pr[tid + 1]);
            tb[tid] = t * t;
        }
        __syncthreads();
        float sum_tb = 0.0f, sum_tt = 0.0f;
        for (int i = 0; i < nt; ++i) {
            sum_tb += bb[i];
            sum_tt += tb[i];
        }
        s_hat = sum_tb / sum_tt;
        const float eps = s_hat - 1.0f;
        k_f = pow_f32((eps * pow_f32(2.0f, mu)) / (1.0f - pow_f32((float)vocab, -eps)), 1.0f / s_hat);
        keep = !(k_f >= 1.0f) ? 1 : (k_f >= (float)kk ? kk : (int)k_f);  // the project's rule where C leaves int(k) open
    } else {  // sample_token_mirostat_v2 (:176-185): the first candidate whose surprise exceeds mu, and everything behind it, go
        if (tid < kk) tb[tid] = -log2f(pr[tid]);
        __syncthreads();
        for (int i = 0; i < kk; ++i) {
            if (tb[i] > mu) {
                keep = i;
                break;
            }
        }
        keep = keep < 1 ? 1 : keep;  // (the reference would read an empty array)
    }
    // sample_token's softmax over the kept: the same maximum, the same expf arguments -- ex[] stands --, a new sum
    float sum2 = 0.0f;
    for (int i = 0; i < keep; ++i) sum2 += ex[i];
    if (tid < keep) fp[tid] = ex[tid] / sum2;
    __syncthreads();
    n = keep;
    choice = n - 1;
    float cdf = 0.0f;
    for (int i = 0; i < n; ++i) {
        cdf += fp[i];
        if (u < cdf) {
            choice = i;
            break;
        }
    }
}
// rule 5: the surprise of the candidate drawn and the mu behind it
__device__ __forceinline__ float miro_surprise(float p) { return -log2f(p); }
__device__ __forceinline__ float miro_update(float mu, float eta, float tau, float surprise) { return mu - eta * (surprise - tau); }
template <bool LSE, bool CON, bool STG = false, bool MIRO = false>
using DrawArgsOf = std::conditional_t<MIRO, MiroArgs<StgArgs<DrawArgsBase<LSE, CON>>>, std::conditional_t<STG, StgArgs<DrawArgsBase<LSE, CON>>, DrawArgsBase<LSE, CON>>>;
template <bool MIRO, class A>
__device__ __forceinline__ int miro_mode(const A &a, int b) {  // the mode that runs for row b: 1, 2, or 0
    if constexpr (MIRO) {
        const int m = a.mrows[b].mode;
        return m == 1 || m == 2 ? m : 0;
    } else {
        return 0;
    }
}
template <bool SPEC, bool LSE, bool CON, bool STG = false, bool MIRO = false>
__global__ __launch_bounds__(kThreads) void sample_draw_kernel(DrawArgsOf<LSE, CON, STG, MIRO> a, [[maybe_unused]] int RT, [[maybe_unused]] int32_t *cand) {
    static_assert(!MIRO || STG, "the mirostat forms stand on the STG = true forms");
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!row_active(a.pos, b, a.pos_bound)) return;
    [[maybe_unused]] float lse = 0.0f;
    if constexpr (LSE) lse = merge_lse(a.partials + (size_t)b * a.nchunks, a.nchunks, tid, wave, lane);
    [[maybe_unused]] const int seq = SPEC ? b / RT : b, vt = SPEC ? b - seq * RT : 0;
    __shared__ u64 sel[kMaxK];
    __shared__ float lg[kMaxK + 8], ex[kMaxK + 8], pr[kMaxK + 8], fp[kMaxK + 8];
    __shared__ int ids[kMaxK];
    __shared__ int cnt[2][4];
    __shared__ int nsel;
    tce_sample_row &r = a.rows[SPEC ? seq : b];
    const int k = row_k(r, a.kbound);
    const int E = a.nchunks * k;  // <= 8192 (checked by the host)

    // ---- the k largest (key, lowest id first) of the chunks' survivors ----
    u64 comp[kMergePerThread];
    int valid = 0;
#pragma unroll
    for (int j = 0; j < kMergePerThread; ++j) {
        const int idx = j * kThreads + tid;
        comp[j] = 0;
        if (idx < E) {
            const int ch = idx / k, s = idx - ch * k;
            const uint2_t ent = a.entries[((size_t)b * a.nchunks + ch) * kMaxK + s];
            if (ent.x != 0u) comp[j] = ((u64)ent.x << 20) | (u64)(0xFFFFFu - ent.y);
        }
        valid += __builtin_popcountll(__ballot(comp[j] != 0));
    }
    if (tid == 0) nsel = 0;
    const int V = block_total(valid, cnt, 0, wave, lane);
    const int kk = V < k ? V : k;  // (>= 1: the vocabulary is not empty)
    if constexpr (CON) {
        if (V == 0) {  // (uniform) rule 6: nothing is emitted
            if (tid == 0) {
                if constexpr (SPEC) {
                    cand[b] = -1;
                    if constexpr (MIRO) a.mws[b].kk = 0;
                } else {
                    a.pos[b] = -1;
                    atomicAdd(a.con.violations, 1u);
                }
            }
            return;
        }
    }
    const int nj = (E + kThreads - 1) / kThreads;
    u64 T = 0;
    for (int bit = 51; bit >= 0; --bit) {
        const u64 cand = T | (1ull << bit);
        int cw = 0;
#pragma unroll
        for (int j = 0; j < kMergePerThread; ++j)
            if (j < nj) cw += __builtin_popcountll(__ballot(comp[j] >= cand));
        if (block_total(cw, cnt, bit, wave, lane) >= kk) T = cand;  // (rounds 51, 50, ...: the LDS row alternates with the count above, round 0)
    }
#pragma unroll
    for (int j = 0; j < kMergePerThread; ++j) {
        if (comp[j] != 0 && comp[j] >= T) {
            const int slot = atomicAdd(&nsel, 1);
            if (slot < kMaxK) sel[slot] = comp[j];
        }
    }
    __syncthreads();
    // rank sort of the kk distinct winners: descending key, ascending id among equal keys
    if (tid < kk) {
        const u64 mine = sel[tid];
        int rank = 0;
        for (int j = 0; j < kk; ++j) rank += sel[j] > mine ? 1 : 0;
        lg[rank] = key_value((unsigned)(mine >> 20));
        ids[rank] = (int)(0xFFFFFu - (unsigned)(mine & 0xFFFFFu));
    }
    __syncthreads();

    if constexpr (STG) {  // the sorted candidates as the debug record shows them: typical permutes lg / ids
        StgLds &S = stg_lds();
        if (tid == 0) {
            S.n1 = S.n2 = kk;
            S.permuted = S.recomputed = 0;
        }
        if (tid < kk) {
            S.sv_lg[tid] = lg[tid];
            S.sv_id[tid] = ids[tid];
        }
    }

    const unsigned gen = SPEC ? r.generated + (unsigned)vt : r.generated;
    float u = 0.0f;
    int n = 1, choice = 0;
    if constexpr (MIRO) {
        MiroLds &M = miro_lds();
        const int mrow = SPEC ? seq : b;
        const int mode = r.temp > 0.0f ? miro_mode<MIRO>(a, mrow) : 0;
        if (tid == 0) {
            M.mode = mode;
            M.s_hat = M.k_f = 0.0f;
        }
        if (mode != 0) {  // (uniform)
            if constexpr (SPEC) {  // the sorted candidates go to the walk launch; the log-sum-exp is this row's whatever token is drawn
                MiroRowWs &w = a.mws[b];
                if (tid < kk) {
                    w.lg[tid] = lg[tid];
                    w.ids[tid] = ids[tid];
                }
                if (tid == 0) {
                    w.kk = kk;
                    if constexpr (LSE) a.cand_lse[b] = lse;
                }
                return;
            } else {
                const tce_mirostat_row &mr = a.mrows[b];
                u = a.uniform_override ? a.uniform_override[b] : (float)(philox4x32_10_first(gen, r.seed_lo, r.seed_hi) >> 8) * 0x1p-24f;
                float s_hat, k_f;
                miro_rule(mode, mr.m, mr.mu, r.temp, a.mvocab, kk, u, tid, lg, ex, pr, fp, stg_lds().sc, stg_lds().pq, n, choice, s_hat, k_f);
                if (tid == 0) {
                    M.s_hat = s_hat;
                    M.k_f = k_f;
                }
                goto drawn;  // (uniform) past the top-p / stages / temperature block
            }
        }
    }
    if (r.temp > 0.0f) {
        // sample_top_p's softmax over the k candidates (Generate.cc:81-100): every thread walks the sums itself (broadcast LDS reads), in sorted order
        const float l0 = lg[0];
        if (tid < kk) ex[tid] = expf(lg[tid] - l0);
        __syncthreads();
        float sum = 0.0f;
        for (int i = 0; i < kk; ++i) sum += ex[i];
        if (tid < kk) pr[tid] = ex[tid] / sum;
        __syncthreads();
        n = kk;
        if constexpr (STG) {
            StgLds &S = stg_lds();
            float *const sc = S.sc, *const pq = S.pq;
            int *const ord = S.ord;
            int n1 = kk, n2;
            bool permuted = false, recomputed = false;
            const tce_stage_row &sr = a.srows[SPEC ? seq : b];
            const float z = sr.tfs_z, typ = sr.typical_p;
            if (!(z >= 1.0f) && kk > 2) {  // sample_tail_free (:203-246) with min_keep 1, on the softmax over the kk
                if (tid < kk - 2) sc[tid] = fabsf((pr[tid] - pr[tid + 1]) - (pr[tid + 1] - pr[tid + 2]));
                __syncthreads();
                float d2sum = 0.0f;
                for (int i = 0; i < kk - 2; ++i) d2sum += sc[i];
                if (tid < kk - 2) pq[tid] = sc[tid] / d2sum;  // the weights, divided side by side: the walk below only adds (a sum of 0: NaN weights, no comparison holds, nothing is cut)
                __syncthreads();
                float cum = 0.0f;
                for (int i = 0; i < kk - 2; ++i) {
                    cum += pq[i];
                    if (cum > z && i >= 1) {
                        n1 = i;
                        break;
                    }
                }
                __syncthreads();  // (sc and pq are written again below)
            }
            n2 = n1;
            if (!(typ >= 1.0f)) {  // sample_typical (:248-302) with min_keep 1, on the softmax over the n1
                if (tid < n1) ex[tid] = expf(lg[tid] - l0);
                __syncthreads();
                float s1 = 0.0f;
                for (int i = 0; i < n1; ++i) s1 += ex[i];
                if (tid < n1) pq[tid] = ex[tid] / s1;
                __syncthreads();
                if (tid < n1) ex[tid] = logf(pq[tid]);
                ord[tid] = tid;  // (a rank that NaNs leave unassigned stays an index of the row)
                __syncthreads();
                float H = 0.0f;
                for (int i = 0; i < n1; ++i) H += -pq[i] * ex[i];
                if (tid < n1) sc[tid] = fabsf(-ex[tid] - H);
                __syncthreads();
                if (tid < n1) {  // ascending score, the earlier candidate first among equals (every score NaN: the order stays)
                    const float mine = sc[tid];
                    int rank = 0;
                    for (int j = 0; j < n1; ++j) rank += (sc[j] < mine || (!(mine < sc[j]) && j < tid)) ? 1 : 0;
                    ord[rank] = tid;
                }
                __syncthreads();
                if (tid < n1) sc[tid] = pq[ord[tid]];  // p in score order, gathered side by side: the walk below reads one word per step
                __syncthreads();
                float cum = 0.0f;
                for (int i = 0; i < n1; ++i) {
                    cum += sc[i];
                    if (cum > typ) {
                        n2 = i + 1;
                        break;
                    }
                }
                float lv = 0.0f;
                int iv = 0;
                if (tid < n2) {
                    lv = lg[ord[tid]];
                    iv = ids[ord[tid]];
                }
                __syncthreads();
                if (tid < n2) {
                    lg[tid] = lv;
                    ids[tid] = iv;
                }
                permuted = true;
                __syncthreads();
            }
            if (!(z >= 1.0f) || !(typ >= 1.0f)) {  // sample_top_p's softmax over the n2 in their current order: data[0] need not be the maximum any more
                const float f0 = lg[0];
                if (tid < n2) ex[tid] = expf(lg[tid] - f0);
                __syncthreads();
                float s2 = 0.0f;
                for (int i = 0; i < n2; ++i) s2 += ex[i];
                if (tid < n2) pq[tid] = ex[tid] / s2;
                __syncthreads();
                recomputed = true;
            }
            if (tid == 0) {  // (for the debug record, behind a barrier)
                S.n1 = n1;
                S.n2 = n2;
                S.permuted = permuted;
                S.recomputed = recomputed;
            }
            n = n2;
            if (r.top_p < 1.0f) {  // sample_top_p over the n2, on the softmax above
                const float *pt = recomputed ? pq : pr;
                float cum = 0.0f;
                for (int i = 0; i < n2; ++i) {
                    cum += pt[i];
                    if (cum > r.top_p && i >= 1) {
                        n = i;
                        break;
                    }
                }
            }
        } else if (r.top_p < 1.0f) {  // sample_top_p (:304-327) with min_keep 1: the candidate that crosses the threshold is dropped
            float cum = 0.0f;
            for (int i = 0; i < kk; ++i) {
                cum += pr[i];
                if (cum > r.top_p && i >= 1) {
                    n = i;
                    break;
                }
            }
        }
        // sample_temperature (:72-76), then sample_token's softmax over the n kept (:103-118)
        const float t0 = lg[0] / r.temp;
        if (tid < n) ex[tid] = expf(lg[tid] / r.temp - t0);
        __syncthreads();
        float sum2 = 0.0f;
        for (int i = 0; i < n; ++i) sum2 += ex[i];
        if (tid < n) fp[tid] = ex[tid] / sum2;
        __syncthreads();
        u = a.uniform_override ? a.uniform_override[b] : (float)(philox4x32_10_first(gen, r.seed_lo, r.seed_hi) >> 8) * 0x1p-24f;
        choice = n - 1;
        float cdf = 0.0f;
        for (int i = 0; i < n; ++i) {
            cdf += fp[i];
            if (u < cdf) {
                choice = i;
                break;
            }
        }
    }
[[maybe_unused]] drawn:  // (only the MIRO = true forms jump here; as a second condition on the block above, the same test moved the MIRO = false forms' registers)
    if constexpr (CON && !SPEC) {  // the drawn token's next state, through one LDS word (0 for an unconstrained row: unused)
        int &con_next = con_next_word();
        if (tid == 0) {
            const tce_constraint_row &cr = a.con.rows[b];
            int v = 0;
            if (cr.fsm >= 0) {
                v = -2;  // invalid
                if (fsm_state_ok(a.con, cr.fsm, cr.state)) {
                    const tce_fsm &f = a.con.fsms[cr.fsm];
                    v = fsm_next(f, cr.state, ids[choice]);
                    if (v < TCE_FSM_DONE || v >= f.states) v = -2;
                }
            }
            con_next = v;
        }
        __syncthreads();
        if (con_next == -2) {  // (uniform) rule 6
            if (tid == 0) {
                a.pos[b] = -1;
                atomicAdd(a.con.violations, 1u);
            }
            return;
        }
    }
    if (a.debug) {
        tce_sample_debug &d = a.debug[b];
        if (tid < kMaxK) {
            const bool in_k = tid < kk, in_n = tid < n && r.temp > 0.0f;
            if constexpr (STG) {  // the sorted top-k candidates, whatever typical made of lg / ids
                d.ids[tid] = in_k ? stg_lds().sv_id[tid] : -1;
                d.logit[tid] = in_k ? stg_lds().sv_lg[tid] : 0.0f;
            } else {
                d.ids[tid] = in_k ? ids[tid] : -1;
                d.logit[tid] = in_k ? lg[tid] : 0.0f;
            }
            d.p[tid] = in_k && r.temp > 0.0f ? pr[tid] : 0.0f;
            d.final_p[tid] = in_n ? fp[tid] : 0.0f;
        }
        if (tid == 0) {
            d.n = n;
            d.k = kk;
            d.u = u;
            d.choice = choice;
        }
    }
    if constexpr (STG) {
        if (a.sdebug) {
            tce_stage_debug &sd = a.sdebug[b];
            StgLds &S = stg_lds();
            __syncthreads();  // (thread 0's words; a greedy row passes no other barrier behind them)
            const float *pt = S.recomputed ? S.pq : pr;
            if (tid < kMaxK) {
                sd.order[tid] = tid < S.n2 ? (S.permuted ? S.ord[tid] : tid) : -1;
                sd.p_top[tid] = tid < S.n2 && r.temp > 0.0f ? pt[tid] : 0.0f;
            }
            if (tid == 0) {
                sd.n_tfs = S.n1;
                sd.n_typ = S.n2;
            }
        }
    }
    // ---- the tail: the token, the log, the ring, the counters, the position ----
    [[maybe_unused]] float lp = 0.0f;
    if constexpr (LSE) {  // (ids[] holds vocabulary indices only; the test keeps the read inside the row whatever happens)
        if (tid == 0) {
            const int tok = ids[choice];
            lp = tok >= 0 && tok < a.vocab ? (float)a.logits[(size_t)b * a.ld + tok] - lse : __builtin_nanf("");
        }
    }
    if constexpr (SPEC) {
        if (tid == 0) {
            cand[b] = ids[choice];
            if constexpr (LSE) {
                a.cand_logprob[b] = lp;
                a.cand_lse[b] = lse;
            }
        }
        return;
    }
    if (tid == 0) {
        const int tok = ids[choice];
        a.next_token[b] = tok;
        if (gen < (unsigned)a.log_stride) a.out_log[(size_t)b * a.log_stride + gen] = tok;
        if constexpr (LSE) {
            if (gen < (unsigned)a.log_stride) a.out_logprob[(size_t)b * a.log_stride + gen] = lp;
            if (a.last_lse) a.last_lse[b] = lse;
        }
        r.ring[r.ring_pushed & 63u] = tok;
        r.ring_pushed = r.ring_pushed + 1u;
        r.generated = gen + 1u;
        bool stop = (int)(gen + 1u) >= r.max_new || gen + 1u >= (unsigned)a.log_stride;
        for (int i = 0; i < a.n_stop; ++i) stop = stop || tok == a.stop_ids[i];
        if constexpr (CON) {
            tce_constraint_row &cr = a.con.rows[b];
            const int nx = con_next_word();
            if (cr.fsm >= 0) {
                if (nx == TCE_FSM_DONE) stop = true;
                else cr.state = nx;
            }
        }
        a.pos[b] = stop ? -1 : a.pos[b] + 1;
        if constexpr (MIRO) {  // mu moves with every token a mirostat row emits; thread 0 wrote M itself
            const MiroLds &M = miro_lds();
            tce_mirostat_row &mr = a.mrows[b];
            float surprise = 0.0f, mu_out = 0.0f;
            if (M.mode != 0) {
                surprise = miro_surprise(fp[choice]);
                mu_out = miro_update(mr.mu, mr.eta, mr.tau, surprise);
            }
            if (a.mdebug) {
                tce_mirostat_debug &md = a.mdebug[b];
                const float mu_in = mr.mu;
                md.mode = M.mode;
                md.kk = kk;
                md.s_hat = M.s_hat;
                md.k_f = M.k_f;
                md.kept = n;
                md.mu_in = mu_in;
                md.mu_out = M.mode != 0 ? mu_out : mu_in;
                md.surprise = surprise;
                md.choice = choice;
                md.final_p = r.temp > 0.0f ? fp[choice] : 0.0f;
            }
            if (M.mode != 0) mr.mu = mu_out;
        }
    }
}

// tce_sample_verify_f16's last launch: thread = sequence.  Walks the chain of candidates and writes state exactly as sample_draw_kernel's tail does, once per emitted token.
// LSE: where y_t is emitted, out_logprob[b][g + t] = cand_logprob[y] (under out_log's bound); last_lse[b] = the last emitted row's; rejected rows write nothing.
struct VerifyLseArgs : VerifyArgs {
    const float *cand_logprob, *cand_lse;
    float *out_logprob, *last_lse;
};

// CON: the sequence's state advances once per emitted token (fsm_next); DONE retires the sequence behind the token; a row that is invalid (rule 6: the base state, no
// candidate -- cand < 0 --, or the token's next outside [-1, states)) emits nothing, retires the sequence behind the tokens already emitted and counts one violation.
// MIRO: behind the tokens it emits the chain stores, for a sequence that runs mirostat, the mu the walk launch left behind the LAST of them.
template <class Base>
struct MiroChainArgs : Base {
    tce_mirostat_row *mrows;  // [batch]
    const MiroRowWs *mws;     // [batch * T]
};
template <bool LSE, bool CON>
using VerifyArgsBase = std::conditional_t<CON, ConArgs<std::conditional_t<LSE, VerifyLseArgs, VerifyArgs>>, std::conditional_t<LSE, VerifyLseArgs, VerifyArgs>>;
template <bool LSE, bool CON, bool MIRO = false>
using VerifyArgsOf = std::conditional_t<MIRO, MiroChainArgs<VerifyArgsBase<LSE, CON>>, VerifyArgsBase<LSE, CON>>;

// tce_sample_verify_mirostat_f16's third launch: workgroup = sequence.  For a sequence whose mode is 1 or 2 and whose temp > 0 it walks the active virtual rows in
// order with mu carried: row t's sorted candidates (left by the SPEC draw form) through miro_rule on the uniform keyed (seed, generated + t), cand[y] = the token,
// mu_after = the mu behind it, and with lp the token's log-probability on the row's own log-sum-exp.  A row without a candidate (rule 6: cand = -1 already) ends the
// walk: the chain ends there too.  Rows behind a rejected draft are walked as well and never read.  Any other sequence: nothing.
struct WalkArgs {
    MiroRowWs *mws;
    const tce_sample_row *rows;
    const tce_mirostat_row *mrows;
    tce_mirostat_debug *mdebug;  // [batch * T] or null
    const int32_t *pos, *row_pos;
    int pos_bound, T, vocab, ld;
    const float *uniform_override;  // [batch * T] or null
    int32_t *cand;
    const half_t *logits;      // null without lp
    float *cand_logprob;
    const float *cand_lse;
};
__global__ __launch_bounds__(kThreads) void sample_miro_walk_kernel(WalkArgs a) {
    const int seq = blockIdx.x, tid = threadIdx.x;
    if (!row_active(a.pos, seq, a.pos_bound)) return;
    const tce_sample_row &r = a.rows[seq];
    const tce_mirostat_row &mr = a.mrows[seq];
    const int mode = mr.mode == 1 || mr.mode == 2 ? mr.mode : 0;
    if (!(r.temp > 0.0f) || mode == 0) return;
    __shared__ float lg[kMaxK + 8], ex[kMaxK + 8], pr[kMaxK + 8], fp[kMaxK + 8], tb[kMaxK + 8], bb[kMaxK + 8];
    float mu = mr.mu;
    for (int t = 0; t < a.T; ++t) {
        const int y = seq * a.T + t;
        if (!row_active(a.row_pos, y, a.pos_bound)) break;  // the active rows are a prefix
        MiroRowWs &w = a.mws[y];
        const int kk = w.kk;
        if (kk < 1 || kk > kMaxK) break;
        if (tid < kk) lg[tid] = w.lg[tid];
        __syncthreads();
        const float u = a.uniform_override ? a.uniform_override[y] : (float)(philox4x32_10_first(r.generated + (unsigned)t, r.seed_lo, r.seed_hi) >> 8) * 0x1p-24f;
        int n, choice;
        float s_hat, k_f;
        miro_rule(mode, mr.m, mu, r.temp, a.vocab, kk, u, tid, lg, ex, pr, fp, tb, bb, n, choice, s_hat, k_f);
        const float p = fp[choice], surprise = miro_surprise(p), mu_out = miro_update(mu, mr.eta, mr.tau, surprise);
        if (tid == 0) {
            const int tok = w.ids[choice];
            a.cand[y] = tok;
            w.mu_after = mu_out;
            if (a.logits) a.cand_logprob[y] = tok >= 0 && tok < a.vocab ? (float)a.logits[(size_t)y * a.ld + tok] - a.cand_lse[y] : __builtin_nanf("");
            if (a.mdebug) {
                tce_mirostat_debug &md = a.mdebug[y];
                md.mode = mode;
                md.kk = kk;
                md.s_hat = s_hat;
                md.k_f = k_f;
                md.kept = n;
                md.mu_in = mu;
                md.mu_out = mu_out;
                md.surprise = surprise;
                md.choice = choice;
                md.final_p = p;
            }
        }
        mu = mu_out;
        __syncthreads();  // (the next row writes lg / ex / fp again)
    }
}

template <bool LSE, bool CON, bool MIRO = false>
__global__ __launch_bounds__(64) void sample_verify_chain_kernel(VerifyArgsOf<LSE, CON, MIRO> a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.batch) return;
    if (!row_active(a.d.pos, b, a.d.pos_bound)) {
        a.emitted[b] = 0;
        return;
    }
    tce_sample_row &r = a.d.rows[b];
    const int p = a.d.pos[b], y0 = b * a.T;
    int n = 0;  // the active rows: a prefix (the drafting launch wrote them so)
    while (n < a.T && a.row_pos[y0 + n] >= 0 && a.row_pos[y0 + n] <= a.d.pos_bound) ++n;
    const unsigned g = r.generated;
    unsigned pushed = r.ring_pushed;
    int t = 0, tok = 0, newpos = -1;
    [[maybe_unused]] std::conditional_t<CON, ChainCon, NoCon> cs;
    if constexpr (CON) {
        cs.fsm = a.con.rows[b].fsm;
        cs.state = a.con.rows[b].state;
        cs.invalid = cs.fsm >= 0 && !fsm_state_ok(a.con, cs.fsm, cs.state);
    }
    for (; t < n; ++t) {
        if constexpr (CON) {
            const int ct = a.cand[y0 + t];
            if (cs.fsm >= 0 && !cs.invalid) {
                cs.nx = ct < 0 ? -2 : fsm_next(a.con.fsms[cs.fsm], cs.state, ct);
                cs.invalid = cs.nx < TCE_FSM_DONE || cs.nx >= a.con.fsms[cs.fsm].states;
            }
            if (cs.invalid) {
                newpos = -1;
                break;
            }
        }
        tok = a.cand[y0 + t];
        if (g + t < (unsigned)a.d.log_stride) a.d.out_log[(size_t)b * a.d.log_stride + g + t] = tok;
        if constexpr (LSE) {
            if (g + t < (unsigned)a.d.log_stride) a.out_logprob[(size_t)b * a.d.log_stride + g + t] = a.cand_logprob[y0 + t];
        }
        r.ring[pushed & 63u] = tok;
        ++pushed;
        if (p + 1 + t < a.hist_stride) a.history[(size_t)b * a.hist_stride + p + 1 + t] = tok;
        bool stop = (int)(g + t + 1u) >= r.max_new || g + t + 1u >= (unsigned)a.d.log_stride;
        for (int i = 0; i < a.d.n_stop; ++i) stop = stop || tok == a.d.stop_ids[i];
        if constexpr (CON) {
            if (cs.fsm >= 0) {
                if (cs.nx == TCE_FSM_DONE) stop = true;
                else cs.state = cs.nx;
            }
        }
        if (stop) {
            ++t;
            break;
        }
        if (t + 1 >= n || a.row_token[y0 + t + 1] != tok) {
            newpos = p + t + 1;
            ++t;
            break;
        }
    }
    // (n == 0 cannot happen for an active sequence -- row 0 is its own position --; it would emit nothing and leave the sequence where it is)
    if constexpr (CON) {
        if (cs.fsm >= 0 && t > 0) a.con.rows[b].state = cs.state;
        if (cs.invalid) {
            a.d.pos[b] = -1;
            atomicAdd(a.con.violations, 1u);
        }
    }
    if (t > 0) {
        a.d.next_token[b] = tok;
        r.ring_pushed = pushed;
        r.generated = g + (unsigned)t;
        a.d.pos[b] = newpos;
        if constexpr (LSE) {
            if (a.last_lse) a.last_lse[b] = a.cand_lse[y0 + t - 1];
        }
        if constexpr (MIRO) {
            tce_mirostat_row &mr = a.mrows[b];
            if ((mr.mode == 1 || mr.mode == 2) && r.temp > 0.0f) mr.mu = a.mws[y0 + t - 1].mu_after;
        }
    }
    a.emitted[b] = t;
}

// tce_draft_ngram: workgroup = sequence.  Row 0 is the sequence's certain next input; rows 1 .. are what followed the most recent earlier occurrence of its last
// `ngram` tokens (prompt lookup), or -- script != null, a test hook -- script[b][p + t] up to the first -1.
__global__ __launch_bounds__(kThreads) void draft_ngram_kernel(const int32_t *history, const int32_t *script, int hist_stride, const int32_t *pos, int pos_bound, int T,
                                                                int ngram, int32_t *row_token, int32_t *row_pos) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ int best;
    const int p = pos[b];
    if (p < 0 || p > pos_bound || p >= hist_stride) {
        if (tid < T) {
            row_token[b * T + tid] = 0;
            row_pos[b * T + tid] = -1;
        }
        return;
    }
    const int32_t *h = history + (size_t)b * hist_stride;
    if (tid == 0) best = -1;
    __syncthreads();
    if (!script && p >= ngram) {
        int mine = -1;
        for (int i = ngram - 1 + tid; i < p; i += kThreads) {
            bool same = true;
            for (int j = 0; j < ngram; ++j) same = same && h[i - j] == h[p - j];
            if (same) mine = i;  // (ascending: the last one stays)
        }
        if (mine >= 0) atomicMax(&best, mine);
    }
    __syncthreads();
    if (tid < T) {
        const int t = tid;
        int tok = 0, rp = -1;
        if (t == 0) {
            tok = h[p];
            rp = p;
        } else if (p + t <= pos_bound) {
            if (script) {
                const int32_t *sc = script + (size_t)b * hist_stride;
                bool ok = p + t < hist_stride;
                for (int j = 1; j <= t && ok; ++j) ok = sc[p + j] >= 0;  // the prefix ends at the first -1
                if (ok) {
                    tok = sc[p + t];
                    rp = p + t;
                }
            } else if (best >= 0 && best + t <= p) {
                tok = h[best + t];
                rp = p + t;
            }
        }
        row_token[b * T + t] = tok;
        row_pos[b * T + t] = rp;
    }
}

// tce_logprobs_f16 (scoring), first launch: grid (chunks, rows); sample_select_kernel's loads, the same chunk_lse_pair
__global__ __launch_bounds__(kThreads) void logprobs_partials_kernel(const half_t *logits, int ld, int vocab, int nchunks, float2_t *partials) {
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const half_t *row = logits + (size_t)b * ld;
    const int i0 = c * kChunk + tid * 16;
    float x[16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        half8_t v = {};
        if (i0 + 8 * h < vocab) v = *reinterpret_cast<const half8_t *>(row + i0 + 8 * h);  // (a piece across `vocab` stays inside the row: vocab <= ld, ld % 8 == 0)
#pragma unroll
        for (int j = 0; j < 8; ++j) x[8 * h + j] = (float)v[j];
    }
    const float2_t pair = chunk_lse_pair(x, i0, vocab, wave, lane);
    if (tid == 0) partials[(size_t)b * nchunks + c] = pair;
}

// second launch: grid (rows); sample_draw_kernel<., true>'s merge, then the target's raw logit.  target -1: "no target" (0.0); any other id outside the vocabulary: NaN
__global__ __launch_bounds__(kThreads) void logprobs_merge_kernel(const half_t *logits, int ld, int vocab, int nchunks, const float2_t *partials, const int32_t *target,
                                                                   float *out_logprob, float *out_lse) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float lse = merge_lse(partials + (size_t)b * nchunks, nchunks, tid, wave, lane);
    if (tid == 0) {
        const int t = target[b];
        out_logprob[b] = t == -1 ? 0.0f : (t >= 0 && t < vocab ? (float)logits[(size_t)b * ld + t] - lse : __builtin_nanf(""));
        if (out_lse) out_lse[b] = lse;
    }
}

__global__ __launch_bounds__(kThreads) void embed_rows_kernel(const uint4_t *table, int vocab, int pieces, const int32_t *token, uint4_t *out, const int32_t *pos, int pos_bound,
                                                               unsigned *violations) {
    const int b = blockIdx.x;
    if (!row_active(pos, b, pos_bound)) return;
    const int tok = token[b];
    const bool ok = tok >= 0 && tok < vocab;
    uint4_t zero = {0u, 0u, 0u, 0u};
    for (int p = threadIdx.x; p < pieces; p += kThreads) out[(size_t)b * pieces + p] = ok ? table[(size_t)tok * pieces + p] : zero;
    if (!ok && threadIdx.x == 0) atomicAdd(violations, 1u);
}

}  // namespace

int sample_chunks(int vocab) { return (vocab + kChunk - 1) / kChunk; }

size_t sample_workspace_bytes(int batch, int vocab) {
    if (batch < 1 || vocab < 1) return 0;
    return 256 + (size_t)batch * sample_chunks(vocab) * kMaxK * sizeof(uint2_t);  // 256 bytes of counters (word 0: tce_embed_rows_f16's refused ids), then the survivors
}

// the logprob workspace: the pairs [rows][chunks], then the verifier's cand_logprob and cand_lse [rows] each
static size_t logprobs_cand_offset(int rows, int vocab) { return (size_t)rows * sample_chunks(vocab) * sizeof(float2_t); }

size_t logprobs_workspace_bytes(int rows, int vocab) {
    if (rows < 1 || vocab < 1) return 0;
    return (logprobs_cand_offset(rows, vocab) + (size_t)rows * 2 * sizeof(float) + 255) & ~(size_t)255;
}

// con == null: the CON = false forms, the launches they were.  Otherwise f(true_type) picks the CON = true form and con_args appends the constraint to its arguments.
template <class F>
static void with_con(const tce_constraint *con, F f) {
    if (con) f(std::true_type{});
    else f(std::false_type{});
}
template <bool CON, class Base>
static auto con_args(const Base &base, const tce_constraint *con) {
    if constexpr (CON) {
        ConArgs<Base> x;
        static_cast<Base &>(x) = base;
        x.con = *con;
        return x;
    } else {
        return base;
    }
}

// tce_sample_stages_f16 / tce_sample_verify_stages_f16's draw launch: the STG = true form for `base` (DrawArgs or DrawLseArgs) with the stage rows behind the
// underlying form's arguments.  Defined behind the two launchers, whose own launches stay as they were.
template <bool SPEC, class Base>
static void launch_draw_stages(const Base &base, const tce_constraint *con, const tce_sample_stages *stg, int rows, int RT, int32_t *cand, hipStream_t stream,
                               const tce_sample_mirostat *mi = nullptr, int vocab = 0, MiroRowWs *mws = nullptr);

// lp == null: tce_sample_f16, the launches they were.  stg (tce_sample_stages_f16): the select launch is the same, the draw launch is its STG = true form.
// mi (tce_sample_mirostat_f16; with stg only): the draw launch is the MIRO = true form on top of it.
int launch_sample_f16(const tce_sample_call &c, const tce_logprob_out *lp, const tce_constraint *con, hipStream_t stream, hipError_t *hip_err, const tce_sample_stages *stg,
                      const tce_sample_mirostat *mi) {
    const tce_constraint cv = con ? *con : tce_constraint{};
    const int nchunks = sample_chunks(c.vocab);
    uint2_t *entries = reinterpret_cast<uint2_t *>(static_cast<char *>(c.workspace) + 256);
    with_con(con, [&](auto tag) {
        constexpr bool CON = decltype(tag)::value;
        if (lp)
            hipLaunchKernelGGL((sample_select_kernel<false, true, CON>), dim3(nchunks, c.batch), dim3(kThreads), 0, stream, static_cast<const half_t *>(c.logits), c.ld, c.vocab,
                               c.rows, c.pos_device, c.pos_bound, c.top_k_bound, entries, nchunks, 1, static_cast<const int32_t *>(nullptr),
                               static_cast<float2_t *>(lp->partials), cv);
        else
            hipLaunchKernelGGL((sample_select_kernel<false, false, CON>), dim3(nchunks, c.batch), dim3(kThreads), 0, stream, static_cast<const half_t *>(c.logits), c.ld, c.vocab,
                               c.rows, c.pos_device, c.pos_bound, c.top_k_bound, entries, nchunks, 1, static_cast<const int32_t *>(nullptr), static_cast<float2_t *>(nullptr),
                               cv);
    });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        DrawArgs a;
        a.entries = entries;
        a.nchunks = nchunks;
        a.kbound = c.top_k_bound;
        a.pos_bound = c.pos_bound;
        a.log_stride = c.log_stride;
        a.rows = c.rows;
        a.pos = c.pos_device;
        a.next_token = c.next_token;
        a.out_log = c.out_log;
        a.uniform_override = c.uniform_override;
        a.debug = c.debug;
        for (int i = 0; i < 4; ++i) a.stop_ids[i] = c.stop_ids[i];
        a.n_stop = c.n_stop;
        if (lp) {
            DrawLseArgs la;
            static_cast<DrawArgs &>(la) = a;
            la.logits = static_cast<const half_t *>(c.logits);
            la.ld = c.ld;
            la.vocab = c.vocab;
            la.partials = static_cast<const float2_t *>(lp->partials);
            la.out_logprob = lp->out_logprob;
            la.last_lse = lp->last_lse;
            la.cand_logprob = la.cand_lse = nullptr;
            if (stg) launch_draw_stages<false>(la, con, stg, c.batch, 1, nullptr, stream, mi, c.vocab);
            else with_con(con, [&](auto tag) {
                constexpr bool CON = decltype(tag)::value;
                hipLaunchKernelGGL((sample_draw_kernel<false, true, CON>), dim3(c.batch), dim3(kThreads), 0, stream, con_args<CON>(la, con), 1, static_cast<int32_t *>(nullptr));
            });
        } else if (stg) {
            launch_draw_stages<false>(a, con, stg, c.batch, 1, nullptr, stream, mi, c.vocab);
        } else {
            with_con(con, [&](auto tag) {
                constexpr bool CON = decltype(tag)::value;
                hipLaunchKernelGGL((sample_draw_kernel<false, false, CON>), dim3(c.batch), dim3(kThreads), 0, stream, con_args<CON>(a, con), 1, static_cast<int32_t *>(nullptr));
            });
        }
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

// the verifier's workspace: tce_sample_f16's layout for batch * rows_per_seq rows, then the candidates int32 [batch * rows_per_seq]
static size_t verify_cand_offset(int batch, int rows_per_seq, int vocab) { return sample_workspace_bytes(batch * rows_per_seq, vocab); }

size_t sample_verify_workspace_bytes(int batch, int rows_per_seq, int vocab) {
    if (batch < 1 || rows_per_seq < 1 || vocab < 1) return 0;
    return verify_cand_offset(batch, rows_per_seq, vocab) + (((size_t)batch * rows_per_seq * 4 + 255) & ~(size_t)255);
}

// the mirostat verifier's workspace: the verifier's, then a MiroRowWs per virtual row
size_t sample_verify_mirostat_workspace_bytes(int batch, int rows_per_seq, int vocab) {
    const size_t base = sample_verify_workspace_bytes(batch, rows_per_seq, vocab);
    return base ? base + (size_t)batch * rows_per_seq * sizeof(MiroRowWs) : 0;
}

// mi (tce_sample_verify_mirostat_f16; with stg only): the draw launch is the SPEC MIRO form, the walk launch follows it, the chain launch is its MIRO form: 4 launches.
int launch_sample_verify_f16(const tce_sample_verify_call &v, const tce_logprob_out *lp, const tce_constraint *con, hipStream_t stream, hipError_t *hip_err,
                             const tce_sample_stages *stg, const tce_sample_mirostat *mi) {
    const tce_sample_call &c = v.s;
    const tce_constraint cv = con ? *con : tce_constraint{};
    const int nchunks = sample_chunks(c.vocab), T = v.rows_per_seq, vrows = c.batch * T;
    uint2_t *entries = reinterpret_cast<uint2_t *>(static_cast<char *>(c.workspace) + 256);
    VerifyArgs a;
    a.d.entries = entries;
    a.d.nchunks = nchunks;
    a.d.kbound = c.top_k_bound;
    a.d.pos_bound = c.pos_bound;
    a.d.log_stride = c.log_stride;
    a.d.rows = c.rows;
    a.d.pos = const_cast<int32_t *>(v.row_pos);  // (the draw launch reads the rows' positions; the chain launch gets the sequences' below)
    a.d.next_token = c.next_token;
    a.d.out_log = c.out_log;
    a.d.uniform_override = c.uniform_override;
    a.d.debug = c.debug;
    for (int i = 0; i < 4; ++i) a.d.stop_ids[i] = c.stop_ids[i];
    a.d.n_stop = c.n_stop;
    a.T = T;
    a.hist_stride = v.hist_stride;
    a.batch = c.batch;
    a.row_token = v.row_token;
    a.row_pos = v.row_pos;
    a.cand = reinterpret_cast<int32_t *>(static_cast<char *>(c.workspace) + verify_cand_offset(c.batch, T, c.vocab));
    a.history = v.history;
    a.emitted = v.emitted;
    MiroRowWs *mws = mi ? reinterpret_cast<MiroRowWs *>(static_cast<char *>(c.workspace) + sample_verify_workspace_bytes(c.batch, T, c.vocab)) : nullptr;
    VerifyLseArgs la;
    DrawLseArgs ld;
    if (lp) {
        float *cl = reinterpret_cast<float *>(static_cast<char *>(lp->partials) + logprobs_cand_offset(vrows, c.vocab));
        ld.logits = static_cast<const half_t *>(c.logits);
        ld.ld = c.ld;
        ld.vocab = c.vocab;
        ld.partials = static_cast<const float2_t *>(lp->partials);
        ld.out_logprob = nullptr;  // (the chain launch writes them)
        ld.last_lse = nullptr;
        ld.cand_logprob = cl;
        ld.cand_lse = cl + vrows;
        la.cand_logprob = cl;
        la.cand_lse = cl + vrows;
        la.out_logprob = lp->out_logprob;
        la.last_lse = lp->last_lse;
        with_con(con, [&](auto tag) {
            constexpr bool CON = decltype(tag)::value;
            hipLaunchKernelGGL((sample_select_kernel<true, true, CON>), dim3(nchunks, vrows), dim3(kThreads), 0, stream, static_cast<const half_t *>(c.logits), c.ld, c.vocab,
                               c.rows, v.row_pos, c.pos_bound, c.top_k_bound, entries, nchunks, T, v.row_token, static_cast<float2_t *>(lp->partials), cv);
        });
    } else {
        with_con(con, [&](auto tag) {
            constexpr bool CON = decltype(tag)::value;
            hipLaunchKernelGGL((sample_select_kernel<true, false, CON>), dim3(nchunks, vrows), dim3(kThreads), 0, stream, static_cast<const half_t *>(c.logits), c.ld, c.vocab,
                               c.rows, v.row_pos, c.pos_bound, c.top_k_bound, entries, nchunks, T, v.row_token, static_cast<float2_t *>(nullptr), cv);
        });
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        if (lp) {
            static_cast<DrawArgs &>(ld) = a.d;
            if (stg) launch_draw_stages<true>(ld, con, stg, vrows, T, a.cand, stream, mi, c.vocab, mws);
            else with_con(con, [&](auto tag) {
                constexpr bool CON = decltype(tag)::value;
                hipLaunchKernelGGL((sample_draw_kernel<true, true, CON>), dim3(vrows), dim3(kThreads), 0, stream, con_args<CON>(ld, con), T, a.cand);
            });
        } else if (stg) {
            launch_draw_stages<true>(a.d, con, stg, vrows, T, a.cand, stream, mi, c.vocab, mws);
        } else {
            with_con(con, [&](auto tag) {
                constexpr bool CON = decltype(tag)::value;
                hipLaunchKernelGGL((sample_draw_kernel<true, false, CON>), dim3(vrows), dim3(kThreads), 0, stream, con_args<CON>(a.d, con), T, a.cand);
            });
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess && mi) {
        WalkArgs w;
        w.mws = mws;
        w.rows = c.rows;
        w.mrows = mi->rows;
        w.mdebug = mi->debug;
        w.pos = c.pos_device;
        w.row_pos = v.row_pos;
        w.pos_bound = c.pos_bound;
        w.T = T;
        w.vocab = c.vocab;
        w.ld = c.ld;
        w.uniform_override = c.uniform_override;
        w.cand = a.cand;
        w.logits = lp ? static_cast<const half_t *>(c.logits) : nullptr;
        w.cand_logprob = lp ? ld.cand_logprob : nullptr;
        w.cand_lse = lp ? ld.cand_lse : nullptr;
        hipLaunchKernelGGL(sample_miro_walk_kernel, dim3(c.batch), dim3(kThreads), 0, stream, w);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        a.d.pos = c.pos_device;
        auto chain = [&](const auto &base, auto lse_tag) {
            constexpr bool LSE = decltype(lse_tag)::value;
            with_con(con, [&](auto tag) {
                constexpr bool CON = decltype(tag)::value;
                if (mi) {
                    MiroChainArgs<VerifyArgsBase<LSE, CON>> x;
                    static_cast<VerifyArgsBase<LSE, CON> &>(x) = con_args<CON>(base, con);
                    x.mrows = mi->rows;
                    x.mws = mws;
                    hipLaunchKernelGGL((sample_verify_chain_kernel<LSE, CON, true>), dim3((c.batch + 63) / 64), dim3(64), 0, stream, x);
                } else {
                    hipLaunchKernelGGL((sample_verify_chain_kernel<LSE, CON>), dim3((c.batch + 63) / 64), dim3(64), 0, stream, con_args<CON>(base, con));
                }
            });
        };
        if (lp) {
            static_cast<VerifyArgs &>(la) = a;
            chain(la, std::true_type{});
        } else {
            chain(a, std::false_type{});
        }
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

template <bool SPEC, class Base>
static void launch_draw_stages(const Base &base, const tce_constraint *con, const tce_sample_stages *stg, int rows, int RT, int32_t *cand, hipStream_t stream,
                               const tce_sample_mirostat *mi, int vocab, MiroRowWs *mws) {
    constexpr bool LSE = std::is_same_v<Base, DrawLseArgs>;
    with_con(con, [&](auto tag) {
        constexpr bool CON = decltype(tag)::value;
        StgArgs<DrawArgsBase<LSE, CON>> x;
        static_cast<DrawArgsBase<LSE, CON> &>(x) = con_args<CON>(base, con);
        x.srows = stg->rows;
        x.sdebug = stg->debug;
        if (mi) {
            MiroArgs<StgArgs<DrawArgsBase<LSE, CON>>> y;
            static_cast<StgArgs<DrawArgsBase<LSE, CON>> &>(y) = x;
            y.mrows = mi->rows;
            y.mdebug = mi->debug;
            y.mvocab = vocab;
            y.mws = mws;
            hipLaunchKernelGGL((sample_draw_kernel<SPEC, LSE, CON, true, true>), dim3(rows), dim3(kThreads), 0, stream, y, RT, cand);
            return;
        }
        hipLaunchKernelGGL((sample_draw_kernel<SPEC, LSE, CON, true>), dim3(rows), dim3(kThreads), 0, stream, x, RT, cand);
    });
}

int launch_logprobs_f16(const void *logits, int ld, int vocab, int rows, const int32_t *target, float *out_logprob, float *out_lse, void *partials, hipStream_t stream,
                        hipError_t *hip_err) {
    const int nchunks = sample_chunks(vocab);
    hipLaunchKernelGGL(logprobs_partials_kernel, dim3(nchunks, rows), dim3(kThreads), 0, stream, static_cast<const half_t *>(logits), ld, vocab, nchunks,
                       static_cast<float2_t *>(partials));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(logprobs_merge_kernel, dim3(rows), dim3(kThreads), 0, stream, static_cast<const half_t *>(logits), ld, vocab, nchunks,
                           static_cast<const float2_t *>(partials), target, out_logprob, out_lse);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

int launch_draft_ngram(const int32_t *history, const int32_t *script, int hist_stride, const int32_t *pos, int pos_bound, int batch, int rows_per_seq, int ngram,
                       int32_t *row_token, int32_t *row_pos, hipStream_t stream, hipError_t *hip_err) {
    hipLaunchKernelGGL(draft_ngram_kernel, dim3(batch), dim3(kThreads), 0, stream, history, script, hist_stride, pos, pos_bound, rows_per_seq, ngram, row_token, row_pos);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

int launch_embed_rows_f16(const void *table, int vocab, int hidden, const int32_t *token, void *out, int batch, const int32_t *pos, int pos_bound, void *workspace,
                          hipStream_t stream, hipError_t *hip_err) {
    hipLaunchKernelGGL(embed_rows_kernel, dim3(batch), dim3(kThreads), 0, stream, static_cast<const uint4_t *>(table), vocab, hidden / 8, token, static_cast<uint4_t *>(out), pos,
                       pos_bound, static_cast<unsigned *>(workspace));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (hip_err) *hip_err = e;
        return TCE_ERR_HIP;
    }
    return TCE_OK;
}

}  // namespace tce
