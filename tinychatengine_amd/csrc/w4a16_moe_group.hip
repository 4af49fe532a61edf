// w4a16_moe_group.hip -- the stable grouping of the routed pairs by expert, in parallel (include/tce_matmul.h, "Mixture of experts": tce_moe_group_parallel,
// tce_moe_route_parallel_f16), gfx950.  The prompt-sized form of w4a16_moe.hip's moe_group_kernel, which is one wave whose lane e walks every pair.
//
//     ids int32 [P]  ->  count int32 [E], list int32 [E][P]:   count[e] = the pairs p with ids[p] == e, list[e][0 .. count[e]) = those p, ascending.
//     A word of ids outside [0, E) is in no list; words of list[e] at and beyond count[e] are not written.
//
// The pairs are cut into chunks of kChunk = 1024; chunk c is one workgroup of 16 waves, ONE PAIR PER LANE: wave s of the workgroup holds the chunk's sub-block s, the
// pairs c * 1024 + 64 s + lane.  The grid is ceil(P / 1024), which the host knows; nothing is read back.  The place of pair p in its expert's list is a sum of three
// COUNTS of pairs that precede it in ascending order, so it depends on ids, P and E alone:
//
//     place(p) = (pairs naming e in the chunks in front of p's)  +  (pairs naming e in the waves in front of p's, inside the chunk)  +  (lanes below p's that name e)
//
//   * the third term and a wave's per-expert counts come from ONE loop over the distinct ids present in the wave (wave_rank): the lowest pending lane's id is read
//     (v_readlane), the lanes that hold it vote (one ballot), a lane's rank is the popcount of the vote below it, the vote's popcount is the wave's count of that
//     id, and the voters leave the pending set.  min(E, 64) rounds at the most, of scalar work; the ids stay in registers (an id is needed by its own lane only, so
//     the chunk is not staged in LDS: the only LDS traffic is the counts);
//   * launch A (moe_group_hist_kernel): the 16 waves' counts meet in LDS [16][64]; lane e of wave 0 adds them and stores hist[c][e];
//   * launch B (moe_group_place_kernel): the same loop again (cheaper than storing and re-reading a rank per pair); meanwhile thread (s, e) adds hist[c'][e] for
//     c' = s, s + 16, ... < c (at most 4 loads at the pair cap: all 1024 threads share the up to 64 chunks in front).  Lane e of wave 0 adds those 16 partial sums
//     and runs the exclusive scan over the 16 waves' counts in place; the last chunk's run ends at count[e].  Then every lane stores its p at list[e][scan + rank].
// No atomics of any kind (every LDS word has one writer: the lane that leads a vote writes its wave's count of that id into the wave's own row, which the wave
// cleared itself), no global counters, no arrival order anywhere.  hist int32 [chunks][E] lies in the head of the workspace's y section, which nothing reads between
// the route and tce_moe_down_f16; the entry points refuse a call whose y section is smaller than hist.
// A captured graph follows a routing that changes: both grids are functions of P.
#include "w4a16_moe.hpp"

namespace tce {
namespace {

constexpr int kChunk = 1024;         // pairs per workgroup: w4a16_moe.hip's kGroupChunk
constexpr int kSubs = kChunk / 64;   // waves per workgroup = sub-blocks of a chunk

// The lane's rank among the lower lanes of its wave that hold the same id, and tab[v] = the wave's count of every id v present (tab: the wave's own 64 words, cleared
// by the wave).  A lane that is not `valid` takes no part: it is in no vote, and its return value is 0.
__device__ __forceinline__ int wave_rank(int id, bool valid, int lane, int32_t *tab) {
    unsigned long long todo = __ballot(valid);
    int rank = 0;
    while (todo) {  // (wave-uniform)
        const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
        const int v = __builtin_amdgcn_readlane(id, first);
        const bool mine = valid && id == v;
        const unsigned long long same = __ballot(mine);
        if (mine) rank = __popcll(same & ((1ull << lane) - 1ull));
        if (lane == first) tab[v] = __popcll(same);
        todo &= ~same;
    }
    return rank;
}

__global__ __launch_bounds__(kChunk) void moe_group_hist_kernel(const int32_t *__restrict__ ids, int32_t *__restrict__ hist, int P, int E) {
    __shared__ int32_t sub[kSubs][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6, p = blockIdx.x * kChunk + threadIdx.x;
    const int id = p < P ? ids[p] : -1;
    sub[s][lane] = 0;
    __builtin_amdgcn_wave_barrier();  // (a wave's LDS operations complete in order: the row is clear before a vote's leader writes into it)
    wave_rank(id, (unsigned)id < (unsigned)E, lane, sub[s]);
    __syncthreads();
    if (threadIdx.x < E) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < kSubs; ++j) n += sub[j][threadIdx.x];
        hist[(size_t)blockIdx.x * E + threadIdx.x] = n;
    }
}

__global__ __launch_bounds__(kChunk) void moe_group_place_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ hist, int32_t *__restrict__ count,
                                                                  int32_t *__restrict__ list, int P, int E) {
    __shared__ int32_t sub[kSubs][64], front[kSubs][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6, c = blockIdx.x, p = c * kChunk + threadIdx.x;
    const int id = p < P ? ids[p] : -1;
    const bool valid = (unsigned)id < (unsigned)E;
    int before = 0;  // expert `lane` in the chunks s, s + 16, ... in front of this one
    if (lane < E)
        for (int cc = s; cc < c; cc += kSubs) before += hist[(size_t)cc * E + lane];
    sub[s][lane] = 0;
    __builtin_amdgcn_wave_barrier();
    const int rank = wave_rank(id, valid, lane, sub[s]);
    front[s][lane] = before;
    __syncthreads();
    if (s == 0) {  // lane = expert: the chunks in front, then the exclusive scan over the waves of this chunk, in place
        int run = 0;
#pragma unroll
        for (int j = 0; j < kSubs; ++j) run += front[j][lane];
#pragma unroll
        for (int j = 0; j < kSubs; ++j) {
            const int n = sub[j][lane];
            sub[j][lane] = run;
            run += n;
        }
        if (c == (int)gridDim.x - 1 && lane < E) count[lane] = run;
    }
    __syncthreads();
    if (valid) list[(size_t)id * P + sub[s][id] + rank] = p;  // (sub[s][id] + rank < count[id] <= P: inside list[id])
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

// hist int32 [chunks][E]: what the grouping borrows from the head of the y section
size_t moe_group_hist_bytes(int rows, int k, int E) { return (((size_t)rows * k + kChunk - 1) / kChunk) * (size_t)E * 4; }

int launch_moe_group_parallel(int rows, int k, int E, int n_max, void *workspace, hipStream_t stream, hipError_t *hip_err) {
    const MoeLayout L = moe_layout(rows, k, E, n_max);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const int32_t *ids = reinterpret_cast<const int32_t *>(ws + L.ids);
    int32_t *hist = reinterpret_cast<int32_t *>(ws + L.y);
    const int P = rows * k, chunks = (P + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(moe_group_hist_kernel, dim3(chunks), dim3(kChunk), 0, stream, ids, hist, P, E);
    if (const int rc = launched(hip_err)) return rc;
    hipLaunchKernelGGL(moe_group_place_kernel, dim3(chunks), dim3(kChunk), 0, stream, ids, hist, reinterpret_cast<int32_t *>(ws + L.count),
                       reinterpret_cast<int32_t *>(ws + L.list), P, E);
    return launched(hip_err);
}

}  // namespace tce
