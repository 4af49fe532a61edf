// w4a16_moe.hpp -- what the two forms of the expert-grouped contraction share (w4a16_moe.hip: passes of 16 pairs; w4a16_moe_tiled.hip: TCE_MOE_TILE_ROWS x
// TCE_MOE_TILE_PAIRS tiles): the caller's workspace layout, the kernels' argument block and the K split that fixes the order of the K sum in both.
#pragma once
#include "tce_common.hpp"

namespace tce {

constexpr int kMoeWaves = 8;        // waves of a pass-form workgroup = K slices of the K sum, in BOTH forms (the tiled form walks them in one wave)

struct MoeLayout {
    size_t ids, weights, count, list, act, y, total;
};
// the caller's workspace: six sections, each a multiple of 256 bytes (tinychatengine_amd/moe.py mirrors it; include/tce_matmul.h states it)
inline MoeLayout moe_layout(int rows, int k, int E, int n_max) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t P = (size_t)rows * k;
    MoeLayout L;
    L.ids = 0;
    L.weights = L.ids + up(P * 4);
    L.count = L.weights + up(P * 4);
    L.list = L.count + up((size_t)E * 4);
    L.act = L.list + up((size_t)E * P * 4);
    L.y = L.act + up(P * (size_t)n_max * 2);
    L.total = L.y + up(P * (size_t)n_max * 4);
    return L;
}

struct MoeArgs {
    const half_t *X;  // the rows the pairs read: x fp16 [rows][ldx] (up stage, row p / k) or act fp16 [rows * k][ldx] (down stage, row p)
    const uint4_t *qweight;
    const half_t *scales;
    const unsigned *zeros;
    const int32_t *count, *list;
    void *out;  // up: act fp16 [P][ld_out]; down: y fp32 [P][ld_out]
    long long ldx;
    int P, k, N, K, ld_out, scales_stride, zeros_stride, gpw;
};

inline int moe_gpw(int K) { return ((K >> 7) + kMoeWaves - 1) / kMoeWaves; }  // k-blocks per K slice: a function of K alone

// one contraction stage's arguments from the entry point's: up (x fp16 [rows][ldx] -> act fp16 [P][N / 2]) or down (act fp16 [P][K] -> y fp32 [P][N])
inline MoeArgs moe_stage_args(bool up, const void *x, int ldx, const void *qweight, const void *scales, const void *zeros, int rows, int k, int E, int N, int K,
                              int scales_stride, int zeros_stride, int n_max, void *workspace) {
    const MoeLayout L = moe_layout(rows, k, E, n_max);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    MoeArgs a{};
    a.X = up ? static_cast<const half_t *>(x) : reinterpret_cast<const half_t *>(ws + L.act);
    a.ldx = up ? ldx : K;
    a.qweight = static_cast<const uint4_t *>(qweight);
    a.scales = static_cast<const half_t *>(scales);
    a.zeros = static_cast<const unsigned *>(zeros);
    a.count = reinterpret_cast<const int32_t *>(ws + L.count);
    a.list = reinterpret_cast<const int32_t *>(ws + L.list);
    a.out = up ? static_cast<void *>(ws + L.act) : static_cast<void *>(ws + L.y);
    a.P = rows * k;
    a.k = k;
    a.N = N;
    a.K = K;
    a.ld_out = up ? N / 2 : N;
    a.scales_stride = scales_stride;
    a.zeros_stride = zeros_stride;
    a.gpw = moe_gpw(K);
    return a;
}

}  // namespace tce
