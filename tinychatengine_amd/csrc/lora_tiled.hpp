// lora_tiled.hpp -- what the tiled LoRA units share (lora_tiled.hip: the shrink and the expand; lora_tiled_seg.hip: the segmented expands): the tile, the staged chunk of
// B and the walk over a tile's distinct adapters.
#pragma once
#include "tce_common.hpp"

namespace tce {
namespace {

constexpr int kTileRows = TCE_LORA_TILE_ROWS;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kExpandCols = 128;   // columns of an expand workgroup: 32 per wave
constexpr int kChunkJ = 64;        // rows of B staged at once
constexpr int kLdB = kExpandCols + 8;  // fp32 row stride of the staged chunk: the four lane groups' rows (2 kq + s) fall on different banks
static_assert(kTileRows == 32, "lane i and lane 32 + i read word i; two MFMA row blocks");
static_assert(kChunkJ * (kExpandCols / 8) == 4 * kThreads && kExpandCols == kWaves * 32, "the expand's request view: four 16-byte pieces per thread; two column blocks per wave");

// the tile's distinct valid adapters, every wave for itself and all waves alike: body(adapter, the 32-bit set of the tile's rows on it)
template <class Body>
__device__ __forceinline__ void walk_adapters(const int32_t *__restrict__ row_adapter, int row0, int rows, int n_adapters, Body body) {
    const int i = row0 + (threadIdx.x & 31);
    const int w = i < rows ? row_adapter[i] : -1;
    const bool valid = w >= 0 && w < n_adapters;
    unsigned pending = (unsigned)__ballot(valid);
    while (pending) {
        const int a = __builtin_amdgcn_readlane(w, __builtin_amdgcn_readfirstlane(__builtin_ctz(pending)));
        const unsigned same = (unsigned)__ballot(valid && w == a);
        pending &= ~same;
        body(a, same);
    }
}

}  // namespace
}  // namespace tce
