// Group copies (w4a16_mfma_layout.hpp: packed_view / group_member_ok) against the single-linear arithmetic applied to the row-concatenated linear.  Host only.
// A member's slice of every part must begin exactly where the concatenation keeps the member's first row / tile, and end where the next member's begins.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "w4a16_mfma_layout.hpp"

using namespace tce;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                 \
        }                                                            \
    } while (0)

static void group(const std::vector<int> &ns, int K, int G) {
    int rows = 0;
    for (int n : ns) rows += n;
    const int NG = K / G;
    int tile0 = 0, row0 = 0;
    for (size_t i = 0; i < ns.size(); ++i) {
        const int N = ns[i];
        CHECK(pk::group_member_ok(N, tile0, rows));
        const pk::PackedView v = pk::packed_view(N, K, G, tile0, rows);
        // the member's first code / constant / scale / zero point, as the copy of the concatenation addresses row `row0`
        CHECK(v.words == pk::word_index(row0, 0, K) * 4);
        CHECK(v.consts == pk::consts_offset(rows, K) + pk::const_index(row0, 0, K, G) * 8);
        CHECK(v.last == pk::last_offset(rows, K, G) + (size_t)row0 * 4);
        CHECK(v.dscales == pk::dscales_offset(rows, K, G) + (size_t)(row0 / 16) * NG * 16 * 2);
        CHECK(v.dzeros == pk::dzeros_offset(rows, K, G) + (size_t)(row0 / 16) * NG * 2 * 4);
        // every (row, k) of the member: the word of the member's own copy, shifted by the slice's start, is the concatenation's word
        for (int n = 0; n < N; n += (N > 64 ? 37 : 1))
            for (int k = 0; k < K; k += 8) CHECK(v.words + pk::word_index(n, k, K) * 4 == pk::word_index(row0 + n, k, K) * 4);
        for (int n = 0; n < N; n += (N > 64 ? 37 : 1))
            for (int g = 0; g < NG; ++g) CHECK(v.consts + pk::const_index(n, g, K, G) * 8 == pk::consts_offset(rows, K) + pk::const_index(row0 + n, g, K, G) * 8);
        // the slice's sizes are the member's own copy's: the next member begins where this one ends
        if (i + 1 < ns.size()) {
            const pk::PackedView w = pk::packed_view(ns[i + 1], K, G, tile0 + N / 16, rows);
            CHECK(w.words == v.words + pk::words_bytes(N, K));
            CHECK(w.consts == v.consts + pk::consts_bytes(N, K, G));
            CHECK(w.last == v.last + pk::last_bytes(N));
            CHECK(w.dscales == v.dscales + pk::dscales_bytes(N, K, G));
            CHECK(w.dzeros == v.dzeros + pk::dzeros_bytes(N, K, G));
        } else {
            CHECK(v.words + pk::words_bytes(N, K) == pk::words_bytes(rows, K));
            CHECK(v.dscales + pk::dscales_bytes(N, K, G) == pk::dscales_offset(rows, K, G) + pk::dscales_bytes(rows, K, G));
            CHECK(v.dzeros + pk::dzeros_bytes(N, K, G) == pk::dzeros_offset(rows, K, G) + pk::dzeros_bytes(rows, K, G));
            CHECK(v.dzeros + pk::dzeros_bytes(N, K, G) <= pk::total_bytes(rows, K, G));
        }
        tile0 += N / 16;
        row0 += N;
    }
}

int main() {
    for (int G : {128, 64, 32})
        for (int K : {128, 1024, 1152, 4096}) {
            group({16, 32}, K, G);
            group({48, 16, 1024}, K, G);
            group({1024, 48, 32, 16}, K, G);
        }
    group({4096, 1024, 1024}, 4096, 128);
    group({14336, 14336}, 4096, 128);
    // an individual copy: 0 / 0, the offsets of the layout as they always were
    const pk::PackedView s = pk::packed_view(40, 256, 64, 0, 0);
    CHECK(s.words == 0 && s.consts == pk::consts_offset(40, 256) && s.last == pk::last_offset(40, 256, 64) && s.dscales == pk::dscales_offset(40, 256, 64) &&
          s.dzeros == pk::dzeros_offset(40, 256, 64));
    CHECK(pk::group_member_ok(40, 0, 0) && !pk::group_member_ok(40, 1, 0));
    // members that cannot be part of a copy
    CHECK(!pk::group_member_ok(40, 0, 80));    // N % 16
    CHECK(!pk::group_member_ok(32, 0, 40));    // the copy's rows % 16
    CHECK(!pk::group_member_ok(32, 2, 48));    // past the copy's end
    CHECK(!pk::group_member_ok(32, -1, 64));
    CHECK(pk::group_member_ok(32, 2, 64));
    if (fails) return 1;
    std::printf("group pack ok\n");
    return 0;
}
