// Host check of tinychatengine_amd/csrc/w4a16_unpack16.hpp (compiled and run by tests/test_w4a16_unpack_host.py with ROCm's clang++, which has
// _Float16 on the host): every lane of every operand is exactly 16 (q - z), in the pair order (q0,q4,q1,q5) / (q2,q6,q3,q7), for both operand
// widths, every nibble position, all 16 codes and all 16 zero points, plus 10^5 random words.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "w4a16_unpack16.hpp"

using namespace tce;
using namespace tce::unpack16;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

// nibble i of the word -> its place in the operands: lo = (q0,q4,q1,q5), hi = (q2,q6,q3,q7), the half8 = lo then hi
static const int kOrder[8] = {0, 4, 1, 5, 2, 6, 3, 7};

static int check_word(uint32_t w, unsigned z) {
    int q[8];
    for (int i = 0; i < 8; ++i) q[i] = (int)((w >> (4 * i)) & 0xFu);
    const half_t c = cz_of(z);
    CHECK((float)c == (float)(1024 + 16 * (int)z));
    const half4_t cz4 = cz4_of(z);
    for (int e = 0; e < 4; ++e) CHECK((float)cz4[e] == (float)c);
    const half4_t lo = operand_lo(w, kMaskHi, cz4), hi = operand_hi(w, kMaskHi, cz4);
    const half8_t all = operand8(w, kMaskHi, cz8_splat(c));
    for (int e = 0; e < 8; ++e) {
        const float want = (float)(16 * (q[kOrder[e]] - (int)z));  // an integer, |.| <= 240: exact in binary16 and in float
        CHECK((float)(e < 4 ? lo[e] : hi[e - 4]) == want);
        CHECK((float)all[e] == want);
    }
    if (z == 8) {  // the zero-point-8 constant gives the same operands
        const half4_t c8 = cz4_of_8(kCz8Bits);
        const half4_t lo8 = operand_lo(w, kMaskHi, c8), hi8 = operand_hi(w, kMaskHi, c8);
        for (int e = 0; e < 4; ++e) {
            CHECK((float)c8[e] == 1152.0f);
            CHECK((float)lo8[e] == (float)lo[e] && (float)hi8[e] == (float)hi[e]);
        }
    }
    return 0;
}

int main() {
    // every nibble position x every code x every zero point, the other nibbles all clear and all set (a neighbour must not leak in)
    for (int pos = 0; pos < 8; ++pos)
        for (unsigned code = 0; code < 16; ++code)
            for (unsigned z = 0; z < 16; ++z)
                for (uint32_t fill : {0x00000000u, 0xFFFFFFFFu, 0x5A5A5A5Au}) {
                    const uint32_t w = (fill & ~(0xFu << (4 * pos))) | (code << (4 * pos));
                    if (check_word(w, z)) return 1;
                }
    uint64_t s = 0x9E3779B97F4A7C15ull;  // splitmix64
    for (int i = 0; i < 100000; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t r = s;
        r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
        r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
        r ^= r >> 31;
        if (check_word((uint32_t)r, (unsigned)(r >> 32) & 15u)) return 1;
    }
    std::printf("w4a16 unpack ok\n");
    return 0;
}
