// test_tuning_modes.cc -- CPU, no HIP: the table of tce_w4a16_set_debug_mode (csrc/tuning_modes.hpp) against what the chain of range checks it replaced did.
// The yardstick is tests/golden/tuning_modes_{product,lab}.txt: the parent commit's function, cut unchanged and compiled against recording stand-ins (plain / -DTCE_LAB),
// called for every mode below with the four host-side settings preset to a sentinel; per mode the setter calls in order, the return code and the four settings
// (`_`: untouched).  The files are run-length folded: `lo hi record`, an integer of the record either literal or `m-c` / `m+c` / `m` (relative to the mode).
// Here the same stand-ins sit behind the table: every mode of -16 .. 70000, INT_MIN and INT_MAX must give the golden's record, in both builds, and no mode may be
// accepted by two rows.  Exit 1 on any difference, each printed with both records.
//     test_tuning_modes GOLDEN_DIR
#include <cctype>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>

#include "tuning_modes.hpp"

static std::string g_log;
static void rec(const char *name, std::initializer_list<long long> a) {
    g_log += name;
    g_log += "(";
    bool first = true;
    for (long long v : a) {
        if (!first) g_log += ",";
        g_log += std::to_string(v);
        first = false;
    }
    g_log += ") ";
}
static const char *ptr_name(const void *p) { return p ? "buf" : "null"; }

namespace tce {
#define S1(n) \
    void n(int a) { rec(#n, {a}); }
#define S2(n) \
    void n(int a, int b) { rec(#n, {a, b}); }
#define SP(n) \
    void n(void *p) { g_log += std::string(#n "(") + ptr_name(p) + ") "; }
S2(set_gemv_ovl_config) S1(set_attention_fast_probe_no_combine) S1(set_attention_fast_fuse) S1(set_attention_fast_waves) S1(set_attention_fast_target)
S1(set_skinny_max_m) S1(set_attention_prefill_waves) S1(set_w8a8_big) S1(set_i8_token_max_units) S1(set_i8_token_mode) SP(set_i8_token_stamps) SP(set_gemv_i8_stamps)
S1(set_w8a8_kslice) S1(set_w8a8_rows32) S1(set_w8a8_xsplit) S1(set_w8a8_deep) S1(set_w8a8_ksplit) S1(set_gemm_pk_ablation) S2(set_gemm_pk_mode) S1(set_gemm_pk_split)
S1(set_gemv_i8_mixed_waves) S1(set_gemm_pk_form16_auto) S1(set_gemm_pk_handoff_delta) S1(set_gemm_pk_prio) S1(set_gemm_pk_handoff) S1(set_gemm_pk_wide_auto)
S1(set_gemm_pk256_auto) S1(set_gemm_dma_mode) S1(set_gemm_xcd_rows) S1(set_gemm_dma_xcd_rows) S1(set_lnq_form) S1(set_skinny_config) S1(set_gemv_order)
S1(set_gemv_debug_mode) SP(set_gemv_ovl_stamps)
void set_gemv_stream_debug(int mode, void *buf) { g_log += "set_gemv_stream_debug(" + std::to_string(mode) + "," + ptr_name(buf) + ") "; }

thread_local TuningState g_tuning;
static char g_buffer_target;
void *g_debug_buffer = &g_buffer_target;  // (preset non-null, as when the goldens were recorded)
thread_local char g_err[512] = "";
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    g_log += "FAIL ";
    return code;
}
}  // namespace tce

constexpr int kSentinel = -777777;

static std::string record_of(int mode, bool lab) {
    g_log.clear();
    tce::g_tuning.pk_mode = tce::g_tuning.skinny_enabled = tce::g_tuning.plan_eager = tce::g_tuning.debug_mode = kSentinel;
    const int rc = tce::apply_debug_mode(mode, lab);
    auto st = [](int v) { return v == kSentinel ? std::string("_") : std::to_string(v); };
    return g_log + "rc=" + std::to_string(rc) + " pk=" + st(tce::g_tuning.pk_mode) + " skinny=" + st(tce::g_tuning.skinny_enabled) + " eager=" + st(tce::g_tuning.plan_eager) +
           " dbg=" + st(tce::g_tuning.debug_mode);
}

static bool word(char c) { return std::isalnum((unsigned char)c) || c == '_'; }

// a folded record for one mode: a stand-alone `m`, `m-c` or `m+c` becomes the number
static std::string unfold(const std::string &t, long long mode) {
    std::string out;
    for (size_t i = 0; i < t.size(); ++i) {
        if (t[i] != 'm' || (i > 0 && word(t[i - 1])) || (i + 1 < t.size() && word(t[i + 1]))) {
            out += t[i];
            continue;
        }
        long long v = mode;
        if (i + 2 < t.size() && (t[i + 1] == '-' || t[i + 1] == '+') && std::isdigit((unsigned char)t[i + 2])) {
            size_t used = 0;
            const long long c = std::stoll(t.substr(i + 2), &used);
            v = t[i + 1] == '-' ? mode - c : mode + c;
            i += 1 + used;
        }
        out += std::to_string(v);
    }
    return out;
}

struct Fold {
    long long hi;
    std::string record;
};

static std::map<long long, Fold> read_golden(const std::string &path) {
    std::map<long long, Fold> g;  // by lo
    std::ifstream f(path);
    if (!f) {
        std::printf("cannot read %s\n", path.c_str());
        std::exit(2);
    }
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        size_t a = 0, b = 0;
        const long long lo = std::stoll(line, &a);
        const long long hi = std::stoll(line.substr(a), &b);
        g[lo] = Fold{hi, line.substr(a + b + 1)};
    }
    return g;
}

static int check_build(const std::string &dir, bool lab) {
    const char *name = lab ? "lab" : "product";
    const auto golden = read_golden(dir + "/tuning_modes_" + name + ".txt");
    int bad = 0, accepted = 0, swept = 0;
    auto one = [&](int mode) {
        ++swept;
        auto it = golden.upper_bound(mode);
        std::string want = "(no golden line covers this mode)";
        if (it != golden.begin() && mode <= (--it)->second.hi) want = unfold(it->second.record, mode);
        const std::string got = record_of(mode, lab);
        if (got.find("rc=0 ") != std::string::npos) ++accepted;
        if (got != want && ++bad <= 40) std::printf("MISMATCH %s mode %d\n  parent: %s\n  table:  %s\n", name, mode, want.c_str(), got.c_str());
        int rows = 0;
        for (const tce::ModeRow &r : tce::kModeRows) rows += tce::mode_row_accepts(r, mode);
        if (rows > 1 && ++bad <= 40) std::printf("MISMATCH %s mode %d is accepted by %d rows\n", name, mode, rows);
    };
    one(INT_MIN);
    for (int m = -16; m <= 70000; ++m) one(m);
    one(INT_MAX);
    std::printf("tuning modes, %s build: %d modes swept, %d accepted, %d differences\n", name, swept, accepted, bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: %s GOLDEN_DIR\n", argv[0]);
        return 2;
    }
    const int bad = check_build(argv[1], false) + check_build(argv[1], true);
    std::printf("tuning modes: %s\n", bad ? "FAILED" : "ok (0 differences)");
    return bad ? 1 : 0;
}
