// tuning_modes.hpp -- the numbered modes of tce_w4a16_set_debug_mode (include/tce_tuning.h) as ONE table: a row per family, the rows' accepted sets pairwise disjoint
// (proved below at compile time), so what a mode means depends on its row alone.  Plain C++17, no HIP include: tce_tuning.hip applies the rows to the real setters,
// tests/host/test_tuning_modes.cc to recording stand-ins (every mode against tests/golden/tuning_modes_{product,lab}.txt).
#pragma once
#include <cstdint>
#include <initializer_list>

#include "tce_matmul.h"
#include "tuning_setters.hpp"
#include "tuning_state.hpp"

namespace tce {

struct ModeRow {
    int lo, hi;
    uint64_t only;               // 0: every mode of lo .. hi; else bit i set = lo + i is accepted (hi - lo < 64)
    bool (*lab_only)(int mode);  // non-null and true: a diagnostic instantiation that only the lab build (-DTCE_LAB) holds -- the product build refuses the mode
    void (*apply)(int mode);
    const char *what;
};

constexpr uint64_t only(std::initializer_list<int> offsets) {
    uint64_t bits = 0;
    for (int o : offsets) bits |= uint64_t(1) << o;
    return bits;
}

// the pre-packed GEMM's forced forms: g_tuning.pk_mode is what use_pk (tce_capi.hip) reads, the form goes to the launcher
inline void pk_forced(int pk_mode, int form) {  // whole tiles
    g_tuning.pk_mode = pk_mode;
    set_gemm_pk_ablation(0);
    set_gemm_pk_split(0);
    set_gemm_pk_mode(form, 0);
}
inline void pk_cut(int pk_mode, int form, int runs) {  // every tile's k range cut into `runs` (0: the cost model's choice)
    g_tuning.pk_mode = pk_mode;
    set_gemm_pk_ablation(0);
    set_gemm_pk_mode(form, 0);
    set_gemm_pk_split(runs);
}
inline void pk_ablated(int pk_mode, int form, int abl) {  // parts of the loop switched off (abl 0: back to automatic)
    g_tuning.pk_mode = abl ? pk_mode : 0;
    set_gemm_pk_mode(abl ? form : 0, 0);
    set_gemm_pk_ablation(abl);
}
inline void attention_target(int mode) { set_attention_fast_target(mode - 3000); }
constexpr const char *kAttentionTargetWhat = "fast attention step: workgroups the key range is cut for (3000: the fitted rule, the default)";

constexpr ModeRow kModeRows[] = {
    {0, 4, 0, [](int m) { return m == 1 || m == 2 || m == 4; },
     [](int m) {
         set_gemv_debug_mode(m);
         set_gemv_stream_debug(m, g_debug_buffer);
         set_gemv_ovl_stamps(m == 2 ? g_debug_buffer : nullptr);
         g_tuning.debug_mode = m;
     },
     "GEMV kernels, M = 1: 0 normal, 1 stream the weights only, 2 normal math plus per-wave timestamps into the debug buffer, 3 / 4 timing variants of the persistent kernel"},
    {10, 12, 0, nullptr, [](int m) { set_gemv_order(m - 10); }, "row-block GEMV, M = 1: 10 the rule (x first when the grid is one generation), 11 x first always, 12 weights first always"},
    {20, 30, 0, nullptr,
     [](int m) {
         g_tuning.skinny_enabled = m != 29;
         set_skinny_config(m == 29 ? 0 : (m == 30 ? 9 : m - 20));
     },
     "small-batch kernel tuning: 20 automatic, 21 / 22 / 24 / 28 = waves per tile, 30 = shared-x form, 29 = off"},
    {40, 48, only({0, 1, 2, 4, 8}), nullptr,
     [](int m) {
         set_gemm_xcd_rows(m - 40);
         set_gemm_dma_xcd_rows(m - 40);
     },
     "GEMM: XCD grid rows (40: automatic for the LDS-DMA kernel)"},
    {50, 52, 0, nullptr, [](int m) { set_gemm_dma_mode(m - 50); }, "LDS-DMA GEMM: wave quartets per tile (50 automatic)"},
    {60, 69, 0, nullptr,
     [](int m) {
         const int f = m - 60;
         g_tuning.pk_mode = f;
         set_gemm_pk_split(0);
         set_gemm_pk_ablation(0);
         set_gemm_pk_mode(f >= 1 && f <= 8 && f != 5 ? f : 0, 0);
     },
     "pre-packed GEMM: 60 automatic, 61 / 62 / 63 / 64 forced 128-row forms, 66 / 67 the 256-row wave tiles (whole tiles / k range cut), 68 the 256-row tile shared by two quartets, 69 off"},
    {70, 74, 0, nullptr, [](int m) { set_w8a8_ksplit(m - 70); }, "W8A8: wave quartets per tile (70 automatic; 73: automatic, without the decode-sized wave-per-column kernels)"},
    {75, 78, 0, nullptr, [](int m) { set_w8a8_big(m == 78 ? 9 : m - 75); }, "W8A8, the 128-row tiles: 75 the rule, 76 / 77 forced with 128 / 64 columns, 78 off"},
    {80, 87, 0, nullptr, [](int m) { set_lnq_form(m - 80); },
     "LayerNormQ + W8A8 group: 81 = the workgroup-per-8-rows form at every k; wide form: 83 no sums (wrong results), 84 no output rows, 85 phase times of workgroup 0 into the debug buffer, 86 "
     "the wide form from k = 256 on, 87 the 4-wave form's single row walked by one wave"},
    {170, 179, only({0, 1, 2, 4, 9}), nullptr, [](int m) { set_w8a8_deep(m - 170); },
     "W8A8, the 64 x 64 tile with 8 k-steps in flight: 170 the rule, 171 / 172 / 174 forced with 1 / 2 / 4 quartets, 179 off"},
    {176, 177, 0, nullptr, [](int m) { set_w8a8_big(m - 173); }, "W8A8, the 128-row tiles with two quartets per tile: 176 / 177 forced with 128 / 64 columns"},
    {180, 188, 0, nullptr, [](int m) { set_w8a8_xsplit(m - 180); },
     "W8A8, a tile's k-steps cut across workgroups (needs tce_w8a8_desc_v2.scratch): 180 the rule, 181 off, 182 / 183 / 184 / 186 / 188 that many runs"},
    {190, 192, 0, nullptr, [](int m) { set_w8a8_rows32(m - 190); }, "W8A8, 32 x 64 tiles (round 6): 190 the rule, 191 forced wherever the 64 x 64 kernel would run, 192 off"},
    {600, 639, 0, [](int m) { return m != 600; }, [](int m) { pk_ablated(1, 1, m - 600); }, "pre-packed GEMM with parts of its loop switched off (timing experiments, one quartet; 600: off)"},
    {640, 644, 0, nullptr, [](int m) { pk_cut(4, 4, m - 640); }, "pre-packed GEMM, k range cut across workgroups: runs per cut tile forced (640: the cost model's choice)"},
    {645, 664, 0, [](int) { return true; }, [](int m) { pk_ablated(1, 1, m - 600); }, "pre-packed GEMM with parts of its loop switched off, continued (600 + a)"},
    {672, 674, 0, nullptr, [](int m) { pk_cut(7, 7, m - 670); }, "pre-packed GEMM, 256-row wave tiles with every tile's k range cut into 2 / 3 / 4 runs"},
    {690, 691, 0, nullptr, [](int m) { set_gemm_pk256_auto(m - 690); }, "pre-packed GEMM: 691 = the dispatcher may pick the 256-row forms (the default), 690 = never (A/B against the 128-row forms)"},
    {692, 693, 0, nullptr, [](int m) { set_gemm_pk_wide_auto(m - 692); }, "pre-packed GEMM: 693 = the dispatcher may pick the wide forms, 692 = never"},
    {694, 695, 0, nullptr, [](int m) { set_gemm_pk_handoff(m - 694); },
     "pre-packed GEMM, k range cut in two: 695 = run 0 hands its tile to run 1 (the default), 694 = both runs meet at the counter (A/B)"},
    {696, 698, 0, nullptr, [](int m) { set_gemm_pk_prio(m == 698 ? -1 : m - 696); }, "pre-packed GEMM, the two waves of a SIMD at different priorities: 696 off, 697 on, 698 the launcher's rule (default)"},
    {1000, 1256, 0, nullptr, [](int m) { set_skinny_max_m(m - 1000); }, "small-batch kernel: largest M it takes"},
    {2600, 2664, 0, [](int m) { return m != 2600; }, [](int m) { pk_ablated(6, 6, m - 2600); }, "the 600 + a switches on the 256-row form (round 5; 2600: off)"},
    {2669, 2676, 0, nullptr, [](int m) { pk_forced(8, m - 2660); },
     "pre-packed GEMM, forms 9 .. 16 forced: 2669 256 x 256 tiles, two quartets side by side; the wide form (128 rows x 64 columns per wave) on 128 x 256 tiles: 2670 one quartet, 2671 two "
     "quartets alternating the k-blocks, 2672 every tile's k range cut across workgroups; on 128 x 192 tiles (48 columns per wave): 2673 one quartet, 2674 two; 2675 on 128 x 512 tiles (two "
     "quartets side by side on one activation ring); 2676 128 x 128 tiles, two quartets alternating a run's k-blocks, every tile's k range handed off between two workgroups"},
    {2682, 2684, 0, nullptr, [](int m) { pk_cut(8, 12, m - 2680); }, "the wide form with every tile's k range cut into 2 / 3 / 4 runs"},
    {2700, 2708, only({0, 4, 8}), nullptr, [](int m) { set_attention_prefill_waves(100 + m - 2700); }, "prefill attention, block pairing forced on: 2700 / 2704 / 2708 as 2950 / 2954 / 2958"},
    {2800, 2808, only({0, 4, 8}), nullptr, [](int m) { set_attention_prefill_waves(200 + m - 2800); }, "prefill attention, block pairing forced off: 2800 / 2804 / 2808 as 2950 / 2954 / 2958"},
    {2900, 2916, 0, nullptr, [](int m) { set_attention_fast_waves(m - 2900); }, "fast attention step: waves per workgroup (2900: by the chunk length, the default; 2904 / 2908 / 2916)"},
    {2920, 2924, 0, nullptr, [](int m) { set_attention_fast_fuse(m - 2920); }, "fast attention step, grouped queries: query heads per workgroup (2920: the rule; 2921 / 2922 / 2924)"},
    {2930, 2931, 0, nullptr, [](int m) { set_attention_fast_probe_no_combine(m - 2930); },
     "fast attention step, timing experiment: 2931 = partial states stored plainly, no combine, the output NOT written (2930: off)"},
    {2950, 2968, only({0, 4, 8, 14, 18}), nullptr, [](int m) { set_attention_prefill_waves(m - 2950); },
     "prefill attention: 2950 automatic; 2954 / 2958: 4 / 8 waves x 1 row tile; 2964 / 2968: x 2 row tiles"},
    {3000, 6915, 0, nullptr, attention_target, kAttentionTargetWhat},
    {6916, 6917, 0, nullptr, [](int m) { set_gemm_pk_form16_auto(m - 6916); }, "pre-packed GEMM: form 16 (2676) offered to the dispatcher (6917, the default) or not (6916)"},
    {6918, 6949, 0, nullptr, attention_target, kAttentionTargetWhat},
    {6950, 6958, 0, nullptr, [](int m) { set_gemm_pk_handoff_delta(m - 6950); }, "pre-packed GEMM, the hand-off's cut: run 0 shorter than run 1 by (mode - 6950) k-blocks (tuning)"},
    {6959, 6971, 0, nullptr, attention_target, kAttentionTargetWhat},
    {6972, 6974, 0, nullptr, [](int m) { set_gemm_pk_prio(m - 6970); }, "pre-packed GEMM, the priorities of 696 .. 698: 6972 priority 3, 6973 priority 1, 6974 by slot parity instead of dispatch round"},
    {6975, 7699, 0, nullptr, attention_target, kAttentionTargetWhat},
    {7700, 7703, 0, [](int m) { return m == 7702; },
     [](int m) {
         if (m <= 7701) set_i8_token_mode(m - 7700);
         else set_i8_token_stamps(m == 7702 ? g_debug_buffer : nullptr);
     },
     "TCE_PLAN_TAGGED on packed copies: 7700 the int8-contraction token kernel where the list allows (default), 7701 never (round 2's kernel); 7702 / 7703: plans built from now on record "
     "per-stage wall-clock stamps in the debug buffer / stop"},
    {7704, 7705, 0, [](int m) { return m == 7704; }, [](int m) { set_gemv_i8_stamps(m == 7704 ? g_debug_buffer : nullptr); },
     "the int8 decode kernel's time budget: plain launches from now on record wave 0's clock readings per workgroup in the debug buffer (7704) / stop (7705)"},
    {7710, 8222, 0, nullptr, [](int m) { set_i8_token_max_units(m - 7710); },
     "the int8 token kernel: a stage with more than (mode - 7710) units per workgroup ends the prefix the kernel takes (7710: the default, 512)"},
    {8223, 11192, 0, nullptr, attention_target, kAttentionTargetWhat},
    {15000, 15001, 0, nullptr, [](int m) { g_tuning.plan_eager = m - 15000; }, "experiment: tce_plan_launch issues a stream-ordered plan's launches eagerly (15001) / replays its graph (15000)"},
    {19000, 19999, 0, nullptr, [](int m) { set_w8a8_kslice(m - 19000); },
     "W8A8, the whole tile in every wave (round 6): 19000 the rule, 19001 off, 19304 / 19404 / 19904 the 32 x 48 / 32 x 64 / 64 x 64 tile forced wherever the 64 x 64 kernel would run"},
    {26000, 26256, 0, [](int m) { return m != 26000; }, [](int m) { pk_ablated(8, 10, m - 26000); },
     "the wide form (one quartet) with parts of its loop switched off (timing experiments; 26000: off)"},
    {50000, 50499, 0, nullptr, [](int m) { set_gemv_ovl_config((m - 50000) % 100, (m - 50000) / 100); },
     "overlapped plans: 50000 + 100 * graph branches (0 = 2) + ring slots per wave (0 = as many as fit, 2..4)"},
    {51000, 51016, 0, nullptr, [](int m) { set_gemv_i8_mixed_waves(m - 51000); }, "the mixed decode launch (tce_w4a16_forward_independent): waves per workgroup forced (51000: the rule)"},
};

constexpr bool mode_row_accepts(const ModeRow &r, int mode) { return mode >= r.lo && mode <= r.hi && (r.only == 0 || ((r.only >> (mode - r.lo)) & 1)); }

constexpr const ModeRow *find_mode_row(int mode) {
    for (const ModeRow &r : kModeRows)
        if (mode_row_accepts(r, mode)) return &r;
    return nullptr;
}

// no mode is accepted by two rows: ranges that overlap must both list their modes, and the lists must not meet
constexpr bool mode_rows_well_formed() {
    for (const ModeRow &a : kModeRows) {
        if (a.lo > a.hi || (a.only && (a.hi - a.lo >= 64 || (a.only >> (a.hi - a.lo)) > 1))) return false;
        for (const ModeRow &b : kModeRows) {
            if (&a == &b || a.hi < b.lo || b.hi < a.lo) continue;
            if (!a.only && !b.only) return false;
            const ModeRow &listed = a.only ? a : b, &other = a.only ? b : a;
            for (int m = listed.lo; m <= listed.hi; ++m)
                if (mode_row_accepts(listed, m) && mode_row_accepts(other, m)) return false;
        }
    }
    return true;
}
static_assert(mode_rows_well_formed(), "tuning_modes.hpp: two rows accept the same mode, or a row is malformed");

#ifdef TCE_LAB
constexpr bool kLabBuild = true;
#else
constexpr bool kLabBuild = false;
#endif

// tce_w4a16_set_debug_mode: the one row that accepts the mode, applied -- or TCE_ERR_BAD_ARG, nothing changed
inline int apply_debug_mode(int mode, bool lab = kLabBuild) {
    const ModeRow *r = find_mode_row(mode);
    if (!r) return fail(TCE_ERR_BAD_ARG, "debug mode %d", mode);
    if (!lab && r->lab_only && r->lab_only(mode))
        return fail(TCE_ERR_BAD_ARG, "debug mode %d selects a diagnostic instantiation that only the lab build holds (python -m tinychatengine_amd.build --lab, TCE_LIB_PATH)", mode);
    r->apply(mode);
    return TCE_OK;
}

}  // namespace tce
