// tce_tuning.hip -- the tuning and diagnostics entry points of libtce_hip.so (include/tce_tuning.h): every function declared there, and the calling thread's settings
// they write (tuning_state.hpp; the dispatch in tce_capi.hip reads them).  No kernel lives here.  The numbered modes are the table of tuning_modes.hpp.
#include "tce_common.hpp"
#include "tuning_modes.hpp"
#include "w4a16_kernels.hpp"

namespace tce {
thread_local TuningState g_tuning;
void *g_debug_buffer = nullptr;
}  // namespace tce

using tce::fail;
using tce::g_tuning;

extern "C" {

int tce_w4a16_set_gemv_config(int rows, int wn, int wk, int depth) {
    if (rows == 0 && wn == 0 && wk == 0) {
        g_tuning.gemv_rows = g_tuning.gemv_wn = g_tuning.gemv_wk = g_tuning.gemv_depth = 0;
        g_tuning.gemv_kernel = 0;
        tce::set_gemv_stream_config(0, 0, 0);
        return TCE_OK;
    }
    if (wk == 0) {  // persistent stream kernel: rows per unit, waves per workgroup, units in flight
        if ((rows % 10 != 0 && rows % 10 != 1 && rows % 10 != 2 && rows % 10 != 4) || rows < 0 || rows >= 90 || wn < 1 || wn > 16 || (depth != 0 && depth != 2 && depth != 3))
            return fail(TCE_ERR_BAD_ARG, "stream GEMV config rows=%d waves=%d depth=%d is not available", rows, wn, depth);
        tce::set_gemv_stream_config(rows, wn, depth);
        g_tuning.gemv_kernel = 2;
        return TCE_OK;
    }
    const int dd = depth ? depth : 2;
    if (!tce::gemv_variant_exists(rows, wn, wk, dd))
        return fail(TCE_ERR_BAD_ARG, "GEMV variant rows=%d wn=%d wk=%d depth=%d was not compiled", rows, wn, wk, dd);
    g_tuning.gemv_rows = rows;
    g_tuning.gemv_wn = wn;
    g_tuning.gemv_wk = wk;
    g_tuning.gemv_depth = dd;
    g_tuning.gemv_kernel = 1;
    return TCE_OK;
}

int tce_w4a16_set_gemv_i8(int mode, int rows) {
    if (mode < 0 || mode > 1 || rows < 0 || rows > 2) return fail(TCE_ERR_BAD_ARG, "tce_w4a16_set_gemv_i8: mode %d rows %d", mode, rows);
    tce::set_gemv_i8_mode(mode, rows);
    return TCE_OK;
}

int tce_attention_set_tuning(int waves_per_workgroup, int workgroups, int heads_per_workgroup) {
    const bool ok = (waves_per_workgroup == 0 || waves_per_workgroup == 4 || waves_per_workgroup == 8 || waves_per_workgroup == 16) &&
                    (workgroups == 0 || (workgroups >= 32 && workgroups <= 8192)) &&
                    (heads_per_workgroup == 0 || heads_per_workgroup == 1 || heads_per_workgroup == 2 || heads_per_workgroup == 4);
    if (!ok) return fail(TCE_ERR_BAD_ARG, "tce_attention_set_tuning(%d, %d, %d)", waves_per_workgroup, workgroups, heads_per_workgroup);
    tce::set_attention_fast_waves(waves_per_workgroup);
    tce::set_attention_fast_target(workgroups);
    tce::set_attention_fast_fuse(heads_per_workgroup);
    return TCE_OK;
}

int tce_w8a8_set_tuning(int quartets_per_tile, int big_tiles, int deep_pipeline) {
    const bool ok = (quartets_per_tile == 0 || quartets_per_tile == 1 || quartets_per_tile == 2 || quartets_per_tile == 4) &&
                    ((big_tiles >= 0 && big_tiles <= 4) || big_tiles == 9) &&
                    (deep_pipeline == 0 || deep_pipeline == 1 || deep_pipeline == 2 || deep_pipeline == 4 || deep_pipeline == 9);
    if (!ok) return fail(TCE_ERR_BAD_ARG, "tce_w8a8_set_tuning(%d, %d, %d)", quartets_per_tile, big_tiles, deep_pipeline);
    tce::set_w8a8_ksplit(quartets_per_tile);
    tce::set_w8a8_big(big_tiles);
    tce::set_w8a8_deep(deep_pipeline);
    return TCE_OK;
}

int tce_w4a16_set_debug_mode(int mode) { return tce::apply_debug_mode(mode); }

int tce_w4a16_set_debug_buffer(void *buf) {
    tce::set_lnq_stamps(buf);
    tce::set_gemv_debug_buffer(buf);
    tce::g_debug_buffer = buf;
    tce::set_gemv_stream_debug(g_tuning.debug_mode, buf);
    tce::set_gemv_ovl_stamps(g_tuning.debug_mode == 2 ? buf : nullptr);
    return TCE_OK;
}

int tce_w4a16_set_gemm_config(int mt, int nt) {
    if (mt == 0 && nt == 0) {
        g_tuning.gemm_mt = g_tuning.gemm_nt = 0;
        return TCE_OK;
    }
    if (!tce::gemm_variant_exists(mt >= 200 ? mt - 200 : mt, nt)) return fail(TCE_ERR_BAD_ARG, "GEMM variant %dx%d was not compiled", mt, nt);
    g_tuning.gemm_mt = mt;
    g_tuning.gemm_nt = nt;
    return TCE_OK;
}

int tce_w4a16_gemv_variant(int idx, int *rows, int *wn, int *wk, int *depth) {
    static const int table[][4] = {
#define TCE_V(R, N_, K_, D_) {R, N_, K_, D_},
        TCE_GEMV_VARIANTS(TCE_V)
#undef TCE_V
    };
    const int n = (int)(sizeof(table) / sizeof(table[0]));
    if (idx < 0 || idx >= n || !rows || !wn || !wk || !depth) return TCE_ERR_BAD_ARG;
    *rows = table[idx][0];
    *wn = table[idx][1];
    *wk = table[idx][2];
    *depth = table[idx][3];
    return TCE_OK;
}

int tce_w4a16_gemm_variant(int idx, int *mt, int *nt) {
    static const int table[][2] = {
#define TCE_V(M_, N_) {M_, N_}, {100 + M_, N_}, {200 + M_, N_},
        TCE_GEMM_VARIANTS(TCE_V)
#undef TCE_V
    };
    const int n = (int)(sizeof(table) / sizeof(table[0]));
    if (idx < 0 || idx >= n || !mt || !nt) return TCE_ERR_BAD_ARG;
    *mt = table[idx][0];
    *nt = table[idx][1];
    return TCE_OK;
}

}  // extern "C"
