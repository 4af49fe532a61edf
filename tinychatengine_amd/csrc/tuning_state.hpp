// tuning_state.hpp -- what the C ABI's units share on the host: the calling thread's tuning settings (written by tce_tuning.hip, read by the dispatch in
// tce_capi.hip), the debug buffer, and the thread's error text.  Plain C++ (no HIP include).
#pragma once

namespace tce {

struct TuningState {
    int gemv_rows = 0, gemv_wn = 0, gemv_wk = 0, gemv_depth = 0;  // tce_w4a16_set_gemv_config: the forced row-block variant
    int gemv_kernel = 0;     // 0 automatic, 1 workgroup-per-row-block kernel forced, 2 persistent stream kernel forced
    int gemm_mt = 0, gemm_nt = 0;  // tce_w4a16_set_gemm_config
    int pk_mode = 0;         // 0 automatic, 1 .. 8 forced form (taken whenever a packed copy is given), 9 off
    int skinny_enabled = 1;  // tuning: tce_w4a16_set_debug_mode(29) routes 3 <= M <= 16 to the GEMV / GEMM kernels again
    int plan_eager = 0;      // experiment (tce_w4a16_set_debug_mode(15001 / 15000)): stream-ordered plans issue their launches one by one instead of replaying the graph
    int debug_mode = 0;      // the GEMV kernels' mode 0 .. 4
};
extern thread_local TuningState g_tuning;  // (tce_tuning.hip)
extern void *g_debug_buffer;               // tce_w4a16_set_debug_buffer: ONE per process, whichever thread set it last (tce_tuning.hip)

extern thread_local char g_err[512];       // tce_last_error (tce_capi.hip)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));  // writes g_err, returns code

}  // namespace tce
