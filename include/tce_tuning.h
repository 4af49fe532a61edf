/* tce_tuning.h -- tuning and diagnostics entry points of libtce_hip.so (round 6: split from tce_matmul.h; implemented in csrc/tce_tuning.hip).
 *
 * NOT part of the operator boundary: a host that drops this library in behind the reference's MatmulOperator never calls anything declared here.
 * These calls select among kernels the dispatcher can reach anyway (forced forms: the parity tests hold every form to the oracle / to each other bit for bit; the
 * sweeps under scripts/ time them) and point diagnostics at a buffer.  Every setting acts on the CALLING THREAD's launches only -- with ONE exception, the debug
 * buffer pointer of tce_w4a16_set_debug_buffer, which is per process -- and computes the same results as the default, except the settings documented as diagnostic
 * instantiations (outputs meaningless), which exist in the lab build only:
 * `python -m tinychatengine_amd.build --lab` -> libtce_hip_lab.so (same sources, -DTCE_LAB); the product library refuses them with TCE_ERR_BAD_ARG. */
#ifndef TCE_TUNING_H
#define TCE_TUNING_H
#include "tce_matmul.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Force a GEMV kernel + launch geometry for every subsequent call from this thread (all 0 = automatic).
 *   waves_k >= 1: the workgroup-per-row-block kernel: rows_per_wave in {1,2,4}, waves_n x waves_k waves per workgroup
 *                 (waves_k of them split K), depth = weight steps kept in flight per wave;
 *   waves_k == 0: the persistent stream kernel: rows_per_wave in {1,2} rows per unit, waves_n (1..16) waves per
 *                 workgroup (one workgroup per CU), depth in {0 = auto, 2, 3} units in flight.
 * TCE_ERR_BAD_ARG if that variant was not compiled. */
TCE_API int tce_w4a16_set_gemv_config(int rows_per_wave, int waves_n, int waves_k, int depth);
/* The decode kernel on pre-packed copies (csrc/w4a16_gemv_i8.hip: M <= 4 rows as an exact int8 contraction on the matrix pipe; taken by tce_w4a16_forward /
 * _forward_group / plans whenever every descriptor of the launch carries `prepacked`, K % 128 == 0 and no fused RMSNorm prologue is asked for; group sizes 64 / 32:
 * M <= 2 / M = 1).  mode 0 = that rule, 1 = off (the fp16 GEMV kernels on the q4_6 arrays take those launches: A/B runs); rows = 16-row tiles per wave for the
 * M = 1, K <= 8192 launches: 0 = the rule (one; two with the RMSNorm prologue where one leaves a short second generation of workgroups), 1, 2.  A row's arithmetic depends on K, the group size and the rows per pass only -- never on N or on
 * `rows`: column shards and grouped launches are bit-identical to the plain launch.  Per host thread (0.1.10: the tuning setters of this header act on the calling thread's launches only -- two host threads driving
 * two devices or streams may force different kernels without a lock; the debug buffer pointer alone is shared); results do not depend on it beyond the kernel family. */
TCE_API int tce_w4a16_set_gemv_i8(int mode, int tiles_per_wave);
/* Tuning / diagnostics switch for the sweeps under scripts/ (per host thread since 0.1.10, never needed by a host).  The modes are the rows of ONE table,
 * csrc/tuning_modes.hpp: a row per family, no mode in two rows; this list is the rows' descriptions, in the table's order.  A value inside a range that the list
 * does not name (2901, 1003) goes to the family's setter as it is.  TCE_ERR_BAD_ARG for every other number.  [lab]: the lab build only.
 *   0..4            GEMV kernels, M = 1: 0 normal; 1 [lab] stream the weights only (no unpack, no dot products: the memory-side ceiling of the access pattern, outputs
 *                   meaningless); 2 [lab] normal math plus per-wave timestamps into the debug buffer; 3 / 4 [4: lab] further timing variants of the persistent kernel
 *   10..12          row-block GEMV, M = 1, issue order: 10 the rule (activations first when the grid is one generation of workgroups, weights first otherwise),
 *                   11 activations first always, 12 weights first always (scripts/gemv_order_ab.py)
 *   20..30          small-batch kernel: 20 automatic, 21 / 22 / 24 / 28 waves per tile, 30 shared-activation form, 29 off
 *   40,41,42,44,48  GEMM XCD grid rows: 40 automatic, 41 / 42 / 44 / 48 forced
 *   50..52          LDS-DMA GEMM wave quartets per tile: 50 automatic, 51 one, 52 two
 *   60..69          pre-packed GEMM: 60 automatic, 61 / 62 / 63 / 64 forced 128-row form (128x128 tile with one quartet / two quartets splitting K / 128x256 tile with two
 *                   quartets side by side / 128x128 with the k range cut across workgroups when a scratch area is given; taken for every M), 66 / 67 the 256-row wave
 *                   tiles (whole tiles / k range cut), 68 the 256-row tile shared by two quartets, 69 off
 *   70..74          W8A8 wave quartets per tile: 70 automatic, 71 / 72 / 74 forced; 73 automatic without the decode-sized wave-per-column kernels
 *   75..78, 176/177 W8A8, the 128-row tiles: 75 the rule, 76 / 77 forced with 128 / 64 columns, 176 / 177 the same with two quartets per tile, 78 off
 *   80..87          LayerNormQ + W8A8 group: 81 the workgroup-per-8-rows form at every k; wide form: 83 no sums (wrong results), 84 no output rows, 85 phase times of
 *                   workgroup 0 into the debug buffer, 86 the wide form from k = 256 on, 87 the 4-wave form's single row walked by one wave
 *   170,171,172,174,179  W8A8, the 64 x 64 tile with 8 k-steps in flight: 170 the rule, 171 / 172 / 174 forced with 1 / 2 / 4 quartets, 179 off
 *   180..188        W8A8, a tile's k-steps cut across workgroups (needs tce_w8a8_desc_v2.scratch): 180 the rule, 181 off, 182 / 183 / 184 / 186 / 188 that many runs
 *   190..192        W8A8, 32 x 64 tiles: 190 the rule, 191 forced wherever the 64 x 64 kernel would run, 192 off
 *   600+a           [lab but 600] a in 0..39, 45..64: pre-packed GEMM, one quartet, with parts of its loop switched off (a: 1 rescale, 2 unpack, 4 fragment reads, 8 MFMAs,
 *                   16 activation DMAs, 32 barriers; only the combinations scripts/gemm_pk_ablation.py uses are compiled); outputs meaningless; 600 back to automatic
 *   640..644        pre-packed GEMM with the k range cut across workgroups: runs per cut tile forced (640: the cost model's choice)
 *   672..674        pre-packed GEMM, 256-row wave tiles with every tile's k range cut into 2 / 3 / 4 runs
 *   690 / 691       the dispatcher may pick the 256-row forms (691, the default) or not (690)
 *   692 / 693       the dispatcher may pick the wide forms (693, the default) or not (692)
 *   694 / 695       a k range cut in two runs: both meet at the counter (694) / run 0 hands its tile to run 1 (695, the default)
 *   696 / 697 / 698 the two waves of a SIMD at different priorities: off / on / the launcher's rule (default)
 *   1000+m          m in 0..256: largest M the small-batch kernel takes (default 1128 = 128; 1016 restricts it to M <= 16)
 *   2600+a          [lab but 2600] a in 0..64: the 600+a switches on the 256-row form (128 / 256: where the refill is issued); outputs meaningless
 *   2669..2676      pre-packed GEMM, forms 9..16 forced: 2669 256 x 256 tiles, two quartets side by side; the wide form (128 rows x 64 columns per wave) on 128 x 256
 *                   tiles: 2670 one quartet, 2671 two quartets alternating the k-blocks, 2672 every tile's k range cut across workgroups; on 128 x 192 tiles (48 columns
 *                   per wave): 2673 one quartet, 2674 two; 2675 on 128 x 512 tiles; 2676 128 x 128 tiles with two quartets AND the k range handed off between two workgroups
 *   2682..2684      the wide form with every tile's k range cut into 2 / 3 / 4 runs
 *   2700,2704,2708 / 2800,2804,2808  prefill attention, block pairing forced on (27xx) / off (28xx); xx = 00 / 04 / 08 as 2950 / 2954 / 2958
 *   2900+w          w in 0..16: fast attention step, waves per workgroup, w in {4, 8, 16} (2900: by the chunk length, the default)
 *   2920+r          r in 0..4: fast attention step, grouped queries: query heads per workgroup, r in {1, 2, 4} (2920: the rule)
 *   2930 / 2931     fast attention step without its combine (2931: timing only, the output is NOT written; 2930: off)
 *   2950,2954,2958,2964,2968  prefill attention: 2950 automatic; 4 / 8 waves x 1 row tile; 2964 / 2968: x 2 row tiles
 *   3000+g          fast attention step: workgroups the key range is cut for (3000: the fitted per-context rule, the default) -- g in 0..8192 LESS the families that lie
 *                   inside the range: the rows are 3000..6915, 6918..6949, 6959..6971, 6975..7699, 8223..11192 (tce_attention_set_tuning reaches every count)
 *   6916 / 6917     form 16 (2676) offered to the dispatcher (6917, the default) or not (6916)
 *   6950+d          d in 0..8: a hand-off's run 0 shorter than run 1 by d k-blocks (default 2)
 *   6972..6974      the priorities of 696..698: level 3 / level 1 / chosen by slot parity
 *   7700..7703      TCE_PLAN_TAGGED on packed copies: the int8 token kernel where the list allows (7700, default) / never (7701); plans built from now on record per-stage
 *                   wall-clock stamps in the debug buffer (7702 [lab]) / stop (7703)
 *   7704 / 7705     the int8 decode kernel (plain M = 1 launches): wave 0 of every workgroup records its clock readings [workgroup][8] in the debug buffer (7704 [lab]) / stop (7705)
 *   7710+u          u in 0..512: a stage with more than u units per workgroup ends the prefix the int8 token kernel takes (7710: the default, 512)
 *   15000 / 15001   plans: graph replay (15000) / eager issue (15001) of a stream-ordered plan
 *   19000..19999    W8A8, the whole tile in every wave, the k-steps dealt to the waves: 19000 the rule, 19001 off, 19304 / 19404 / 19904 the 32 x 48 / 32 x 64 / 64 x 64
 *                   tile forced wherever the 64 x 64 kernel would run
 *   26000+a         [lab but 26000] a in 0..256: the wide form (one quartet) with parts of its loop switched off (as 600+a); outputs meaningless
 *   50000..50499    overlapped plans: 50000 + 100 * graph branches (0 = 2) + ring slots per wave (0 = as many as fit, 2..4)
 *   51000..51016    the mixed decode launch (tce_w4a16_forward_independent): waves per workgroup forced (51000: the rule -- the width that launches the fewest waves)
 *   (6262 / 6263 of round 5 are gone: the two-quartet forms are offered for every group size again -- isa_lint.py RULE 1, profiles/r6/pk_lost_lanes_rule.md)
 * Every setting computes correct results except GEMV modes 1, 3, 4, the "switched off" ablations (600+a, 2600+a, 26000+a), 83 and 2931. */
TCE_API int tce_w4a16_set_debug_mode(int mode);
/* The same knobs per kernel family, by name (round 4: one numbered mode space for every family had already produced an A/B that compared a setting with itself, and
 * a mode of one family landing in another's range).  Per host thread (0.1.10), for tuning sweeps and tests; 0 everywhere = the fitted rules.  Every setting computes the same results.
 *   tce_attention_set_tuning: the fast decode attention step -- waves per workgroup (0 | 4 | 8 | 16), workgroups the key range is cut for (0 | 32..8192),
 *                             query heads per workgroup for grouped queries (0 | 1 | 2 | 4)
 *   tce_w8a8_set_tuning:      wave quartets per 64 x 64 tile (0 | 1 | 2 | 4); the 128-row tiles (0 the rule | 1 / 2: forced with 128 / 64 columns | 3 / 4: the same with two
 *                             quartets | 9 off); the 64 x 64 tile with eight k-steps in flight (0 the rule | 1 / 2 / 4: forced with that many quartets | 9 off) */
TCE_API int tce_attention_set_tuning(int waves_per_workgroup, int workgroups, int heads_per_workgroup);
TCE_API int tce_w8a8_set_tuning(int quartets_per_tile, int big_tiles, int deep_pipeline);
/* mode 2: every wave writes {start, x staged, math done, end} (100 MHz wall clock, 4 x u64 per wave) to this device buffer.  The pointer is kept PER PROCESS (the
 * calling thread's kernels are pointed at it at once; modes 0..4, 7702 and 7704 set by any thread later hand on the pointer the last caller left). */
TCE_API int tce_w4a16_set_debug_buffer(void *device_buffer);
/* Force an MFMA GEMM tile (m_tiles x n_tiles of 16x16 per wave); 0,0 = automatic. */
TCE_API int tce_w4a16_set_gemm_config(int m_tiles, int n_tiles);
/* Enumerate the compiled kernel variants (for tuning sweeps / tests): returns 0 and fills the outputs, or
 * TCE_ERR_BAD_ARG when idx is past the end. */
TCE_API int tce_w4a16_gemv_variant(int idx, int *rows_per_wave, int *waves_n, int *waves_k, int *depth);
TCE_API int tce_w4a16_gemm_variant(int idx, int *m_tiles, int *n_tiles);

#ifdef __cplusplus
}
#endif
#endif /* TCE_TUNING_H */
