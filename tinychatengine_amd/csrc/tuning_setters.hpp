// tuning_setters.hpp -- the per-thread tuning setters of the kernel units, one prototype each.  Plain C++ (no HIP include): w4a16_kernels.hpp includes it for the
// translation units, tuning_modes.hpp for the table of tce_w4a16_set_debug_mode, tests/host/test_tuning_modes.cc defines recording stand-ins with these names.
#pragma once

namespace tce {

// w4a16_gemv.hip
void set_gemv_debug_mode(int mode);
void set_gemv_order(int force);
void set_gemv_debug_buffer(void *p);
// w4a16_gemv_stream.hip, w4a16_gemv_ovl.hip
void set_gemv_stream_config(int rows, int nw, int depth);
void set_gemv_stream_debug(int mode, void *buf);
void set_gemv_ovl_config(int depth, int chains);
void set_gemv_ovl_stamps(void *buf);
// w4a16_gemv_i8.hip, w4a16_gemv_i8_token.hip
void set_gemv_i8_mode(int mode, int rows);  // mode 0 automatic (taken wherever a packed copy comes with the descriptors), 1 off; rows 0 the rule, 1 / 2 tiles per wave
void set_gemv_i8_mixed_waves(int w);  // tuning: 0 the rule
void set_gemv_i8_stamps(void *buf);  // non-null (lab build): the plain decode launches record [workgroup][8] clock readings there (csrc/w4a16_gemv_i8.hip I8Stamps; scripts/decode_head_timeline.py)
void set_i8_token_stamps(void *buf);  // non-null: plans built from now on record [workgroup][stage][8] wall-clock stamps there (scripts/token_timeline.py)
void set_i8_token_max_units(int u);   // a stage with more units (16-row tile x 1024-k chunk) per workgroup ends the prefix the kernel takes (default 512)
void set_i8_token_mode(int mode);     // 0: tagged plans take this kernel where the list allows (default), 1: never (round 2's token kernel on the fp16 body)
// w4a16_gemm.hip, w4a16_gemm_dma.hip
void set_gemm_xcd_rows(int xm);      // tuning: XCD grid of xm x (8 / xm) over (row blocks x column blocks)
void set_gemm_dma_xcd_rows(int xm);
void set_gemm_dma_mode(int mode);    // timing experiments, see w4a16_gemm_dma.hip
// w4a16_gemm_pk.hip
void set_gemm_pk256_auto(int on);    // 0: the dispatcher never picks the 256-row forms by itself
void set_gemm_pk_wide_auto(int on);  // 1: the dispatcher may pick the wide forms (128 rows x 64 columns per wave)
void set_gemm_pk_form16_auto(int on);
void set_gemm_pk_handoff_delta(int d);
void set_gemm_pk_prio(int on);
void set_gemm_pk_handoff(int on);    // 0: a two-run k cut exchanges through the last arriver (A/B), 1: run 0 hands its tile to run 1
void set_gemm_pk_split(int s);
void set_gemm_pk_mode(int ks, int xm);  // tuning: forced wave quartets per tile / XCD rows (0 = automatic)
void set_gemm_pk_ablation(int abl);  // timing experiments (results meaningless): see w4a16_gemm_pk_kernel
// w4a16_skinny.hip
void set_skinny_config(int ks);  // tuning: waves per 16-row tile, 0 = automatic
void set_skinny_max_m(int m);    // largest M the small-batch kernel takes (16-row slices of the batch on gridDim.y)
// w8a8_gemm.hip, w8a8_lnq_fused.hip
void set_w8a8_ksplit(int ks);       // wave quartets per tile (0 = automatic)
void set_w8a8_deep(int d);          // W8A8 64 x 64 tile with 8 k-steps in flight: 0 the rule, 1 / 2 / 4 quartets forced, 9 off
void set_w8a8_rows32(int r);        // W8A8 32 x 64 tiles (round 6): 0 the rule, 1 forced, 2 off
void set_w8a8_kslice(int code);     // W8A8, the whole tile in every wave (round 6): 0 the rule, 1 off, else a forced form (w8a8_gemm.hip)
void set_w8a8_big(int b);           // W8A8 128-row tiles: 0 the rule, 1 / 2 forced (128 / 64 columns), 9 off
void set_w8a8_xsplit(int xs);       // W8A8, a tile's k-steps cut across workgroups: 0 the rule, 1 off, 2 .. 8 that many runs
void set_lnq_stamps(void *p);
void set_lnq_form(int f);           // 1: the workgroup-per-8-rows form of the LayerNormQ + W8A8 launch at every k
// attention_fast.hip, attention_prefill.hip
void set_attention_fast_target(int wgs);
void set_attention_fast_waves(int nw);
void set_attention_fast_fuse(int r);
void set_attention_fast_probe_no_combine(int on);  // timing experiment: partial states stored, no combine, `out` not written
void set_attention_prefill_waves(int w);  // 0 automatic, 4 / 8 forced

}  // namespace tce
