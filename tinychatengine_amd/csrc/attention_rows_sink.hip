// attention_rows_sink.hip -- the multi-row paged step with attention sinks (speculative decoding on a StreamingLLM-style layer: window + sinks):
// attn_decode_fast_kernel<.., ROWS, WINDOW, SINK> with all three set, on fp16 and e4m3 pools, and its launcher.
//
// A unit of its own because attention_fast.o is held to the kernels it had (tests/test_attn_forms_isa.py): the device text is attention_fast_kernel.hpp, shared with
// attention_fast.hip, and the two instantiations below are this object's only kernels.  What the form is stands at the kernel ("ROWS && WINDOW && SINK"); what it
// promises in include/tce_matmul.h ("ATTENTION SINKS", rows): row (b, t) bit-identical to t + 1 successive one-row sink steps.
//
// The cut is the one-row sink step's (attention_sink_cut_keys: pos_bound, window and sinks decide it, the same for every row), the grid the windowed rows step's
// (padded (key / value head, chunk slot) pairs x rep, rows, batch), the workspace the multi-row step's (one slice per virtual row).
#include "attention_fast_kernel.hpp"

namespace tce {

// the C ABI has refused everything it names (tce_capi.hip: paged_step); what is tested again here is what an address or the grid is formed from
int launch_attention_decode_paged_rows_sink(const KvPages &pg, const AttnStepArgs &s, int rows, hipStream_t stream, hipError_t *hip_err) {
    const int batch = s.batch, heads = s.heads, kv_heads = s.kv_heads, hd = s.hd, pos_bound = s.pos_bound, table_stride = pg.table_stride;
    const int shift = page_shift_of(pg.page_keys);
    if (hd != kHD || kv_heads <= 0 || heads % kv_heads != 0 || batch <= 0 || batch > 65535 || !s.pos_device || !pg.table || shift < 0 || table_stride < 1 ||
        (long long)pos_bound >= ((long long)table_stride << shift))
        return TCE_ERR_UNSUPPORTED_SHAPE;
    if (pg.fp8 && !(fp8_log2_ok(pg.k_scale_log2) && fp8_log2_ok(pg.v_scale_log2))) return TCE_ERR_UNSUPPORTED_SHAPE;
    // window >= rows: no in-call key is a sink key and every in-call key lies inside its row's window -- what the kernel's one shift per row rests on
    if (rows < 1 || rows > TCE_SPEC_MAX_ROWS || s.sinks < 1 || s.sinks > 16 || s.window < rows) return TCE_ERR_UNSUPPORTED_SHAPE;
    PagedRowsSinkAttnArgs a{};
    a.qkv = static_cast<const half_t *>(s.qkv);
    a.kc = static_cast<half_t *>(pg.k_pool);
    a.vc = static_cast<half_t *>(pg.v_pool);
    a.cosv = static_cast<const half_t *>(s.cosv);
    a.sinv = static_cast<const half_t *>(s.sinv);
    a.out = static_cast<half_t *>(s.out);
    const size_t cnt_bytes = ((size_t)heads * 4 + 255) & ~(size_t)255;
    a.cnt = static_cast<unsigned *>(s.workspace);
    a.part = reinterpret_cast<float *>(static_cast<unsigned char *>(s.workspace) + cnt_bytes);
    a.heads = heads;
    a.kv_heads = kv_heads;
    a.rep = heads / kv_heads;
    a.hd = hd;
    a.max_keys = table_stride << shift;  // (the workspace slices' size; no cache address is formed from it)
    a.pos = pos_bound;
    a.keys = pos_bound + 1;
    a.pos_dev = s.pos_device;
    a.table = pg.table;
    a.table_stride = table_stride;
    a.page_shift = shift;
    int nw = 4;
    describe_attention_decode_sink(heads, kv_heads, pos_bound, s.window, s.sinks, &a.chunk, &a.chunks, &nw);
    if (a.chunks > 1024 || nw != 4) return TCE_ERR_UNSUPPORTED_SHAPE;
    half_t ah;
    __builtin_memcpy(&ah, &s.alpha_bits, 2);
    a.alpha = (float)ah;
    if (pg.fp8) {
        a.k_scale = host_pow2(pg.k_scale_log2);
        a.v_scale = host_pow2(pg.v_scale_log2);
        a.k_inv = host_pow2(-pg.k_scale_log2);
        a.v_inv = host_pow2(-pg.v_scale_log2);
    }
    a.rows_per_seq = rows;
    a.window = s.window;
    a.sinks = s.sinks;
    a.sink_row = (long long)s.sinks + s.window - 1 < (long long)pos_bound ? s.sinks + s.window - 1 : pos_bound;
    const dim3 grid((kv_heads * a.chunks + 7) / 8 * 8 * a.rep, rows, batch);
    if (pg.fp8) hipLaunchKernelGGL((attn_decode_fast_kernel<false, 4, 1, true, true, true, true, true, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((attn_decode_fast_kernel<false, 4, 1, true, true, false, true, true, true>), grid, dim3(256), 0, stream, a);
    return launch_status(hip_err);
}

}  // namespace tce
