"""The two ways to run the attention step and o_proj behind it (a helper for tests/test_gpu_deferred_attention.py and tests/test_gpu_attention_adversarial.py; no tests
here): plain -- tce_attention_decode_step_pos_f16 + tce_w4a16_forward --, and deferred -- tce_attention_decode_step_deferred_f16 + tce_w4a16_forward_deferred_attention,
o_proj combining the chunks' partial states in its prologue.  Both return o_proj's input row and its output (the residual added)."""
import ctypes as C

import torch


def plain(att, o, qkv, res, pos, pos_t=None):
    from tinychatengine_amd import capi
    x = torch.full((1, o.in_features), float("nan"), dtype=torch.float16, device=qkv.device)
    y = res.clone()
    att.step(qkv, pos, out=x.view(att.heads, 128), pos_device=pos_t)
    capi.check(capi.w4a16_forward(o.desc(x, y, flags=capi.TCE_W4_ADD_TO_C), torch.cuda.current_stream().cuda_stream))
    return x, y


def deferred(att, o, qkv, res, pos, pos_t=None):
    from tinychatengine_amd import capi
    x = torch.full((1, o.in_features), float("nan"), dtype=torch.float16, device=qkv.device)
    y = res.clone()
    att.step(qkv, pos, out=x.view(att.heads, 128), pos_device=pos_t, defer=True)
    capi.check(capi.lib().tce_w4a16_forward_deferred_attention(C.byref(o.desc(x, y, flags=capi.TCE_W4_ADD_TO_C)), C.byref(att.deferred),
                                                               C.c_void_p(pos_t.data_ptr() if pos_t is not None else 0), int(pos), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return x, y, att.deferred.slots
