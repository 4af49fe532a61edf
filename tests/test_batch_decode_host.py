"""CPU (no GPU): the batched attention step's C ABI -- exports, workspace size, the cut it describes, and argument validation before any HIP call."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


NAMES = ("tce_attention_decode_batch_workspace_bytes", "tce_attention_decode_describe_batch", "tce_attention_decode_step_batch_f16")


def test_batch_symbols_are_exported(capi):
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTS
        assert hasattr(L, n)


def test_batch_workspace_is_batch_single_workspaces(capi):
    L = capi.lib()
    for heads, max_keys in ((32, 512), (32, 4096), (8, 100), (4, 64)):
        one = int(L.tce_attention_decode_workspace_bytes(heads, max_keys, 128))
        assert one > 0
        for b in (1, 3, 8, 16):
            assert int(L.tce_attention_decode_batch_workspace_bytes(b, heads, max_keys, 128)) == b * one
    assert int(L.tce_attention_decode_batch_workspace_bytes(4, 32, 512, 64)) == 0
    assert int(L.tce_attention_decode_batch_workspace_bytes(0, 32, 512, 128)) == 0
    assert int(L.tce_attention_decode_batch_workspace_bytes(-2, 32, 512, 128)) == 0


@pytest.mark.parametrize("heads,kv_heads", [(32, 8), (32, 32), (4, 1)])
@pytest.mark.parametrize("pos_bound", [0, 319, 320, 1023, 4095])
def test_batch_describe_is_the_single_cut_times_batch(capi, heads, kv_heads, pos_bound):
    for b in (1, 3, 16):
        got = capi.describe_attention_batch(b, heads, kv_heads, pos_bound)
        one = capi.describe_attention_step(heads, pos_bound + 1, kv_heads)
        for k in ("chunks", "keys-per-chunk", "waves", "combine"):
            assert got[k] == one[k], (k, got, one)
        assert got["workgroups"] == b * one["workgroups"]
        assert got["batch"] == b
        assert got["waves"] == 4


def test_batch_describe_ignores_the_threads_attention_tuning(capi):
    """The batched entry runs the fitted rule only: a forced workgroup target or wave count on the calling thread changes the single step's cut, not this one."""
    L = capi.lib()
    base = capi.describe_attention_batch(2, 32, 8, 2047)
    try:
        assert L.tce_w4a16_set_debug_mode(3000 + 1024) == 0
        assert capi.describe_attention_step(32, 2048, 8)["chunks"] != base["chunks"]  # the setting acts on the single step
        assert capi.describe_attention_batch(2, 32, 8, 2047) == base
        assert L.tce_w4a16_set_debug_mode(2908) == 0
        assert capi.describe_attention_batch(2, 32, 8, 2047) == base
    finally:
        L.tce_w4a16_set_debug_mode(3000)
        L.tce_w4a16_set_debug_mode(2900)
        L.tce_w4a16_set_debug_mode(0)


def test_batch_describe_validates(capi):
    L = capi.lib()
    buf = C.create_string_buffer(160)
    for args in ((0, 32, 8, 10), (2, 32, 5, 10), (2, 0, 1, 10), (2, 32, 8, -1)):
        assert L.tce_attention_decode_describe_batch(*args, buf, 160) == capi.TCE_ERR_BAD_ARG, args
    assert L.tce_attention_decode_describe_batch(2, 32, 8, 10, None, 160) == capi.TCE_ERR_BAD_ARG


def test_batch_step_argument_validation_needs_no_gpu(capi):
    """Every refusal happens before a HIP call: host buffers stand in for the device pointers and are never dereferenced."""
    L = capi.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    vp = C.c_void_p

    def step(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return L.tce_attention_decode_step_batch_f16(vp(g("qkv", p)), vp(g("kc", p)), vp(g("vc", p)), vp(g("cos", None)), vp(g("sin", None)), vp(g("out", p)),
                                                     vp(g("ws", p)), g("batch", 2), g("heads", 4), g("kv", 2), g("hd", 128), g("mk", 64), vp(g("pos", p)),
                                                     g("bound", 10), 0x2DA8, None)

    for name in ("qkv", "kc", "vc", "out", "ws", "pos"):
        assert step(**{name: None}) == capi.TCE_ERR_BAD_ARG, name
    assert "null pointer" in capi.last_error()
    assert step(batch=0) == capi.TCE_ERR_BAD_ARG
    assert step(batch=-1) == capi.TCE_ERR_BAD_ARG
    assert step(kv=3) == capi.TCE_ERR_BAD_ARG and "do not divide" in capi.last_error()
    assert step(bound=-1) == capi.TCE_ERR_BAD_ARG
    assert step(bound=64) == capi.TCE_ERR_BAD_ARG          # pos_bound == max_keys
    assert step(cos=p) == capi.TCE_ERR_BAD_ARG             # cos without sin
    assert step(sin=p) == capi.TCE_ERR_BAD_ARG             # sin without cos
    assert step(hd=64) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert step(batch=65536) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "65535" in capi.last_error()
    for name in ("qkv", "kc", "vc"):
        assert step(**{name: p + 8}) == capi.TCE_ERR_UNSUPPORTED_SHAPE, name
    assert step(cos=p + 2, sin=p) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert step(cos=p, sin=p + 4) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    # the single step returns the same codes for the same faults
    single = lambda **kw: L.tce_attention_decode_step_pos_f16(vp(kw.get("qkv", p)), vp(p), vp(p), None, None, None, vp(p), vp(p), 4, kw.get("kv", 2), kw.get("hd", 128), 64,
                                                              vp(p), kw.get("bound", 10), 0x2DA8, None)
    assert single(kv=3) == step(kv=3) and single(hd=64) == step(hd=64) and single(bound=64) == step(bound=64) and single(qkv=p + 8) == step(qkv=p + 8)
