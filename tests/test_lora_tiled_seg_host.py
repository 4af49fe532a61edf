"""The segmented tiled expands without a GPU: every refusal of tce_lora_expand_silu_mul_tiled_f16 / tce_lora_expand_add_segmented_tiled_f16 happens before any HIP call,
every argument refusal before the first shape refusal; LoraPool(segmented=) validation and the workspace shapes with and without the flag."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def L():
    from tinychatengine_amd import build as B
    from tinychatengine_amd import capi
    B.build()
    return capi.lib()


def test_segmented_entry_points_refuse_before_any_hip_call(L):
    from tinychatengine_amd import capi
    p, q, far, null = C.c_void_p(0x10000), C.c_void_p(0x10004), C.c_void_p(0x40000000), C.c_void_p(0)  # never dereferenced: 16-byte and 4-byte aligned
    BAD, SHAPE = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE

    def silu(part=q, Bg=p, Bu=p, scale=q, ra=q, y=p, ldy=128, Cm=far, ldc=64, rows=3, N=64, K=64, R=8, n=2):
        return L.tce_lora_expand_silu_mul_tiled_f16(part, Bg, Bu, scale, ra, y, ldy, Cm, ldc, rows, N, K, R, n, null)

    def seg(part=q, Bm=p, scale=q, ra=q, Cm=p, ldc=384, rows=3, N=384, K=64, R=24, n=2, cols=(0, 128, 256, 384), segments=None):
        arr = None if cols is None else (C.c_int * len(cols))(*cols)
        return L.tce_lora_expand_add_segmented_tiled_f16(part, Bm, scale, ra, Cm, ldc, rows, N, K, R, n, arr, len(cols or ()) - 1 if segments is None else segments, null)

    for kw in ({"part": null}, {"Bg": null}, {"Bu": null}, {"scale": null}, {"ra": null}, {"y": null}, {"Cm": null}, {"rows": 0}, {"N": 0}, {"K": 0}, {"K": -8}, {"R": 0}, {"n": 0},
               {"ldy": 120}, {"ldc": 56}, {"Cm": p}, {"Cm": C.c_void_p(0x10000 + 2 * 128 * 2 + 64)}):  # (the last two: C overlaps y)
        assert silu(**kw) == BAD and capi.last_error().startswith("tce_lora_expand_silu_mul_tiled_f16"), kw
    for kw in ({"N": 12, "ldy": 24, "ldc": 16}, {"ldy": 132}, {"ldc": 68}, {"K": 12}, {"R": 4}, {"R": 104}, {"n": 65}, {"rows": 65535 * 4 + 1}, {"Bg": q}, {"Bu": q},
               {"y": C.c_void_p(0x10008)}, {"Cm": C.c_void_p(0x40000008)}, {"scale": C.c_void_p(0x10002)}, {"part": C.c_void_p(0x10001)}, {"ra": C.c_void_p(0x10002)}):
        assert silu(**kw) == SHAPE, kw
    assert silu(Cm=null, N=12, R=200) == BAD and silu(K=0, R=12) == BAD and silu(Cm=p, K=12) == BAD
    for kw in ({"cols": None, "segments": 3}, {"segments": 0}, {"segments": 5, "cols": (0, 64, 128, 192, 256, 384)}, {"cols": (128, 256, 384)}, {"cols": (0, 128, 256)},
               {"cols": (0, 256, 128, 384)}, {"cols": (0, 128, 128, 384)}, {"part": null}, {"Bm": null}, {"Cm": null}, {"K": 0}, {"rows": 0}, {"ldc": 376}):
        assert seg(**kw) == BAD and capi.last_error().startswith("tce_lora_expand_add_segmented_tiled_f16"), kw
    for kw in ({"K": 12}, {"R": 200}, {"n": 65}, {"Bm": q}, {"R": 16}, {"R": 32}, {"cols": (0, 64, 256, 384)}, {"cols": (0, 128, 200, 384)}, {"cols": (0, 192, 384), "R": 16}):
        assert seg(**kw) == SHAPE, kw
    assert seg(cols=(0, 64, 384), Bm=null) == BAD and seg(cols=(0, 256, 128, 384), R=16, K=12) == BAD and seg(R=16, K=0) == BAD


def test_pool_validates_segmented_and_only_the_flag_changes_the_workspace(L):
    from tinychatengine_amd.lora import LoraPool
    shapes, kw = {"hidden": 512, "heads": 4, "kv_heads": 1, "ffn": 1408}, {"layers": 1, "max_adapters": 2, "rank": 8, "device": "cpu", "gate_up": True}
    with pytest.raises(ValueError, match="segmented"):
        LoraPool(shapes, **kw, segmented=True)
    S = L.tce_lora_tiled_slices(512)
    tiled, seg = LoraPool(shapes, **kw, tiled_from=16).layer(0), LoraPool(shapes, **kw, tiled_from=16, segmented=True).layer(0)
    assert seg.pool.qkv_seg_cols == (0, 512, 640, 768)
    for rows in (15, 16, 600):
        a, b = ({t: tuple(v.shape) for t, v in lv.workspace(rows).items()} for lv in (tiled, seg))
        assert a["gate_up"] == (rows, 16) and b["gate_up"] == ((rows, 16) if rows < 16 else (S, rows, 16)) and {**b, "gate_up": a["gate_up"]} == a
        assert seg.tiled("gate_up", rows) == (rows >= 16) and not tiled.tiled("gate_up", rows)
    assert not LoraPool(shapes, **dict(kw, gate_up=False), tiled_from=16, segmented=True).layer(0).tiled("gate_up", 600)
