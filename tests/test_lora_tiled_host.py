"""The tiled form of the adapted linear without a GPU: every refusal of tce_lora_shrink_tiled_f16 / tce_lora_expand_add_tiled_f16 happens before any HIP call, in the
4-row pair's order (arguments before shapes); the K slices and the workspace size; LoraPool(tiled_from=) validation, and the default's workspace shapes."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

SHAPES = {"hidden": 512, "heads": 4, "kv_heads": 1, "ffn": 1408}


@pytest.fixture(scope="module")
def L():
    from tinychatengine_amd import build as B
    from tinychatengine_amd import capi
    B.build()
    return capi.lib()


def test_tiled_entry_points_refuse_before_any_hip_call(L):
    from tinychatengine_amd import capi
    p, q, null = C.c_void_p(0x10000), C.c_void_p(0x10004), C.c_void_p(0)  # never dereferenced: 16-byte and 4-byte aligned
    BAD, SHAPE = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE

    def shrink(x=p, ldx=64, A=p, ra=q, part=q, rows=3, K=64, R=8, n=2):
        return L.tce_lora_shrink_tiled_f16(x, ldx, A, ra, part, rows, K, R, n, null)

    def expand(part=q, Bm=p, scale=q, ra=q, Cm=p, ldc=64, rows=3, N=64, K=64, R=8, n=2):
        return L.tce_lora_expand_add_tiled_f16(part, Bm, scale, ra, Cm, ldc, rows, N, K, R, n, null)

    for kw in ({"x": null}, {"A": null}, {"ra": null}, {"part": null}, {"rows": 0}, {"K": 0}, {"K": -8}, {"R": 0}, {"n": 0}, {"rows": -1}, {"ldx": 56}, {"ldx": 0}):
        assert shrink(**kw) == BAD, kw
        assert capi.last_error().startswith("tce_lora_shrink_tiled_f16")
    for kw in ({"K": 12, "ldx": 16}, {"ldx": 68}, {"R": 4}, {"R": 12}, {"R": 200}, {"n": 65}, {"rows": 65535 * 4 + 1}, {"x": q}, {"A": q}, {"part": C.c_void_p(0x10002)},
               {"ra": C.c_void_p(0x10001)}):
        assert shrink(**kw) == SHAPE, kw
    for kw in ({"part": null}, {"Bm": null}, {"scale": null}, {"ra": null}, {"Cm": null}, {"rows": 0}, {"N": 0}, {"K": 0}, {"R": 0}, {"n": 0}, {"ldc": 56}, {"N": -8}):
        assert expand(**kw) == BAD, kw
        assert capi.last_error().startswith("tce_lora_expand_add_tiled_f16")
    for kw in ({"N": 12, "ldc": 16}, {"ldc": 68}, {"K": 12}, {"R": 4}, {"R": 200}, {"n": 65}, {"rows": 65535 * 4 + 1}, {"Bm": q}, {"Cm": q}, {"scale": C.c_void_p(0x10002)},
               {"part": C.c_void_p(0x10001)}, {"ra": C.c_void_p(0x10002)}):
        assert expand(**kw) == SHAPE, kw
    assert shrink(x=null, K=12, R=200) == BAD and shrink(rows=0, R=4, n=65) == BAD and shrink(A=null, x=q) == BAD
    assert expand(Cm=null, N=12, R=200) == BAD and expand(n=0, R=12) == BAD and expand(scale=null, Bm=q) == BAD and expand(K=0, N=12) == BAD


def test_slices_and_workspace_are_functions_of_the_shape_alone(L):
    from tinychatengine_amd import capi
    assert [L.tce_lora_tiled_slices(K) for K in (8, 1024, 1032, 14336, 16384, 16392, 1 << 20)] == [1, 1, 2, 14, 16, 15, 16]  # (16392: runs of 1152)
    assert L.tce_lora_tiled_slices(0) == 0 and L.tce_lora_tiled_slices(-8) == 0 and capi.TCE_LORA_TILED_MAX_SLICES == 16 and capi.TCE_LORA_TILE_ROWS == 32
    assert L.tce_lora_tiled_workspace_bytes(130, 2056, 48) == 3 * 130 * 48 * 4 and L.tce_lora_tiled_workspace_bytes(1, 8, 8) == 32
    assert L.tce_lora_tiled_workspace_bytes(262140, 14336, 192) == 14 * 262140 * 192 * 4  # (more than 2^31 bytes)
    assert [L.tce_lora_tiled_workspace_bytes(*a) for a in ((0, 8, 8), (1, 0, 8), (1, 8, 0))] == [0, 0, 0]


def test_pool_validates_tiled_from_and_the_default_keeps_its_workspace(L):
    from tinychatengine_amd.lora import LoraPool
    kw = {"layers": 1, "max_adapters": 2, "rank": 8, "device": "cpu"}
    for bad in (0, -1, 1.5, "16", True):
        with pytest.raises(ValueError, match="tiled_from"):
            LoraPool(SHAPES, **kw, tiled_from=bad)
    default, tiled = LoraPool(SHAPES, **kw).layer(0), LoraPool(SHAPES, **kw, tiled_from=16).layer(0)
    plain = {"qkv": (24, 512), "o": (8, 512), "down": (8, 1408)}  # target: (R, K)
    for rows in (1, 15, 16, 600):
        assert {t: tuple(v.shape) for t, v in default.workspace(rows).items()} == {t: (rows, R) for t, (R, K) in plain.items()}
        want = {t: (rows, R) if rows < 16 else (L.tce_lora_tiled_slices(K), rows, R) for t, (R, K) in plain.items()}
        assert {t: tuple(v.shape) for t, v in tiled.workspace(rows).items()} == want
    ws = LoraPool(SHAPES, **kw, gate_up=True, rows_per_seq=4, tiled_from=1).layer(0).workspace(8)  # a pool for rows takes it too; gate_up keeps the 4-row shrink's t
    assert tuple(ws["gate_up"].shape) == (8, 16) and tuple(ws["down"].shape) == (2, 8, 8)
