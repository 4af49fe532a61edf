"""Gate/up adapters and speculative-row pools without a GPU (tinychatengine_amd/lora.py, csrc/lora.hip: tce_lora_expand_silu_mul_f16).

* the SEGMENTED sums the gate/up kernel computes (gate's over gate's R rows of t and Bg, up's over up's) give, bit for bit, the g and u of the existing expand on the
  block-structured B' [2R][2N] (gate's rows in the even columns, up's in the odd, zeros elsewhere): lora_cases.emulate_fp32 in both of its orders, exact and bounded
  cases, every word pattern.  The steps the segmented form leaves out are acc + t * 0 on an accumulator that started at +0 and therefore is never -0;
* exact cases: SiLU * mul of those g and u is lora_gate_up_reference, bit for bit;
* LoraPool(gate_up=True): shapes, packing (stacked A, Bg / Bu without a zero block), a missing projection is zeros, unload, the workspace;
* LoraPool(rows_per_seq=T): batch * T words, set_slot writes T of them; every refusal of the new opt-ins, and the default pool's refusals unchanged;
* the new entry point's refusals through capi.lib(), TCE_ERR_BAD_ARG before TCE_ERR_UNSUPPORTED_SHAPE, before any HIP call.
"""
import ctypes as C

import numpy as np
import pytest

import lora_cases as lc
import lora_gate_up_cases as gc

torch = pytest.importorskip("torch")


def _deinterleaved(out):
    return np.ascontiguousarray(out[:, 0::2]), np.ascontiguousarray(out[:, 1::2])


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("shape", gc.HOST_SHAPES)
def test_segmented_sums_equal_the_block_structured_expand_bit_for_bit(kind, shape):
    rows, K, N, R, n = shape
    case = gc.gate_up_case(kind, 51, *shape)
    block, gate, up = gc.block_structured(case), gc.segment(case, "gate"), gc.segment(case, "up")
    assert block["B"].shape == (n, 2 * R, 2 * N) and not block["B"][:, :R, 1::2].any() and not block["B"][:, R:, 0::2].any()
    for name, words in gc.words_patterns(rows, n).items():
        for order in ("sequential", "lanes"):
            g_block, u_block = _deinterleaved(lc.emulate_fp32(block, words, order))
            g_seg, u_seg = lc.emulate_fp32(gate, words, order), lc.emulate_fp32(up, words, order)
            assert np.array_equal(g_seg.view(np.uint16), g_block.view(np.uint16)), f"{name} / {order}: gate differs"
            assert np.array_equal(u_seg.view(np.uint16), u_block.view(np.uint16)), f"{name} / {order}: up differs"
        off = ~((words >= 0) & (words < n))
        assert np.array_equal(g_seg[off].view(np.uint16), case["y"][off][:, 0::2].view(np.uint16)) and np.array_equal(u_seg[off].view(np.uint16), case["y"][off][:, 1::2].view(np.uint16))
    g_one = lc.emulate_fp32(gate, gc.words_patterns(rows, n)["one"], "sequential")
    assert np.any(g_one != case["y"][:, 0::2]), "the adapter must change something"


def test_a_sum_from_plus_zero_is_never_minus_zero():
    """What the equality rests on: fp32 acc = +0; acc += t * b.  A product of -0 (t < 0, b = +0: the block-structured form's zero block) added to +0 is +0, and an exact
    cancellation is +0 under round-to-nearest -- so the steps over a zero block leave acc's bits alone."""
    f32 = np.float32
    acc = f32(0.0)
    for t, b in ((f32(-3.0), f32(0.0)), (f32(2.0), f32(-0.0)), (f32(1.5), f32(2.0)), (f32(-1.5), f32(2.0)), (f32(-7.0), f32(0.0))):
        acc = f32(acc + f32(t * b))
        assert not np.signbit(acc) or acc != 0
    assert acc == 0 and not np.signbit(acc)


@pytest.mark.parametrize("shape", gc.HOST_SHAPES)
def test_exact_cases_equal_the_gate_up_reference(shape):
    from oracle.oracle import Oracle
    from tinychatengine_amd.lora import lora_gate_up_reference
    rows, K, N, R, n = shape
    case = gc.gate_up_case("exact", 52, *shape)
    orc = Oracle()
    for name, words in gc.words_patterns(rows, n).items():
        ref = lora_gate_up_reference(case["x"], case["A"], case["Bg"], case["Bu"], case["scale"], words, case["y"], silu_mul=orc.silu_mul_half)
        assert ref.shape == (rows, N) and ref.dtype == np.float16
        g, u = lc.emulate_fp32(gc.segment(case, "gate"), words, "lanes"), lc.emulate_fp32(gc.segment(case, "up"), words, "lanes")
        assert np.array_equal(orc.silu_mul_half(g, u).view(np.uint16), ref.view(np.uint16)), name


def test_the_numpy_restatement_of_silu_mul_follows_the_oracle():
    """every finite binary16 gate against three ups: the numpy restatement differs from the oracle only where numpy's exp and the C library's expf differ in the last
    float bit on a rounding boundary -- by one ulp of the result, in well under 1 element of 1000"""
    from oracle.oracle import Oracle
    from tinychatengine_amd.lora import silu_mul_reference
    bits = np.arange(1 << 16, dtype=np.uint16)
    g = bits.view(np.float16)[np.isfinite(bits.view(np.float16))]
    for uv in (1.0, -0.37, 1234.0):
        u = np.full(g.shape, uv, np.float16)
        got, want = silu_mul_reference(g, u), Oracle().silu_mul_half(g, u)
        same = (got.view(np.uint16) == want.view(np.uint16)) | (np.isnan(got) & np.isnan(want))
        assert (~same).sum() <= g.size // 1000, f"{int((~same).sum())} of {g.size} differ"
        assert np.all(np.abs(got[~same].view(np.int16).astype(np.int32) - want[~same].view(np.int16).astype(np.int32)) <= 1)


# ---- LoraPool(gate_up=True) on host tensors ----
SHAPES = {"hidden": 512, "heads": 4, "kv_heads": 1, "ffn": 1408}
DIMS = {"q_proj": (512, 512), "k_proj": (512, 128), "v_proj": (512, 128), "o_proj": (512, 512), "down_proj": (1408, 512), "gate_proj": (512, 1408), "up_proj": (512, 1408)}


def _peft(rng, r, names):
    return {nm: (rng.normal(0, 1, (r, DIMS[nm][0])).astype(np.float16), rng.normal(0, 1, (DIMS[nm][1], r)).astype(np.float16)) for nm in names}


def test_gate_up_pool_packs_the_fourth_target():
    from tinychatengine_amd.lora import LoraPool, lora_gate_up_reference, pack_adapter, target_shapes
    rng = np.random.default_rng(0)
    pool = LoraPool(SHAPES, layers=2, max_adapters=3, rank=16, device="cpu", gate_up=True)
    assert {t: tuple(pool.A[t].shape) for t in pool.A} == {"qkv": (2, 3, 48, 512), "o": (2, 3, 16, 512), "down": (2, 3, 16, 1408), "gate_up": (2, 3, 32, 512)}
    assert set(pool.B) == {"qkv", "o", "down"} and tuple(pool.Bg.shape) == tuple(pool.Bu.shape) == (2, 3, 16, 1408)
    assert target_shapes(SHAPES, 16, gate_up=True)["gate_up"] == (32, 512, 1408) and "gate_up" not in target_shapes(SHAPES, 16)
    w0 = _peft(rng, 8, ["gate_proj", "up_proj", "q_proj", "down_proj"])  # rank 8 in a pool of 16: zero-padded
    w1 = _peft(rng, 8, ["up_proj"])                                        # gate_proj missing: zeros
    pool.load(1, [w0, w1], alpha=4.0)
    assert float(pool.scale[1]) == 0.5 and pool.loaded == {1: 0.5}
    lv0, lv1 = pool.layer(0), pool.layer(1)
    A, Bg, Bu = lv0.A["gate_up"][1].numpy(), lv0.Bg[1].numpy(), lv0.Bu[1].numpy()
    assert np.array_equal(A[:8], w0["gate_proj"][0]) and np.array_equal(A[16:24], w0["up_proj"][0]) and not A[8:16].any() and not A[24:].any()
    assert np.array_equal(Bg[:8], w0["gate_proj"][1].T) and np.array_equal(Bu[:8], w0["up_proj"][1].T) and not Bg[8:].any() and not Bu[8:].any()
    assert np.array_equal(lv0.A["qkv"][1].numpy()[:8], w0["q_proj"][0]) and lv0.A["down"][1].any(), "the three existing targets are packed as before"
    assert not lv1.A["gate_up"][1][:16].any() and not lv1.Bg[1].any() and lv1.Bu[1].any(), "a missing projection is zeros"
    assert not pool.A["gate_up"][:, 0].any() and not pool.Bg[:, 2].any()
    # the packed arrays serve the definition: against the two projections computed separately
    x, y = rng.normal(0, 1, (2, 512)).astype(np.float16), rng.normal(0, 1, (2, 2816)).astype(np.float16)
    from oracle.oracle import Oracle
    got = lora_gate_up_reference(x, lv0.A["gate_up"].numpy(), lv0.Bg.numpy(), lv0.Bu.numpy(), pool.scale.numpy(), [1, -1], y, silu_mul=Oracle().silu_mul_half)
    sep = lambda nm, c: (c.astype(np.float64) + 0.5 * ((x[:1].astype(np.float64) @ w0[nm][0].astype(np.float64).T) @ w0[nm][1].astype(np.float64).T)).astype(np.float16)
    want0 = Oracle().silu_mul_half(sep("gate_proj", y[:1, 0::2]), sep("up_proj", y[:1, 1::2]))
    want1 = Oracle().silu_mul_half(np.ascontiguousarray(y[1:, 0::2]), np.ascontiguousarray(y[1:, 1::2]))
    assert np.array_equal(got[0].view(np.uint16), want0[0].view(np.uint16)) and np.array_equal(got[1].view(np.uint16), want1[0].view(np.uint16))
    # the workspace, and unload
    ws = lv0.workspace(5)
    assert {k: tuple(v.shape) for k, v in ws.items()} == {"qkv": (5, 48), "o": (5, 16), "down": (5, 16), "gate_up": (5, 32)} and ws["gate_up"].dtype == torch.float32
    ptrs = (pool.A["gate_up"].data_ptr(), pool.Bg.data_ptr(), pool.Bu.data_ptr())
    pool.unload(1)
    assert not pool.A["gate_up"].any() and not pool.Bg.any() and not pool.Bu.any() and not pool.A["qkv"].any() and pool.loaded == {}
    assert ptrs == (pool.A["gate_up"].data_ptr(), pool.Bg.data_ptr(), pool.Bu.data_ptr()), "fixed storage"
    packed = pack_adapter(SHAPES, 16, {}, gate_up=True)
    assert [a.shape for a in packed["gate_up"]] == [(32, 512), (16, 1408), (16, 1408)] and set(pack_adapter(SHAPES, 16, {})) == {"qkv", "o", "down"}


def test_the_default_pool_is_unchanged_and_the_opt_ins_refuse_what_they_must():
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.lora import LoraLayer, LoraPool
    from tinychatengine_amd.speculative import SpeculativeGenerator
    pool = LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu")
    assert pool.gate_up is False and pool.rows_per_seq is None and set(pool.A) == {"qkv", "o", "down"} and pool.Bg is None and pool.Bu is None
    for name in ("gate_proj", "up_proj"):
        with pytest.raises(ValueError, match="gate / up"):
            pool.load(0, [{name: (np.zeros((8, 512), np.float16), np.zeros((1408, 8), np.float16))}], alpha=1.0)
    assert pool.loaded == {} and set(LoraLayer(pool, 0).workspace(2)) == {"qkv", "o", "down"}
    assert pool.bind(4).tolist() == [-1] * 4
    pool.set_slot(2, 1)
    assert pool.row_adapter.tolist() == [-1, -1, 1, -1]
    pool.set_slot(2, None)
    assert pool.row_adapter.tolist() == [-1] * 4
    # a gate_up pool: its own refusals
    gu = LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu", gate_up=True)
    with pytest.raises(ValueError):
        gu.load(0, [{"lm_head": (np.zeros((8, 512), np.float16), np.zeros((4096, 8), np.float16))}], alpha=1.0)
    with pytest.raises(ValueError):  # a wrong shape: B [hidden][r] where [ffn][r] belongs
        gu.load(0, [{"gate_proj": (np.zeros((8, 512), np.float16), np.zeros((512, 8), np.float16))}], alpha=1.0)
    with pytest.raises(ValueError):  # a rank above the pool's
        gu.load(0, [{"up_proj": (np.zeros((16, 512), np.float16), np.zeros((1408, 16), np.float16))}], alpha=1.0)
    with pytest.raises(ValueError):  # two ranks in one adapter
        gu.load(0, [{"up_proj": (np.zeros((8, 512), np.float16), np.zeros((1408, 8), np.float16)), "gate_proj": (np.zeros((4, 512), np.float16), np.zeros((1408, 4), np.float16))}], alpha=1.0)
    assert gu.loaded == {} and not gu.A["gate_up"].any(), "a refused load writes nothing"
    # pools for speculative rows
    for bad in (0, 9, 2.5, -1):
        with pytest.raises(ValueError):
            LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu", rows_per_seq=bad)
    pt = LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu", rows_per_seq=4)
    ra = pt.bind(3)
    assert ra.dtype == torch.int32 and ra.tolist() == [-1] * 12 and pt.bind(3) is ra
    with pytest.raises(ValueError):
        pt.bind(12)
    pt.set_slot(1, 0)
    assert ra.tolist() == [-1] * 4 + [0] * 4 + [-1] * 4
    pt.set_slot(2, 1)
    pt.set_slot(1, None)
    assert ra.tolist() == [-1] * 8 + [1] * 4
    # the decoders: a pool's rows_per_seq must be the step's (refused before the block is touched)
    with pytest.raises(ValueError, match="rows_per_seq"):
        BatchedDecoder(None, 3, rows=12, lora=LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu").layer(0))
    with pytest.raises(ValueError, match="rows_per_seq"):
        BatchedDecoder(None, 3, lora=pt.layer(0))
    with pytest.raises(ValueError, match="rows_per_seq"):
        BatchedDecoder(None, 3, rows=6, lora=pt.layer(0))

    class _Dec:  # (the refusal reads nothing of a decoder but its rows_per_seq, and comes first)
        rows_per_seq = 2

    for refused in (pool, pt):  # not built for rows; built for another T
        with pytest.raises(ValueError, match="speculative"):
            SpeculativeGenerator([_Dec()], None, None, None, max_new=4, lora=refused)
    with pytest.raises(ValueError, match="speculative"):
        SpeculativeGenerator(None, None, None, None, max_new=4, lora=pool)


# ---- the C ABI's refusals: before any HIP call, so they need no GPU ----
def test_the_new_entry_point_refuses_before_any_hip_call():
    from tinychatengine_amd import build as B
    B.build()
    entry_point_refusals()


def entry_point_refusals():
    """every refusal of tce_lora_expand_silu_mul_f16 on the loaded library (tests/test_gpu_lora_gate_up.py runs the table again beside a device)"""
    from tinychatengine_amd import capi
    L = capi.lib()
    p, q = C.c_void_p(0x10000), C.c_void_p(0x10004)  # never dereferenced: 16-byte and 4-byte aligned
    far = C.c_void_p(0x40000000)                      # C, far behind y
    null = C.c_void_p(0)
    BAD, SHAPE = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE

    def call(t=q, Bg=p, Bu=p, scale=q, ra=q, y=p, ldy=128, Cm=far, ldc=64, rows=3, N=64, R=8, n=2):
        return L.tce_lora_expand_silu_mul_f16(t, Bg, Bu, scale, ra, y, ldy, Cm, ldc, rows, N, R, n, null)

    for kw in ({"t": null}, {"Bg": null}, {"Bu": null}, {"scale": null}, {"ra": null}, {"y": null}, {"Cm": null}, {"rows": 0}, {"rows": -1}, {"N": 0}, {"N": -8}, {"R": 0},
               {"n": 0}, {"ldy": 120}, {"ldy": 64}, {"ldc": 56}, {"ldc": 0},
               {"Cm": p}, {"Cm": C.c_void_p(0x10000 + 2 * (2 * 128 + 128) - 16)}, {"y": C.c_void_p(0x40000000 + 2 * (2 * 64 + 64) - 16)}):  # C on y; C's head in y's tail; y's head in C's tail
        assert call(**kw) == BAD, kw
        assert capi.last_error().startswith("tce_lora_expand_silu_mul_f16")
    # touching ranges that do not overlap are accepted as arguments (they fail later, on a shape)
    assert call(Cm=C.c_void_p(0x10000 + 2 * (2 * 128 + 128)), R=4) == SHAPE
    for kw in ({"N": 12, "ldy": 24, "ldc": 16}, {"ldy": 132}, {"ldc": 68}, {"R": 4}, {"R": 12}, {"R": 104}, {"R": 200}, {"n": 65}, {"rows": 65535 * 4 + 1}, {"Bg": q}, {"Bu": q},
               {"y": q}, {"Cm": C.c_void_p(0x40000004)}, {"scale": C.c_void_p(0x10002)}, {"t": C.c_void_p(0x10001)}, {"ra": C.c_void_p(0x10002)}):
        assert call(**kw) == SHAPE, kw
        assert capi.last_error().startswith("tce_lora_expand_silu_mul_f16")
    # an argument refusal comes before a shape refusal
    assert call(Cm=null, N=12, R=200) == BAD and call(n=0, R=12) == BAD and call(scale=null, Bg=q) == BAD and call(Cm=p, R=4) == BAD
    assert "tce_lora_expand_silu_mul_f16" in capi.EXPORTS
