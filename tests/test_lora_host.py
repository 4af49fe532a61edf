"""Multi-LoRA without a GPU: the designed cases of tests/lora_cases.py are what they claim, LoraPool packs what lora.py documents, and every refusal happens before a
device is touched.

* `exact` cases: an fp32 numpy emulation of the two kernels in two different summation orders equals lora_reference (float64, one rounding) BIT FOR BIT -- the cases'
  claim that no fp32 partial result rounds, in any order;
* `bounded` cases: the same emulations stay inside lora_cases.bound -- a correct fp32 implementation in either order meets the bound the GPU test enforces;
* LoraPool: q/k/v packed into the fused form against three separate references, zero padding of a smaller rank, unload;
* the C ABI's refusals through capi.lib(), TCE_ERR_BAD_ARG before TCE_ERR_UNSUPPORTED_SHAPE;
* the ValueErrors of the Python surface that need no device.
"""
import ctypes as C

import numpy as np
import pytest

import lora_cases as lc

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("shape", lc.HOST_SHAPES)
def test_exact_cases_are_exact_in_fp32_in_any_order(shape):
    case = lc.exact_case(11, *shape)
    for name, words in lc.patterns(shape[0], shape[4]).items():
        ref = lc.reference(case, words)
        for order in ("sequential", "lanes"):
            got = lc.emulate_fp32(case, words, order)
            assert np.array_equal(got.view(np.uint16), ref.view(np.uint16)), f"{name} / {order}: an fp32 partial result rounded"
        untouched = ~((words >= 0) & (words < shape[4]))
        assert np.array_equal(ref[untouched].view(np.uint16), case["C"][untouched].view(np.uint16))
    assert np.any(lc.reference(case, lc.patterns(shape[0], shape[4])["one"]) != case["C"]), "the adapter must change something"


@pytest.mark.parametrize("shape", lc.HOST_SHAPES)
def test_bounded_cases_hold_their_bound_under_fp32_emulation(shape):
    case = lc.bounded_case(12, *shape)
    rows, n = shape[0], shape[4]
    assert np.abs(case["x"][rows - 1].astype(np.float64)).max() > 2.0 ** 13 or shape[1] < 64, "the outlier row"
    for name, words in lc.patterns(rows, n).items():
        ref64, b = lc.reference64(case, words), lc.bound(case, words)
        assert np.abs(ref64).max() < 60000, "the reference must stay a finite binary16 number"
        for order in ("sequential", "lanes"):
            err = np.abs(lc.emulate_fp32(case, words, order).astype(np.float64) - ref64)
            assert np.all(err <= b), f"{name} / {order}: worst ratio {float((err / np.maximum(b, 1e-300)).max())}"
    if rows >= 4:  # a cancellation row under the pattern it was designed for: the result is far below both terms
        words = lc.patterns(rows, n)["different"]
        assert np.abs(lc.reference64(case, words)[0]).max() < 2.0 ** -6 * np.abs(lc.delta64(case, words)[0]).max()


def test_lora_reference_leaves_rows_without_an_adapter_alone():
    case = lc.bounded_case(3, 6, 16, 8, 8, 2)
    case["C"].view(np.uint16)[1] = [0x8000, 0x7E01, 0xFDFF, 0x7C00, 0x0001, 0x8001, 0xFC00, 0x7FFF]  # -0.0, NaN payloads, infinities, subnormals
    words = np.array([0, -1, 2, -7, lc.INT32_MAX, 1])
    ref = lc.reference(case, words)
    for i in (1, 2, 3, 4):
        assert np.array_equal(ref[i].view(np.uint16), case["C"][i].view(np.uint16))
    for i in (0, 5):
        assert not np.array_equal(ref[i].view(np.uint16), case["C"][i].view(np.uint16))


# ---- LoraPool on host tensors ----
SHAPES = {"hidden": 512, "heads": 4, "kv_heads": 1, "ffn": 1408}


def _peft(rng, r, names, shapes=SHAPES):
    dims = {"q_proj": (shapes["hidden"], shapes["heads"] * 128), "k_proj": (shapes["hidden"], shapes["kv_heads"] * 128), "v_proj": (shapes["hidden"], shapes["kv_heads"] * 128),
            "o_proj": (shapes["heads"] * 128, shapes["hidden"]), "down_proj": (shapes["ffn"], shapes["hidden"])}
    return {nm: (rng.normal(0, 1, (r, dims[nm][0])).astype(np.float16), rng.normal(0, 1, (dims[nm][1], r)).astype(np.float16)) for nm in names}


def _separate(x, a, b, scale, c):
    """One projection by the definition: fp16(c + scale * (x A^T) B^T) in float64"""
    return (c.astype(np.float64) + scale * ((x.astype(np.float64) @ a.astype(np.float64).T) @ b.astype(np.float64).T)).astype(np.float16)


def test_pool_packs_qkv_into_the_fused_form_and_pads_a_smaller_rank():
    from tinychatengine_amd.lora import LoraPool, lora_reference
    rng = np.random.default_rng(0)
    pool = LoraPool(SHAPES, layers=2, max_adapters=3, rank=16, device="cpu")
    assert {t: tuple(pool.A[t].shape) for t in pool.A} == {"qkv": (2, 3, 48, 512), "o": (2, 3, 16, 512), "down": (2, 3, 16, 1408)}
    assert {t: tuple(pool.B[t].shape) for t in pool.B} == {"qkv": (2, 3, 48, 768), "o": (2, 3, 16, 512), "down": (2, 3, 16, 512)}
    w0 = _peft(rng, 8, ["q_proj", "k_proj", "v_proj", "o_proj", "down_proj"])  # rank 8 in a pool of 16: zero-padded
    w1 = _peft(rng, 8, ["k_proj", "down_proj"])                                # a subset: the rest is zeros
    pool.load(1, [w0, w1], alpha=4.0)
    assert float(pool.scale[1]) == 0.5 and float(pool.scale[0]) == 0.0 and pool.loaded == {1: 0.5}
    x = rng.normal(0, 1, (3, 512)).astype(np.float16)
    c = rng.normal(0, 1, (3, 768)).astype(np.float16)
    words = np.array([1, 1, 1])
    for layer, w in ((0, w0), (1, w1)):
        lv = pool.layer(layer)
        got = lora_reference(x, lv.A["qkv"].numpy(), lv.B["qkv"].numpy(), pool.scale.numpy(), words, c)
        col = 0
        for nm, width in (("q_proj", 512), ("k_proj", 128), ("v_proj", 128)):
            want = _separate(x, *w[nm], 0.5, c[:, col:col + width]) if nm in w else c[:, col:col + width]
            assert np.array_equal(got[:, col:col + width].view(np.uint16), want.view(np.uint16)), f"layer {layer} {nm}"
            col += width
        A, B = lv.A["qkv"][1].numpy(), lv.B["qkv"][1].numpy()
        for p, (nm, c0, width) in enumerate((("q_proj", 0, 512), ("k_proj", 512, 128), ("v_proj", 640, 128))):
            assert not A[p * 16 + 8:(p + 1) * 16].any() and not B[p * 16 + 8:(p + 1) * 16].any(), "rows past the adapter's rank are zero"
            off = np.ones(768, bool)
            off[c0:c0 + width] = False
            assert not B[p * 16:(p + 1) * 16][:, off].any(), "B is zero off its block"
            if nm in w:
                assert np.array_equal(A[p * 16:p * 16 + 8], w[nm][0]) and np.array_equal(B[p * 16:p * 16 + 8, c0:c0 + width], w[nm][1].T)
    xo, co = rng.normal(0, 1, (2, 1408)).astype(np.float16), rng.normal(0, 1, (2, 512)).astype(np.float16)
    lv = pool.layer(1)
    got = lora_reference(xo, lv.A["down"].numpy(), lv.B["down"].numpy(), pool.scale.numpy(), [1, 0], co)
    assert np.array_equal(got[0].view(np.uint16), _separate(xo[:1], *w1["down_proj"], 0.5, co[:1])[0].view(np.uint16))
    assert np.array_equal(got[1].astype(np.float64), co[1].astype(np.float64)), "an adapter that was never loaded adds 0"
    assert not pool.layer(1).A["o"].numpy().any(), "a missing target is zeros"


def test_pool_unload_and_reload():
    from tinychatengine_amd.lora import LoraPool
    rng = np.random.default_rng(1)
    pool = LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu")
    pool.load(0, [_peft(rng, 8, ["q_proj", "o_proj"])], alpha=16.0)
    pool.load(1, {0: _peft(rng, 4, ["down_proj"])}, alpha=1.0)
    assert float(pool.scale[0]) == 2.0 and float(pool.scale[1]) == 0.25
    ptrs = {t: pool.A[t].data_ptr() for t in pool.A}
    keep = pool.A["down"][0, 1].clone()
    pool.unload(0)
    assert all(not pool.A[t][:, 0].any() and not pool.B[t][:, 0].any() for t in pool.A) and float(pool.scale[0]) == 0.0 and pool.loaded == {1: 0.25}
    assert torch.equal(pool.A["down"][0, 1], keep) and keep.any(), "the neighbour stays"
    pool.load(0, [_peft(rng, 8, ["v_proj"])], alpha=8.0)  # a reload leaves nothing of the earlier adapter behind
    assert not pool.A["o"][0, 0].any() and not pool.A["qkv"][0, 0, :16].any() and pool.A["qkv"][0, 0, 16:24].any()
    assert {t: pool.A[t].data_ptr() for t in pool.A} == ptrs, "fixed storage: a captured graph keeps these pointers"
    ra = pool.bind(4)
    assert ra.dtype == torch.int32 and ra.tolist() == [-1] * 4 and pool.bind(4) is ra
    with pytest.raises(ValueError):
        pool.bind(5)


def test_python_surface_refusals():
    from tinychatengine_amd.lora import LoraPool
    from tinychatengine_amd.speculative import SpeculativeGenerator
    rng = np.random.default_rng(2)
    pool = LoraPool(SHAPES, layers=1, max_adapters=2, rank=8, device="cpu")
    for name in ("gate_proj", "up_proj"):
        bad = {name: (np.zeros((8, 512), np.float16), np.zeros((1408, 8), np.float16))}
        with pytest.raises(ValueError, match="gate / up"):
            pool.load(0, [bad], alpha=1.0)
    with pytest.raises(ValueError):
        pool.load(0, [{"lm_head": (np.zeros((8, 512), np.float16), np.zeros((4096, 8), np.float16))}], alpha=1.0)
    with pytest.raises(ValueError):  # a rank above the pool's
        pool.load(0, [_peft(rng, 16, ["q_proj"])], alpha=1.0)
    with pytest.raises(ValueError):  # two ranks in one adapter
        pool.load(0, [{**_peft(rng, 8, ["q_proj"]), **_peft(rng, 4, ["o_proj"])}], alpha=1.0)
    with pytest.raises(ValueError):  # a wrong shape
        pool.load(0, [{"q_proj": (np.zeros((8, 256), np.float16), np.zeros((512, 8), np.float16))}], alpha=1.0)
    with pytest.raises(ValueError):
        pool.load(0, [{}, {}], alpha=1.0)  # a layer the pool does not have
    with pytest.raises(IndexError):
        pool.load(2, [_peft(rng, 8, ["q_proj"])], alpha=1.0)
    assert pool.loaded == {} and not pool.A["qkv"].any(), "a refused load writes nothing"
    for kw in ({"rank": 4}, {"rank": 12}, {"rank": 72}, {"max_adapters": 0}, {"max_adapters": 65}, {"layers": 0}):
        with pytest.raises(ValueError):
            LoraPool(SHAPES, **{"layers": 1, "max_adapters": 2, "rank": 8, "device": "cpu", **kw})
    with pytest.raises(ValueError, match="speculative"):  # before anything else of the constructor runs
        SpeculativeGenerator(None, None, None, None, max_new=4, lora=pool)


# ---- the C ABI's refusals: before any HIP call, so they need no GPU ----
def test_entry_points_refuse_before_any_hip_call():
    from tinychatengine_amd import build as B
    from tinychatengine_amd import capi
    B.build()
    L = capi.lib()
    p, q = C.c_void_p(0x10000), C.c_void_p(0x10004)  # never dereferenced: 16-byte and 4-byte aligned
    null = C.c_void_p(0)
    BAD, SHAPE = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE

    def shrink(x=p, ldx=64, A=p, ra=q, t=q, rows=3, K=64, R=8, n=2):
        return L.tce_lora_shrink_f16(x, ldx, A, ra, t, rows, K, R, n, null)

    def expand(t=q, Bm=p, scale=q, ra=q, Cm=p, ldc=64, rows=3, N=64, R=8, n=2):
        return L.tce_lora_expand_add_f16(t, Bm, scale, ra, Cm, ldc, rows, N, R, n, null)

    for kw in ({"x": null}, {"A": null}, {"ra": null}, {"t": null}, {"rows": 0}, {"K": 0}, {"K": -8}, {"R": 0}, {"n": 0}, {"rows": -1}, {"ldx": 56}, {"ldx": 0}):
        assert shrink(**kw) == BAD, kw
        assert capi.last_error().startswith("tce_lora_shrink_f16")
    for kw in ({"K": 12, "ldx": 16}, {"ldx": 68}, {"R": 4}, {"R": 12}, {"R": 200}, {"n": 65}, {"rows": 65535 * 4 + 1}, {"x": q}, {"A": q}, {"t": C.c_void_p(0x10002)},
               {"ra": C.c_void_p(0x10001)}):
        assert shrink(**kw) == SHAPE, kw
    for kw in ({"t": null}, {"Bm": null}, {"scale": null}, {"ra": null}, {"Cm": null}, {"rows": 0}, {"N": 0}, {"R": 0}, {"n": 0}, {"ldc": 56}, {"N": -8}):
        assert expand(**kw) == BAD, kw
        assert capi.last_error().startswith("tce_lora_expand_add_f16")
    for kw in ({"N": 12, "ldc": 16}, {"ldc": 68}, {"R": 4}, {"R": 200}, {"n": 65}, {"rows": 65535 * 4 + 1}, {"Bm": q}, {"Cm": q}, {"scale": C.c_void_p(0x10002)},
               {"t": C.c_void_p(0x10001)}, {"ra": C.c_void_p(0x10002)}):
        assert expand(**kw) == SHAPE, kw
    # an argument refusal comes before a shape refusal
    assert shrink(x=null, K=12, R=200) == BAD and shrink(rows=0, R=4, n=65) == BAD and shrink(A=null, x=q) == BAD
    assert expand(Cm=null, N=12, R=200) == BAD and expand(n=0, R=12) == BAD and expand(scale=null, Bm=q) == BAD
    assert capi.TCE_LORA_MAX_RANK == 192 and capi.TCE_LORA_MAX_ADAPTERS == 64
