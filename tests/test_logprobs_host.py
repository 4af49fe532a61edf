"""CPU (no GPU): log-probabilities (tinychatengine_amd/generate.py: logprob_reference, perplexity, score_plan; include/tce_matmul.h: tce_logprobs_f16,
tce_sample_logprobs_f16, tce_sample_verify_logprobs_f16).

* logprob_reference on rows computed by hand, its degenerate rows, perplexity;
* the chunked fp32 scheme of csrc/sampling.hip restated in numpy in the kernels' summation order, against float64: the accuracy contract (2^-16 for |x| <= 64) has
  margin for that order;
* every refusal of the three entry points happens before any launch (the calls below carry pointers that are never followed);
* score()'s bookkeeping: slots, reservations, packed tokens and targets, chunks, the split of the values -- and all-or-nothing on a host PageAllocator."""
import ctypes as C
import math

import numpy as np
import pytest

BOUND = 2.0 ** -16


def test_logprob_reference_on_hand_computed_rows():
    from tinychatengine_amd.generate import logprob_reference, perplexity
    f16 = lambda *v: np.array(v, np.float16)
    assert logprob_reference(f16(0.0, 0.0), 0) == pytest.approx(-math.log(2.0), abs=1e-15)
    assert logprob_reference(f16(5.5), 0) == 0.0  # one entry: probability 1
    lse = math.log(math.e + math.e ** 2 + math.e ** 3)
    for t, x in enumerate((1.0, 2.0, 3.0)):
        assert logprob_reference(f16(1.0, 2.0, 3.0), t) == pytest.approx(x - lse, abs=1e-14)
    # four equal entries: log(1/4) whatever the value, large magnitudes included (the maximum is subtracted first)
    for v in (-60000.0, 0.0, 3.25, 60000.0):
        assert logprob_reference(np.full(4, v, np.float16), 2) == pytest.approx(-math.log(4.0), abs=1e-15 + 2 * math.ulp(abs(v)))  # (x_t - lse rounds at |v|)
    # a -inf entry has probability 0 and takes no part in the others' values
    assert logprob_reference(f16(-np.inf, 0.0, 0.0), 1) == pytest.approx(-math.log(2.0), abs=1e-15)
    assert logprob_reference(f16(-np.inf, 0.0, 0.0), 0) == -math.inf
    # "no target", a target outside the row, and the degenerate rows
    assert logprob_reference(f16(1.0, 2.0), -1) == 0.0
    for t in (2, -2, 1 << 30):
        assert math.isnan(logprob_reference(f16(1.0, 2.0), t))
    for row in (f16(1.0, np.nan, 2.0), f16(1.0, np.inf, 2.0), f16(-np.inf, -np.inf)):
        assert math.isnan(logprob_reference(row, 0))
    # the fp16 words are widened exactly: 0.1 is 0.0999755859375 in binary16
    assert logprob_reference(f16(0.1, 0.0), 0) == pytest.approx(0.0999755859375 - math.log(math.exp(0.0999755859375) + 1.0), abs=1e-15)
    assert perplexity(np.full(5, -math.log(7.0))) == pytest.approx(7.0, rel=1e-12)
    assert perplexity([np.array([-1.0, -2.0], np.float32), np.array([-3.0], np.float32)]) == pytest.approx(math.exp(2.0), rel=1e-12)


def _butterfly(v: np.ndarray, op) -> np.float32:
    """64 lanes: v[l] = op(v[l], v[l ^ off]) for off = 1, 2, .. 32 (fp32; every lane ends with the same bits)."""
    v = v.astype(np.float32)
    for off in (1, 2, 4, 8, 16, 32):
        v = op(v, v[np.arange(64) ^ off]).astype(np.float32)
    assert np.all((v == v[0]) | (np.isnan(v) & np.isnan(v[0])))
    return v[0]


def device_scheme(x16: np.ndarray, target: int) -> np.float32:
    """csrc/sampling.hip's chunk_lse_pair + merge_lse in numpy fp32, in the kernels' order: per thread 16 values in index order, a wave butterfly, waves 0 .. 3 in order;
    then the chunk pairs through a butterfly and (w0 + w1) + (w2 + w3)."""
    f = np.float32
    V = x16.size
    nch = (V + 4095) // 4096
    x = np.full(nch * 4096, -np.inf, np.float32)
    x[:V] = x16.astype(np.float32)
    pm, ps = np.full(256, -np.inf, np.float32), np.zeros(256, np.float32)
    for c in range(nch):
        xc = x[c * 4096:(c + 1) * 4096].reshape(4, 64, 16)  # [wave][lane][e]
        m = np.fmax.reduce([_butterfly(np.fmax.reduce(xc[w], axis=1), np.fmax) for w in range(4)])  # (fmaxf: a NaN is never the maximum)
        with np.errstate(invalid="ignore"):
            e = np.where(xc == -np.inf, f(0), np.exp((xc - m).astype(np.float32))).astype(np.float32)
        t = np.zeros((4, 64), np.float32)
        for i in range(16):
            t = (t + e[:, :, i]).astype(np.float32)
        ws = [_butterfly(t[w], np.add) for w in range(4)]
        pm[c], ps[c] = m, f(f(f(ws[0] + ws[1]) + ws[2]) + ws[3])
    M = np.fmax.reduce([_butterfly(pm[w * 64:(w + 1) * 64], np.fmax) for w in range(4)])
    with np.errstate(invalid="ignore"):
        term = np.where(ps == 0, f(0), ps * np.exp((pm - M).astype(np.float32))).astype(np.float32)
    ws = [_butterfly(term[w * 64:(w + 1) * 64], np.add) for w in range(4)]
    S = f(f(ws[0] + ws[1]) + f(ws[2] + ws[3]))
    with np.errstate(divide="ignore"):
        lse = f(M + f(np.log(S)))
    with np.errstate(invalid="ignore"):
        return f(x[target] - lse)


@pytest.mark.parametrize("vocab", [1, 7, 4096, 4097, 12328, 128256])
def test_the_kernels_summation_order_in_fp32_keeps_the_accuracy_contract(vocab):
    """Gaussian sigma 4 and sigma 16 (clipped to +-64), flat, spiked and half-integer tie rows: the fp32 scheme in the prescribed order stays within 2^-16 of float64
    (with room: the depth of the sums is 16 + 6 + 3 + 8 additions, every term <= 1)."""
    from tinychatengine_amd.generate import logprob_reference
    rng = np.random.default_rng(vocab)
    rows = {"gauss4": rng.normal(0, 4, vocab), "gauss16": rng.normal(0, 16, vocab).clip(-64, 64), "flat": np.full(vocab, 3.25),
            "spike": np.where(np.arange(vocab) == vocab // 3, 60.0, rng.normal(0, 1, vocab)), "ties": rng.integers(-8, 8, vocab) * 0.5}
    worst = 0.0
    for name, r in rows.items():
        x16 = r.astype(np.float16)
        for t in {0, vocab - 1, int(np.argmax(x16)), int(np.argmin(x16))}:
            err = abs(float(device_scheme(x16, t)) - logprob_reference(x16, t))
            worst = max(worst, err)
            assert err <= BOUND, f"{name} vocab {vocab} target {t}: {err:.3e}"
    print(f"vocab {vocab}: worst |fp32 scheme - float64| = {worst:.3e} = {worst / BOUND:.2f} of 2^-16")


def test_the_scheme_defines_the_degenerate_rows():
    from tinychatengine_amd.generate import logprob_reference
    rng = np.random.default_rng(3)
    x = rng.normal(0, 4, 12328).astype(np.float16)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[5000] = bad
        assert math.isnan(device_scheme(y, 0)) and math.isnan(logprob_reference(y, 0))
    assert math.isnan(device_scheme(np.full(4097, -np.inf, np.float16), 0))
    y = x.copy()
    y[4096:8192] = -np.inf  # one whole chunk of -inf beside finite chunks
    assert abs(float(device_scheme(y, 7)) - logprob_reference(y, 7)) <= BOUND
    assert device_scheme(y, 5000) == -np.inf
    y[4100] = np.nan  # ... and a NaN hidden in it is still seen
    assert math.isnan(device_scheme(y, 7))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# refusals: before any launch
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    capi.lib()
    return capi


P = 0x7F0000001000  # a 4096-aligned address nobody follows


def test_exports_and_struct(capi):
    for n in ("tce_logprobs_workspace_bytes", "tce_sample_logprobs_f16", "tce_sample_verify_logprobs_f16", "tce_logprobs_f16"):
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
    assert C.sizeof(capi.LogprobOut) == 24
    L = capi.lib()
    assert L.tce_version() == capi.TCE_ABI_VERSION  # additive: the number did not move
    # pairs [rows][chunks] of 8 bytes + two floats per row, rounded up to 256
    assert L.tce_logprobs_workspace_bytes(3, 12328) == 256 and L.tce_logprobs_workspace_bytes(1, 1) == 256
    assert L.tce_logprobs_workspace_bytes(256, 128256) == (256 * 32 * 8 + 256 * 8 + 255) // 256 * 256
    for rows, vocab in ((0, 100), (-1, 100), (65536, 100), (4, 0), (4, (1 << 20) + 1)):
        assert L.tce_logprobs_workspace_bytes(rows, vocab) == 0


def test_logprobs_f16_refusals(capi):
    ok = dict(logits_ptr=P, ld=4104, vocab=4097, rows=3, target_ptr=P, out_logprob_ptr=P, out_lse_ptr=None, partials_ptr=P)
    bad = [({"logits_ptr": 0}, capi.TCE_ERR_BAD_ARG), ({"target_ptr": 0}, capi.TCE_ERR_BAD_ARG), ({"out_logprob_ptr": 0}, capi.TCE_ERR_BAD_ARG),
           ({"partials_ptr": 0}, capi.TCE_ERR_BAD_ARG), ({"rows": 0}, capi.TCE_ERR_BAD_ARG), ({"vocab": 0}, capi.TCE_ERR_BAD_ARG),
           ({"vocab": 4105}, capi.TCE_ERR_BAD_ARG),  # vocab > ld
           ({"rows": 65536}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"vocab": (1 << 20) + 8, "ld": (1 << 20) + 8}, capi.TCE_ERR_UNSUPPORTED_SHAPE),
           ({"ld": 4100}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"logits_ptr": P + 8}, capi.TCE_ERR_UNSUPPORTED_SHAPE),
           ({"partials_ptr": P + 4}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"target_ptr": P + 2}, capi.TCE_ERR_UNSUPPORTED_SHAPE),
           ({"out_logprob_ptr": P + 1}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"out_lse_ptr": P + 2}, capi.TCE_ERR_UNSUPPORTED_SHAPE)]
    for change, code in bad:
        assert capi.logprobs_f16(**{**ok, **change}, stream=None) == code, change
        assert "tce_logprobs_f16" in capi.last_error()


def _sample_call(capi, **change):
    c = capi.SampleCall(logits=P, ld=4104, vocab=4097, batch=3, top_k_bound=8, rows=P, pos_device=P, pos_bound=63, log_stride=8, next_token=P, out_log=P,
                        uniform_override=None, debug=None, workspace=P, n_stop=0, mirostat=0, tfs_z=1.0, typical_p=1.0)
    for k, v in change.items():
        setattr(c, k, v)
    return c


def test_sample_logprobs_refusals(capi):
    lp = lambda **kw: capi.LogprobOut(**{**dict(out_logprob=P, last_lse=None, partials=P), **kw})
    L = capi.lib()
    assert L.tce_sample_logprobs_f16(C.byref(_sample_call(capi)), None, None) == capi.TCE_ERR_BAD_ARG and "tce_logprob_out" in capi.last_error()
    assert L.tce_sample_logprobs_f16(None, C.byref(lp()), None) == capi.TCE_ERR_BAD_ARG
    for kw, code in (({"out_logprob": None}, capi.TCE_ERR_BAD_ARG), ({"partials": None}, capi.TCE_ERR_BAD_ARG), ({"partials": P + 4}, capi.TCE_ERR_UNSUPPORTED_SHAPE),
                     ({"out_logprob": P + 2}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"last_lse": P + 1}, capi.TCE_ERR_UNSUPPORTED_SHAPE)):
        assert capi.sample_logprobs_f16(_sample_call(capi), lp(**kw), None) == code, kw
        assert "tce_sample_logprobs_f16" in capi.last_error()
    # tce_sample_f16's own refusals come first, under the new entry point's name
    for change, code in (({"ld": 4100}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"vocab": 4105}, capi.TCE_ERR_BAD_ARG), ({"logits": P + 8}, capi.TCE_ERR_UNSUPPORTED_SHAPE),
                         ({"vocab": (1 << 20) + 8, "ld": (1 << 20) + 8}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"top_k_bound": 257}, capi.TCE_ERR_UNSUPPORTED_SHAPE),
                         ({"tfs_z": 0.5}, capi.TCE_ERR_UNSUPPORTED_SHAPE), ({"out_log": None}, capi.TCE_ERR_BAD_ARG)):
        assert capi.sample_logprobs_f16(_sample_call(capi, **change), lp(), None) == code, change
        assert capi.sample_f16(_sample_call(capi, **change), None) == code, change  # ... and are tce_sample_f16's


def test_sample_verify_logprobs_refusals(capi):
    lp = lambda **kw: capi.LogprobOut(**{**dict(out_logprob=P, last_lse=None, partials=P), **kw})
    v = lambda s=None, **kw: capi.SampleVerifyCall(**{**dict(s=s or _sample_call(capi), rows_per_seq=4, hist_stride=72, row_token=P, row_pos=P, history=P, emitted=P), **kw})
    L = capi.lib()
    assert L.tce_sample_verify_logprobs_f16(C.byref(v()), None, None) == capi.TCE_ERR_BAD_ARG
    assert L.tce_sample_verify_logprobs_f16(None, C.byref(lp()), None) == capi.TCE_ERR_BAD_ARG
    assert capi.sample_verify_logprobs_f16(v(), lp(out_logprob=None), None) == capi.TCE_ERR_BAD_ARG
    assert capi.sample_verify_logprobs_f16(v(), lp(partials=None), None) == capi.TCE_ERR_BAD_ARG
    assert capi.sample_verify_logprobs_f16(v(), lp(partials=P + 4), None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    for call, code in ((v(rows_per_seq=9), capi.TCE_ERR_UNSUPPORTED_SHAPE), (v(hist_stride=63), capi.TCE_ERR_BAD_ARG), (v(emitted=None), capi.TCE_ERR_BAD_ARG),
                       (v(s=_sample_call(capi, ld=4100)), capi.TCE_ERR_UNSUPPORTED_SHAPE)):
        assert capi.sample_verify_logprobs_f16(call, lp(), None) == code
        assert "tce_sample_verify_logprobs_f16" in capi.last_error()
        assert capi.sample_verify_f16(call, None) == code


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# score()'s bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_score_plan_slots_targets_chunks_and_split():
    from tinychatengine_amd.generate import score_plan
    prompts = [[7], [1, 2], list(range(10, 27)), [5] * 40]
    plan = score_plan(prompts, free_slots=[1, 2, 3], max_keys=64, vocab=100, chunk_rows=8)
    assert plan["work"] == [1, 2, 3] and plan["slots"] == [1, 2, 3]
    assert plan["reserve"] == [(1, 1), (2, 16), (3, 39)]  # the last key index of each prompt
    assert plan["tokens"] == [1, 2] + list(range(10, 27)) + [5] * 40
    assert plan["targets"] == [2, -1] + list(range(11, 27)) + [-1] + [5] * 39 + [-1]  # the next token; -1 for a prompt's last row
    assert plan["chunk"] == 8 and plan["chunks"] == [(r, 8) for r in range(0, 56, 8)] + [(56, 3)] and sum(m for _, m in plan["chunks"]) == 59
    values = np.arange(59, dtype=np.float32)
    out = plan["split"](values)
    assert [a.size for a in out] == [0, 1, 16, 39] and all(a.dtype == np.float32 for a in out)
    assert out[1].tolist() == [0.0] and out[2].tolist() == list(range(2, 18)) and out[3].tolist() == list(range(19, 58))  # the rows of the -1 targets are dropped
    one = score_plan(prompts, [0, 1, 2, 3], 64, 100, 256)
    assert one["chunk"] == 59 and one["chunks"] == [(0, 59)] and one["slots"] == [0, 1, 2]
    nothing = score_plan([[3], [4]], [], 64, 100)
    assert nothing["work"] == [] and [a.size for a in nothing["split"](np.zeros(0, np.float32))] == [0, 0]
    for bad, kw in (([[1, 2], [3, 4]], dict(free_slots=[0])), ([[]], {}), ([[1] * 65], {}), ([[1, 100]], {}), ([[1, -1]], {}), ([[1, 2]], dict(chunk_rows=0))):
        with pytest.raises(ValueError):
            score_plan(bad, **{**dict(free_slots=[0, 1], max_keys=64, vocab=100, chunk_rows=8), **kw})


def test_score_reservation_is_all_or_nothing_on_a_host_allocator():
    from tinychatengine_amd.generate import score_plan
    from tinychatengine_amd.paged_kv import PageAllocator, PagePoolExhausted
    alloc = PageAllocator(num_pages=6, page_keys=16, batch=4, max_pages_per_seq=4, device="cpu")
    alloc.reserve(0, 20)  # a live sequence holds two pages
    before = (list(alloc.free), [list(p) for p in alloc.pages], list(alloc.refcount), alloc.table.clone())
    plan = score_plan([[1] * 40, [2] * 30], free_slots=[1, 2, 3], max_keys=64, vocab=100)  # 3 + 2 pages, 4 free
    with pytest.raises(PagePoolExhausted):
        alloc.reserve_many(plan["reserve"])
    assert (list(alloc.free), [list(p) for p in alloc.pages], list(alloc.refcount)) == before[:3] and bool((alloc.table == before[3]).all())
    plan = score_plan([[1] * 33, [2] * 16], free_slots=[1, 2, 3], max_keys=64, vocab=100)  # 3 + 1 pages
    alloc.reserve_many(plan["reserve"])
    assert alloc.pages_in_use() == 6
    for s in plan["slots"]:
        alloc.release(s)
    alloc.check_invariants()
    assert alloc.pages_in_use() == 2 and sorted(alloc.free) == sorted(before[0])
