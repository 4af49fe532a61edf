"""CPU (no GPU): the host side of generation (tinychatengine_amd/generate.py).

* sample_reference -- the numpy restatement of the sampling chain, the yardstick the device sampler is held to -- against the results of the reference's own code
  (tests/golden/sampling_golden.npz, recorded from llm/src/Generate.cc by tests/golden/make_sampling_golden.py) under the rules of tests/sampling_rules.py;
* the fixture's own soundness: the accepted band of n is a single value in at least 95 % of the rows of every configuration;
* the generator's restatement against the Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors: the three philox4x32 10-round lines),
  checked here additionally against a second restatement written from the paper's round / key-bump definition, and its independence of slot and batch;
* ring and row bookkeeping, the page reservations of run(n) on a device="cpu" allocator, and the argument checks of the new entry points (no HIP call is reached).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


def _params(name):
    from tinychatengine_amd.generate import SamplingParams
    k, top_p, temp, sigma, rp, af, ap, rows, seed = R.CONFIGS[name]
    return SamplingParams(temp=temp, top_k=k, top_p=top_p, repeat_penalty=rp, alpha_frequency=af, alpha_presence=ap, repeat_last_n=64)


SAMPLED = [n for n, c in R.CONFIGS.items() if c[2] > 0]


def test_the_issue_configurations_are_in_the_fixture(fixture):
    have = {(c[0], c[1], c[2], c[3]) for c in R.CONFIGS.values()}
    for want in [(40, 0.95, 0.8, 2.5), (256, 0.9, 0.7, 2.5), (40, 0.95, 0.8, 4.0), (64, 0.5, 1.3, 3.0)]:
        assert want in have
    assert any(c[0] == 1 for c in R.CONFIGS.values()) and any(c[2] <= 0 for c in R.CONFIGS.values())
    assert {c[4] for c in R.CONFIGS.values()} >= {1.0, 1.1} and any(c[5] != 0 and c[6] != 0 for c in R.CONFIGS.values())
    assert os.path.getsize(R.maker.OUT) < 1 << 20
    for name, c in R.CONFIGS.items():
        assert fixture[name + "/greedy"].shape == (c[7],)


@pytest.mark.parametrize("name", SAMPLED)
def test_the_band_of_n_is_exact_in_95_percent_of_the_rows(fixture, name):
    """From the fixture alone: what keeps the tolerance band of n from hiding a failure."""
    k, top_p = R.CONFIGS[name][0], R.CONFIGS[name][1]
    rows = fixture[name + "/n"].size
    exact = 0
    for r in range(rows):
        lo, hi = R.n_band(fixture[name + "/p"][r], top_p, k)
        assert lo <= int(fixture[name + "/n"][r]) <= hi, f"{name} row {r}: the reference's own n lies outside the band"
        exact += lo == hi
    print(f"{name}: band exact in {exact} of {rows} rows")
    assert exact >= 0.95 * rows


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_sample_reference_against_the_references_own_code(fixture, name):
    from tinychatengine_amd.generate import draw_reference, sample_reference
    k, top_p, temp, sigma, rp, af, ap, rows, seed = R.CONFIGS[name]
    params = _params(name)
    worst_p = worst_fp = 0.0
    for r, (logits, recent) in enumerate(R.config_inputs(name, fixture)):
        what = f"{name} row {r}"
        x = R.penalised(logits, recent, rp, af, ap)
        got = sample_reference(logits, recent, params, 0.5)
        if temp <= 0:
            assert got["token"] == int(fixture[name + "/greedy"][r]), f"{what}: greedy id"
            continue
        greedy = sample_reference(logits, recent, type(params)(**{**params.__dict__, "temp": 0.0}), 0.5)
        assert greedy["token"] == int(fixture[name + "/greedy"][r]), f"{what}: greedy id"
        R.check_candidates(what, x, got["ids"], got["logits"], fixture[name + "/ids"][r], fixture[name + "/logit"][r])
        worst_p = max(worst_p, R.check_p(what + " p", got["p"], fixture[name + "/p"][r], k))
        lo, hi = R.n_band(fixture[name + "/p"][r], top_p, k)
        assert lo <= got["n"] <= hi, f"{what}: n = {got['n']} outside [{lo}, {hi}]"
        n_ref = int(fixture[name + "/n"][r])
        if got["n"] == n_ref:
            worst_fp = max(worst_fp, R.check_p(what + " final p", got["final_p"], fixture[name + "/final_p"][r][:n_ref], k))
            for u, ok in R.draw_points(fixture[name + "/final_p"][r][:n_ref], k, seed * 1000 + r):
                i = draw_reference(got["final_p"], u)
                assert i in ok, f"{what}: u = {u!r} drew position {i}, accepted {sorted(ok)}"
    print(f"{name}: worst relative error of p {worst_p:.2e}, of the final p {worst_fp:.2e} (tolerance {R.tol(k):.2e})")


def test_philox_known_answers_and_independence():
    from tinychatengine_amd.generate import philox4x32_10, uniform

    def second(c, k):  # the paper's definition, written separately: round(), then nine times bumpkey() + round()
        def mulhilo(a, b):
            p = a * b
            return (p >> 32) & 0xFFFFFFFF, p & 0xFFFFFFFF
        c, k = list(c), list(k)
        for r in range(10):
            if r:
                k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
            hi0, lo0 = mulhilo(0xD2511F53, c[0])
            hi1, lo1 = mulhilo(0xCD9E8D57, c[2])
            c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        return tuple(c)

    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        assert philox4x32_10(c, k) == want == second(c, k)
    rng = np.random.default_rng(5)
    for _ in range(50):
        c, k = [int(v) for v in rng.integers(0, 2 ** 32, 4)], [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        assert philox4x32_10(c, k) == second(c, k)
    # a function of (seed, index) alone, in [0, 1), on the 2^-24 grid, and not constant
    us = [uniform(77, i) for i in range(2000)]
    assert all(0.0 <= float(u) < 1.0 and float(u) * 2 ** 24 == int(float(u) * 2 ** 24) for u in us)
    assert abs(float(np.mean(us)) - 0.5) < 0.03 and len(set(float(u) for u in us)) > 1990
    assert uniform(77, 5) == us[5] and uniform(78, 5) != us[5] and uniform(77 + (1 << 32), 5) != us[5]
    assert float(uniform(1, 0)) == ((philox4x32_10((0, 0, 0, 0), (1, 0))[0] >> 8) / 2 ** 24)


def test_rows_and_rings():
    from tinychatengine_amd import capi
    from tinychatengine_amd.generate import SamplingParams, make_row, ring_window
    assert C.sizeof(capi.SampleRow) == 304 and C.sizeof(capi.SampleDebug) == 16 + 4 * 1024 and C.sizeof(capi.SampleCall) == 120
    r = make_row(SamplingParams(), seed=(5 << 32) | 9, max_new=7)
    assert list(r.ring) == [0] * 64 and r.ring_pushed == 0 and r.generated == 0 and (r.seed_lo, r.seed_hi) == (9, 5) and r.top_k == 40
    assert ring_window(np.array(r.ring), 0, 64).tolist() == [0] * 64  # the reference's last_n_tokens: token 0 is in the window until 64 tokens have passed
    prompt = list(range(100, 170))  # 70 tokens: the ring has wrapped
    r = make_row(SamplingParams(repeat_last_n=16), 1, 4, prompt)
    assert r.ring_pushed == 70 and sorted(r.ring) == list(range(106, 170))
    assert ring_window(np.array(r.ring), 70, 16).tolist() == list(range(169, 153, -1))
    r = make_row(SamplingParams(), 1, 4, [11, 12, 13])
    assert sorted(ring_window(np.array(r.ring), 3, 64).tolist()) == [0] * 61 + [11, 12, 13]
    for bad in (SamplingParams(top_k=0), SamplingParams(top_k=300), SamplingParams(tfs_z=0.9), SamplingParams(typical_p=0.5), SamplingParams(mirostat=2),
                SamplingParams(repeat_last_n=65)):
        with pytest.raises(ValueError):
            bad.check()
    SamplingParams(temp=0.0, top_k=0).check()  # greedy does not look at top_k


def test_sample_reference_corner_cases():
    from tinychatengine_amd.generate import SamplingParams, sample_reference
    x = np.zeros(1000, np.float16)
    x[[7, 300, 999]] = 3.0
    x[5] = 2.0
    off = dict(repeat_penalty=1.0, repeat_last_n=0)
    assert sample_reference(x, [], SamplingParams(temp=0.0, **off), 0.0)["token"] == 7  # the lowest id among the maxima
    got = sample_reference(x, [], SamplingParams(top_k=2, top_p=1.0, **off), 0.99)
    assert got["ids"].tolist() == [7, 300] and got["n"] == 2 and got["token"] == 300  # a tie across the top-k boundary: the lowest ids
    got = sample_reference(x, [], SamplingParams(top_k=6, top_p=0.5, **off), 0.0)
    assert got["ids"].tolist() == [7, 300, 999, 5, 0, 1] and got["n"] == 1  # cum_1 = 0.58 > 0.5 at i = 1: the candidate that crosses is dropped
    assert sample_reference(x, [], SamplingParams(top_k=6, top_p=1e-9, **off), 0.9)["n"] == 1  # at least one is kept
    # the penalty: once per distinct id; the frequency term per occurrence; token 0 of the initial zeros is penalised
    got = sample_reference(x, [7, 7, 0], SamplingParams(top_k=3, top_p=1.0, repeat_penalty=2.0, alpha_frequency=0.25, alpha_presence=0.5, repeat_last_n=64), 0.0)
    assert got["ids"].tolist() == [300, 999, 5] and got["logits"].tolist() == [3.0, 3.0, 2.0]
    full = sample_reference(x, [7, 7, 0], SamplingParams(top_k=1000, top_p=1.0, repeat_penalty=2.0, alpha_frequency=0.25, alpha_presence=0.5), 0.0)
    at = {int(i): float(v) for i, v in zip(full["ids"], full["logits"])}
    assert at[7] == 3.0 / 2.0 - (2 * 0.25 + 0.5) and at[0] == 0.0 * 2.0 - (0.25 + 0.5)


def test_run_reserves_pages_for_the_next_n_positions_all_or_nothing():
    """SlotBook + PageAllocator(device="cpu"): what BatchedGenerator.run(n) does before it replays -- no launch involved."""
    from tinychatengine_amd.generate import SlotBook
    from tinychatengine_amd.paged_kv import PageAllocator, PagePoolExhausted
    alloc = PageAllocator(num_pages=8, page_keys=16, batch=4, max_pages_per_seq=4, device="cpu")
    book = SlotBook(4, alloc.max_keys)
    book.admit(0, 30, 100)   # next position 30: page 1
    book.admit(2, 3, 5)      # five tokens at most
    alloc.reserve_many([(0, 29), (2, 2)])
    assert book.wanted(8) == [(0, 37), (2, 6)]          # slot 2: one token is out (admission), four replays are left: positions 3 .. 6
    assert book.wanted(1) == [(0, 30), (2, 3)]
    book.reserve(alloc, 8)
    assert [len(p) for p in alloc.pages] == [3, 0, 1, 0]
    alloc.check_invariants()
    book.update([38, -1, -1, -1], [9, 0, 5, 0])         # after the run: slot 0 advanced, slot 2 used its budget
    assert book.live() == [0] and book.generated[2] == 5
    assert book.wanted(100) == [(0, 63)]                 # never beyond the cache's last key
    with pytest.raises(ValueError):
        book.admit(0, 4, 4)                              # live
    book.admit(1, 40, 50)
    book.admit(3, 40, 50)
    alloc.reserve_many([(1, 39)])                        # 3 + 1 + 3 = 7 of 8 pages
    before = ([list(p) for p in alloc.pages], list(alloc.free), alloc.table.clone())
    with pytest.raises(PagePoolExhausted):
        book.reserve(alloc, 30)                          # slot 0 needs 1 more, slot 1 one more, slot 3 four: nothing may change
    assert ([list(p) for p in alloc.pages], list(alloc.free)) == before[:2] and bool((alloc.table == before[2]).all())
    alloc.check_invariants()
    assert book.update([38, 40, -1, 64], [9, 1, 5, 1]) == [3]  # a position past the last key is inactive by the rule: retired
    book.clear(0)
    assert alloc.release(0) and book.live() == [1]


def test_new_entry_points_refuse_bad_arguments_before_any_hip_call():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    L = capi.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    assert int(L.tce_sample_workspace_bytes(16, 128256)) == 256 + 16 * 32 * 256 * 8 and int(L.tce_sample_workspace_bytes(0, 128256)) == 0
    assert int(L.tce_sample_workspace_bytes(1, (1 << 20) + 1)) == 0

    def call(**kw):
        c = capi.SampleCall(logits=p, ld=128256, vocab=128256, batch=2, top_k_bound=40, rows=p, pos_device=p, pos_bound=63, log_stride=8, next_token=p, out_log=p,
                            workspace=p, n_stop=0, mirostat=0, tfs_z=1.0, typical_p=1.0)
        for k, v in kw.items():
            setattr(c, k, v)
        return capi.sample_f16(c, None)

    assert L.tce_sample_f16(None, None) == capi.TCE_ERR_BAD_ARG
    for field in ("logits", "rows", "pos_device", "next_token", "out_log", "workspace"):
        assert call(**{field: None}) == capi.TCE_ERR_BAD_ARG, field
    assert call(batch=0) == capi.TCE_ERR_BAD_ARG and call(log_stride=0) == capi.TCE_ERR_BAD_ARG and call(n_stop=5) == capi.TCE_ERR_BAD_ARG
    assert call(ld=128000) == capi.TCE_ERR_BAD_ARG and "vocab" in capi.last_error()
    for kw in (dict(top_k_bound=0), dict(top_k_bound=-1), dict(top_k_bound=257), dict(tfs_z=0.95), dict(typical_p=0.9), dict(mirostat=1), dict(mirostat=2)):
        assert call(**kw) == capi.TCE_ERR_UNSUPPORTED_SHAPE, kw
    assert "not built" in capi.last_error()
    assert call(logits=p + 2) == capi.TCE_ERR_UNSUPPORTED_SHAPE and call(ld=128260) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert call(vocab=131073, ld=131080, top_k_bound=256) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "survivors" in capi.last_error()
    vp = C.c_void_p
    emb = lambda **kw: L.tce_embed_rows_f16(vp(kw.get("table", p)), kw.get("vocab", 100), kw.get("hidden", 512), vp(kw.get("token", p)), vp(kw.get("out", p)), kw.get("batch", 2),
                                            vp(kw.get("pos", p)), kw.get("bound", 63), vp(kw.get("ws", p)), None)
    for field in ("table", "token", "out", "pos", "ws"):
        assert emb(**{field: None}) == capi.TCE_ERR_BAD_ARG, field
    assert emb(vocab=0) == capi.TCE_ERR_BAD_ARG and emb(batch=0) == capi.TCE_ERR_BAD_ARG and emb(bound=-1) == capi.TCE_ERR_BAD_ARG
    assert emb(hidden=510) == capi.TCE_ERR_UNSUPPORTED_SHAPE and emb(out=p + 8) == capi.TCE_ERR_UNSUPPORTED_SHAPE
