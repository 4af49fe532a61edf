"""The proof that the designed attention rows of tests/attention_cases.py discriminate (CPU only).

emulate_decode_step restates the ORDER OF OPERATIONS of the decode step (csrc/attention_fast.hip) in fp32 numpy: pick_chunk's rule, 4 waves x 4 slots per workgroup,
a wave's run cut into 16-key blocks of which a slot holds keys s, s + 4, s + 8, s + 12, one update of a slot's (m, l, o) state per block, the merge of the workgroup's
16 states, the merge of the chunks' partial states, the final division rounded to binary16.  Its exponential is fp32 np.exp, not the device's.

Held to the bound of attention_cases.bound on every family and every size, it is the yardstick for "a correct fp32 implementation meets the bound on this data";
its MUTANTS -- the subtle ways the kernel could be wrong -- must each miss the bound (or leave the finite numbers) on the family that was designed against them.  The
first of them, a running maximum that never moves after a state's first block, passes every Gaussian case, a 40-nat sink and a 0.5-nat-per-key ramp: that is the gap
in the suite these families close."""
import numpy as np
import pytest

import attention_cases as ac

NEG_BIG = np.float32(-1.0e30)


def pick_chunk(keys, rep, waves=4):
    """csrc/attention_fast.hip pick_chunk, the fitted rule."""
    if keys <= 320:
        chunk = keys
    elif keys <= (640 if rep >= 4 else 1024):
        chunk = (keys + 3) >> 2
    else:
        chunk = min((keys + 7) >> 3, 512)
    return (chunk + 4 * waves - 1) // (4 * waves) * (4 * waves)


def emulate_decode_step(q, K, V, rep=1, mask=None, mutant=None, waves=4):
    """q fp16 [heads][hd], K / V fp16 [heads][n][hd] (repeated per query head) -> fp16 [heads][hd]; all heads at once, everything in fp32."""
    f32 = np.float32
    heads, n = q.shape[0], K.shape[1]
    Vf = V.astype(f32)
    if mutant == "flush_v":  # binary16 subnormals read as zero
        Vf = np.where(np.abs(Vf) < f32(2.0 ** -14), f32(0), Vf)
    with np.errstate(all="ignore"):
        s = f32(ac.ALPHA) * np.einsum("hd,hkd->hk", q.astype(f32), K.astype(f32), dtype=f32)
        if mask is not None:
            s = s + mask.astype(f32)[None, :]
        live = np.ones(s.shape, bool)
        out_of_range = ~(np.abs(s) <= f32(65504.0))
        if mutant == "saturate":
            s = np.where(out_of_range, np.where(s < 0, f32(-65504.0), f32(65504.0)), s)
        elif mutant == "weighs_nothing":
            live = ~out_of_range
        else:
            s = np.where(out_of_range, f32(-65504.0), s)
        chunk = pick_chunk(n, rep, waves)
        per_wave = chunk // waves
        parts = []
        for key0 in range(0, n, chunk):
            key1 = min(key0 + chunk, n)
            states = []
            for w in range(waves):
                kw0 = key0 + w * per_wave
                kw1 = min(kw0 + per_wave, key1)
                for slot in range(4):
                    m = np.full(heads, NEG_BIG, f32)
                    l = np.zeros(heads, f32)
                    o = np.zeros((heads, ac.HD), f32)
                    for b0 in range(kw0, kw0 + per_wave, 16):
                        ks = [k for k in range(b0 + slot, b0 + 16, 4) if k < kw1]
                        sb = np.full((heads, 4), NEG_BIG, f32)
                        ok = np.zeros((heads, 4), bool)
                        for u, k in enumerate(ks):
                            ok[:, u] = live[:, k]
                            sb[:, u] = np.where(live[:, k], s[:, k], NEG_BIG)
                        mn = np.maximum(m, sb.max(axis=1))
                        if mutant == "frozen_max" and b0 > kw0:
                            mn = m
                        sc = np.exp(m - mn)
                        p = np.where(ok, np.exp(sb - mn[:, None]), f32(0))
                        m = mn
                        l = l * sc + ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3]))
                        o = o * sc[:, None]
                        for u, k in enumerate(ks):
                            o = o + p[:, u:u + 1] * Vf[:, k]
                    states.append((m, l, o))
            parts.append(_merge(states, first_max=mutant == "merge_first_max"))
        M, L, O = parts[0] if len(parts) == 1 else _merge(parts)
        return (O / L[:, None]).astype(np.float16)


def _merge(states, first_max=False):
    f32 = np.float32
    Mx = states[0][0] if first_max else np.maximum.reduce([m for m, _, _ in states] + [np.full_like(states[0][0], NEG_BIG)])
    L = np.zeros_like(states[0][1])
    O = np.zeros_like(states[0][2])
    for m, l, o in states:
        w = np.exp(m - Mx).astype(f32)
        L = L + l * w
        O = O + o * w[:, None]
    return Mx, L, O


HEADS, KV_HEADS = 4, 1  # a = 1, -1, 1/2, 2 over one key / value head: rep 4, the chunk rule's 640-key threshold


def _case(family, n):
    return ac.make_case(family, n, HEADS, KV_HEADS, seed=11)


def _ratio(case, **kw):
    Kr, Vr = case.repeated()
    got = emulate_decode_step(case.q[0], Kr, Vr, rep=case.rep, **kw)
    return ac.error_ratio(got, case.reference())


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_the_correct_emulation_meets_the_bound(family):
    worst = {}
    for n in ac.SIZES:
        worst[n] = _ratio(_case(family, n))
    print(f"emulation {family}: " + " ".join(f"{n}:{r:.3f}" for n, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_the_chunk_rule_is_the_kernels():
    """pick_chunk above against the library's own account of its cut (tce_attention_decode_describe_gqa: no GPU needed) for every size and every number of
    query heads per key / value head the tests use, and at the rule's thresholds.  One chunk up to 320 keys; four up to 640 (four or more query heads per
    key / value head) or 1024; eight slots beyond (641 keys in eight chunks of 81, rounded up to 96, leave seven live); a multiple of 16 always."""
    from tinychatengine_amd import capi
    for heads, kv_heads in ((4, 1), (4, 2), (2, 2), (8, 2), (32, 8)):
        rep = heads // kv_heads
        for n in ac.SIZES + (319, 322, 640, 1024, 2048, 4100):
            d = capi.describe_attention_step(heads, n, kv_heads)
            assert (d["keys-per-chunk"], d["chunks"], d["waves"]) == (pick_chunk(n, rep), -(-n // pick_chunk(n, rep)), 4), (heads, kv_heads, n, d)
    chunks = lambda n, rep: -(-n // pick_chunk(n, rep))
    assert [chunks(n, 4) for n in ac.SIZES] == [1, 1, 1, 1, 1, 4, 7, 8]
    assert [chunks(n, 1) for n in ac.SIZES] == [1, 1, 1, 1, 1, 4, 4, 8]


@pytest.mark.parametrize("mutant,family,sizes", [("frozen_max", "stairs_up", (128, 320, 321, 641, 1025)),
                                                  ("merge_first_max", "stairs_up", (128, 320, 321, 641, 1025)),
                                                  ("saturate", "out_of_range", ac.SIZES[1:]),  # (one key: every softmax returns its value row)
                                                  ("weighs_nothing", "all_out_of_range", ac.SIZES),
                                                  ("flush_v", "subnormal_v", ac.SIZES)])
def test_every_mutant_is_killed_by_its_family(mutant, family, sizes):
    for n in sizes:
        r = _ratio(_case(family, n), mutant=mutant)
        assert not r <= 1.0, f"{mutant} survives {family} at n = {n}: ratio {r:.3f}"


@pytest.mark.parametrize("family", ["sink_first", "sink_last", "sink_own", "ramp_up", "flat"])
def test_a_frozen_maximum_survives_sinks_and_ramps(family):
    """Why the staircase exists: a 40-nat sink and a ramp of 0.5 nats per key leave exp() far from its overflow at 88.7 nats, and a running maximum that never
    moves is then mathematically exact.  (If this ever fails the families got sharper, which is fine: drop the family from the list.)"""
    for n in ac.SIZES:
        assert _ratio(_case(family, n), mutant="frozen_max") <= 1.0, n


def test_masking_the_sink_hands_the_row_to_the_rest():
    for family in ("sink_first", "sink_last"):
        for n in (17, 321):
            case = _case(family, n)
            mask, win = ac.masked_sink(case)
            Kr, Vr = case.repeated()
            got = emulate_decode_step(case.q[0], Kr, Vr, rep=case.rep, mask=mask)
            ref = case.reference(mask=mask)
            assert ac.error_ratio(got, ref) <= 1.0
            assert np.abs(ref[0] - Vr[0, win].astype(np.float64)).max() > 0.1  # head 0 (a = 1) no longer returns the sink's value row


def test_the_bound_without_its_subnormal_term_fails_a_correct_implementation():
    """The 2^-25 of attention_cases.bound: on `subnormal_v` the output itself is a binary16 subnormal and its final rounding alone exceeds the two relative terms."""
    worst = 0.0
    for n in ac.SIZES:
        case = _case("subnormal_v", n)
        Kr, Vr = case.repeated()
        got = emulate_decode_step(case.q[0], Kr, Vr, rep=case.rep).astype(np.float64)
        ref = case.reference()
        worst = max(worst, float((np.abs(got - ref) / (ac.bound(ref) - 2.0 ** -25)).max()))
    assert worst > 1.0, worst


def test_e4m3_cases_are_on_the_grid_and_keep_their_property():
    from tinychatengine_amd.paged_kv import fp8_dequantize_reference, fp8_quantize_reference
    for family in ac.FAMILIES:
        for ve in (0, -8):
            if family == "subnormal_v" and ve == 0:
                continue  # (e4m3's smallest value at exponent 0 is 2^-9: the family exists on the grid of exponent -8 only)
            case = ac.make_case(family, 321, 4, 2, seed=5, e4m3=True, ve=ve, step=200.0)  # (make_case asserts the property after the rounding)
            for x, e in ((case.K, case.ke), (case.V, ve)):
                again = fp8_dequantize_reference(fp8_quantize_reference(np.ascontiguousarray(x), e), e)
                assert np.array_equal(again.view(np.uint16), x.view(np.uint16))
            assert _ratio(case) <= 1.0, (family, ve)


def test_designed_rows_survive_the_oracles_rotation(oracle):
    """A decode step with RoPE gets the UN-rotated q and own key (attention_cases.unrotate); what the oracle's RotaryPosEmb makes of them is within binary16
    rounding of the design, and the family's property -- asserted again on the rotated q and key -- still holds."""
    for family in ("sink_first", "sink_last", "sink_own", "two_peaks", "stairs_up"):
        for n in (17, 321, 1025):
            case = ac.make_case(family, n, 4, 2, seed=2)
            cos, sin = ac.rope_tables(n, seed=n)
            q_raw = ac.unrotate(case.q[0], cos[n - 1], sin[n - 1])
            k_raw = ac.unrotate(case.K[:, n - 1], cos[n - 1], sin[n - 1])
            q_rot, _ = oracle.rope_half(q_raw[:, None, :], q_raw[:, None, :], cos, sin, n - 1)
            _, k_rot = oracle.rope_half(k_raw[:, None, :], k_raw[:, None, :], cos, sin, n - 1)
            assert np.abs(q_rot[:, 0].astype(np.float64) - case.q[0].astype(np.float64)).max() <= 2.0 ** -8 * max(1.0, float(np.abs(case.q[0].astype(np.float64)).max()))
            case.q[0] = q_rot[:, 0]
            case.K[:, n - 1] = k_rot[:, 0]
            case.check()
            assert _ratio(case) <= 1.0, (family, n)


def test_prefill_rows_keep_their_property():
    """rows > 1: a rotates over (row + head), so one K serves ascending, descending, gentler and steeper query rows; make_case asserts the property for every row."""
    for family in ("sink_first", "two_peaks", "stairs_up", "stairs_down", "out_of_range", "all_out_of_range", "subnormal_v"):
        for pos, m in ((0, 30), (17, 64), (5, 1)):
            case = ac.make_case(family, pos + m, 4, 2, seed=100, rows=m)
            assert case.q.shape == (m, 4, ac.HD) and case.K.shape == (2, pos + m, ac.HD)
            # a causal row sees keys 0 .. pos + r: `visible` must give what the truncated K / V give -- a cut key weighs nothing, it is not clamped
            keys = np.arange(pos + m)
            for r in sorted({0, m // 2, m - 1}):
                ref = case.reference(row=r, visible=keys <= pos + r)
                cut = case.reference(row=r, upto=pos + r + 1)
                assert np.isfinite(ref).all() and np.abs(ref - cut).max() <= 1e-12 * max(1.0, np.abs(cut).max()), (family, pos, m, r)
                if r < m - 1 and family not in ("subnormal_v", "all_out_of_range"):
                    assert np.abs(ref - case.reference(row=r)).max() > 0.0, (family, pos, m, r)  # (and the cut changes the answer)
