"""The proof that the designed rows of tests/glue_cases.py are sound and that they discriminate (CPU only; -s prints the tables).

Sound: every family keeps the property it is named for at every width (the generators assert it; they all run here); two restatements of RMSNorm -- the oracle's
(the reference kernel's own order) and a numpy fp32 restatement of this project's slot order -- stay inside (0.5 + M_MARGIN) ulp16 of float64 on every case, with the
share of the margin they use printed; the ambiguous set of the SiLU reference is inside its cap; the oracle's SiLU*mul and add equal the references outside it.

Discriminate: every mutant of glue_cases fails on at least one case, and CAUGHT_BY names the families that must catch it.  One mutant is caught by nothing and
cannot be: `skip_first_rounding` (x * rs * gamma rounded once instead of twice on the way to half) -- see CAUGHT_BY.
"""
import numpy as np
import pytest

import glue_cases as gc

FUSED_WIDTHS = tuple(n for n in gc.WIDTHS if n % 128 == 0 and n <= 16384)


@pytest.fixture(scope="module")
def launches():
    """Every stand-alone launch the GPU test runs, built once (the generators assert every family's property while they build)."""
    return {(n, eps): gc.rms_launches(n, eps) for n in gc.WIDTHS for eps in gc.EPS_VALUES}


def test_every_family_holds_at_every_width(launches):
    for (n, eps), ls in launches.items():
        fams = {f for L in ls for f, _ in L.rows}
        assert fams == set(gc.RMS_FAMILIES), (n, eps, set(gc.RMS_FAMILIES) - fams)
        assert {L.m for L in ls} == {1, 3}
        hot = {v for L in ls for f, v in L.rows if f == "one_hot"}
        assert hot == {(p, m) for p in gc.one_hot_positions(n) for m in gc.ONE_HOT_MAGS}
        for L in ls:  # and once more from the outside, on what the launch holds
            for r, (f, v) in enumerate(L.rows):
                if f not in ("saturate", "negative_gamma"):
                    gc.check_row(f, L.x[r], v)
                elif r == 0:
                    gc.check_gamma(f, L.x[0], L.gamma, eps)
            assert np.isfinite(L.reference()).all()
    for n in FUSED_WIDTHS:  # the rows of the fused forms
        for eps in gc.EPS_VALUES:
            for f in gc.RMS_FAMILIES:
                v = {"one_hot": (n - 1, gc.ONE_HOT_MAGS[0]), "nonfinite": "nan"}.get(f)
                assert gc.rms_row_launch(f, n, eps, v).m == 1
    assert gc.one_hot_positions(24584) == (0, 7, 8, 511, 512, 8191, 8192, 24576, 24583)


def test_nan_row_comes_out_finite():
    """What is pinned about non-finite rows: a NaN makes rs NaN and every product NaN, and rmsnorm_out sends a NaN product to -64504 (the comparison `f > 0` is false,
    fmaxf(NaN, -64504) is -64504): the whole row is -64512 after the rounding.  An inf makes rs 0: its own element is NaN -> -64512, every other element a signed zero."""
    n = 64
    for kind in gc.NONFINITE_KINDS:
        L = gc.rms_row_launch("nonfinite", n, 1e-6, kind)
        ref = gc.h16(L.reference()[0])
        bad = ~np.isfinite(L.x[0].astype(np.float64))
        assert np.all(ref[bad] == np.float16(-64512.0))
        if kind == "nan":
            assert np.all(ref == np.float16(-64512.0))
        else:
            assert not ref[~bad].any()


def test_two_restatements_stay_inside_the_bound(launches, oracle):
    worst = {"oracle": {}, "slot order": {}}
    for (n, eps), ls in launches.items():
        for L in ls:
            for name, got in (("oracle", oracle.rmsnorm_half(L.x, L.gamma, eps)), ("slot order", gc.rmsnorm_project(L.x, L.gamma, eps))):
                for f, r in L.judge(got).items():
                    k = (f, n)
                    worst[name][k] = max(worst[name].get(k, 0.0), r)
    print()
    for name, w in worst.items():
        for f in gc.RMS_FAMILIES:
            r, n = max((v, k[1]) for k, v in w.items() if k[0] == f)
            print(f"    {name:12s} {f:16s} worst ratio {r:.4f} at n = {n:5d}   margin used {gc.margin_used(r):+.3f}")
        top = max(w.values())
        assert top <= 1.0, (name, {k: v for k, v in w.items() if v > 1.0})
        # "with room": the derivation gives 21 u for this project's order (0.66 of the margin) and 33 u for the oracle's at the widest row (1.03 by the worst-case
        # count, which no data reaches); measured, neither uses a quarter of it
        assert gc.margin_used(top) <= 0.25, (name, gc.margin_used(top))


def test_ambiguous_set_is_small():
    sizes = {t: int(gc.ambiguous_gates(gc.ALL_GATES, t).sum()) for t in (1, 2, 4, 8)}
    print(f"\n    ambiguous gates at T = 1 / 2 / 4 / 8 fp32 ulps: {sizes}")
    assert sizes == {1: 7, 2: 13, 4: 26, 8: 53}
    s = gc.ambiguous_set()
    assert s.size == sizes[gc.T_ULPS] <= gc.AMBIGUOUS_CAP
    g = s.view(np.float16).astype(np.float64)
    assert np.isfinite(g).all() and np.abs(g).max() < 12.0


def test_silu_reference_edges():
    """The definition at its edges."""
    ref = lambda g, u=1.0: gc.silu_mul_ref(gc.h16([g]), gc.h16([u]))[0][0]
    assert np.isnan(ref(-np.inf))                                          # exp = inf, r = 0, -inf * 0
    assert ref(-11.1).view(np.uint16) == 0x8000 and ref(-11.1, -1.0).view(np.uint16) == 0  # hexp = inf: r = +0, g * r = -0, times u
    assert ref(-11.08) != 0
    assert np.isnan(ref(-20.0, np.inf)) and np.isnan(ref(1.0, np.nan))
    assert ref(0.0).view(np.uint16) == 0 and ref(-0.0).view(np.uint16) == 0x8000
    assert ref(2.0 ** -24).view(np.uint16) == 0 and ref(2.0 ** -23).view(np.uint16) == 1  # r = 0.5: 2^-25 is a tie and goes to the even +0
    assert np.isinf(ref(30000.0, 3.0)) and ref(np.inf) == np.inf


def test_oracle_silu_and_add_equal_the_references(oracle):
    for tail in (0, 3):
        g, u = gc.silu_operands(tail)
        assert g.size == 9 * 65536 - tail
        ref, alt = gc.silu_mul_ref(g, u)
        got = oracle.silu_mul_half(g, u)
        bad = gc.silu_mismatches(got, ref, alt)
        assert bad.size == 0, [(hex(g.view(np.uint16)[i]), float(u[i]), got[i], ref[i]) for i in bad[:8]]
        amb = gc.ambiguous_gates(g)
        assert gc.same_half(got[~amb], ref[~amb]).all()
        assert amb.sum() == gc.ambiguous_set().size * 9 - (0 if not tail else int(gc.ambiguous_gates(gc.ALL_GATES[-tail:]).sum()))
    for n in (65536, 65536 - 5):
        a, b, where = gc.add_operands()
        a, b = a[:n], b[:n]
        assert gc.same_half(oracle.add_half(a, b), gc.add_ref(a, b)).all()
        assert set(where) == {"overflow", "just_below_overflow", "cancel_to_plus_zero", "signed_zeros", "subnormal_sums", "ties", "inf_and_nan"}


# mutant -> the families that MUST catch it (asserted as a subset of what does; the full table is printed).  () = caught by nothing, by necessity.
CAUGHT_BY = {
    "no_eps": ("zeros", "eps_rules", "one_hot"),           # zeros: 0 * inf = NaN -> -64504 instead of a signed zero
    "eps_times_n": ("eps_rules", "one_hot"),
    "padded_n": ("gauss", "all_max", "one_hot"),           # (at the widths that are no multiple of 64)
    "drop_second_round": ("one_hot", "gauss", "all_max"),  # one_hot at element 8192
    "drop_partial_term": ("one_hot", "gauss", "all_max"),  # one_hot at n - 8 / n - 1 of n = 520, 8200, 24584
    "fp16_accumulate": ("all_max", "gauss", "one_hot"),    # 65504^2 is inf in binary16
    "clamp_65504": ("saturate",),
    "clamp_before_gamma": ("saturate",),
    "flush_denormals": ("eps_rules",),
    # (x * rs * gamma) rounded once: f moves by at most one fp32 ulp in front of the same conversion to half, so the output differs only where f sits within 2^-13
    # binary16 ulps of a tie, and then both neighbours are within (0.5 + M_MARGIN) ulp of float64.  A bound on the error against float64 cannot tell two correct
    # evaluations apart -- NOT OBSERVABLE, and rightly so.  What pins the order of roundings is the bit-for-bit tie of every fused form to
    # tce_rmsnorm_half in the GPU test.
    "skip_first_rounding": (),
}


def test_every_rms_mutant_is_caught(launches):
    assert set(CAUGHT_BY) == set(gc.RMS_MUTANTS)
    print()
    for mutant in gc.RMS_MUTANTS:
        caught, control_only = {}, True
        for (n, eps), ls in launches.items():
            for L in ls:
                for f, r in L.judge(gc.rmsnorm_project(L.x, L.gamma, eps, fault=mutant)).items():
                    if not r <= 1.0:
                        caught.setdefault(f, set()).add(n)
        print(f"    {mutant:22s} caught by " + (", ".join(f"{f} (n = {sorted(ns)[0]}{'...' if len(ns) > 1 else ''})" for f, ns in sorted(caught.items())) or "NOTHING"))
        if CAUGHT_BY[mutant]:
            assert set(CAUGHT_BY[mutant]) <= set(caught), (mutant, sorted(caught))
        else:
            assert not caught, (mutant, caught)


def test_every_silu_and_add_mutant_is_caught():
    g, u = gc.silu_operands()
    ref, alt = gc.silu_mul_ref(g, u)
    print()
    for mutant in gc.SILU_MUTANTS:
        bad = gc.silu_mismatches(gc.silu_mul_mutant(g, u, mutant), ref, alt)
        print(f"    {mutant:22s} {bad.size} of {g.size} elements differ")
        assert bad.size > 0, mutant
    # exp_saturates is caught only below the edge: there the definition gives -0 * u
    bad = gc.silu_mismatches(gc.silu_mul_mutant(g, u, "exp_saturates"), ref, alt)
    assert np.all(g[bad].astype(np.float64) < -11.0)
    a, b, where = gc.add_operands()
    ref = gc.add_ref(a, b)
    for mutant in gc.ADD_MUTANTS:
        bad = np.flatnonzero(~gc.same_half(gc.add_mutant(a, b, mutant), ref))
        hit = sorted(k for k, i in where.items() if np.intersect1d(i, bad).size)
        print(f"    {mutant:22s} {bad.size} of {a.size} elements differ; designed pairs that catch it: {hit}")
        assert {"ties", "overflow"} <= set(hit), hit


def test_one_hot_linear_outputs_are_exact_products():
    """The fused-epilogue operands: the float64 product of the one-hot activations with the dequantized weights IS the designed value, for every row and column."""
    for (M, N, K, G) in ((1, 72, 4096, 128), (4, 40, 1408, 64), (16, 18, 128, 128), (200, 136, 384, 128)):
        lin = gc.OneHotLinear(M, N, K, G, lambda g: gc.epilogue_values(N, shift=7 * g))
        deq = ((lin.codes.astype(np.float64).reshape(N, K // G, G) - 8.0) * lin.s.astype(np.float64)[:, :, None]).reshape(N, K)
        y = lin.a.astype(np.float64) @ deq.T
        assert np.array_equal(y, lin.y.astype(np.float64))
        gates, ups = lin.y[:, 0::2], lin.y[:, 1::2]
        g64 = gates.astype(np.float64)
        ref, _ = gc.silu_mul_ref(gates, ups)
        s = gc.add_ref(gc.residual_for(lin.y[0]), lin.y[0])
        # what even the narrowest launch (nine pairs) holds: hexp = inf, the edge itself, a zero gate, a subnormal one, an overflowing product; sums that overflow and cancel
        assert (g64 <= -11.1).any() and (np.abs(g64 + 11.09) < 0.01).any() and (g64 == 0).any() and ((np.abs(g64) < gc.SUB) & (g64 != 0)).any() and (g64 >= 1000).any()
        assert np.isinf(ref.astype(np.float64)).any() and (ref.view(np.uint16) == 0x8000).any(), "no product overflows, or no -0"
        assert np.isinf(s.astype(np.float64)).any() and (s.view(np.uint16) == 0).any()
        if np.unique(gates.view(np.uint16)).size >= 36:  # gates on both sides of the edge, next to it
            assert (g64[np.abs(g64 + 11.09) < 0.05] < -11.0901).any() and (g64[np.abs(g64 + 11.09) < 0.05] > -11.0901).any()
    assert gc.GATE_VALUES.size == 51 and np.unique(gc.GATE_VALUES.view(np.uint16)).size == 51
