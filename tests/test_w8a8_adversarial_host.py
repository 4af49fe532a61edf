"""The proof that the designed accumulators of tests/w8a8_cases.py are sound and that they discriminate (CPU only).

Sound: every case the GPU test launches (the same generator calls, from the one table in w8a8_cases) keeps its family's property on a non-empty judged set, and the exact
reference -- one np.float32 operation per step -- equals the oracle on every element of every case and output kind, and the reference's own code on the smallest case of
each family (live where oracle/_ref is built, from tests/golden/reference_vectors.npz elsewhere).

Discriminate: numpy emulations of epilogues with one defect each (w8a8_cases.mutant).  Each differs from the exact reference on the judged set of the family built for it;
the table printed with -s also says whether the random operands every earlier W8A8 test drew (test_gpu_w8a8._data at 64 x 64 x 64, both scalar pairs) catch it:
  fused                 fl(f * alpha + u) in one rounding                 separate_roundings.  NOT caught by random operands under (ALPHA, BETA): ALPHA = 33 * 2^-16, the product
                                                                          is exact for |acc| < 2^24 / 33 and both evaluations are the same number (asserted).
  half_even             ties to even instead of away from zero            round_ties
  cvt_truncates         int -> fp32 drops the bits below the 24th         cvt_inexact (int8 and fp32 outputs)
  cvt_half_up           int -> fp32 rounds ties up in magnitude           cvt_inexact (fp32 outputs: the accumulators that are 1 mod 4)
  narrow_before_clamp   the rounded value wraps into int8, then clamps    clamp_far
  saturating_narrow     clamps to -128 .. 127 whatever q_min / q_max say  clamp_narrow, the ReLU form of clamp_edges
  bias_before_scaling   (f + u) * alpha                                   any family with a bias
  minus128_as_plus128   -128 read as +128 in A                            minus128
  accumulate_in_double  C0 + f * alpha + u in double, rounded once        accumulate
  clamp_before_rounding round(clamp(v)): the SAME function for integer bounds (rounding is monotone and leaves the bounds in place) -- asserted equal everywhere, not a defect.
"""
import numpy as np
import pytest

import w8a8_cases as wc
from conftest import reference_vectors

SHAPE = (70, 100)
HOST_KS = {f: (1536 if f in wc.LONG_K_FAMILIES else 1088) for f in wc.FAMILIES}
SMALLEST = {f: ((2, 8, 1536) if f in wc.LONG_K_FAMILIES else (5, 7, 33)) for f in wc.FAMILIES}


def _bits(x):
    return x.view(np.uint8) if x.dtype == np.int8 else x.view(np.uint32)


def _oracle_out(lib, case, kind):
    """The project's restatement (or the reference's own code: the same call surface) on a case."""
    M, N, K = case.M, case.N, case.K
    A, B = case.A, case.B
    lo, hi = case.bounds(kind)
    if case.per_row:
        return lib.int8_matmul_nobias_i8(A, B, case.alpha, lo, hi, M, N, K, batch=True) if kind == "i8_nobias" else lib.int8_matmul_nobias_f32(A, B, case.alpha, M, N, K, batch=True)
    if kind in ("i8_bias", "relu"):
        return lib.int8_matmul_bias_i8(A, B, case.bias8, case.alpha, case.beta, lo, hi, M, N, K)
    if kind == "i8_nobias":
        return lib.int8_matmul_nobias_i8(A, B, case.alpha, lo, hi, M, N, K)
    if kind == "f32_nobias":
        return lib.int8_matmul_nobias_f32(A, B, case.alpha, M, N, K)
    out = lib.int8_matmul_bias_f32(A, B, case.biasf, case.alpha, M, N, K)
    return case.C0 + out if kind == "f32_acc" else out  # add(a, b, c): one fp32 addition


def test_the_conversion_of_the_reference_rounds_to_nearest_even():
    acc = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), -(2 ** 24 + 3), 2 ** 25 + 2, 2 ** 25 + 6, 33_423_359], np.int64)
    assert np.array_equal(acc.astype(np.float32).astype(np.int64), [2 ** 24, 2 ** 24 + 4, -(2 ** 24), -(2 ** 24 + 4), 2 ** 25, 2 ** 25 + 8, 33_423_360])
    v = np.array([0.49999997, -0.49999997, 0.5, -0.5, 1.5, 2.5, -2.5, 8388609.0], np.float32)
    assert np.array_equal(wc.round_half_away(v), [0, -0.0, 1, -1, 2, 3, -3, 8388609])


def test_design_row_reaches_every_target():
    rng = np.random.default_rng(5)
    for K in (33, 64, 1088, 1536, 2048):
        a, p1, p127 = wc.base_row(K, rng)
        assert a[p1] == 1 and a[p127] == 127 and np.all((np.abs(np.delete(a, [p1, p127])) >= 96) & (np.abs(np.delete(a, [p1, p127])) <= 127))
        cap = wc.capacity(a, p1, p127)
        if K == 1536:
            assert cap >= 2 ** 24 + 4_000_000
        for T in [0, 1, -1, 127, -16001, cap, -cap, cap // 2 + 1] + [int(t) for t in rng.integers(-cap, cap + 1, 40)]:
            b = wc.design_row(a, p1, p127, T, rng)
            assert b.dtype == np.int8 and int(a @ b.astype(np.int64)) == T and np.abs(b.astype(np.int64)).max() <= 127


@pytest.mark.parametrize("family", wc.FAMILIES)
def test_builder_invariants(family):
    M, N = SHAPE
    case = wc.make_case(family, M, N, HOST_KS[family])
    counts = {k: int(case.judged(k).sum()) for k in case.kinds}
    print(f"\n{family}: alpha = {case.alpha!r}, judged per kind {counts}")
    plus = [r for r, s in case.rows.items() if s > 0]
    minus = [r for r, s in case.rows.items() if s < 0]
    assert 0 in case.rows and M - 1 in case.rows and 63 in case.rows and 64 in case.rows and plus and (minus or family == "separate_roundings")
    if family not in ("minus128",):
        assert np.abs(case.A.astype(np.int64)).max() <= 127 and np.abs(case.B.astype(np.int64)).max() <= 127
    r0 = plus[0]
    v = {k: case.expected(k)[1] for k in case.kinds}
    if family == "round_ties":
        assert np.log2(case.alpha) % 1 == 0
        for kind in wc.INT8_KINDS:
            assert counts[kind] >= 0.4 * case.designed.sum()
        assert counts["i8_bias"] == case.designed.sum()  # with the bias every designed element is a tie, in both row signs
        js = set(np.abs(v["i8_bias"][r0]) - 0.5)
        assert set(float(j) for j in wc.ROUND_J) <= js
        for r in (r0, minus[0]):
            assert (v["i8_bias"][r] > 0).any() and (v["i8_bias"][r] < 0).any()
    elif family in wc.EDGES:
        e = -int(np.log2(case.alpha))
        want = {val + st * 2.0 ** -e for val, st in wc.EDGES[family]}
        assert want <= set(float(x) for x in v["i8_bias"][r0]), "an edge value is missing from the designed row"
        assert want <= set(float(x) for x in v["i8_nobias"][r0][case.bias8 == 0]) and want <= set(float(x) for x in v["i8_bias"][r0][case.bias8 != 0])
        if family == "clamp_edges":
            assert e >= 16, "127.49.. is not within two fp32 ulps of 127.5"
            assert {-0.5, -0.5 + 2.0 ** -e, -1.5, 0.5} <= set(float(x) for x in v["relu"][r0]) and case.bounds("relu") == (0, 127)
        if family == "clamp_narrow":
            assert (case.qmin, case.qmax) == (-5, 9)
        if family == "clamp_far":
            out = case.expected("i8_nobias")[0]
            wrapped = wc.round_half_away(v["i8_nobias"]).astype(np.int64).astype(np.int8)
            assert (case.judged("i8_nobias") & (wrapped != out) & (np.sign(wrapped) != np.sign(out))).sum() >= 32  # wraps to the other side
    elif family == "cvt_inexact":
        a = np.abs(case.acc[case.designed])
        assert np.all((a >= 2 ** 24) & (a < 2 ** 25) & (a % 2 == 1)) and counts["i8_nobias"] == case.designed.sum()
        T = case.acc[r0]
        for sign in (1, -1):
            assert {1, 3} <= set(int(x) for x in (np.abs(T[np.sign(T) == sign]) % 4))
        tie_cols = np.arange(case.N) % 3 == 0
        j = (np.abs(T[tie_cols]) + 1) // 2 ** 17  # T = (2j + 1) * 2^17 - 1
        assert np.all(j % 2 == 1) and np.array_equal(np.abs(case.expected("i8_nobias")[0][r0][tie_cols].astype(np.int64)), (j - 1) // 2 + 1)
    elif family == "separate_roundings":
        assert counts["i8_bias"] >= 32 and counts["f32_bias"] >= 32 and counts["relu"] >= 1 and counts["f32_acc"] >= 1
    elif family == "minus128":
        assert case.K == 1536 and case.acc.max() == 16384 * 1536 and case.acc.min() == -128 * 127 * 1536 and counts["i8_bias"] >= 32
    elif family == "accumulate":
        assert case.kinds == ("f32_acc",) and set(np.unique(case.acc_marks)) == {0, 1, 2, 3, 4}
        for mark in (1, 2, 3, 4):
            for rows in (plus, minus):
                assert (case.acc_marks[rows] == mark).any()
    for kind in case.kinds:
        if not (family == "separate_roundings" and "nobias" in kind):
            assert counts[kind] > 0, f"{family} / {kind}: nothing is judged"


def test_small_launches_keep_32_elements_that_tell_fused_from_separate():
    for M, N, K in ((5, 7, 33), (1, 70, 1536), (2, 70, 1536), (8, 70, 2048)):
        case = wc.make_case("separate_roundings", M, N, K)
        assert case.judged("i8_bias").sum() >= 32 and case.judged("f32_bias").sum() >= 32, (M, N, K)


def test_exact_reference_equals_the_oracle_on_every_launched_case(oracle):
    n = 0
    for key in wc.launched_cases():
        case = wc.make_case(*key)
        for kind in (("i8_nobias", "f32_nobias") if case.per_row else case.kinds):
            want = _oracle_out(oracle, case, kind)
            got = case.expected(kind)[0]
            assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), f"{key} {kind}: {(_bits(got) != _bits(want)).sum()} elements differ from the oracle"
            n += got.size
    print(f"\n{n} outputs of {len(wc.launched_cases())} cases: the exact reference equals the oracle")


@pytest.mark.parametrize("family", wc.FAMILIES)
def test_exact_reference_equals_the_reference_code_on_the_smallest_case(reference, family):
    case = wc.make_case(family, *SMALLEST[family])
    for kind in case.kinds:
        inputs = [case.A, case.B, case.bias8, case.biasf, case.C0, np.array([case.alpha, case.beta], np.float32), np.array(case.bounds(kind), np.int32)]
        (theirs,) = reference_vectors(f"w8a8_adversarial_{family}_{kind}", inputs, lambda: [_oracle_out(reference, case, kind)], reference is not None)
        got = case.expected(kind)[0]
        assert got.dtype == theirs.dtype and np.array_equal(_bits(got), _bits(theirs)), f"{family} {kind}: differs from the reference's own code"


def _random_case(alpha, beta):
    """The operands of the existing W8A8 tests as a case without designed rows."""
    from test_gpu_w8a8 import _data
    A, B, b8, bf = _data(64, 64, 64, seed=192)
    C0 = np.random.default_rng(192).standard_normal((64, 64)).astype(np.float32)
    return wc.Case("random", A, B, alpha, beta, b8, bf, -128, 127, C0, rows={})


def test_every_mutant_is_caught_by_its_family():
    from test_gpu_w8a8 import ALPHA, BETA
    random_cases = {"ALPHA, BETA": _random_case(ALPHA, BETA), "0.0071, 0.13": _random_case(*wc.NONDYADIC)}
    M, N = SHAPE
    print()
    for name, targets in wc.MUTANTS.items():
        for family, kind in targets:
            for shape in ((M, N, HOST_KS[family]), SMALLEST[family]):
                case = wc.make_case(family, *shape)
                diff = _bits(wc.mutant(case, kind, name)) != _bits(case.expected(kind)[0])
                assert (diff & case.judged(kind)).any(), f"{name} passes {family} / {kind} at {shape}"
                if shape[0] == M:
                    print(f"{name:22s} {family:18s} {kind:10s} differs on {int((diff & case.judged(kind)).sum()):4d} of {int(case.judged(kind).sum()):4d} judged elements")
        for label, rc in random_cases.items():
            caught = {k: int((_bits(wc.mutant(rc, k, name)) != _bits(rc.expected(k)[0])).sum()) for k in wc.KINDS}
            print(f"{name:22s} random 64x64x64 ({label}): elements that differ per kind {caught}")
            if name == "fused" and label == "ALPHA, BETA":
                assert not any(caught.values()), "the exactness argument for ALPHA = 33 * 2^-16 does not hold on these operands"
    for family in wc.FAMILIES:  # the correct epilogue differs nowhere, and neither does its equivalent form
        case = wc.make_case(family, M, N, HOST_KS[family])
        for kind in case.kinds:
            assert np.array_equal(_bits(wc.mutant(case, kind, "none")), _bits(case.expected(kind)[0]))
            for same in wc.EQUIVALENT:
                assert np.array_equal(_bits(wc.mutant(case, kind, same)), _bits(case.expected(kind)[0])), f"{same} differs on {family} / {kind}"


def test_every_form_of_the_launch_table_is_named_by_the_dispatcher():
    """The table the GPU test launches from: under each form's switches tce_w8a8_describe_dispatch (no device needed) names that form at every K it runs, the entries of a
    batch share their scalars and biases, and every switch is back at its rule afterwards."""
    from tinychatengine_amd import capi
    L = capi.lib()

    def named(form, K):
        lda, ldb, ldc = form.ld
        d = capi.W8A8Desc(M=form.M, N=form.N, K=K, batch=form.batch, A=4096, B=4096, C=4096, strideA=form.M * (lda or K), strideB=0 if form.per_row else form.N * (ldb or K),
                          strideC=form.M * (ldc or form.N), alpha=1.0, q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_NONE, out_kind=capi.TCE_OUT_INT8,
                          b_per_row=1 if form.per_row else 0, lda=lda, ldb=ldb, ldc=ldc)
        return capi.describe_w8a8_dispatch(d, with_scratch=form.scratch)

    plain = {(f.name, K): named(f, K) for f in wc.FORMS for K in f.Ks}
    for form in wc.FORMS:
        try:
            capi.w8a8_set_tuning(*form.tuning)
            for mode in form.modes:
                capi.check(L.tce_w4a16_set_debug_mode(mode))
            for K in form.Ks:
                assert named(form, K) == form.describe, (form.name, K)
        finally:
            capi.w8a8_set_tuning()
            for mode in wc.RESTORE_MODES:
                L.tce_w4a16_set_debug_mode(mode)
        for fam, K, off in form.cases():
            cases = [wc.make_case(fam, form.M, form.N, K, b, form.per_row, off) for b in range(form.batch)]
            for c in cases[1:]:
                assert c.alpha == cases[0].alpha and c.beta == cases[0].beta and np.array_equal(c.bias8, cases[0].bias8) and np.array_equal(_bits(c.biasf), _bits(cases[0].biasf))
                assert not np.array_equal(c.B, cases[0].B)  # (but operands of their own)
    assert plain == {(f.name, K): named(f, K) for f in wc.FORMS for K in f.Ks}, "a switch was left on"
    assert len(set(f.describe for f in wc.FORMS)) >= 24


@pytest.mark.parametrize("m,n", [(6, 252), (1025, 1028), (6, 256), (6, 1024)])
def test_layernorm_rows_hold_ties_and_wrapping_outputs(oracle, m, n):
    """The rows the GPU test gives tce_layernorm_q alone: the sequential-sum restatement equals the oracle, every tie column is an exact tie in every row, outputs wrap."""
    x, w, b, want, f, cols = wc.layernorm_rows(m, n)
    assert np.array_equal(want, oracle.layernorm_q(x, w, b))
    assert wc.is_tie(f[:, cols]).all() and (f[:, cols] > 0).any() and (f[:, cols] < 0).any() and (np.abs(f) > 128.5).sum() >= 32
    assert np.all(x[0] == x[0, 0]) and np.abs(x[1]).max() == 1.0e4


@pytest.mark.parametrize("m,k", [(3, 256), (8, 512), (2, 1024), (3, 1536)])
def test_designed_activations_give_a_designable_row(oracle, m, k):
    """The x the GPU test gives tce_layernorm_q_w8a8_group: LayerNormQ (restatement == oracle) turns it into +-(one row) with magnitudes 96 .. 127 and the two reserved
    columns, and the families built against those rows keep their judged sets for the int8-bias, the fp32-bias and the ReLU linear."""
    x, lw, lb, p1, p127 = wc.designed_activations(m, k, 3)
    q, _ = wc.layernorm_q_exact(x, lw, lb)
    assert np.array_equal(q, oracle.layernorm_q(x, lw, lb)) and np.array_equal(q[1], -q[0].astype(np.int64)) and abs(q[0, p1]) == 1 and abs(q[0, p127]) == 127
    for family in ("round_ties", "clamp_edges", "separate_roundings"):
        for seed, kind in enumerate(("i8_bias", "f32_bias", "relu")):
            case = wc.build_case(family, m, 40, k, seed=seed, given=(q, {0: 1, 1: -1}, p1, p127))
            assert case.judged(kind).any() and np.array_equal(_bits(case.expected(kind)[0]), _bits(_oracle_out(oracle, case, kind)))
            if family == "separate_roundings" and kind != "relu":
                assert case.judged(kind).sum() >= 32


@pytest.mark.parametrize("heads,hd,m,pos,max_keys", [(2, 64, 3, 20, 64), (2, 128, 2, 37, 64), (3, 64, 1, 5, 16)])
def test_attention_tie_case_against_the_oracle_composition(oracle, heads, hd, m, pos, max_keys):
    """The decode step the GPU test gives tce_opt_attention_decode, through the oracle's composition (qk BMM, batch_Add + softmax + int8, pv BMM): both probabilities of
    every row are 64 (libm's expf(0) = 1 and expf of the masked difference = 0), and the attention rows are the exact reference's, at least a quarter of them exact ties."""
    a_qk, a_pv = wc.ATTENTION_SCALES
    q, k, v, kc0, vt0, mask, pairs, want, ties = wc.attention_tie_case(heads, hd, m, pos, max_keys)
    tgz = pos + m
    kc, vt = kc0.copy(), vt0.copy()
    for h in range(heads):  # the KV append
        kc[h, pos:tgz] = k[:, h * hd:(h + 1) * hd]
        vt[h, :, pos:tgz] = v[:, h * hd:(h + 1) * hd].T
    scores = np.stack([oracle.int8_matmul_nobias_f32(q[:, h * hd:(h + 1) * hd], kc[h, :tgz], a_qk, m, tgz, hd) for h in range(heads)])
    probs = oracle.opt_softmax_q(scores, mask)
    assert set(np.unique(probs)) == {0, 64} and np.all((probs == 64).sum(axis=2) == 2)
    for r, (c1, c2) in enumerate(pairs):
        assert np.all(probs[:, r, [c1, c2]] == 64) and c1 < pos <= c2
    out = np.concatenate([oracle.int8_matmul_nobias_i8(probs[h], np.ascontiguousarray(vt[h, :, :tgz]), a_pv, -128, 127, m, hd, tgz) for h in range(heads)], axis=1)
    assert np.array_equal(out, want) and ties >= m * heads * hd // 4 and want.min() == -128 and want.max() == 127
