"""Every W8A8 kernel form on the designed accumulators of tests/w8a8_cases.py (run with -m gpu on an MI355X; -s prints the judged elements compared per form and family).

The operands, the exact reference and the judged sets are w8a8_cases'; that the cases are sound and that they catch epilogues that are subtly wrong is
tests/test_w8a8_adversarial_host.py.  Here: every launch goes through the C ABI as tests/test_gpu_w8a8.py reaches it, capi.describe_w8a8_dispatch is asserted to name
the intended form before each launch, output buffers start as a canary (0x55 bytes for int8, NaN bits for fp32 -- under `accumulate` the columns behind N), the columns
behind N are asserted untouched, every switch is restored in a finally, and the comparison is np.array_equal on int8 and on fp32 bits: the contract is bit-exactness, so
there is no tolerance anywhere in this file.

A (form, family) cell that is known to mismatch would be listed in KNOWN_DEFECTS with its measured count, left out of its form's sweep and run by test_known_defect as a
strict expected failure that only a value mismatch (ValueMismatch) may cause.  The table is empty.

The copies of the epilogue outside w8a8_gemm.hip: tce_layernorm_q_w8a8_group (narrow and wide form) on activations that are LayerNormQ's own output from a designed x,
tce_layernorm_q alone on every branch of its dispatcher, and tce_opt_attention_decode on exact ties of its pv product (two equal scores -> both probabilities 64).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import w8a8_cases as wc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY8 = 0x55
CANARYF = np.uint32(0x7FC55555)  # a NaN

# (form name, family) -> mismatching elements measured on an MI355X.  EMPTY: every form gives the exact reference's bits on every family.
KNOWN_DEFECTS = {}


class ValueMismatch(Exception):
    """An output differs from the exact reference (an exception of its own: it is the only thing an expected failure below may stand for)."""


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from tinychatengine_amd import capi
    capi.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _nothing_more_after_a_device_error():
    """A value mismatch is a finding and the run goes on; a device error is not survivable: nothing more is launched in this session."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping the session: {e}", returncode=3)


def _t(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return x.view(np.uint8) if x.dtype == np.int8 else x.view(np.uint32)


@contextlib.contextmanager
def _switches(form):
    from tinychatengine_amd import capi
    L = capi.lib()
    try:
        capi.w8a8_set_tuning(*form.tuning)
        for mode in form.modes:
            capi.check(L.tce_w4a16_set_debug_mode(mode))
        yield
    finally:
        capi.w8a8_set_tuning()
        for mode in wc.RESTORE_MODES:
            L.tce_w4a16_set_debug_mode(mode)


def _compare(what, case, kind, got):
    want = case.expected(kind)[0]
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = _bits(got) != _bits(want)
    if bad.any():
        m, n = (int(i) for i in np.argwhere(bad)[0])
        raise ValueMismatch(f"{what}: {int(bad.sum())} of {bad.size} elements differ ({int((bad & case.judged(kind)).sum())} of them judged); first at ({m}, {n}): "
                            f"acc = {int(case.acc[m, n])}, v = {float(case.expected(kind)[1][m, n])!r}, got {got[m, n]!r}, want {want[m, n]!r}")
    return int(case.judged(kind).sum())


def _launch(dev, form, K, cases, kind):
    """One launch of `kind` on the batch entries `cases` through tce_w8a8_matmul (tce_w8a8_matmul_v2 with the scratch area for the forms that need one) -> [out per entry]."""
    from tinychatengine_amd import capi
    M, N, batch = form.M, form.N, form.batch
    c0 = cases[0]
    for c in cases[1:]:  # one launch: one alpha, one beta, one bias
        assert c.alpha == c0.alpha and c.beta == c0.beta and np.array_equal(c.bias8, c0.bias8) and np.array_equal(_bits(c.biasf), _bits(c0.biasf))
    lda, ldb, ldc = (form.ld[0] or K, form.ld[1] or K, form.ld[2] or N)
    rng = np.random.default_rng(K + N)
    A = rng.integers(-128, 128, (batch, M, lda)).astype(np.int8)  # (garbage behind K)
    for i, c in enumerate(cases):
        A[i, :, :K] = c.A
    if form.per_row:
        B = np.ascontiguousarray(c0.B)
    else:
        B = rng.integers(-128, 128, (batch, N, ldb)).astype(np.int8)
        for i, c in enumerate(cases):
            B[i, :, :K] = c.B
    fp32 = kind.startswith("f32")
    if fp32:
        C0 = np.full((batch, M, ldc), CANARYF, np.uint32).view(np.float32)
        if kind == "f32_acc":
            for i, c in enumerate(cases):
                C0[i, :, :N] = c.C0
    else:
        C0 = np.full((batch, M, ldc), CANARY8, np.uint8).view(np.int8)
    tA, tB, tC = _t(dev, A), _t(dev, B), _t(dev, C0)
    lo, hi = c0.bounds(kind)
    d = capi.W8A8Desc(M=M, N=N, K=K, batch=batch, A=tA.data_ptr(), B=tB.data_ptr(), C=tC.data_ptr(), strideA=M * lda, strideB=N * ldb, strideC=M * ldc,
                      alpha=c0.alpha, beta=c0.beta, q_min=lo, q_max=hi, bias_kind=capi.TCE_BIAS_NONE, out_kind=capi.TCE_OUT_FP32 if fp32 else capi.TCE_OUT_INT8,
                      b_per_row=1 if form.per_row else 0, accumulate=1 if kind == "f32_acc" else 0, lda=form.ld[0], ldb=form.ld[1], ldc=form.ld[2])
    keep = None
    if kind in ("i8_bias", "relu"):
        keep = _t(dev, c0.bias8)
        d.bias, d.bias_kind = keep.data_ptr(), capi.TCE_BIAS_INT8
    elif kind in ("f32_bias", "f32_acc"):
        keep = _t(dev, c0.biasf)
        d.bias, d.bias_kind = keep.data_ptr(), capi.TCE_BIAS_FP32
    if form.per_row:
        d.strideB = 0
    named = capi.describe_w8a8_dispatch(d, with_scratch=form.scratch)
    assert named == form.describe, f"{form.name}: the dispatcher would run '{named}', not '{form.describe}'"
    st = torch.cuda.current_stream().cuda_stream
    if form.scratch:
        capi.check(capi.w8a8_matmul_v2(d, st, capi.w8a8_scratch(dev).data_ptr()))
    else:
        capi.check(capi.w8a8_matmul(d, st))
    torch.cuda.synchronize()
    got = tC.cpu().numpy()
    if ldc > N:
        assert np.all(_bits(got[:, :, N:]) == (CANARYF if fp32 else CANARY8)), f"{form.name} {kind}: columns behind N were written"
    return [np.ascontiguousarray(got[i, :, :N]) for i in range(batch)]


def _sweep(dev, form, include_known=False, only=None):
    """Every family the form can express x every output kind; prints the judged elements compared per family, raises ValueMismatch on the first difference."""
    print(f"\n{form.name}  ({form.M} x {form.N}, K = {form.Ks}, batch {form.batch}): '{form.describe}'")
    judged = {}
    with _switches(form):
        for fam, K, off in form.cases():
            if only is not None and fam != only:
                continue
            if (form.name, fam) in KNOWN_DEFECTS and not include_known:
                continue
            cases = [wc.make_case(fam, form.M, form.N, K, b, form.per_row, off) for b in range(form.batch)]
            for kind in form.kinds():
                if kind not in cases[0].kinds:
                    continue
                outs = _launch(dev, form, K, cases, kind)
                for b, (case, got) in enumerate(zip(cases, outs)):
                    n = _compare(f"{fam} on {form.name}, K = {K}, {kind}, batch entry {b}, targets from {off}", case, kind, got)
                    judged[(fam, K)] = judged.get((fam, K), 0) + n
    for (fam, K), n in judged.items():
        print(f"    {fam:20s} K = {K:5d}: {n:6d} judged elements, all equal")
    known = [k[1] for k in KNOWN_DEFECTS if k[0] == form.name]
    if known and not include_known:
        print(f"    known defects, run by test_known_defect: {known}")
    assert judged or only is not None


@pytest.mark.parametrize("form", wc.FORMS, ids=[f.name.replace(" ", "_").replace(",", "") for f in wc.FORMS])
def test_form_on_the_designed_accumulators(dev, form):
    """One kernel form of launch_w8a8 (forced by its switches, named by the dispatcher) on every family it can express, six output kinds each."""
    _sweep(dev, form)


if KNOWN_DEFECTS:  # (no empty parameter set: pytest would report it as a skip)
    @pytest.mark.parametrize("name,family", [pytest.param(n, f, id=f"{n}-{f}", marks=pytest.mark.xfail(strict=True, raises=ValueMismatch, reason=f"open defect: {v} mismatching elements"))
                                             for (n, f), v in KNOWN_DEFECTS.items()])
    def test_known_defect(dev, name, family):
        _sweep(dev, next(f for f in wc.FORMS if f.name == name), include_known=True, only=family)


def test_switches_are_back_at_the_rules(dev):
    """After the sweeps: a launch the rules send to the k-slice form still goes there (a switch left on by a test above would name another form)."""
    from tinychatengine_amd import capi
    d = capi.W8A8Desc(M=70, N=100, K=1536, batch=1, A=4096, B=4096, C=4096, alpha=1.0, q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_NONE, out_kind=capi.TCE_OUT_INT8)
    with _switches(wc.FORMS[6]):
        assert capi.describe_w8a8_dispatch(d) == "w8a8 tile=64x64 quartets=1"
    assert capi.describe_w8a8_dispatch(d) == "w8a8 k-slice tile=32x48 waves=4 workgroups=9"
    assert capi.describe_w8a8_dispatch(d, with_scratch=True) == "w8a8 k-slice tile=32x48 waves=4 workgroups=9"


@pytest.mark.parametrize("family", ["round_ties", "clamp_edges"])
def test_matmul_operator_members_on_ties_and_clamp_edges(dev, family):
    """The MatmulOperator members, once each, at the shape the rules give them (70 x 100 x 1088 -> the k-slice form; 1 x 70 x 1536 for the over_column members; the *_batch
    members on a B per row)."""
    from tinychatengine_amd.matmul import MatmulOperator, matmul_params, matrix
    op = MatmulOperator()

    def run(member, case, kind):
        fp32 = kind.startswith("f32")
        out = torch.from_numpy((np.full((case.M, case.N), CANARYF, np.uint32).view(np.float32) if fp32 else np.full((case.M, case.N), CANARY8, np.uint8).view(np.int8))).to(dev)
        p = matmul_params(A=matrix(case.M, case.K, _t(dev, case.A)), B=matrix(case.K, case.N, _t(dev, case.B)), C=matrix(case.M, case.N, out), alpha=case.alpha, beta=case.beta)
        if kind in ("i8_bias", "relu"):
            p.bias = matrix(1, case.N, _t(dev, case.bias8))
        elif kind == "f32_bias":
            p.bias = matrix(1, case.N, _t(dev, case.biasf))
        p.C.qparams.q_min, p.C.qparams.q_max = case.bounds(kind)
        getattr(op, member)(p)
        torch.cuda.synchronize()
        return _compare(f"{family}: MatmulOperator.{member} ({kind})", case, kind, out.cpu().numpy())

    tiled, row, per_row = wc.make_case(family, 70, 100, 1088), wc.make_case(family, 1, 70, 1536), wc.make_case(family, 5, 9, 1536, 0, True)
    n = 0
    for member, case, kind in (("mat_mul_accelerator_int8_fast_2x2_32unroll", tiled, "i8_bias"), ("mat_mul_accelerator_int8_fast_2x2_32unroll", tiled, "relu"),
                               ("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias", tiled, "i8_nobias"), ("mat_mul_accelerator_int8_fast_32unroll_over_column", row, "i8_bias"),
                               ("mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32", tiled, "f32_bias"),
                               ("mat_mul_accelerator_int8_fast_2x2_32unroll_bfp32_ofp32_over_column", row, "f32_bias"),
                               ("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32", tiled, "f32_nobias"),
                               ("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_batch", per_row, "i8_nobias"),
                               ("mat_mul_accelerator_int8_fast_2x2_32unroll_nobias_ofp32_batch", per_row, "f32_nobias")):
        n += run(member, case, kind)
    print(f"\n{family}: {n} judged elements through the MatmulOperator members, all equal")


@pytest.mark.parametrize("m,k", [(3, 256), (8, 512), (2, 1024), (3, 1536)], ids=["narrow", "narrow-8-rows", "wide", "wide-24-steps"])
@pytest.mark.parametrize("family", ["round_ties", "clamp_edges", "separate_roundings"])
def test_layernorm_q_group_epilogues_on_designed_accumulators(dev, oracle, family, m, k):
    """tce_layernorm_q_w8a8_group (its own copy of the epilogue): the workgroup-per-8-rows form (k < 1024) and the weights-resident form (k >= 1024), an int8-bias, an
    fp32-bias and a ReLU linear in one launch, B designed against the rows LayerNormQ makes of a designed x."""
    from tinychatengine_amd import capi
    x, lw, lb, p1, p127 = wc.designed_activations(m, k, 3)
    q, _ = wc.layernorm_q_exact(x, lw, lb)
    assert np.array_equal(q, oracle.layernorm_q(x, lw, lb)), "the numpy restatement of LayerNormQ differs from the oracle"
    rows = {0: 1, 1: -1} if m > 1 else {0: 1}
    N = 40
    kinds = ("i8_bias", "f32_bias", "relu")
    cases = [wc.build_case(family, m, N, k, seed=i, given=(q, rows, p1, p127)) for i in range(3)]
    tx, tw, tb = _t(dev, x), _t(dev, lw), _t(dev, lb)
    ln_out = torch.full((m, k), CANARY8, dtype=torch.int8, device=dev)
    keep, outs, descs = [], [], []
    for case, kind in zip(cases, kinds):
        fp32 = kind == "f32_bias"
        out = torch.from_numpy(np.full((m, N), CANARYF, np.uint32).view(np.float32) if fp32 else np.full((m, N), CANARY8, np.uint8).view(np.int8)).to(dev)
        tB, tbias = _t(dev, case.B), _t(dev, case.biasf if fp32 else case.bias8)
        keep += [tB, tbias]
        outs.append(out)
        lo, hi = case.bounds(kind)
        descs.append(capi.W8A8Desc(M=m, N=N, K=k, batch=1, A=None, B=tB.data_ptr(), bias=tbias.data_ptr(), C=out.data_ptr(), alpha=case.alpha, beta=0.0 if fp32 else case.beta,
                                   q_min=lo, q_max=hi, bias_kind=capi.TCE_BIAS_FP32 if fp32 else capi.TCE_BIAS_INT8, out_kind=capi.TCE_OUT_FP32 if fp32 else capi.TCE_OUT_INT8))
    arr = (capi.W8A8Desc * 3)(*descs)
    capi.check(capi.lib().tce_layernorm_q_w8a8_group(tx.data_ptr(), tw.data_ptr(), tb.data_ptr(), m, k, arr, 3, C.c_void_p(ln_out.data_ptr()),
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(ln_out.cpu().numpy(), q), "the launch's LayerNormQ output is not the restatement's"
    n = 0
    for case, kind, out in zip(cases, kinds, outs):
        assert case.judged(kind).any()
        n += _compare(f"{family} through tce_layernorm_q_w8a8_group, m = {m}, k = {k}, {kind}", case, kind, out.cpu().numpy())
    print(f"\nlayernorm_q + linears, {family}, m = {m}, k = {k}: {n} judged elements, all equal")


@pytest.mark.parametrize("m,n,branch", [(6, 252, "one wave, prefetched parameters"), (1025, 1028, "one wave, parameters read behind the sums"), (6, 256, "4 waves"), (6, 1024, "16 waves")])
def test_layernorm_q_branches_on_designed_rows(dev, oracle, m, n, branch):
    """tce_layernorm_q on every branch of its dispatcher at the smallest m, n that reach it: constant rows, rows with one outlier, columns with w = 0 and b = j + 0.5 in
    both signs (exact ties of the final rounding, whatever the row), columns whose outputs lie beyond +-127 (the narrowing wraps like the reference's cast).  Bit-exact."""
    from tinychatengine_amd import capi
    x, w, b, want, f, cols = wc.layernorm_rows(m, n)
    assert np.array_equal(want, oracle.layernorm_q(x, w, b)), "the numpy restatement of LayerNormQ differs from the oracle"
    out = torch.full((m, n), CANARY8, dtype=torch.int8, device=dev)
    tx, tw, tb = _t(dev, x), _t(dev, w), _t(dev, b)
    capi.check(capi.lib().tce_layernorm_q(tx.data_ptr(), tw.data_ptr(), tb.data_ptr(), out.data_ptr(), m, n, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = got != want
    assert not bad.any(), f"{branch}: {int(bad.sum())} of {bad.size} outputs differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}: f = {float(f[tuple(np.argwhere(bad)[0])])!r}"
    print(f"\nlayernorm_q, {branch}: {m * cols.size} exact ties and {int((np.abs(f) > 128.5).sum())} wrapping outputs, all equal")


@pytest.mark.parametrize("heads,hd,m,pos,max_keys", [(2, 64, 3, 20, 64), (2, 128, 2, 37, 64), (3, 64, 1, 5, 16)])
def test_opt_attention_decode_on_exact_ties_of_the_pv_product(dev, oracle, heads, hd, m, pos, max_keys):
    """tce_opt_attention_decode and the pv BMM it fuses: every row sees two keys with equal scores (one from the cache, one appended by the launch; every other key carries
    the mask's lowest value), so both probabilities are exactly 0.5, both int8 probabilities 64, acc = 64 (v1 + v2), and with a_pv = 2^-7 every odd v1 + v2 is a tie of
    the final rounding -- from -127.5 (-> -128, the bound) to 126.5 (-> 127).  Asserted exactly against the exact reference, for the one launch and for the four it replaces."""
    from tinychatengine_amd import capi
    L = capi.lib()
    E, tgz = heads * hd, pos + m
    a_qk, a_pv = wc.ATTENTION_SCALES
    q, k, v, kc0, vt0, mask, pairs, want, ties = wc.attention_tie_case(heads, hd, m, pos, max_keys)
    tq, tk, tv, tm = _t(dev, q), _t(dev, k), _t(dev, v), _t(dev, mask)
    st = torch.cuda.current_stream().cuda_stream
    vp = lambda t: C.c_void_p(t.data_ptr())
    # the four launches
    kc_a, vt_a = _t(dev, kc0), _t(dev, vt0)
    capi.check(L.tce_opt_kv_append(vp(tk), vp(tv), vp(kc_a), vp(vt_a), heads, hd, m, pos, max_keys, C.c_void_p(st)))
    scores = torch.zeros((heads, m, tgz), dtype=torch.float32, device=dev)
    d = capi.W8A8Desc(M=m, N=tgz, K=hd, batch=heads, A=tq.data_ptr(), B=kc_a.data_ptr(), C=scores.data_ptr(), strideA=hd, strideB=max_keys * hd, strideC=m * tgz, lda=E, alpha=a_qk,
                      q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_NONE, out_kind=capi.TCE_OUT_FP32)
    capi.check(capi.w8a8_matmul(d, st))
    ldp = (tgz + 15) // 16 * 16
    probs = torch.zeros((heads, m, ldp), dtype=torch.int8, device=dev)
    capi.check(L.tce_opt_softmax_q(vp(scores), vp(tm), vp(probs), heads, m, tgz, ldp, C.c_void_p(st)))
    out_a = torch.full((m, E), CANARY8, dtype=torch.int8, device=dev)
    d = capi.W8A8Desc(M=m, N=hd, K=tgz, batch=heads, A=probs.data_ptr(), B=vt_a.data_ptr(), C=out_a.data_ptr(), strideA=m * ldp, strideB=hd * max_keys, strideC=hd, lda=ldp, ldb=max_keys,
                      ldc=E, alpha=a_pv, q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_NONE, out_kind=capi.TCE_OUT_INT8)
    capi.check(capi.w8a8_matmul(d, st))
    # the one launch
    kc_b, vt_b = _t(dev, kc0), _t(dev, vt0)
    out_b = torch.full((m, E), CANARY8, dtype=torch.int8, device=dev)
    capi.check(L.tce_opt_attention_decode(vp(tq), vp(tk), vp(tv), vp(kc_b), vp(vt_b), vp(tm), vp(out_b), heads, hd, m, pos, max_keys, 0, a_qk, a_pv, C.c_void_p(st)))
    torch.cuda.synchronize()
    got_probs = probs.cpu().numpy()[:, :, :tgz]
    want_probs = np.zeros((heads, m, tgz), np.int8)
    for r, (c1, c2) in enumerate(pairs):
        want_probs[:, r, [c1, c2]] = 64
    assert np.array_equal(got_probs, want_probs), "the int8 probabilities are not 64 / 64: the device's expf(0) is not 1, or expf of the masked difference is not 0"
    assert np.array_equal(got_probs, oracle.opt_softmax_q(scores.cpu().numpy(), mask))
    for name, got in (("the four launches", out_a.cpu().numpy()), ("tce_opt_attention_decode", out_b.cpu().numpy())):
        bad = got != want
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} attention outputs differ from the exact reference, first at {tuple(int(i) for i in np.argwhere(bad)[0])}"
    assert torch.equal(kc_a, kc_b) and torch.equal(vt_a, vt_b), "caches"
    print(f"\nopt attention decode, heads {heads} x {hd}, m = {m}, pos = {pos}: {ties} exact ties of the pv product, all equal")
