"""Every W4A16 kernel family on the designed operands of tests/w4a16_cases.py (run with -m gpu on an MI355X; -s prints the worst ratio per case).

The operands, the float64 reference, the judged sets and the bound (conftest.w4a16_close, unchanged, per activation row and judged set) are w4a16_cases'; that the
cases are sound and that they catch kernels that are subtly wrong is tests/test_w4a16_adversarial_host.py.  Here: every launch goes through the C ABI as the parity tests
reach it, capi.describe_dispatch is asserted to name the intended kernel, output buffers start as NaN, every switch is restored in a finally.

A (kernel, case) cell that is known to miss the bound would be listed in KNOWN_DEFECTS with its measured ratio, left out of its kernel's sweep and run by
test_known_defect as a strict expected failure that only the bound (BoundMissed) may cause.  The table is empty: the defect these tests found is fixed.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import w4a16_cases as wc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU (they must not silently pass without it)"
    from tinychatengine_amd import capi
    capi.lib()
    capi.set_gemv_config()
    capi.set_gemm_config()
    capi.set_gemv_i8()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case_cached(key):
    return wc.make_case(**dict(key))


def case_of(kw):
    """One case per argument set for the whole module: built, and its float64 reference computed, once."""
    return _case_cached(tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items() if v is not None)))


_LIN = {}  # the linear of the case in hand: uploaded (and packed) once for all the variants that run on it


def _lin(dev, case, prepack=False):
    from tinychatengine_amd.linear import Linear_half_int4
    key = (id(case.codes), id(case.s), prepack)
    if key not in _LIN:
        _LIN.clear()
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        lin = Linear_half_int4(t(case.qw.view(np.int32)), t(case.sc), t(case.zp.view(np.int32)), case.G)
        assert lin.zeros_are_8 == case.zeros_are_8
        _LIN[key] = (lin.prepack() if prepack else lin, case)  # (the case is held so that its ids stay its own)
    lin = _LIN[key][0]
    lin.zeros_are_8 = case.zeros_are_8
    return lin


class DispatchError(Exception):
    """The library would run another kernel than the test means to hold to the bound (not an AssertionError: an expected failure must not hide it)."""


def _forward(dev, lin, a, expect, flags=0):
    """One tce_w4a16_forward on a NaN-filled output.  expect: the words the dispatch must hold, the first of them at its start."""
    from tinychatengine_amd import capi
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = torch.full((a.shape[0], lin.out_features), float("nan"), dtype=torch.float16, device=dev)
    d = lin.desc(x, out, flags=flags)
    what = capi.describe_dispatch(d)
    expect = (expect,) if isinstance(expect, str) else tuple(expect)
    if not (any(what.startswith(e) for e in expect[0].split("|")) and all(e in what for e in expect[1:])):
        raise DispatchError(f"wanted {expect!r}, the library would run {what!r}")
    capi.check(capi.w4a16_forward(d, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- the kernel families: (dev, case, variant) -> output; `variants(shape)` lists what a family runs per case ----
def run_gemv(dev, case, variant):
    from tinychatengine_amd import capi
    cfg, promise = variant
    lin = _lin(dev, case)
    if not promise:
        lin.zeros_are_8 = False  # the zero points are read
    try:
        capi.set_gemv_config(*cfg)
        return _forward(dev, lin, case.a, f"gemv passes={(case.M + 3) // 4} kernel=row-block", flags=capi.TCE_W4_FORCE_GEMV)
    finally:
        capi.set_gemv_config()


def run_stream(dev, case, variant):
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import forward_group
    lin = _lin(dev, case)
    x = torch.from_numpy(case.a).to(dev)
    out = torch.full((case.M, case.N), float("nan"), dtype=torch.float16, device=dev)
    try:
        capi.set_gemv_config(variant[0], variant[1], 0, variant[2])
        what = capi.describe_dispatch(lin.desc(x, out))
        if what != "gemv passes=1 kernel=persistent":
            raise DispatchError(what)
        forward_group([lin], x, [out])
        torch.cuda.synchronize()
    finally:
        capi.set_gemv_config()
    return out.cpu().numpy()


def run_i8(dev, case, variant):
    from tinychatengine_amd import capi
    tiles, promise = variant
    lin = _lin(dev, case, prepack=True)
    if not promise:
        lin.zeros_are_8 = False
    try:
        capi.set_gemv_i8(0, tiles)
        return _forward(dev, lin, case.a, "gemv-i8")
    finally:
        capi.set_gemv_i8()


def run_skinny(dev, case, variant):
    from tinychatengine_amd import capi
    L = capi.lib()
    try:
        capi.check(L.tce_w4a16_set_debug_mode(variant))
        return _forward(dev, _lin(dev, case), case.a, "small-batch")
    finally:
        L.tce_w4a16_set_debug_mode(20)


def run_gemm(dev, case, variant):
    from tinychatengine_amd import capi
    try:
        capi.set_gemm_config(*(variant or (0, 0)))
        if variant is None:
            expect = "gemm-dma tile="
        else:  # tile ids 200 + m_tiles force the LDS-DMA GEMM, the others the older GEMM (100 + m_tiles: its second pipeline form)
            mt, nt = variant
            expect = f"gemm-dma tile={(mt - 200) * 16}x{nt * 64} " if mt >= 200 else f"gemm tile={(mt % 100) * 16}x{nt * 64}"
        return _forward(dev, _lin(dev, case), case.a, expect, flags=capi.TCE_W4_FORCE_GEMM)
    finally:
        capi.set_gemm_config()


PK_MODES = (61, 62, 63, 64, 66, 67, 672, 68, 2669, 2670, 2671, 2672, 2683, 2673, 2674, 2675, 2676, 60)  # the list of test_pk_gemm_matches_oracle


def _scratch_faults(dev):
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import gemm_scratch
    n = C.c_uint32(0)
    capi.check(capi.lib().tce_w4a16_gemm_scratch_faults(C.c_void_p(gemm_scratch(dev).data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(n)))
    return n.value


def _pk_expect(case, mode):
    """What the dispatch must say under a forced mode, as test_pk_gemm_matches_oracle asserts it: the wide forms run only on zero points that are all 8, groups of
    128 and more than 128 rows (other linears keep the narrow forms under these modes -- which is why the z = 8 cases are in this family's table)."""
    wide = case.zeros_are_8 and case.G == 128 and case.M > 128
    if mode == 60:  # automatic: the cost models of the two GEMMs decide
        return ("gemm-pk tile=|gemm-dma tile=",)
    want = ["gemm-pk tile="]
    if mode in (2670, 2671, 2672, 2683, 2675) and wide:
        want.append("wave=128x64")
    if mode in (2673, 2674) and wide:
        want.append("wave=128x48")
    if mode == 2676 and case.G == 128 and case.K >= 1024:
        want.append("quartets=2 ksplit=2")
    return want


def run_pk(dev, case, variant):
    from tinychatengine_amd import capi
    L = capi.lib()
    try:
        capi.check(L.tce_w4a16_set_debug_mode(variant))
        got = _forward(dev, _lin(dev, case, prepack=True), case.a, _pk_expect(case, variant))
        assert _scratch_faults(dev) == 0, f"mode {variant}: the k-cut exchange counted a fault"
        return got
    finally:
        L.tce_w4a16_set_debug_mode(60)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def run_awq(dev, case, variant):
    """tce_w4a16_gemm_awq: an entry point of its own, no dispatch to describe."""
    from tinychatengine_amd.matmul import MatmulOperator, matmul_params, matrix
    assert case.zeros_are_8
    oracle = _oracle()
    q5, s5, _ = oracle.pack_q4_5(case.codes, case.s.astype(np.float32).reshape(-1), case.N, case.K, case.G)
    assert np.array_equal(s5.view(np.uint16), np.ascontiguousarray(case.s.T).view(np.uint16)), "the AWQ scales are not the case's"
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = torch.full((case.M, case.N), float("nan"), dtype=torch.float16, device=dev)
    p = matmul_params(A=matrix(case.M, case.K, t(case.a)), B=matrix(case.K, case.N // 8, t(q5.view(np.int32))), C=matrix(case.M, case.N, out),
                      half_scales=t(s5.view(np.float16)), block_size=case.G)
    MatmulOperator().gemm_forward_cuda(p, 8)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _gemv_variants(shape):
    from tinychatengine_amd import capi
    return [(v, False) for v in capi.gemv_variants()]


def _gemm_variants(shape):
    from tinychatengine_amd import capi
    vs = capi.gemm_variants()
    return [None] + (vs if shape[3] == 128 else [])  # (groups of 64 / 32 have the LDS-DMA form only: a forced tile of the other GEMM is a GEMV launch, test_gemv_row_block's)


STREAM_CFGS = ((2, 16, 2), (2, 15, 3), (1, 16, 3), (1, 9, 2), (2, 4, 2), (1, 1, 2))  # test_stream_kernel_every_config's
FAMILIES = {
    "gemv": (run_gemv, _gemv_variants),
    "stream": (run_stream, lambda shape: list(STREAM_CFGS)),
    "i8": (run_i8, lambda shape: [(1, False), (2, False)]),
    "skinny": (run_skinny, lambda shape: [m for m in (20, 21, 22, 30) if not 20 < m < 30 or m - 20 <= shape[2] // 128]),
    "gemm": (run_gemm, _gemm_variants),
    "pk": (run_pk, lambda shape: list(PK_MODES)),
    "awq": (run_awq, lambda shape: [None]),
}

# (kernel family, shape, case label) -> the worst ratio measured on an MI355X: a cell that is known to miss the bound.  The sweeps leave such a cell out and
# test_known_defect runs it as a strict expected failure.  EMPTY: the one defect these tests found -- the zero point removed algebraically, in fp32, by the kernels that
# unpack to halves (row-block / stream / overlap GEMV, skinny, and through it the AWQ entry: 1.8 - 376 times the bound on `dc x balanced`, `outlier x null_at_outlier`
# and `mixed_rows`) -- is fixed in the kernels; every cell is back in its sweep.
KNOWN_DEFECTS = {}


class BoundMissed(Exception):
    """A kernel's worst |err| / bound is past 1 (an exception of its own: it is the only thing an expected failure below may stand for)."""


def _sweep(dev, family, shape, cases, extra_variants=None, include_known=False):
    """Every case x every variant of the family; prints the worst ratio per case, then asserts.  Returns {label: (ratio, variant)}."""
    from tinychatengine_amd import capi
    run, variants = FAMILIES[family]
    vs = variants(shape)
    worst, refused = {}, set()
    for label, kw in cases:
        if (family, shape, label) in KNOWN_DEFECTS and not include_known:
            continue
        case = case_of(kw)
        todo = list(vs) + (extra_variants(case) if extra_variants else [])
        w, ran = (-1.0, None), 0
        for v in todo:
            try:
                got = run(dev, case, v)
            except capi.TceError as e:
                if e.code == capi.TCE_ERR_UNSUPPORTED_SHAPE or "no kernel variant for this shape" in str(e):
                    refused.add(str(v))  # a forced geometry that has no kernel for this shape: refused loudly, nothing ran
                    continue
                raise
            ran += 1
            r = wc.judge(case, got)
            if r > w[0]:
                w = (r, v)
        assert ran, f"{family} {shape} {label}: no variant ran"
        worst[label] = w
    print(f"\n{family} {shape}" + (f"  (refused by the library, nothing ran: {sorted(refused)})" if refused else ""))
    for label, (r, v) in worst.items():
        print(f"    {label:60s} {r:10.3f}   worst at {v}")
    skipped = [k[2] for k in KNOWN_DEFECTS if k[0] == family and k[1] == shape]
    if skipped and not include_known:
        print(f"    known defects, run by test_known_defect: {skipped}")
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    if bad:
        raise BoundMissed(f"{family} {shape}: worst |err| / bound past 1.0 on {bad}")
    return worst


_EXTRA = {"gemv": lambda case: [((0, 0, 0, 0), True)] if case.zeros_are_8 else [],  # the all-8 promise on the cases that can make it
          "i8": lambda case: [(1, True), (2, True)] if case.zeros_are_8 else []}


def _family(dev, family, shape, include_known=False, only=None):
    cases = [c for c in wc.family_cases(family, shape) if only is None or c[0] == only]
    assert cases
    return _sweep(dev, family, shape, cases, extra_variants=_EXTRA.get(family), include_known=include_known)


@pytest.mark.parametrize("shape", wc.GEMV_SHAPES, ids=str)
def test_gemv_row_block(dev, shape):
    """Every compiled geometry under TCE_W4_FORCE_GEMV with the zero points read; the cases whose zero points are 8 also with the all-8 promise (automatic geometry)."""
    _family(dev, "gemv", shape)


@pytest.mark.parametrize("shape", wc.STREAM_SHAPES, ids=str)
def test_stream_kernel(dev, shape):
    _family(dev, "stream", shape)


@pytest.mark.parametrize("shape", wc.I8_SHAPES, ids=str)
def test_i8_gemv(dev, shape):
    """One and two tiles per wave with the zero points read; the all-8 promise on the cases that can make it; the outlier in the first and in the last wave's block."""
    _family(dev, "i8", shape)


@pytest.mark.parametrize("shape", wc.SKINNY_SHAPES, ids=str)
def test_skinny_kernel(dev, shape):
    _family(dev, "skinny", shape)


@pytest.mark.parametrize("shape", wc.GEMM_SHAPES, ids=str)
def test_prefill_gemms(dev, shape):
    """Automatic (the LDS-DMA GEMM) and every compiled tile of both GEMMs under TCE_W4_FORCE_GEMM, each asserted by its tile in the dispatch."""
    _family(dev, "gemm", shape)


@pytest.mark.parametrize("shape", wc.PK_SHAPES, ids=str)
def test_packed_gemm(dev, shape):
    """Every form of the pre-packed GEMM: the rescale chain on `scale_ladder`, rows of one tile 2^22 apart on `mixed_rows`, partial accumulators in different units
    through the two-quartet join and the k-cut hand-off; no exchange may count a fault.  The wide forms (128 x 64 / 128 x 48 per wave) take only linears whose zero
    points are all 8: `random`, `scale_ladder`, `null_at_outlier` and both `mixed_rows` run a second time with z = 8, and the form is asserted in the dispatch."""
    _family(dev, "pk", shape)


@pytest.mark.parametrize("shape", wc.AWQ_SHAPES, ids=str)
def test_awq_layout_gemm(dev, shape):
    """tce_w4a16_gemm_awq on the cases whose zero points are 8: the two pairs that have them by design and the families built with z = 8."""
    _family(dev, "awq", shape)


def _known_params():
    cells = {}
    for (family, shape, label), v in KNOWN_DEFECTS.items():
        cells.setdefault((family, label), []).append((shape, v))
    return [pytest.param(family, label, tuple(s for s, _ in sv), id=f"{family}-{label}",
                         marks=pytest.mark.xfail(strict=True, raises=BoundMissed, reason="open defect (DESIGN.md 4.2): worst |err| / bound " + ", ".join(f"{v} at {s}" for s, v in sv)))
            for (family, label), sv in cells.items()]


if KNOWN_DEFECTS:  # (no empty parameter set: pytest would report it as a skip)
    @pytest.mark.parametrize("family,label,shapes", _known_params())
    def test_known_defect(dev, family, label, shapes):
        """One (kernel, case) cell of KNOWN_DEFECTS on every shape it is listed for.  Expected to fail by the BOUND only (raises=BoundMissed: an assertion of the harness is an AssertionError, another dispatch a
        DispatchError, a refusal a TceError -- neither counts), and on EVERY listed shape: a shape that comes to pass is reported, so that it goes back to its sweep."""
        passed = []
        for shape in shapes:
            try:
                _family(dev, family, shape, include_known=True, only=label)
                passed.append(shape)
            except BoundMissed:
                pass
        if passed and len(passed) < len(shapes):
            raise RuntimeError(f"{family} {label}: meets the bound on {passed} now -- take those shapes out of KNOWN_DEFECTS")
        if not passed:
            raise BoundMissed(f"{family} {label}: misses the bound on every listed shape")  # (all of them pass: the strict mark reports it)


NONFINITE = [("gemv", (4, 40, 1408, 64), ((0, 0, 0, 0), False)), ("i8", (2, 72, 4096, 64), (0, False)), ("i8", (4, 72, 4096, 128), (0, False)), ("i8", (1, 72, 4096, 128), (1, False)), ("i8", (1, 72, 4096, 128), (2, False)),
             ("stream", (1, 72, 4096, 128), (2, 16, 2)), ("skinny", (5, 40, 256, 128), 20), ("awq", (4, 136, 1024, 128), None),
             ("gemm", (33, 200, 1024, 128), None), ("gemm", (70, 136, 512, 32), None), ("pk", (200, 136, 384, 128), 61), ("pk", (260, 300, 1408, 128), 2676)]


@pytest.mark.parametrize("family,shape,variant", NONFINITE, ids=lambda v: str(v))
def test_nonfinite_activation_poisons_its_row_only(dev, family, shape, variant):
    """An inf, then a NaN, at one k of one activation row: every output of that row is non-finite, every other row is bit-identical to the launch without it."""
    case, row, k = wc.nonfinite_case(*shape, z8=family == "awq")
    run = FAMILIES[family][0]
    clean = run(dev, case, variant)
    assert wc.judge(case, clean) <= 1.0
    for bad in (np.float16("inf"), np.float16("nan")):
        c2 = case.with_rows(case.M)
        c2.a[row, k] = bad
        got = run(dev, c2, variant)
        assert not np.isfinite(got[row].astype(np.float32)).any(), f"{family} {shape}: {bad} at [{row}][{k}] left finite outputs in its row"
        others = np.delete(np.arange(case.M), row)
        assert np.array_equal(got[others].view(np.uint16), clean[others].view(np.uint16)), f"{family} {shape}: {bad} in row {row} changed another row"


def test_token_kernel_plan(dev):
    """The persistent token kernel has a conversion of its own (csrc/w4a16_gemv_i8_token.hip): one two-launch plan on outlier x null_at_outlier and ladder x scale_ladder
    operands (zero points 8: the kernel takes no others), TCE_PLAN_TAGGED against the stream-ordered plan bit for bit, both against float64."""
    from tinychatengine_amd import capi
    M, N, K, G = wc.TOKEN_SHAPE
    cases = [case_of(kw) for kw in wc.TOKEN_CASES]
    lins = [_lin(dev, c, prepack=True) for c in cases]
    xs = [torch.from_numpy(c.a).to(dev) for c in cases]
    outs = [torch.full((M, N), float("nan"), dtype=torch.float16, device=dev) for _ in cases]
    launches = [[l.desc(x, o)] for l, x, o in zip(lins, xs, outs)]
    for d in launches:
        assert capi.describe_dispatch(d[0]).startswith("gemv-i8"), capi.describe_dispatch(d[0])
    plain, tok = capi.Plan(launches), capi.Plan(launches, tagged=True)
    try:
        assert tok.kind == 4 and tok.tagged and not plain.chained and tok.geometry()["rows"] == len(launches), (tok.kind, tok.geometry())
        s = torch.cuda.current_stream().cuda_stream
        res = []
        for plan in (plain, tok):
            for o in outs:
                o.fill_(float("nan"))
            plan.launch(s)
            plan.status()
            torch.cuda.synchronize()
            res.append([o.cpu().numpy().copy() for o in outs])
        print("\ntoken kernel plan")
        for c, a, b in zip(cases, *res):
            ra, rb = wc.judge(c, a), wc.judge(c, b)
            print(f"    {c.name:60s} stream-ordered {ra:8.3f}   tagged {rb:8.3f}")
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), f"{c.name}: the token kernel differs from the stream-ordered plan"
            assert ra <= 1.0 and rb <= 1.0, (c.name, ra, rb)
    finally:
        plain.close()
        tok.close()
