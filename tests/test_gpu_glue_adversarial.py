"""The glue between the W4A16 linears -- RMSNorm in its six places, SiLU*mul and the residual add stand-alone and as epilogues -- on the designed rows of
tests/glue_cases.py (run with -m gpu on an MI355X; -s prints the worst ratio per case).

The rows, the float64 references, the bound (0.5 + M_MARGIN) ulp16 and the ambiguous set are glue_cases'; that they are sound and that they catch wrong kernels is
tests/test_glue_adversarial_host.py.  Here: every launch goes through the C ABI as the parity tests reach it, capi.describe_dispatch is asserted to name the intended
kernel wherever a form is forced, output buffers start as NaN, every switch is restored in a finally.  The existing "<= 1 step, < 8 %" tests stay as they are: this
bound stands beside them.

A (kernel, case) cell that is known to miss its check would be listed in KNOWN_DEFECTS with what was measured and run as a strict expected failure that only the
check itself (CheckMissed) may cause -- the protocol of tests/test_gpu_w4a16_adversarial.py.  The table is empty.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import glue_cases as gc
import w4a16_cases as wc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (kernel form, K, row) -> what was measured on an MI355X: a cell that is known to miss its check.  The sweep leaves such a cell out and test_known_defect runs it as a
# strict expected failure.  EMPTY: the two defects these tests found -- the sign of an exactly zero output of the packed GEMM, and the int8-contraction GEMV's NORM
# prologue on a row that holds a NaN at a K with a ragged last wave -- are fixed in the kernels.
KNOWN_DEFECTS = {}


class CheckMissed(Exception):
    """A kernel's output is outside the bound / is not the reference's bits (an exception of its own: the only thing an expected failure may stand for)."""


class DispatchError(Exception):
    """The library would run another kernel than the test means to check."""


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU (they must not silently pass without it)"
    from tinychatengine_amd import capi
    capi.lib()
    capi.set_gemv_config()
    capi.set_gemm_config()
    capi.set_gemv_i8()
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16)


def _expect(desc, *words):
    """describe_dispatch must start with one of words[0].split('|') and hold the other words."""
    from tinychatengine_amd import capi
    what = capi.describe_dispatch(desc)
    if not (any(what.startswith(w) for w in words[0].split("|")) and all(w in what for w in words[1:])):
        raise DispatchError(f"wanted {words!r}, the library would run {what!r}")
    return what


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# tce_rmsnorm_half: every family x width x eps against float64
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _rmsnorm(dev, x16, gamma32, eps):
    from tinychatengine_amd.linear import rmsnorm_half
    x = _t(dev, x16)
    out = _nan(dev, *x.shape)
    rmsnorm_half(x, _t(dev, gamma32), eps, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("eps", gc.EPS_VALUES)
@pytest.mark.parametrize("n", gc.WIDTHS)
def test_rmsnorm_half(dev, n, eps):
    """Launches of one row and of three rows of different families; a row's bits must not depend on its neighbours."""
    worst, alone = {}, {}
    for L in gc.rms_launches(n, eps):
        got = _rmsnorm(dev, L.x, L.gamma, eps)
        for f, r in L.judge(got).items():
            worst[f] = max(worst.get(f, 0.0), r)
        for r, row in enumerate(L.rows):
            key = (row, L.x[r].tobytes(), L.gamma.tobytes())
            if L.m == 1:
                alone[key] = got[0]
            elif key in alone and not np.array_equal(alone[key].view(np.uint16), got[r].view(np.uint16)):
                raise CheckMissed(f"n = {n}: row {r} of '{L.label}' differs from the same row launched alone")
    print(f"\ntce_rmsnorm_half n = {n} eps = {eps:g}")
    for f in gc.RMS_FAMILIES:
        print(f"    {f:16s} worst ratio {worst[f]:.4f}   margin used {gc.margin_used(worst[f]):+.3f}")
    bad = {f: r for f, r in worst.items() if not r <= 1.0}
    if bad:
        raise CheckMissed(f"tce_rmsnorm_half n = {n} eps = {eps:g}: past (0.5 + 2^-8) ulp16 of float64 on {bad}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the fused RMSNorm prologues: bit for bit tce_rmsnorm_half followed by the same linear without prologue
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
FUSED_WIDTHS = tuple(n for n in gc.WIDTHS if n % 128 == 0 and n <= 16384)  # (520, 8200 and 24584 are no multiple of a group: no linear has such a K)
ROW_BLOCK_CFGS = (None, (2, 4, 1, 2), (4, 4, 1, 1), (1, 2, 2, 1), (2, 2, 2, 2), (1, 2, 4, 1))  # test_rmsnorm_prologue_fused's forced geometries
PERSISTENT_CFGS = ((2, 8, 0, 2), (1, 16, 0, 3), (4, 16, 0, 2))
I8_TILES = (0, 1, 2)
GROUPS = ((72,), (72, 264), (72, 264, 72))


@functools.lru_cache(maxsize=None)
def _fused_rows(K, eps):
    rows = [(f, None) for f in ("gauss", "eps_rules", "zeros", "all_max", "wide", "saturate", "negative_gamma")]
    rows += [("one_hot", (K - 1, gc.ONE_HOT_MAGS[0])), ("one_hot", (min(8192, K - 8), gc.ONE_HOT_MAGS[1])), ("nonfinite", "+inf"), ("nonfinite", "-inf"), ("nonfinite", "nan")]
    return [gc.rms_row_launch(f, K, eps, v) for f, v in rows]


@pytest.fixture(scope="module")
def norm_linears(dev):
    """Per K: three small linears (N = 72, 264, 72) and an interleaved gate/up pair (2 x 72 rows), plain and with packed copies -- built once."""
    from tinychatengine_amd.linear import Linear_half_int4
    cache = {}

    def get(K):
        if K not in cache:
            g = torch.Generator(device=dev).manual_seed(K)
            mk = lambda n: Linear_half_int4.from_float(torch.empty(n, K, device=dev).normal_(0, 0.05, generator=g))
            plain = [mk(n) for n in GROUPS[2]]
            pair = Linear_half_int4.interleave(mk(72), mk(72))
            clone = lambda l: Linear_half_int4(l.weight, l.scale, l.zero_point, l.group_size).prepack()
            cache[K] = dict(plain=plain, pair=pair, packed=[clone(l) for l in plain], packed_pair=clone(pair))
        return cache[K]
    return get


def _prologue_case(dev, lins, L, flags, expect):
    """One fused launch (grouped where len(lins) > 1) against tce_rmsnorm_half + the same launch without prologue; returns the number of differing outputs."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import forward_group_rmsnorm, rmsnorm_half
    x, gamma = _t(dev, L.x), _t(dev, L.gamma)
    width = lambda l: l.out_features // 2 if flags & capi.TCE_W4_SILU_MUL_PAIRS else l.out_features
    fused = [_nan(dev, 1, width(l)) for l in lins]
    two = [_nan(dev, 1, width(l)) for l in lins]
    for l, o in zip(lins, fused):
        _expect(l.desc(x, o, flags=flags, gamma=gamma, eps=L.eps), *expect)
    if len(lins) > 1:
        assert not flags
        forward_group_rmsnorm(lins, x, fused, gamma, L.eps)
    else:
        capi.check(capi.w4a16_forward(lins[0].desc(x, fused[0], flags=flags, gamma=gamma, eps=L.eps), _stream()))
    xn = rmsnorm_half(x, gamma, L.eps)
    if len(lins) > 1:
        plain = [l.desc(xn, o) for l, o in zip(lins, two)]
        for d in plain:
            _expect(d, *expect)
        capi.check(capi.w4a16_forward_group(plain, _stream()))
    else:
        _expect(lins[0].desc(xn, two[0], flags=flags), *expect)
        capi.check(capi.w4a16_forward(lins[0].desc(xn, two[0], flags=flags), _stream()))
    torch.cuda.synchronize()
    return sum(int((_bits(a) != _bits(b)).sum().item()) for a, b in zip(fused, two))


def _prologue_sweep(dev, K, form, cfgs, lins_of, pair_of, expect, set_cfg, reset_cfg, only_known=False):
    """Every row x eps x geometry x (groups of 1, 2, 3 linears; the interleaved pair with TCE_W4_SILU_MUL_PAIRS).  A row listed in KNOWN_DEFECTS for (form, K) is left
    out, or -- only_known -- is the only one run."""
    from tinychatengine_amd import capi
    worst, ran, refused, differ, rows = {}, 0, set(), {}, 0
    try:
        for eps in gc.EPS_VALUES:
            for L in _fused_rows(K, eps):
                if ((form, K, L.label) in KNOWN_DEFECTS) != only_known:
                    continue
                rows += 1
                fam = L.rows[0][0]
                # the stand-alone kernel on this very row against float64 (once per row)
                worst[fam] = max(worst.get(fam, 0.0), gc.rmsnorm_ratio(_rmsnorm(dev, L.x, L.gamma, eps)[0], L.reference()[0]))
                for cfg in cfgs:
                    set_cfg(cfg)
                    for lins, flags in [(lins_of(len(g)), 0) for g in GROUPS] + [([pair_of()], capi.TCE_W4_SILU_MUL_PAIRS)]:
                        try:
                            d = _prologue_case(dev, lins, L, flags, expect)
                        except capi.TceError as e:
                            if e.code == capi.TCE_ERR_UNSUPPORTED_SHAPE or "no kernel variant for this shape" in str(e):
                                refused.add(str(cfg))  # a forced geometry that has no kernel for this K: refused loudly, nothing ran
                                continue
                            raise
                        ran += 1
                        if d:
                            differ[(L.label, eps, str(cfg), len(lins), flags)] = d
    finally:
        reset_cfg()
    print(f"\nfused RMSNorm prologue, {form}, K = {K}: {ran} launches" + (f"  (refused by the library, nothing ran: {sorted(refused)})" if refused else ""))
    for f, r in worst.items():
        print(f"    {f:16s} tce_rmsnorm_half on the row: worst ratio {r:.4f}")
    known = [k[2] for k in KNOWN_DEFECTS if k[:2] == (form, K)]
    if known and not only_known:
        print(f"    known defects, run by test_known_defect: {known}")
    assert rows and ran >= rows * 4, f"{form} K = {K}: only {ran} launches ran on {rows} rows"
    assert all(r <= 1.0 for r in worst.values()), worst
    if differ:
        raise CheckMissed(f"{form} K = {K}: fused prologue != tce_rmsnorm_half + plain launch on {len(differ)} launches, e.g. {list(differ.items())[:6]}")


@pytest.mark.parametrize("K", FUSED_WIDTHS)
def test_rmsnorm_prologue_row_block(dev, norm_linears, K):
    from tinychatengine_amd import capi
    ls = norm_linears(K)
    _prologue_sweep(dev, K, "row-block GEMV", ROW_BLOCK_CFGS, lambda c: ls["plain"][:c], lambda: ls["pair"], ("gemv passes=1 kernel=row-block",),
                    lambda cfg: capi.set_gemv_config(*(cfg or (0, 0, 0, 0))), capi.set_gemv_config)


@pytest.mark.parametrize("K", FUSED_WIDTHS)
def test_rmsnorm_prologue_persistent(dev, norm_linears, K):
    from tinychatengine_amd import capi
    ls = norm_linears(K)
    _prologue_sweep(dev, K, "persistent GEMV", PERSISTENT_CFGS, lambda c: ls["plain"][:c], lambda: ls["pair"], ("gemv passes=1 kernel=persistent",),
                    lambda cfg: capi.set_gemv_config(*cfg), capi.set_gemv_config)


@pytest.mark.parametrize("K", FUSED_WIDTHS)
def test_rmsnorm_prologue_i8(dev, norm_linears, K):
    """The NORM form of the int8-contraction GEMV on packed copies (its clamp is one v_med3_f32: `saturate` is the comparison that tells it from rmsnorm_out; K = 4096
    and 8192 take its fast branch, 11008 and 16384 the general one).  The `nonfinite` rows stay in: the kernel's row poisoning looks at the NORMALISED row, which is
    finite (a NaN product is clamped to -64504), on both sides of the comparison.  K = 11008 is the one K here whose last wave is ragged: its chunks past K
    must stay zero on a NaN row too (they did not: DESIGN.md 4.5)."""
    _i8_prologue(dev, norm_linears, K)


def _i8_prologue(dev, norm_linears, K, only_known=False):
    from tinychatengine_amd import capi
    ls = norm_linears(K)
    _prologue_sweep(dev, K, "int8-contraction GEMV", I8_TILES, lambda c: ls["packed"][:c], lambda: ls["packed_pair"], ("gemv-i8",),
                    lambda t: capi.set_gemv_i8(0, t), capi.set_gemv_i8, only_known=only_known)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# tce_w4a16_forward_residual_rmsnorm (RNORM): the residual row against the exact add, the normalised row against float64 on the row read back
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _one_hot_linear(dev, oh, prepack):
    from tinychatengine_amd.linear import Linear_half_int4
    qw, sc, zp = wc.pack_q4_6(oh.codes, oh.z, oh.s, oh.G)
    lin = Linear_half_int4(_t(dev, qw.view(np.int32)), _t(dev, sc), _t(dev, zp.view(np.int32)), oh.G)
    assert lin.zeros_are_8
    return lin.prepack() if prepack else lin


RNORM_ROWS = [(f, None) for f in ("gauss", "eps_rules", "zeros", "all_max", "wide", "saturate", "negative_gamma")] + [("nonfinite", k) for k in gc.NONFINITE_KINDS]


@pytest.mark.parametrize("N", [264, 4096, 8200, 16384])  # (8200: N % 16 = 8, a ragged last tile, and one piece in the second round of slots)
def test_residual_rmsnorm_epilogue(dev, N):
    """One-hot activations make the linear's output exact, so the row after the residual add is known in advance and lands in each family.  Every (family, eps) is a
    launch of its own on ONE workspace, one after the other: the counter must be back at zero after each.  eps travels as a bit-cast here: both values are run."""
    from tinychatengine_amd import capi
    K, G = 256, 128
    ws = torch.zeros(int(capi.lib().tce_w4a16_residual_rmsnorm_workspace_bytes()), dtype=torch.uint8, device=dev)
    rows = RNORM_ROWS + [("one_hot", (p, m)) for p, m in ((0, gc.ONE_HOT_MAGS[1]), (N - 1, gc.ONE_HOT_MAGS[0]), (min(8192, N - 8), gc.ONE_HOT_MAGS[0]))]
    worst, wrong_c = {}, []
    for fam, variant in rows:
        for eps in gc.EPS_VALUES:
            y, res, c_want, gamma = gc.rnorm_operands(fam, N, eps, variant)
            oh = gc.OneHotLinear(1, N, K, G, lambda g: y if g == 0 else gc.h16(np.ones(N)))
            assert np.array_equal(oh.y[0].view(np.uint16), y.view(np.uint16))
            lin = _one_hot_linear(dev, oh, prepack=True)
            x, c, gm, xn = _t(dev, oh.a), _t(dev, res[None, :]), _t(dev, gamma), _nan(dev, 1, N)
            d = lin.desc(x, c, flags=capi.TCE_W4_ADD_TO_C)
            _expect(d, "gemv-i8")
            capi.check(capi.w4a16_forward_residual_rmsnorm(d, gm.data_ptr(), eps, xn.data_ptr(), ws.data_ptr(), _stream()))
            torch.cuda.synchronize()
            assert int(ws.view(torch.int32)[2048].item()) == 0, f"{fam} eps = {eps:g}: the workspace counter did not return to zero"
            c_got, xn_got = c.cpu().numpy()[0], xn.cpu().numpy()
            if not gc.same_half(c_got, c_want).all():
                wrong_c.append((fam, variant, eps, int((~gc.same_half(c_got, c_want)).sum())))
            worst[fam] = max(worst.get(fam, 0.0), gc.rmsnorm_ratio(xn_got, gc.rmsnorm_ref(c_got[None, :], gamma, eps)))
    print(f"\ntce_w4a16_forward_residual_rmsnorm N = {N}")
    for f, r in worst.items():
        print(f"    {f:16s} worst ratio {r:.4f}   margin used {gc.margin_used(r):+.3f}")
    if wrong_c:
        raise CheckMissed(f"N = {N}: the residual row is not the exact binary16 sum on {wrong_c}")
    bad = {f: r for f, r in worst.items() if not r <= 1.0}
    if bad:
        raise CheckMissed(f"N = {N}: the normalised row is past (0.5 + 2^-8) ulp16 of float64 on {bad}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# tce_silu_mul_half and tce_add_half stand-alone
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 3])
def test_silu_mul_half_every_gate(dev, tail):
    """All 65536 gate patterns against the nine up values, one launch of 9 * 65536 elements (less 3: the kernel's scalar tail)."""
    from tinychatengine_amd import capi
    g, u = gc.silu_operands(tail)
    ref, alt = gc.silu_mul_ref(g, u)
    a, b = _t(dev, g), _t(dev, u)
    capi.check(capi.lib().tce_silu_mul_half(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_longlong(g.size), C.c_void_p(_stream())))
    torch.cuda.synchronize()
    got = a.cpu().numpy()
    bad = gc.silu_mismatches(got, ref, alt)
    amb = gc.ambiguous_gates(g)
    took_alt = int((~gc.same_half(got, ref) & amb).sum())
    print(f"\ntce_silu_mul_half n = {g.size}: {bad.size} elements differ from the reference; {took_alt} of the {int(amb.sum())} ambiguous elements took the other neighbour of e")
    if bad.size:
        raise CheckMissed(f"{bad.size} elements differ, e.g. (gate bits, up, got, want) " + str([(hex(int(g.view(np.uint16)[i])), float(u[i]), float(got[i]), float(ref[i])) for i in bad[:8]]))


@pytest.mark.parametrize("n", [65536, 65536 - 5])
def test_add_half_designed_pairs(dev, n):
    from tinychatengine_amd import capi
    a, b, where = gc.add_operands()
    a, b = a[:n], b[:n]
    ref = gc.add_ref(a, b)
    ta, tb, tc = _t(dev, a), _t(dev, b), _nan(dev, n)
    capi.check(capi.lib().tce_add_half(C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()), C.c_void_p(tc.data_ptr()), C.c_longlong(n), C.c_void_p(_stream())))
    torch.cuda.synchronize()
    bad = np.flatnonzero(~gc.same_half(tc.cpu().numpy(), ref))
    print(f"\ntce_add_half n = {n}: {bad.size} elements differ from the exact sum")
    if bad.size:
        raise CheckMissed(f"{bad.size} elements differ; designed pairs hit: {sorted(k for k, i in where.items() if np.intersect1d(i, bad).size)}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the pair and residual epilogues of every GEMV / GEMM family on designed values
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _even(shape):
    M, N, K, G = shape
    return (M, N + N % 2, K, G)


def _epilogue_check(dev, name, shape, prepack, expect, setup=None, restore=None, force=0):
    """The unfused launch must give the designed values exactly (one product each); the pair epilogue must equal the SiLU*mul reference on them (outside the ambiguous
    set: either neighbour), the residual epilogue the exact add."""
    from tinychatengine_amd import capi
    M, N, K, G = shape
    oh = gc.OneHotLinear(M, N, K, G, lambda g: gc.epilogue_values(N, shift=7 * g))
    lin = _one_hot_linear(dev, oh, prepack)
    x = _t(dev, oh.a)
    res = np.stack([gc.residual_for(oh.y[r], shift=r) for r in range(M)])
    try:
        if setup:
            setup()
        outs = {}
        for what, flags in (("plain", 0), ("pairs", capi.TCE_W4_SILU_MUL_PAIRS), ("add", capi.TCE_W4_ADD_TO_C)):
            out = _t(dev, res) if what == "add" else _nan(dev, M, N // 2 if what == "pairs" else N)
            d = lin.desc(x, out, flags=flags | force)
            _expect(d, *(expect(what) if callable(expect) else expect))
            capi.check(capi.w4a16_forward(d, _stream()))
            torch.cuda.synchronize()
            outs[what] = out.cpu().numpy()
    finally:
        if restore:
            restore()
    return _epilogue_judge(name, shape, oh, res, outs)


def _epilogue_judge(name, shape, oh, res, outs):
    miss = []
    if not np.array_equal(outs["plain"].view(np.uint16), oh.y.view(np.uint16)):
        i = np.argwhere(outs["plain"].view(np.uint16) != oh.y.view(np.uint16))
        miss.append(f"the unfused outputs are not the designed products at {len(i)} places, e.g. {[(tuple(j), float(outs['plain'][tuple(j)]), float(oh.y[tuple(j)])) for j in i[:4]]}")
    ref, alt = gc.silu_mul_ref(oh.y[:, 0::2], oh.y[:, 1::2])
    bad = gc.silu_mismatches(outs["pairs"].ravel(), ref.ravel(), alt.ravel())
    if bad.size:
        g, u = oh.y[:, 0::2].ravel(), oh.y[:, 1::2].ravel()
        miss.append(f"pair epilogue: {bad.size} outputs differ, e.g. (gate, up, got, want) {[(float(g[i]), float(u[i]), float(outs['pairs'].ravel()[i]), float(ref.ravel()[i])) for i in bad[:6]]}")
    want = gc.add_ref(res, oh.y)
    bad = np.argwhere(~gc.same_half(outs["add"], want))
    if len(bad):
        miss.append(f"residual epilogue: {len(bad)} outputs differ, e.g. (residual, y, got, want) {[(float(res[tuple(j)]), float(oh.y[tuple(j)]), float(outs['add'][tuple(j)]), float(want[tuple(j)])) for j in bad[:6]]}")
    print(f"    {name:34s} {str(shape):24s} " + ("ok" if not miss else "; ".join(miss)))
    return [f"{name} {shape}: {m}" for m in miss]


def _raise(miss):
    if miss:
        raise CheckMissed("\n".join(miss))


def test_epilogues_row_block_gemv(dev):
    """Every compiled geometry under TCE_W4_FORCE_GEMV, on the three GEMV shapes (groups of 128, 64, 32; M = 1, 4, 2)."""
    from tinychatengine_amd import capi
    print("\nrow-block GEMV")
    miss = []
    for shape in map(_even, wc.GEMV_SHAPES):
        cfgs, ran = [(0, 0, 0, 0)] + capi.gemv_variants(), 0
        for cfg in cfgs:
            try:
                miss += _epilogue_check(dev, f"row-block {cfg}", shape, False, (f"gemv passes={(shape[0] + 3) // 4} kernel=row-block",),
                                        lambda: capi.set_gemv_config(*cfg), capi.set_gemv_config, force=capi.TCE_W4_FORCE_GEMV)
                ran += 1
            except capi.TceError as e:
                if not (e.code == capi.TCE_ERR_UNSUPPORTED_SHAPE or "no kernel variant for this shape" in str(e)):
                    raise
                print(f"    row-block {cfg} {shape}: refused by the library, nothing ran")
        # (measured: one geometry, (2, 8, 1, 2), is refused at the two shapes with groups of 64 and 32; a library that refused the forced geometries wholesale would
        #  leave the automatic form alone to pass this test)
        assert ran >= len(cfgs) - 2 and ran >= 12, f"{shape}: only {ran} of {len(cfgs)} geometries ran"
    _raise(miss)


def test_epilogues_persistent_gemv(dev):
    from tinychatengine_amd import capi
    print("\npersistent GEMV")
    miss = []
    for cfg in PERSISTENT_CFGS:
        miss += _epilogue_check(dev, f"persistent {cfg}", _even(wc.STREAM_SHAPES[0]), False, ("gemv passes=1 kernel=persistent",), lambda: capi.set_gemv_config(*cfg), capi.set_gemv_config)
    _raise(miss)


def test_epilogues_i8_gemv(dev):
    """One, two and four rows per pass (groups of 128 and 64), one and two tiles per wave."""
    from tinychatengine_amd import capi
    print("\nint8-contraction GEMV")
    miss = []
    for shape in ((1, 72, 4096, 128), (2, 72, 4096, 64), (4, 72, 4096, 128)):
        for tiles in I8_TILES:
            miss += _epilogue_check(dev, f"gemv-i8 tiles per wave {tiles}", shape, True, ("gemv-i8",), lambda: capi.set_gemv_i8(0, tiles), capi.set_gemv_i8)
    _raise(miss)


def test_epilogues_skinny(dev):
    print("\nsmall-batch kernel")
    miss = []
    for shape in map(_even, wc.SKINNY_SHAPES):
        miss += _epilogue_check(dev, "small-batch", shape, False, ("small-batch",))
    _raise(miss)


PK_MODES = (61, 66, 2670, 2676)  # forced forms of the packed GEMM (test_pk_gemm_matches_oracle's numbering): 128- and 256-row tiles, a wide form, two quartets with a k cut


def test_epilogues_prefill_gemm(dev):
    """The packed GEMM under the automatic dispatch (the pair flag takes it; the plain and residual launches of this small batch go to the LDS-DMA GEMM) and with its
    forms forced, where all three launches run on it -- its rescale chain multiplies the accumulator by ratios of SIGNED scales, so an output that is exactly zero must
    still come out as +0; without a packed copy the LDS-DMA GEMM (its residual epilogue; the pair flag runs on the GEMV kernel there, as test_gpu_epilogues.py says)."""
    from tinychatengine_amd import capi
    L = capi.lib()
    print("\nprefill GEMMs")
    shape = _even(wc.PK_SHAPES[0])
    miss = _epilogue_check(dev, "packed copy, automatic", shape, True, lambda what: ("gemm-pk",) if what == "pairs" else ("gemm-pk|gemm-dma",))
    for mode in PK_MODES:
        miss += _epilogue_check(dev, f"packed copy, mode {mode}", shape, True, ("gemm-pk tile=",), lambda: capi.check(L.tce_w4a16_set_debug_mode(mode)), lambda: L.tce_w4a16_set_debug_mode(60))
    miss += _epilogue_check(dev, "no packed copy", shape, False, lambda what: ("gemv passes=",) if what == "pairs" else ("gemm-dma|gemm tile",))
    _raise(miss)


def test_epilogues_token_kernel(dev):
    """The persistent token kernel (TCE_PLAN_TAGGED on packed copies, TOKEN_SHAPE's K): a plan of three launches -- plain, pair epilogue, residual epilogue -- on the
    designed values, against the stream-ordered plan bit for bit and against the references."""
    from tinychatengine_amd import capi
    M, N, K, G = wc.TOKEN_SHAPE
    oh = gc.OneHotLinear(M, N, K, G, lambda g: gc.epilogue_values(N, shift=7 * g))
    lin = _one_hot_linear(dev, oh, prepack=True)
    x = _t(dev, oh.a)
    res = np.stack([gc.residual_for(oh.y[r], shift=r) for r in range(M)])
    bufs = dict(plain=_nan(dev, M, N), pairs=_nan(dev, M, N // 2), add=_t(dev, res))
    flags = dict(plain=0, pairs=capi.TCE_W4_SILU_MUL_PAIRS, add=capi.TCE_W4_ADD_TO_C)
    launches = [[lin.desc(x, bufs[k], flags=flags[k])] for k in ("plain", "pairs", "add")]
    for d in launches:
        _expect(d[0], "gemv-i8")
    plain, tok = capi.Plan(launches), capi.Plan(launches, tagged=True)
    print("\ntoken kernel plan")
    try:
        if not (tok.kind == 4 and tok.tagged and not plain.chained):
            raise DispatchError(f"the tagged plan is of kind {tok.kind}, the plain one chained = {plain.chained}")
        got = []
        for name, plan in (("stream-ordered plan", plain), ("token kernel", tok)):
            bufs["plain"].fill_(float("nan")); bufs["pairs"].fill_(float("nan")); bufs["add"].copy_(_t(dev, res))
            plan.launch(_stream())
            plan.status()
            torch.cuda.synchronize()
            got.append({k: v.cpu().numpy().copy() for k, v in bufs.items()})
        miss = _epilogue_judge("stream-ordered plan", wc.TOKEN_SHAPE, oh, res, got[0]) + _epilogue_judge("token kernel", wc.TOKEN_SHAPE, oh, res, got[1])
        for k in bufs:
            if not np.array_equal(got[0][k].view(np.uint16), got[1][k].view(np.uint16)):
                miss.append(f"token kernel: '{k}' differs from the stream-ordered plan")
    finally:
        plain.close()
        tok.close()
    _raise(miss)


def _known_params():
    cells = {}
    for (form, K, row), v in KNOWN_DEFECTS.items():
        cells.setdefault((form, K), []).append(f"{row}: {v}")
    return [pytest.param(form, K, id=f"{form}-{K}", marks=pytest.mark.xfail(strict=True, raises=CheckMissed, reason="open defect (DESIGN.md 4.5): " + "; ".join(v)))
            for (form, K), v in cells.items()]


if KNOWN_DEFECTS:  # (no empty parameter set: pytest would report it as a skip)
    @pytest.mark.parametrize("form,K", _known_params())
    def test_known_defect(dev, norm_linears, form, K):
        """The rows of KNOWN_DEFECTS for one (kernel form, K).  Expected to fail by the CHECK only (raises=CheckMissed: an assertion of the harness is an AssertionError,
        another dispatch a DispatchError, a refusal a TceError -- none of them counts); when the kernel comes to pass, the strict mark reports it."""
        assert form == "int8-contraction GEMV"
        _i8_prologue(dev, norm_linears, K, only_known=True)
