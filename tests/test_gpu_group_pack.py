"""GPU: group copies -- q/k/v, gate+up packed as ONE row-concatenated linear (tce_w4a16_prepack_group) and launched on it as one linear (csrc/w4a16_gemv_i8.hip).

What must hold, for groups of 2 / 3 / 4 members with N from {16, 32, 48, 1024} (one tile, ragged tile counts, member boundaries inside a workgroup's range when two
tiles per wave are forced), K from {128, 1024, 1152, 4096} (one unit, one whole wave, a ragged last wave, four waves) and once 14336 (fourteen waves), M 1 / 2 / 4,
groups of 128 / 64, zero point 8 and random zero points, plain / TCE_W4_ADD_TO_C / TCE_W4_SILU_MUL_PAIRS members, the fused RMSNorm prologue, members with their own
C buffers and with a shared row at different offsets:
  * the group copy is byte-identical to tce_w4a16_prepack of the concatenated linear (every part; the alignment padding between parts is nobody's);
  * the grouped launch on it is bit-identical to the same group on individual copies and to each member launched alone;
  * against the oracle: the suite's W4A16 tolerance (conftest.w4a16_close), unchanged;
  * a member list out of order, or with a gap, runs today's grouped path: the same bits;
  * M > 128: the prefill GEMM on a member of a group copy gives the member's output on its own copy, bit for bit;
  * a plan built on group copies equals the plan on individual copies (two blocks, data-flow wiring, every output as int16).
"""
import numpy as np
import pytest

from conftest import w4a16_close

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


def _stream():
    return torch.cuda.current_stream().cuda_stream


_cache = {}


def _group(oracle, dev, Ns, K, G, random_zeros):
    """(members on ONE group copy, the same members on individual copies, the concatenated linear with its own copy, the numpy q4_6 arrays per member) -- built once
    per shape and shared by the tests (nothing writes to them)."""
    key = (Ns, K, G, random_zeros)
    if key in _cache:
        return _cache[key]
    from tinychatengine_amd.linear import Linear_half_int4
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    arrays, shared, own = [], [], []
    for i, N in enumerate(Ns):
        rng = np.random.default_rng(1000 * K + 10 * N + i + (7 if random_zeros else 0) + G)
        w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
        qw, sc, zp, _, _ = oracle.quantize_q4_6(w, G)
        if random_zeros:
            nib = rng.integers(0, 16, (N, zp.shape[1] * 8), dtype=np.uint32)
            zp = (nib.reshape(N, -1, 8) << (np.arange(8, dtype=np.uint32) * 4)).sum(axis=2).astype(np.uint32)
        arrays.append((qw, sc, zp))
        tq, ts, tz = t(qw.view(np.int32)), t(sc.view(np.float16)), t(zp.view(np.int32))
        shared.append(Linear_half_int4(tq, ts, tz, G))
        own.append(Linear_half_int4(tq, ts, tz, G).prepack())
    assert Linear_half_int4.prepack_group(shared), "the members must be able to share a copy"
    cat = Linear_half_int4(torch.cat([l.weight for l in own]), torch.cat([l.scale for l in own]), torch.cat([l.zero_point for l in own]), G).prepack()
    torch.cuda.synchronize()
    _cache[key] = (shared, own, cat, arrays)
    return _cache[key]


def _parts(N, K, G):
    """[(offset, bytes)] of words, constants, last scales, decode scales, decode zero points of a packed copy (csrc/w4a16_mfma_layout.hpp)"""
    nt, a = (N + 15) // 16, lambda x: (x + 255) & ~255
    sizes = [nt * (K // 128) * 1024, nt * (K // G) * 128, nt * 64, nt * (K // G) * 32, nt * (K // G) * 8]
    out, off = [], 0
    for s in sizes:
        out.append((off, s))
        off += a(s)
    return out, off


def _x(M, K, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((M, K)).astype(np.float16))


def _run_group(lins, x, flags=None, outs=None, order=None):
    """one grouped launch; outs: preset buffers (residuals), else NaN-filled.  order: the members' order in the launch"""
    from tinychatengine_amd import capi
    flags = flags or [0] * len(lins)
    m = x.shape[0]
    if outs is None:
        outs = [torch.full((m, l.out_features // 2 if f & capi.TCE_W4_SILU_MUL_PAIRS else l.out_features), float("nan"), dtype=torch.float16, device=x.device) for l, f in zip(lins, flags)]
    descs = [l.desc(x, o, flags=f) for l, o, f in zip(lins, outs, flags)]
    for d in descs:
        assert capi.describe_dispatch(d).startswith("gemv-i8"), capi.describe_dispatch(d)
    if order is not None:
        descs = [descs[i] for i in order]
    capi.check(capi.w4a16_forward_group(descs, _stream()))
    torch.cuda.synchronize()
    return outs


def _run_alone(lins, x, flags=None, outs=None):
    from tinychatengine_amd import capi
    flags = flags or [0] * len(lins)
    m = x.shape[0]
    if outs is None:
        outs = [torch.full((m, l.out_features // 2 if f & capi.TCE_W4_SILU_MUL_PAIRS else l.out_features), float("nan"), dtype=torch.float16, device=x.device) for l, f in zip(lins, flags)]
    for l, o, f in zip(lins, outs, flags):
        capi.check(capi.w4a16_forward(l.desc(x, o, flags=f), _stream()))
    torch.cuda.synchronize()
    return outs


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.float()).any(), f"{what}: member {i} has NaN / unwritten elements"
        assert torch.equal(u.view(torch.int16), v.view(torch.int16)), f"{what}: member {i} differs ({int((u.view(torch.int16) != v.view(torch.int16)).sum())} elements)"


G2, G3, G4 = (16, 32), (48, 16, 1024), (1024, 48, 32, 16)
# (Ns, K, M, G, random zero points)
CASES = [(Ns, K, 1, 128, False) for Ns in (G2, G3, G4) for K in (128, 1024, 1152, 4096)] + [
    (G2, 128, 1, 128, True), (G3, 1152, 1, 128, True), (G4, 4096, 1, 128, True),
    (G3, 1152, 2, 128, False), (G2, 4096, 2, 128, True), (G4, 1024, 4, 128, False), (G2, 1152, 4, 128, True),
    (G3, 1152, 1, 64, False), (G2, 4096, 2, 64, True), (G4, 128, 1, 64, True), (G3, 1024, 2, 64, False),
    ((16, 48), 14336, 1, 128, False),
]


@pytest.mark.parametrize("Ns,K,M,G,rz", CASES)
def test_group_copy_bytes_and_bits(dev, oracle, Ns, K, M, G, rz):
    from tinychatengine_amd import capi
    shared, own, cat, arrays = _group(oracle, dev, Ns, K, G, rz)
    # the copy: byte for byte the copy of the concatenation
    parts, total = _parts(sum(Ns), K, G)
    assert shared[0].packed.numel() == cat.packed.numel() == total == int(capi.lib().tce_w4a16_prepack_bytes(sum(Ns), K, G))
    assert all(l.packed.data_ptr() == shared[0].packed.data_ptr() for l in shared)
    for name, (off, n) in zip(("words", "consts", "last", "dscales", "dzeros"), parts):
        assert torch.equal(shared[0].packed[off:off + n], cat.packed[off:off + n]), f"{name} differ from the concatenated linear's copy"
    x = _x(M, K, K + M).to(dev)
    for tiles in ((0, 2) if (M == 1 and G == 128 and K <= 8192) else (0,)):  # two tiles per wave forced: member boundaries inside a workgroup's range
        capi.set_gemv_i8(0, tiles)
        try:
            ref = _run_group(own, x)
            _same(_run_group(shared, x), ref, f"grouped on the shared copy (tiles per wave {tiles})")
            _same(_run_alone(shared, x), ref, f"members alone on the shared copy (tiles per wave {tiles})")
            _same(_run_alone(own, x), ref, f"members alone on their own copies (tiles per wave {tiles})")
            # out of order / with a gap: today's grouped path on the members' slices
            _same(_run_group(shared, x, order=list(range(len(Ns)))[::-1]), ref, "members out of order")
            if len(Ns) > 2:
                outs = _run_group([shared[0], shared[2]], x)
                _same(outs, [ref[0], ref[2]], "members with a gap")
                outs = _run_group(shared[1:], x)  # a consecutive sub-range that does not begin at the copy's first tile
                _same(outs, ref[1:], "a sub-range of the copy")
        finally:
            capi.set_gemv_i8()
    # the whole concatenation as one linear: the same rows
    whole = _run_alone([cat], x)[0]
    _same([whole], [torch.cat(ref, dim=1)], "the concatenated linear")
    # the oracle, the suite's tolerance
    a = x.cpu().numpy()
    for i, (N, (qw, sc, zp)) in enumerate(zip(Ns, arrays)):
        ref32, _ = oracle.w4a16_gemv_q4_6(a, qw, sc, zp, M, N, K, G)
        ok, worst = w4a16_close(ref[i].cpu().numpy(), ref32)
        print(f"member {i} N={N}: worst |err| / tol = {worst:.3f}")
        assert ok, f"member {i}: worst |err|/tol = {worst:.3f} (tol = 1e-3*max(|ref|, rms/64))"


@pytest.mark.parametrize("Ns,K,M,G,rz", [(G3, 1152, 1, 128, False), (G4, 4096, 2, 128, True), (G2, 1024, 4, 128, False), (G3, 1024, 2, 64, False), (G4, 1024, 1, 128, True)])
def test_group_copy_epilogues_and_output_placement(dev, oracle, Ns, K, M, G, rz):
    """members with different epilogues in one launch -- plain, residual add, SiLU * mul pairs -- into their own buffers and into ONE row at different offsets"""
    from tinychatengine_amd import capi
    shared, own, _, _ = _group(oracle, dev, Ns, K, G, rz)
    x = _x(M, K, 3 * K + M).to(dev)
    kinds = [capi.TCE_W4_ADD_TO_C, capi.TCE_W4_SILU_MUL_PAIRS, 0, capi.TCE_W4_ADD_TO_C][:len(Ns)]
    widths = [N // 2 if f & capi.TCE_W4_SILU_MUL_PAIRS else N for N, f in zip(Ns, kinds)]
    g = torch.Generator(device=dev).manual_seed(K + M)
    resid = [torch.empty((M, w), dtype=torch.float32, device=dev).normal_(0, 1, generator=g).half() for w in widths]
    for tiles in ((0, 2) if (M == 1 and G == 128) else (0,)):
        capi.set_gemv_i8(0, tiles)
        try:
            ref = _run_group(own, x, kinds, [r.clone() for r in resid])
            _same(_run_group(shared, x, kinds, [r.clone() for r in resid]), ref, "own buffers")
            _same(_run_alone(shared, x, kinds, [r.clone() for r in resid]), ref, "members alone")
            _same(_run_alone(own, x, kinds, [r.clone() for r in resid]), ref, "members alone, own copies")
            # one row [M][sum widths + 8 per member], every member at its offset (ldc = the row's width)
            ld = sum(widths) + 8 * len(widths)
            row = torch.full((M, ld), float("nan"), dtype=torch.float16, device=dev)
            offs, o = [], 0
            for w_, r in zip(widths, resid):
                row[:, o:o + w_] = r
                offs.append(o)
                o += w_ + 8
            descs = [l.desc(x, row.view(-1)[off:], ldc=ld, flags=f) for l, off, f in zip(shared, offs, kinds)]
            capi.check(capi.w4a16_forward_group(descs, _stream()))
            torch.cuda.synchronize()
            for i, (off, w_) in enumerate(zip(offs, widths)):
                assert torch.equal(row[:, off:off + w_].contiguous().view(torch.int16), ref[i].view(torch.int16)), f"member {i} in the shared row"
                assert torch.isnan(row[:, off + w_:off + w_ + 8].float()).all(), f"member {i} wrote past its columns"
        finally:
            capi.set_gemv_i8()


@pytest.mark.parametrize("Ns,K,rz", [(G3, 1152, False), (G4, 4096, True), (G2, 128, False), (G4, 1024, False)])
def test_group_copy_with_the_rmsnorm_prologue(dev, oracle, Ns, K, rz):
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import forward_group_rmsnorm
    shared, own, _, _ = _group(oracle, dev, Ns, K, 128, rz)
    x = _x(1, K, 5 * K).to(dev)
    gamma = (1.0 + 0.1 * torch.from_numpy(np.random.default_rng(K).standard_normal(K).astype(np.float32))).to(dev)
    mk = lambda: [torch.full((1, N), float("nan"), dtype=torch.float16, device=dev) for N in Ns]
    for tiles in (0, 2):
        capi.set_gemv_i8(0, tiles)
        try:
            ref, got = mk(), mk()
            forward_group_rmsnorm(own, x, ref, gamma, 1e-6)
            forward_group_rmsnorm(shared, x, got, gamma, 1e-6)
            torch.cuda.synchronize()
            _same(got, ref, f"norm prologue (tiles per wave {tiles})")
            alone = mk()
            for l, o in zip(shared, alone):
                forward_group_rmsnorm([l], x, [o], gamma, 1e-6)
            torch.cuda.synchronize()
            _same(alone, ref, f"norm prologue, members alone (tiles per wave {tiles})")
        finally:
            capi.set_gemv_i8()


@pytest.mark.parametrize("Ns,K,M,G,rz", [(G3, 1152, 160, 128, False), (G4, 1024, 129, 128, True), (G3, 1024, 200, 64, False)])
def test_prefill_gemm_on_a_member_of_a_group_copy(dev, oracle, Ns, K, M, G, rz):
    """M > 128: the prefill GEMM (csrc/w4a16_gemm_pk.hip) addresses the member's slice of the shared copy -- the member's output on its own copy, bit for bit; the
    member's neighbours in the copy must not show (first, inner and last members, ragged N against the GEMM's 128-column tiles)"""
    from tinychatengine_amd import capi
    shared, own, _, _ = _group(oracle, dev, Ns, K, G, rz)
    x = _x(M, K, 7 * K + M).to(dev)
    L = capi.lib()
    try:
        for mode in (61, 62, 64):  # the packed GEMM forced (tests/test_gpu_w4a16_pk.py): one quartet per tile, two quartets, the k range cut across workgroups
            capi.check(L.tce_w4a16_set_debug_mode(mode))
            for i, (s, o) in enumerate(zip(shared, own)):
                outs = []
                for l in (s, o):
                    out = torch.full((M, l.out_features), float("nan"), dtype=torch.float16, device=dev)
                    d = l.desc(x, out)
                    assert capi.describe_dispatch(d).startswith("gemm-pk"), capi.describe_dispatch(d)
                    capi.check(capi.w4a16_forward(d, _stream()))
                    outs.append(out)
                torch.cuda.synchronize()
                _same(outs[:1], outs[1:], f"member {i} (N={Ns[i]}) through the prefill GEMM, mode {mode}")
    finally:
        L.tce_w4a16_set_debug_mode(60)


def test_plan_on_group_copies_equals_plan_on_individual_copies(dev):
    """a two-block token with data-flow wiring: the plan (one graph) on group copies against the plan on individual copies, every output compared as int16"""
    from tinychatengine_amd.decode import SHAPES, DecodeLinears
    grouped = DecodeLinears(SHAPES["tiny"], device=dev, layers=2, dataflow=True, prepack=True)
    single = DecodeLinears(SHAPES["tiny"], device=dev, layers=2, dataflow=True, prepack=False)
    for l in single.all_linears():
        l.prepack()
    assert all(l.group_rows == sum(SHAPES["tiny"].qkv) for l in grouped.blocks[0]["qkv"]) and grouped.blocks[1]["up"].group_tile0 == SHAPES["tiny"].ffn // 16
    assert all(l.group_rows == 0 and l.packed is not None for l in single.all_linears())
    assert grouped.lm_head.group_rows == 0 and grouped.blocks[0]["o"].group_rows == 0
    # no second copy: the members of a group share one allocation
    assert len({l.packed.data_ptr() for l in grouped.blocks[0]["qkv"]}) == 1
    outs = lambda dl: [*dl.out_qkv, dl.out_o, dl.out_gate, dl.out_up, dl.out_down, dl.logits]
    res = []
    for dl in (grouped, single):
        plan = dl.make_plan()
        for o in outs(dl):
            o.fill_(float("nan"))
        for _ in range(2):
            plan.launch(_stream())
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs(dl)])
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.isfinite(a.float()).all(), f"output {i} is not finite"
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"output {i} differs"
