"""The mixture-of-experts launches through the C ABI (tce_moe_route_f16, tce_moe_gate_up_f16, tce_moe_down_f16, tce_moe_combine_add_f16) against moe_reference's
float64 definition, on the operands of tests/moe_cases.py (which says why each shape is there), and the layer through MoeFFN and the generators."""
import numpy as np
import pytest

import moe_cases as mc
from conftest import record_parity, w4a16_close

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAN32 = 0x7FC12345  # an fp32 NaN payload: y where nothing was written


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available() and capi.lib()
    return torch.device("cuda:0")


def _t(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _route(dev, x, Wr, k, renormalize=True):
    from tinychatengine_amd import moe
    ws = moe.MoeWorkspace(x.shape[0], k, Wr.shape[0], 64, dev)
    moe.route(*_t(dev, x, Wr), ws, renormalize)
    return tuple(v.cpu().numpy() for v in (ws.ids, ws.weights, ws.count, ws.list))


def _grouping_is_stable(ids, count, lst, E):
    from tinychatengine_amd.moe import group_reference
    rc, rl = group_reference(ids, E)
    assert np.array_equal(count, rc) and all(np.array_equal(lst[e, :rc[e]], rl[e]) for e in range(E))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("E,k", mc.EK)
@pytest.mark.parametrize("K", mc.KS)
def test_route(dev, K, E, k, exact):
    """exact: integer operands (every partial sum exact) with ties at slot k and inside the selected set (asserted): ids word for word, the grouping stable.
    bounded: Gaussian rows whose gap at slot k exceeds 2 logit_error (asserted): ids equal, weights within moe_cases.weight_rel_bound (derived there)"""
    from tinychatengine_amd.moe import route_reference
    (x, Wr), renorm = (mc.route_exact if exact else mc.route_bounded)(K, E, k), K == 128  # (renormalised at one K, plain softmax weights at the other)
    rid, rw, l = route_reference(x, Wr, k, renorm)
    d, srt = mc.logit_error(x, Wr), -np.sort(-l, axis=1)
    if exact:
        assert (srt[:, k - 1] == srt[:, k]).any() and (k == 1 or (srt[:, :k - 1] == srt[:, 1:k]).any()), "the data must hold both kinds of tie"
    else:
        assert ((srt[:, k - 1] - srt[:, k]) > 2 * d).all()
    ids, w, count, lst = _route(dev, x, Wr, k, renorm)
    assert np.array_equal(ids, rid)
    if exact:
        _grouping_is_stable(ids, count, lst, E)
    else:
        assert (np.abs(w.astype(np.float64) - rw) <= mc.weight_rel_bound(d, srt[:, 0] - srt[:, -1], E, k, renorm)[:, None] * rw + 2.0 ** -126).all()


def test_route_nonfinite_rows(dev):
    """a row of NaNs and a row of +-65504 among ordinary rows: their ids are in range, the other rows' ids and weights keep their bits and the lists their order"""
    K, E, k = 128, 8, 2
    x, Wr = mc.route_bounded(K, E, k)
    plain, odd, keep = _route(dev, x, Wr, k), x.copy(), np.delete(np.arange(len(x)), [3, 7])
    odd[3], odd[7] = np.nan, np.where(np.arange(K) % 2, 65504, -65504)
    ids, w, count, lst = _route(dev, odd, Wr, k)
    assert ((ids >= 0) & (ids < E)).all()
    assert np.array_equal(ids[keep], plain[0][keep]) and np.array_equal(w[keep].view(np.int32), plain[1][keep].view(np.int32))
    own = lambda lst_, cnt: [[p for p in lst_[e, :cnt[e]] if p // k not in (3, 7)] for e in range(E)]
    assert own(lst, count) == own(plain[3], plain[2])


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("K,N,E,k", mc.STAGES)
def test_stage_against_float64(dev, K, N, E, k, up):
    """on designed_ids.  gate_up: act within act_bound of float64, |g| < 8 asserted; down: y within w4a16_close per pair row, the bad pair's row and the bytes behind y keep the poison"""
    from tinychatengine_amd import moe
    ids, arrays, rng = mc.designed_ids(E, k), mc.stacked(E, N, K, seed=K + E), np.random.default_rng(K + N + E)
    W, ws = moe.dequantize_stacked(*arrays), moe.MoeWorkspace(len(ids), k, E, max(N, K), dev)
    ws.write_routing(ids, np.ones(ids.shape))
    src = rng.normal(0, 1, (len(ids) * (1 if up else k), K)).astype(np.float16)
    ws.buf[ws.offsets[5]:].view(torch.int32).fill_(NAN32)
    if up:
        moe.gate_up(_t(dev, src)[0], _t(dev, *arrays), ws)
    else:
        ws.act(K).copy_(_t(dev, src)[0])
        moe.down(_t(dev, *arrays), ws)
    out, src, worst = (ws.act(N // 2) if up else ws.y(N)).cpu().numpy(), src.astype(np.float64), 0.0
    for p, e in enumerate(ids.reshape(-1)):
        if not 0 <= e < E:
            assert up or (out[p].view(np.int32) == NAN32).all()
        elif up:
            gu = W[e] @ src[p // k]
            g, u = gu[0::2], gu[1::2]
            assert np.abs(g).max() < 8
            worst = max(worst, float((np.abs(out[p].astype(np.float64) - g / (1 + np.exp(-g)) * u) / mc.act_bound(g, u)).max()))
        else:
            worst = max(worst, w4a16_close(out[p], W[e] @ src[p])[1])
    record_parity(f"moe_{'gate_up' if up else 'down'}_K{K}_N{N}_E{E}_k{k}", {"worst_ratio": worst})
    assert worst <= 1.0 and (up or (ws.buf[ws.offsets[5] + out.nbytes:].view(torch.int32) == NAN32).all())


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("E,k", mc.EK)
def test_combine(dev, E, k, exact):
    """exact operands (every partial sum exact, asserted): the definition bit for bit; Gaussian ones: half an fp16 ulp + k 2^-24 sum_s |w_s y_s|.  A skipped slot's y
    is NaN and is not read; padding columns (ldc = N + 16) and a guard row keep their bits (-0.0 and a NaN payload among them)"""
    from tinychatengine_amd import moe
    rows, N, rng = 5, 40, np.random.default_rng(E + k)
    ids = rng.integers(0, E, (rows, k)).astype(np.int32)
    ids[1, 0], ids[rows - 1, k - 1] = -1, E
    if exact:
        w = 2.0 ** rng.integers(-3, 1, (rows, k))
        y, C = rng.integers(-64, 65, (rows * k, N)) / 64.0, (rng.integers(-64, 65, (rows, N)) / 64.0).astype(np.float16)
        assert (np.abs(y).max() * k + 1) * 2 ** 9 < 2 ** 24  # multiples of 2^-9 below 2^15: every partial sum and the add to C are exact
    else:
        w, y, C = rng.uniform(0, 1, (rows, k)), rng.normal(0, 1, (rows * k, N)), rng.normal(0, 1, (rows, N)).astype(np.float16)
    w, y, skipped = w.astype(np.float32), y.astype(np.float32), ((ids < 0) | (ids >= E)).reshape(-1)
    y[skipped] = np.nan
    full = np.tile(np.array([0x8000, 0x7E01, 0x3C00, 0xFC00], np.uint16), (rows + 1) * (N + 16) // 4).reshape(rows + 1, N + 16)
    full[:rows, :N] = C.view(np.uint16)
    ws, c_dev = moe.MoeWorkspace(rows, k, E, N, dev), _t(dev, full.view(np.float16))[0]
    ws.write_routing(ids, w)
    ws.y(N).copy_(_t(dev, y)[0])
    moe.combine_add(c_dev[:rows, :N], ws)
    after = c_dev.cpu().numpy().view(np.uint16)
    assert np.array_equal(after[rows], full[rows]) and np.array_equal(after[:, N:], full[:, N:])
    wy = np.where(skipped[:, None], 0.0, w.reshape(-1, 1).astype(np.float64) * y).reshape(rows, k, N)
    ref, got = C.astype(np.float64) + wy.sum(axis=1), after[:rows, :N].view(np.float16)
    if exact:
        assert np.array_equal(got.view(np.uint16), ref.astype(np.float16).view(np.uint16))
    else:
        bound = 0.5 * np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64) + k * 2.0 ** -24 * np.abs(wy).sum(axis=1)
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all()


def _ffn(dev, seed=1):
    from tinychatengine_amd.moe import MoeFFN
    return MoeFFN(128, 128, 4, 2, dev, seed=seed)


def _forward_bits(ffn, x, C):
    xt, ct = _t(ffn.device, x, C)
    ffn.forward(xt, ct)
    ws, k = ffn.workspace(len(x)), ffn.top_k
    a, y, c = ws.act(ffn.ffn).cpu().numpy(), ws.y(ffn.hidden).cpu().numpy(), ct.cpu().numpy()
    return [(a[i * k:(i + 1) * k].tobytes(), y[i * k:(i + 1) * k].tobytes(), c[i].tobytes()) for i in range(len(x))]


def test_a_rows_bits_do_not_depend_on_its_neighbours_nor_on_a_graph(dev):
    """act, y and C of a row: alone, first, last, and among 520 rows that pile 33 passes onto its experts (1040 pairs: two chunks of the grouping).  Then the five
    launches in one torch.cuda.graph: replays after x is rewritten on the device (another routing) equal the eager results"""
    ffn, rng = _ffn(dev), np.random.default_rng(11)
    x, C = rng.normal(0, 1, (6, 128)).astype(np.float16), rng.normal(0, 1, (6, 128)).astype(np.float16)
    cases = [(x, C), (np.roll(x, -1, axis=0), np.roll(C, -1, axis=0)), (x[::-1], C)]
    alone, eager, routed = _forward_bits(ffn, x[:1], C[:1])[0], [], set()
    for v, c in cases:
        eager.append(_forward_bits(ffn, v, c))
        routed.add(ffn.workspace(6).ids.cpu().numpy().tobytes())
    assert eager[0][0] == alone and eager[1][5] == alone and len(routed) == 3
    crowd = _forward_bits(ffn, np.repeat(x[:1], 520, axis=0), np.repeat(C[:1], 520, axis=0))
    ws = ffn.workspace(520)
    assert ws.count.cpu().numpy().max() == 520 and all(r == alone for r in crowd)
    _grouping_is_stable(ws.ids.cpu().numpy(), ws.count.cpu().numpy(), ws.list.cpu().numpy(), 4)
    xt, ct, s = *_t(dev, x, C), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ffn.forward(xt, ct)  # (warm-up on the capture stream)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ffn.forward(xt, ct)
    for (v, c), want in zip(cases, eager):
        xt.copy_(_t(dev, v)[0])
        ct.copy_(_t(dev, c)[0])
        graph.replay()
        assert [r[2] for r in want] == [row.tobytes() for row in ct.cpu().numpy()]


def test_forward_against_the_definition(dev):
    """B = 3 against moe_reference on the device's ids: half an fp16 ulp + sum_s w_s (w4_tol(y) + |W_down| act_bound + (weight_rel_bound + k 2^-24) |y|)"""
    from tinychatengine_amd import moe
    ffn, rng = _ffn(dev, seed=2), np.random.default_rng(13)
    x, C = rng.normal(0, 1, (3, 128)).astype(np.float16), rng.normal(0, 1, (3, 128)).astype(np.float16)
    xt, ct = _t(dev, x, C)
    ffn.forward(xt, ct)
    k, ids = ffn.top_k, ffn.workspace(3).ids.cpu().numpy()
    Wr, gu, dn = ffn.Wr.cpu().numpy(), *(tuple(a.cpu().numpy() for a in arrs) for arrs in (ffn.gate_up, ffn.down))
    ref, logits = moe.moe_reference(x, Wr, gu, dn, k, C, ids=ids), moe.route_reference(x, Wr, k)[2]
    Wgu, Wd, w, y = moe.dequantize_stacked(*gu), moe.dequantize_stacked(*dn), ref["weights"], ref["y"].reshape(3, k, -1)
    w_rel = mc.weight_rel_bound(mc.logit_error(x, Wr), logits.max(1) - logits.min(1), ffn.experts, k, True) + k * 2.0 ** -24
    exact = C.astype(np.float64) + (w[..., None] * y).sum(1)
    bound = 0.5 * np.spacing(np.abs(exact).astype(np.float16)).astype(np.float64)
    for i, s in np.ndindex(3, k):
        gu_ = Wgu[ids[i, s]] @ x[i].astype(np.float64)
        bound[i] += w[i, s] * (mc.w4_tol(y[i, s]) + np.abs(Wd[ids[i, s]]) @ mc.act_bound(gu_[0::2], gu_[1::2]) + w_rel[i] * np.abs(y[i, s]))
    assert (np.abs(ct.cpu().numpy().astype(np.float64) - exact) <= bound).all()


def _moe_blocks(dev, n, keys=64):
    from tinychatengine_amd.decoder_block import DecoderBlock
    ang = np.random.default_rng(21).uniform(0, 2 * np.pi, (keys, 64))
    cos, sin = _t(dev, np.concatenate([np.cos(ang)] * 2, 1).astype(np.float16), np.concatenate([np.sin(ang)] * 2, 1).astype(np.float16))
    return [DecoderBlock(256, 2, 128, keys, dev, cos, sin, seed=70 + i, kv_heads=1, moe={"experts": 4, "top_k": 2}) for i in range(n)]


@pytest.mark.parametrize("paged", [True, False])
def test_a_40_row_prefill_feeds_the_experts_as_40_one_row_calls(dev, paged, monkeypatch):
    """prefill_many / DecoderBlock.prefill over 40 rows: an expert gets more than 16 pairs; each pair's act, y and C are a one-row forward's on the row the layer fed in"""
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    blk, seen = _moe_blocks(dev, 1)[0], []
    ffn, inner = blk.moe, blk.moe.forward
    monkeypatch.setattr(ffn, "forward", lambda xn, rows: (seen.append((xn.cpu().numpy(), rows.cpu().numpy())), inner(xn, rows)))
    rows = _t(dev, np.random.default_rng(14).normal(0, 1, (40, 256)).astype(np.float16))[0]
    PagedBatchedDecoder(blk, PageAllocator(8, 16, 2, 4, dev)).prefill_many([(1, rows, 0)]) if paged else blk.prefill(rows, 0)
    monkeypatch.undo()
    ws = ffn.workspace(40)
    assert ws.count.cpu().numpy().max() > 16
    a, y, c, ((xn, before),) = ws.act(128).cpu().numpy(), ws.y(256).cpu().numpy(), rows.cpu().numpy(), seen
    for i in range(40):
        assert _forward_bits(ffn, xn[i:i + 1], before[i:i + 1])[0] == (a[2 * i:2 * i + 2].tobytes(), y[2 * i:2 * i + 2].tobytes(), c[i].tobytes()), i


def test_generator_over_moe_layers_equals_the_host_driven_loop(dev):
    """two MoE layers (E = 4, k = 2) under BatchedGenerator's captured graph, greedy, on pages: token for token the host-driven loop's"""
    from tinychatengine_amd.generate import BatchedGenerator, HostDrivenLoop, SamplingParams
    from tinychatengine_amd.linear import Linear_half_int4
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    hidden, vocab, rng, blocks = 256, 512, np.random.default_rng(21), _moe_blocks(dev, 2)
    rnd = lambda *shape: torch.empty(*shape, device=dev).normal_(0.0, 1.0, generator=torch.Generator(device=dev).manual_seed(7 + len(shape)))
    gamma, lm_head, table = 1.0 + 0.1 * rnd(hidden), Linear_half_int4.from_float(rnd(vocab, hidden) * hidden ** -0.5).prepack(), rnd(vocab, hidden).half()
    stack = lambda alloc: [PagedBatchedDecoder(b, alloc) for b in blocks]
    gen = BatchedGenerator(stack(PageAllocator(12, 16, 3, 4, dev)), gamma, lm_head, table, max_new=12, graph=True)
    host = HostDrivenLoop(stack(PageAllocator(12, 16, 3, 4, dev)), gamma, lm_head, table)
    assert gen.decoders[0].LAUNCHES == 10
    for s, n in [(0, 9), (2, 4)]:
        prompt = rng.integers(0, vocab, n).tolist()
        gen.admit(s, prompt, SamplingParams(temp=0.0, repeat_penalty=1.0), 0, 12)
        host.admit(s, prompt, 12)
    gen.run(14)
    [host.step() for _ in range(14)]
    assert all(gen.tokens(s) == host.out[s] and len(gen.tokens(s)) == 12 for s in (0, 2))
