"""The tiled form of the two expert contractions (tce_moe_gate_up_tiled_f16, tce_moe_down_tiled_f16; MoeFFN(..., tiled_from=)): word for word the pass form's results,
and against float64 on its own, on routings whose lists end on every side of a tile edge (tests/moe_tiled_cases.py)."""
import numpy as np
import pytest

import moe_cases as mc
import moe_tiled_cases as tc
from conftest import w4a16_close
from test_gpu_moe import NAN32, _forward_bits, _moe_blocks, _t, dev  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NEVER = 1 << 30  # a tiled_from no call reaches: the pass form


def _tile_rows():
    from tinychatengine_amd import moe
    return moe.TILE_ROWS


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("E,k", tc.EK)
@pytest.mark.parametrize("K,N", [(128, 40), (1408, None)])
def test_stage_equals_the_pass_form_and_float64(dev, K, N, E, k, up):
    """N None: TILE_ROWS + 8, a second tile with 8 live rows.  (a) the output section and everything behind it, poisoned before each run, is the pass form's byte for
    byte; (b) every pair within act_bound (|g| < 8 asserted) / w4a16_close of float64; (c) the out-of-range pair's row of y and the bytes behind y keep the poison.
    (Gaussian rows of deviation 0.5: moe_cases.stacked sizes its scales for 20 rows of deviation 1, and |g| < 8 has to hold over 35 times as many pairs)"""
    from tinychatengine_amd import moe
    N = N or _tile_rows() + 8
    ids, arrays, rng = tc.tiled_ids(E, k, moe.TILE_PAIRS), mc.stacked(E, N, K, seed=K + E), np.random.default_rng(K + N + E)
    W, ws = moe.dequantize_stacked(*arrays), moe.MoeWorkspace(len(ids), k, E, max(N, K), dev)
    ws.write_routing(ids, np.ones(ids.shape))
    src = rng.normal(0, 0.5, (len(ids) * (1 if up else k), K)).astype(np.float16)
    xs, arrs, tail = _t(dev, src)[0], _t(dev, *arrays), ws.buf[ws.offsets[4 if up else 5]:]

    def run(tiled):
        tail.view(torch.int32).fill_(NAN32)
        if up:
            moe.gate_up(xs, arrs, ws, tiled=tiled)
        else:
            ws.act(K).copy_(xs)
            moe.down(arrs, ws, tiled=tiled)
        return tail.cpu().numpy().copy()

    passes, tiles = run(False), run(True)
    assert np.array_equal(passes, tiles)
    out, src, worst = (ws.act(N // 2) if up else ws.y(N)).cpu().numpy(), src.astype(np.float64), 0.0
    for p, e in enumerate(ids.reshape(-1)):
        if not 0 <= e < E:
            assert (out[p].view(np.int32) == NAN32).all()  # (act was poisoned too: neither form writes a row for this pair)
        elif up:
            gu = W[e] @ src[p // k]
            g, u = gu[0::2], gu[1::2]
            assert np.abs(g).max() < 8
            worst = max(worst, float((np.abs(out[p].astype(np.float64) - g / (1 + np.exp(-g)) * u) / mc.act_bound(g, u)).max()))
        else:
            worst = max(worst, w4a16_close(out[p], W[e] @ src[p])[1])
    print(f"worst ratio {worst:.3f}")
    assert worst <= 1.0 and (up or (tiles[out.nbytes:].view(np.int32) == NAN32).all())


def _crowd(rng, hidden, n=270):
    """6 ordinary rows and n copies of the first: more than 2 TILE_PAIRS pairs on each of its experts"""
    x, C = rng.normal(0, 1, (6, hidden)).astype(np.float16), rng.normal(0, 1, (6, hidden)).astype(np.float16)
    return np.concatenate([x, np.repeat(x[:1], n, axis=0)]), np.concatenate([C, np.repeat(C[:1], n, axis=0)])


def test_layer_equals_the_pass_form_and_follows_a_graph(dev):
    """MoeFFN(256, 128, 4, 2): act, y and C of every row, tiled_from = 0 against the pass form; then the five launches in one torch.cuda.graph: replays after x is
    rewritten on the device (another routing) equal the eager results, twice each"""
    from tinychatengine_amd import moe
    ffn, rng = moe.MoeFFN(256, 128, 4, 2, dev, seed=1, tiled_from=0), np.random.default_rng(17)
    x, C = _crowd(rng, 256)
    cases = [(x, C), (x[::-1].copy(), C)]
    tiled = [_forward_bits(ffn, v, c) for v, c in cases]
    assert ffn.workspace(len(x)).count.cpu().numpy().max() > 2 * moe.TILE_PAIRS
    ffn.tiled_from = NEVER
    assert [_forward_bits(ffn, v, c) for v, c in cases] == tiled
    ffn.tiled_from = 0
    xt, ct, s = *_t(dev, x, C), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ffn.forward(xt, ct)  # (warm-up on the capture stream)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ffn.forward(xt, ct)
    for (v, c), want in list(zip(cases, tiled)) * 2:
        xt.copy_(_t(dev, v)[0])
        ct.copy_(_t(dev, c)[0])
        graph.replay()
        assert [r[2] for r in want] == [row.tobytes() for row in ct.cpu().numpy()]


def test_a_300_row_prefill_feeds_the_experts_as_one_row_calls(dev, monkeypatch):
    """DecoderBlock.prefill over 300 rows with tiled_from = 0: for eight rows -- the first, the last, the two on either side of the first tile edge of the fullest
    expert's list, four more -- act, y and C are a one-row forward's (the pass form) on the row the layer fed in"""
    from tinychatengine_amd import moe
    blk, seen = _moe_blocks(dev, 1, keys=320)[0], []
    ffn, inner = blk.moe, blk.moe.forward
    ffn.tiled_from = 0
    monkeypatch.setattr(ffn, "forward", lambda xn, rows: (seen.append((xn.cpu().numpy(), rows.cpu().numpy())), inner(xn, rows)))
    rows = _t(dev, np.random.default_rng(15).normal(0, 1, (300, 256)).astype(np.float16))[0]
    blk.prefill(rows, 0)
    monkeypatch.undo()
    ws = ffn.workspace(300)
    count, lst = ws.count.cpu().numpy(), ws.list.cpu().numpy()
    full = int(count.argmax())
    assert count[full] > moe.TILE_PAIRS
    a, y, c, ((xn, before),) = ws.act(128).cpu().numpy(), ws.y(256).cpu().numpy(), rows.cpu().numpy(), seen
    ffn.tiled_from = NEVER
    for i in [0, 299, int(lst[full, moe.TILE_PAIRS - 1]) // 2, int(lst[full, moe.TILE_PAIRS]) // 2, 63, 64, 150, 257]:
        assert _forward_bits(ffn, xn[i:i + 1], before[i:i + 1])[0] == (a[2 * i:2 * i + 2].tobytes(), y[2 * i:2 * i + 2].tobytes(), c[i].tobytes()), i
