"""The parallel grouping of the routed pairs (tce_moe_group_parallel, tce_moe_route_parallel_f16; MoeFFN(..., parallel_group_from=)): moe.group_reference's count and
lists exactly, at the chunk (1024 pairs) and wave (64) edges, and word for word what the one-wave grouping of tce_moe_route_f16 leaves."""
import numpy as np
import pytest

from test_gpu_moe import NAN32, _forward_bits, _t, dev  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NEVER, SENTINEL = 1 << 30, -7  # a parallel_group_from no call reaches; a word no list holds
PATTERNS = ["first", "last", "round_robin", "one_unnamed", "out_of_range", "random"]


def _ids(pattern, P, E):
    rng, p = np.random.default_rng(P * 64 + E), np.arange(P)
    if pattern in ("first", "last"):
        return np.full(P, 0 if pattern == "first" else E - 1, np.int32)
    if pattern == "round_robin":
        return (p % E).astype(np.int32)
    if pattern == "one_unnamed":  # expert E // 2 has an empty list (E = 1: every list is empty)
        others = np.delete(np.arange(E), E // 2)
        return rng.choice(others, P).astype(np.int32) if E > 1 else np.full(P, -1, np.int32)
    ids = rng.integers(0, E, P).astype(np.int32)
    if pattern == "out_of_range":
        bad = rng.random(P) < 0.3
        ids[bad] = np.array([-1, E, 2 ** 31 - 1], np.int32)[p[bad] % 3]
    return ids


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("E", [1, 3, 64])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097])
def test_group_parallel_is_the_reference(dev, P, E, pattern):
    """count and list[e][:count[e]] exactly; every list word at and beyond count[e] keeps the sentinel; act and y behind the grouping's scratch (the head of y: one
    int32 per chunk and expert) keep their poison"""
    from tinychatengine_amd import moe
    ws, ids = moe.MoeWorkspace(P, 1, E, 64, dev), _ids(pattern, P, E)
    ws.ids.copy_(_t(dev, ids.reshape(P, 1))[0])
    ws.list.fill_(SENTINEL)
    ws.buf[ws.offsets[4]:].view(torch.int32).fill_(NAN32)
    moe.group_parallel(ws)
    count, lst, tail = ws.count.cpu().numpy(), ws.list.cpu().numpy(), ws.buf[ws.offsets[4]:].view(torch.int32).cpu().numpy()
    rc, rl = moe.group_reference(ids, E)
    assert np.array_equal(count, rc)
    for e in range(E):
        assert np.array_equal(lst[e, :rc[e]], rl[e]) and (lst[e, rc[e]:] == SENTINEL).all(), e
    y0, scratch = (ws.offsets[5] - ws.offsets[4]) // 4, -(-P // 1024) * E
    assert (tail[:y0] == NAN32).all() and (tail[y0 + scratch:] == NAN32).all()


def test_route_parallel_is_route(dev):
    """600 rows (a row of NaNs among them), k = 2 of 8: 1200 pairs, two chunks -- ids and weights bit for bit, count and the live part of the lists equal"""
    from tinychatengine_amd import moe
    rng = np.random.default_rng(5)
    x, Wr = rng.normal(0, 1, (600, 128)).astype(np.float16), rng.normal(0, 1, (8, 128)).astype(np.float16)
    x[77] = np.nan
    got = []
    for parallel in (False, True):
        ws = moe.MoeWorkspace(600, 2, 8, 128, dev)
        moe.route(*_t(dev, x, Wr), ws, parallel=parallel)
        got.append([v.cpu().numpy() for v in (ws.ids, ws.weights.view(torch.int32), ws.count, ws.list)])
    (ids, w, count, lst), (pids, pw, pcount, plst) = got
    assert np.array_equal(ids, pids) and np.array_equal(w, pw) and np.array_equal(count, pcount) and count.sum() == 1200
    assert all(np.array_equal(lst[e, :count[e]], plst[e, :count[e]]) for e in range(8))


def test_layer_is_the_same_and_follows_a_graph(dev):
    """MoeFFN(256, 128, 4, 2) over 300 rows: act, y and C with parallel_group_from = 0 are those of a threshold never reached; then the six launches in one
    torch.cuda.graph: replays after x is rewritten on the device (another routing) equal the eager results, twice each"""
    from tinychatengine_amd import moe
    ffn, rng = moe.MoeFFN(256, 128, 4, 2, dev, seed=1, parallel_group_from=0), np.random.default_rng(19)
    x, C = rng.normal(0, 1, (300, 256)).astype(np.float16), rng.normal(0, 1, (300, 256)).astype(np.float16)
    cases = [(x, C), (x[::-1].copy(), C)]
    parallel = [_forward_bits(ffn, v, c) for v, c in cases]
    ffn.parallel_group_from = NEVER
    assert [_forward_bits(ffn, v, c) for v, c in cases] == parallel
    ffn.parallel_group_from = 0
    xt, ct, s = *_t(dev, x, C), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ffn.forward(xt, ct)  # (warm-up on the capture stream)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ffn.forward(xt, ct)
    for (v, c), want in list(zip(cases, parallel)) * 2:
        xt.copy_(_t(dev, v)[0])
        ct.copy_(_t(dev, c)[0])
        graph.replay()
        assert [r[2] for r in want] == [row.tobytes() for row in ct.cpu().numpy()]
