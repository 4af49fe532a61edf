"""The tiled form of the adapted linear (tce_lora_shrink_tiled_f16, tce_lora_expand_add_tiled_f16; LoraPool(..., tiled_from=)) on the designed operands of
tests/lora_cases.py, against lora_reference / float64.  SHAPES (rows, K, N, R, n): K shorter than an MFMA step; a K tail; two slices with an 8-k remainder; the largest
K (14 slices) and R; R with half an MFMA tile (8, 24); tiles of 1, 17, 33 and 130 rows.  Every launch pair runs on padded leading dimensions (x K + 8, C N + 16), with a
guard row behind C and behind the partial sums, and poisoned memory (-0.0, NaN payloads) wherever nothing may be written or read."""
import numpy as np
import pytest

import lora_cases as lc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = np.array([0x8000, 0x7E01, 0xFDFF, 0x7C00, 0x8001, 0x7FFF, 0xFC00, 0x3C00], np.uint16)  # -0.0, NaN payloads, +inf, a subnormal, NaN, -inf, 1.0
P_POISON = 0x7FC12345  # an fp32 NaN payload: a partial sum nothing wrote
SHAPES = [(1, 8, 8, 8, 1), (17, 40, 40, 24, 4), (33, 2056, 1032, 48, 4), (130, 2056, 136, 8, 4), (17, 14336, 8, 192, 1)]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available() and capi.lib()
    return torch.device("cuda:0")


def runs(rows, n):
    """contiguous runs of lengths 5, 16, 1, 20, ... over adapters 0 .. n - 1 and -1: 32-row tiles hold several adapters and tile edges fall inside runs"""
    lengths, vals, out, i = (5, 16, 1, 20, 3, 11), list(range(n)) + [-1], [], 0
    while len(out) < rows:
        out += [vals[i % len(vals)]] * lengths[i % len(lengths)]
        i += 1
    return np.array(out[:rows], np.int64)


def _poisoned(rows, cols):
    return np.tile(POISON, (rows * cols + 7) // 8)[:rows * cols].reshape(rows, cols).copy()


class _Device:
    """A case on the device: x with ldx = K + 8, the pool; per run a poisoned C (ldc = N + 16, one guard row) and poisoned partial sums (one guard row)."""

    def __init__(self, dev, case):
        from tinychatengine_amd.lora import tiled_slices
        self.dev, self.case = dev, case
        self.rows, self.K = case["x"].shape
        self.N, self.R, self.n = case["C"].shape[1], case["A"].shape[1], case["A"].shape[0]
        xh = _poisoned(self.rows, self.K + 8)
        xh[:, :self.K] = case["x"].view(np.uint16)
        self.x = torch.from_numpy(xh.view(np.float16)).to(dev)[:, :self.K]
        self.A, self.B, self.scale = (torch.from_numpy(case[k]).to(dev) for k in ("A", "B", "scale"))
        self.S = tiled_slices(self.K)

    def fresh(self, on):
        ch = _poisoned(self.rows + 1, self.N + 16)
        ch[:self.rows, :self.N][on] = self.case["C"].view(np.uint16)[on]
        part = torch.full((self.S * self.rows + 1, self.R), P_POISON, dtype=torch.int32, device=self.dev).view(torch.float32)
        return ch, torch.from_numpy(ch.view(np.float16)).to(self.dev), part

    def launch(self, words_t, c_full, part):
        from tinychatengine_amd.lora import expand_add_tiled, shrink_tiled
        p = part[:self.S * self.rows].view(self.S, self.rows, self.R)
        shrink_tiled(self.x, self.A, words_t, p)
        expand_add_tiled(p, self.B, self.scale, words_t, c_full[:self.rows, :self.N], self.K)

    def run(self, words):
        """-> (C as uint16 bits [rows][N], the partial sums as int32 bits [S][rows][R]); asserts that everything that must stay untouched kept its bits"""
        on = (np.asarray(words) >= 0) & (np.asarray(words) < self.n)
        before, c_full, part = self.fresh(on)
        self.launch(torch.from_numpy(np.asarray(words).astype(np.int64).astype(np.int32)).to(self.dev), c_full, part)
        torch.cuda.synchronize()
        after, pb = c_full.cpu().numpy().view(np.uint16), part.cpu().numpy().view(np.int32)
        assert np.array_equal(after[self.rows], before[self.rows]) and np.array_equal(after[:, self.N:], before[:, self.N:]), "C's guard row or padding was written"
        assert np.array_equal(after[:self.rows, :self.N][~on], before[:self.rows, :self.N][~on]), "a row without an adapter lost its bits"
        pb, guard = pb[:-1].reshape(self.S, self.rows, self.R), pb[-1]
        assert np.all(guard == P_POISON) and np.all(pb[:, ~on] == P_POISON), "a partial sum of a row without an adapter, or behind the workspace, was written"
        return after[:self.rows, :self.N].copy(), pb


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "rows{}-K{}-N{}-R{}-n{}".format(*s))
def test_tiled_kernels_on_designed_cases(dev, shape):
    rows, n = shape[0], shape[4]
    exact, bounded = lc.exact_case(51, *shape), lc.bounded_case(52, *shape)
    de, db = _Device(dev, exact), _Device(dev, bounded)
    for name, words in {**lc.patterns(rows, n), "runs": runs(rows, n)}.items():
        on = (words >= 0) & (words < n)
        got, _ = de.run(words)
        ref = lc.reference(exact, words).view(np.uint16)
        assert np.array_equal(got[on], ref[on]), f"exact / {name}: {int((got[on] != ref[on]).sum())} elements differ from lora_reference"
        got, _ = db.run(words)
        b = lc.bound(bounded, words)[on]
        err = np.abs(got.view(np.float16)[on].astype(np.float64) - lc.reference64(bounded, words)[on])
        ratio = float((err / np.maximum(b, 1e-300)).max()) if b.size else 0.0
        print(f"lora tiled bounded {shape} {name}: worst |err| / bound = {ratio:.4f}")
        assert np.all(err <= b), f"bounded / {name}: worst |err| / bound = {ratio}"


def test_a_rows_bits_do_not_depend_on_its_index_its_neighbours_or_rows(dev):
    """Row 5 of a 17-row bounded case on adapter 2 (K 2056: two slices; R 48; N 136), moved and surrounded"""
    rows, K, N, R, n = 17, 2056, 136, 48, 4
    case = lc.bounded_case(61, rows, K, N, R, n)
    base = np.arange(rows) % n
    base[5] = 2
    c, p = _Device(dev, case).run(base)
    want_c, want_p = c[5], p[:, 5]
    assert np.any(want_c != case["C"][5].view(np.uint16))

    def moved(index, total, words, nan_neighbours=False):
        src = np.arange(total) % rows
        src[index] = 5
        c2 = dict(case, x=case["x"][src].copy(), C=case["C"][src].copy())
        if nan_neighbours:
            c2["x"][np.arange(total) != index] = np.nan
        w = np.asarray(words).copy()
        w[index] = 2
        gc, gp = _Device(dev, c2).run(w)
        return gc[index], gp[:, index]

    for what, args in {"same adapter everywhere": (5, rows, np.full(rows, 2)), "no other adapter": (5, rows, np.full(rows, -1)), "alone": (0, 1, np.array([2])),
                       "index 40 of 45": (40, 45, np.arange(45) % n), "NaN neighbours on its adapter": (5, rows, np.full(rows, 2), True),
                       "NaN neighbours on other adapters": (40, 45, (np.arange(45) + 1) % n, True)}.items():
        gc, gp = moved(*args)
        assert np.array_equal(gp, want_p), f"{what}: the partial sums differ"
        assert np.array_equal(gc, want_c), f"{what}: C differs"


def test_graph_replay_follows_the_words_and_the_pool(dev):
    rows, K, N, R, n = 40, 2056, 136, 48, 4
    case = lc.bounded_case(71, rows, K, N, R, n)
    d = _Device(dev, case)
    first, second = runs(rows, n), lc.patterns(rows, n)["mixed"]
    words_t = torch.from_numpy(first.astype(np.int32)).to(dev)
    _, c0, part = d.fresh(np.ones(rows, bool))
    c_full = c0.clone()
    d.launch(words_t, c_full, part)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c_full.copy_(c0)
        d.launch(words_t, c_full, part)

    def replayed():
        g.replay()
        torch.cuda.synchronize()
        return c_full[:rows, :N].cpu().numpy().view(np.uint16)

    def eager(dd, words):  # (run() poisons the rows without an adapter; in the graph they hold the case's C and must keep it)
        on = (words >= 0) & (words < n)
        want = case["C"].view(np.uint16).copy()
        want[on] = dd.run(words)[0][on]
        return want

    assert np.array_equal(replayed(), eager(d, first)) and np.array_equal(replayed(), eager(d, first)), "graph replays differ from the eager run"
    words_t.copy_(torch.from_numpy(second.astype(np.int64).astype(np.int32)))  # other words, written on the device between replays
    assert np.array_equal(replayed(), eager(d, second)), "the replay did not pick up the new row_adapter words"
    for held in (d.A, d.B, d.scale):  # an adapter reloaded between replays: adapter 0 takes adapter 3's contents
        held[0:1].copy_(held[3:4])
    swapped = {k: v.copy() for k, v in case.items() if k != "kind"}
    swapped["A"][0], swapped["B"][0], swapped["scale"][0] = case["A"][3], case["B"][3], case["scale"][3]
    got = replayed()
    assert np.array_equal(got, eager(_Device(dev, swapped), second)) and not np.array_equal(got, eager(_Device(dev, case), second)), "the replay did not pick up the reloaded adapter"


def test_lora_layer_dispatches_on_tiled_from(dev):
    """tiled_from=16: 40 rows run the tiled entry points, 15 rows the 4-row pair; a prefill_many of 24 + 17 rows (slot 0 on adapter 0, slot 1 on -1: lb.WORDS)"""
    import layer_bits_cases as lb
    from tinychatengine_amd import lora
    model = lb.Model(dev)

    def pool(**kw):
        p = lora.LoraPool(model.blocks[0], lb.LAYERS, lb.MAX_ADAPTERS, lb.RANK, dev, **kw)
        p.load(0, lb._adapter(1, lb.FIVE), alpha=8.0)
        p.load(1, lb._adapter(2, lb.FIVE, r=4), alpha=8.0)
        return p

    tiled = pool(tiled_from=16)
    lv, K = tiled.layer(0), lb.HEADS * lb.HD
    for m, fns in ((40, (lora.shrink_tiled, lambda t, *a: lora.expand_add_tiled(t, *a, K))), (15, (lora.shrink, lora.expand_add))):
        x, c0 = model.rows(m, 80 + m), model.rows(m, 90 + m)
        words = torch.from_numpy((runs(m, 2)).astype(np.int32)).to(dev)
        ws, c_layer, c_direct = lv.workspace(m), c0.clone(), c0.clone()
        assert tuple(ws["o"].shape) == ((lora.tiled_slices(K), m, lb.RANK) if m == 40 else (m, lb.RANK))
        lv.shrink("o", x, ws["o"], words)
        lv.expand_add("o", ws["o"], c_layer, words)
        t = torch.empty_like(ws["o"])
        fns[0](x, lv.A["o"], words, t)
        fns[1](t, lv.B["o"], tiled.scale, words, c_direct)
        assert torch.equal(c_layer.view(torch.int16), c_direct.view(torch.int16)) and not torch.equal(c_layer, c0), f"{m} rows: LoraLayer ran another form"

    out = {}
    for name, p in (("tiled", tiled), ("default", pool()), ("none", None)):
        adm = [(0, model.rows(24, 101), 0), (1, model.rows(17, 102), 0)]
        for d in model.decoders(True, p):
            d.prefill_many(adm)
        torch.cuda.synchronize()
        out[name] = [rows.cpu().numpy() for _, rows, _ in adm]
    assert np.array_equal(out["tiled"][1].view(np.uint16), out["default"][1].view(np.uint16)), "the slot without an adapter differs from the default pool's"
    assert np.isfinite(out["tiled"][0].astype(np.float32)).all() and not np.array_equal(out["tiled"][0], out["none"][0])
