"""The segmented tiled expands (tce_lora_expand_silu_mul_tiled_f16, tce_lora_expand_add_segmented_tiled_f16; LoraPool(..., tiled_from=, segmented=True)) on the designed
operands of tests/lora_cases.py / lora_gate_up_cases.py.  No tolerance: on the SAME partial sums they give the bits of tce_lora_expand_add_tiled_f16 on the block-structured
B (gate/up: then de-interleave and tce_silu_mul_half).  Padded leading dimensions (x K + 8, y 2N + 16, C N + 16) and a poisoned guard row behind C throughout."""
import numpy as np
import pytest

import lora_cases as lc
import lora_gate_up_cases as gc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = np.array([0x8000, 0x7E01, 0xFDFF, 0x7C00, 0x8001, 0x7FFF, 0xFC00, 0x3C00], np.uint16)  # -0.0, NaN payloads, +inf, a subnormal, NaN, -inf, 1.0
# (rows, K, N, R, n): one row; an N tail inside a 64-column tile; two K slices; three column tiles, the last of 8 columns; five row tiles; 2R = 192 with two chunks of j
SHAPES = [(1, 8, 8, 8, 1), (17, 40, 40, 24, 4), (33, 2056, 136, 48, 4), (130, 520, 72, 8, 4), (17, 2056, 8, 96, 1)]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available() and capi.lib()
    return torch.device("cuda:0")


def runs(rows, n):  # contiguous runs of lengths 5, 16, 1, 20, 3, 11 over adapters 0 .. n - 1 and -1: a 32-row tile holds several adapters, -1 rows and run edges
    return np.repeat(np.resize(np.r_[np.arange(n), -1], rows), np.resize([5, 16, 1, 20, 3, 11], rows))[:rows].astype(np.int64)  # (more runs than needed, cut)


def _padded(dev, a, pad, guard=0):
    """fp16 [rows][cols] -> (its bits inside a poisoned [rows + guard][cols + pad], that buffer on the device)"""
    h = np.resize(POISON, (a.shape[0] + guard) * (a.shape[1] + pad)).reshape(a.shape[0] + guard, a.shape[1] + pad).copy()
    h[:a.shape[0], :a.shape[1]] = a.view(np.uint16)
    return h, torch.from_numpy(h.view(np.float16)).to(dev)


def _words(dev, words):
    return torch.from_numpy(np.asarray(words).astype(np.int64).astype(np.int32)).to(dev)


def _silu_mul(dev, g, u):
    """tce_silu_mul_half on numpy fp16 -> fp16"""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import _stream
    gt, ut = torch.from_numpy(np.ascontiguousarray(g)).to(dev), torch.from_numpy(np.ascontiguousarray(u)).to(dev)
    capi.check(capi.lib().tce_silu_mul_half(gt.data_ptr(), ut.data_ptr(), gt.numel(), _stream()))
    return gt.cpu().numpy()


def _gate_up(dev, case, words, finite=True):
    """-> (C's bits from the tiled gate/up expand, the composition's bits), both from ONE shrink; y, C's guard row and its padding must keep their bits"""
    from tinychatengine_amd import lora
    (rows, K), (n, R, N), wt = case["x"].shape, case["Bg"].shape, _words(dev, words)
    A, Bg, Bu, scale, Bblock = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (case["A"], case["Bg"], case["Bu"], case["scale"], gc.block_structured(case)["B"]))
    x, (y_bits, y), (before, c) = _padded(dev, case["x"], 8)[1][:, :K], _padded(dev, case["y"], 16), _padded(dev, np.zeros((rows, N), np.float16), 16, guard=1)
    part = lora.tiled_workspace(rows, K, 2 * R, dev).fill_(float("nan"))  # (a partial nothing wrote must not be read)
    lora.shrink_tiled(x, A, wt, part)
    on = torch.from_numpy(np.nonzero((np.asarray(words) >= 0) & (np.asarray(words) < n))[0]).to(dev)
    assert not finite or bool(torch.isfinite(part[:, on]).all()), "a partial sum is not finite"
    lora.expand_silu_mul_tiled(part, Bg, Bu, scale, wt, y[:, :2 * N], c[:rows, :N], K)
    yc = y[:, :2 * N].clone(memory_format=torch.contiguous_format)
    lora.expand_add_tiled(part, Bblock, scale, wt, yc, K)
    y2, after = yc.cpu().numpy(), c.cpu().numpy().view(np.uint16)
    assert np.array_equal(y.cpu().numpy().view(np.uint16), y_bits), "y was written"
    assert np.array_equal(after[rows], before[rows]) and np.array_equal(after[:, N:], before[:, N:]), "C's guard row or padding was written"
    return after[:rows, :N].copy(), _silu_mul(dev, y2[:, 0::2], y2[:, 1::2]).view(np.uint16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "rows{}-K{}-N{}-R{}-n{}".format(*s))
def test_gate_up_tiled_is_the_tiled_expand_on_the_block_structured_b(dev, shape):
    from tinychatengine_amd.lora import lora_gate_up_reference
    rows, n = shape[0], shape[4]
    for kind, seed in (("exact", 81), ("bounded", 82)):
        case = gc.gate_up_case(kind, seed, *shape)
        plain = _silu_mul(dev, case["y"][:, 0::2], case["y"][:, 1::2]).view(np.uint16)
        changed = False
        for name, words in {**gc.words_patterns(rows, n), "runs": runs(rows, n)}.items():
            on = (words >= 0) & (words < n)
            got, want = _gate_up(dev, case, words)
            assert np.array_equal(got, want), f"{kind} / {name}: {int((got != want).sum())} elements differ from expand_add_tiled + de-interleave + silu_mul"
            assert np.array_equal(got[~on], plain[~on]), f"{kind} / {name}: a row without an adapter is not tce_silu_mul_half of y's columns"
            changed = changed or bool(np.any(got[on] != plain[on]))
            if kind == "exact":  # the anchor outside the kernels under comparison: g and u by the float64 definition
                ref = lora_gate_up_reference(case["x"], case["A"], case["Bg"], case["Bu"], case["scale"], words, case["y"], silu_mul=lambda g, u: _silu_mul(dev, g, u))
                assert np.array_equal(got, ref.view(np.uint16)), f"exact / {name}: differs from lora_gate_up_reference"
        assert changed, "the adapters changed nothing"


@pytest.mark.parametrize("rows,R,seg", [(17, 24, (0, 128, 256, 384)), (33, 48, (0, 128, 256, 384)), (33, 48, (0, 128, 136))], ids=str)
def test_segmented_expand_is_the_tiled_expand_and_reads_its_blocks_only(dev, rows, R, seg):
    """N 384 in three segments of 128 (three column tiles, one per segment), and N 136 in two (the last bound is N: an 8-column tail); K 2056 (two slices).  The tiled
    expand runs on B with zeros off the blocks; the segmented one on the same B with NaN there: it may not read them."""
    from tinychatengine_amd import lora
    K, N, n, segments = 2056, seg[-1], 4, len(seg) - 1
    case = lc.bounded_case(91, rows, K, N, R, n)
    off = np.ones((R, N), bool)
    for s in range(segments):
        off[s * R // segments:(s + 1) * R // segments, seg[s]:seg[s + 1]] = False
    Bz, Bnan = case["B"].copy(), case["B"].copy()
    Bz[:, off], Bnan[:, off] = 0, np.nan
    x, (A, scale, Bz, Bnan) = _padded(dev, case["x"], 8)[1][:, :K], (torch.from_numpy(a).to(dev) for a in (case["A"], case["scale"], Bz, Bnan))
    for name, words in {**lc.patterns(rows, n), "runs": runs(rows, n)}.items():
        on, wt = (words >= 0) & (words < n), _words(dev, words)
        part = lora.tiled_workspace(rows, K, R, dev).fill_(float("nan"))
        before, c_seg = _padded(dev, case["C"], 16, guard=1)
        c_tiled = c_seg.clone()
        lora.shrink_tiled(x, A, wt, part)
        lora.expand_add_tiled(part, Bz, scale, wt, c_tiled[:rows, :N], K)
        lora.expand_add_segmented_tiled(part, Bnan, scale, wt, c_seg[:rows, :N], K, seg)
        got, want = c_seg.cpu().numpy().view(np.uint16), c_tiled.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} elements differ from expand_add_tiled (guard row and padding included)"
        assert np.array_equal(got[:rows][~on], before[:rows][~on]), f"{name}: a row without an adapter lost its bits"
        assert not on.any() or np.any(got[:rows, :N][on] != before[:rows, :N][on]), f"{name}: the adapters changed nothing"


def test_a_gate_up_rows_bits_do_not_depend_on_its_index_its_neighbours_or_rows(dev):
    """Row 5 of a 17-row bounded case on adapter 2 (K 2056: two slices; 2R 48; N 136: three column tiles), moved and surrounded"""
    rows, K, N, R, n = 17, 2056, 136, 24, 4
    case = gc.gate_up_case("bounded", 101, rows, K, N, R, n)

    def row5(index, total, words, nan_neighbours=False):
        src, w = np.arange(total) % rows, np.asarray(words).copy()
        src[index], w[index] = 5, 2
        c2 = dict(case, x=case["x"][src].copy(), y=case["y"][src].copy())
        if nan_neighbours:
            c2["x"][np.arange(total) != index] = np.nan
        return _gate_up(dev, c2, w, finite=False)[0][index]

    want = row5(5, rows, np.arange(rows) % n)
    for what, args in {"same adapter everywhere": (5, rows, np.full(rows, 2)), "no other adapter": (5, rows, np.full(rows, -1)), "alone": (0, 1, np.array([2])),
                       "index 40 of 45": (40, 45, np.arange(45) % n), "NaN neighbours on its adapter": (5, rows, np.full(rows, 2), True),
                       "NaN neighbours on other adapters": (40, 45, (np.arange(45) + 1) % n, True)}.items():
        assert np.array_equal(row5(*args), want), f"{what}: C differs"


def test_lora_layer_dispatches_on_segmented(dev):
    """gate_up=True, tiled_from=16, segmented=True: 40 rows run the two segmented entry points, 15 rows the 4-row kernels; a prefill_many of 24 + 17 rows (slot 0 on
    adapter 0, slot 1 on -1: lb.WORDS)"""
    import layer_bits_cases as lb
    from tinychatengine_amd import lora
    model = lb.Model(dev)

    def pool(**kw):
        p = lora.LoraPool(model.blocks[0], lb.LAYERS, lb.MAX_ADAPTERS, lb.RANK, dev, gate_up=True, **kw)
        p.load(0, lb._adapter(1, tuple(lb.DIMS)), alpha=8.0)
        p.load(1, lb._adapter(2, ("gate_proj", "up_proj"), r=4), alpha=8.0)
        return p

    seg = pool(tiled_from=16, segmented=True)
    lv, K, S = seg.layer(0), lb.HIDDEN, lora.tiled_slices(lb.HIDDEN)
    for m in (40, 15):
        wide = torch.cat([model.rows(m, 70 + i + m) for i in range(6)], 1)
        x, c0, y, words = model.rows(m, 80 + m), wide[:, :768].contiguous(), wide[:, :2 * lb.FFN], torch.from_numpy(runs(m, 2).astype(np.int32)).to(dev)
        ws, c_layer, c_direct, a_layer, a_direct = lv.workspace(m), c0.clone(), c0.clone(), *torch.zeros(2, m, lb.FFN, dtype=torch.float16, device=dev)
        assert {t: tuple(ws[t].shape) for t in ("qkv", "gate_up")} == {t: ((S, m, r) if m == 40 else (m, r)) for t, r in (("qkv", 3 * lb.RANK), ("gate_up", 2 * lb.RANK))}
        lv.shrink("qkv", x, ws["qkv"], words)
        lv.expand_add("qkv", ws["qkv"], c_layer, words)
        lv.shrink("gate_up", x, ws["gate_up"], words)
        lv.expand_silu_mul(ws["gate_up"], y, a_layer, words)
        tq, tg = torch.empty_like(ws["qkv"]), torch.empty_like(ws["gate_up"])
        for A, t in ((lv.A["qkv"], tq), (lv.A["gate_up"], tg)):
            (lora.shrink_tiled if m == 40 else lora.shrink)(x, A, words, t)
        if m == 40:
            lora.expand_add_segmented_tiled(tq, lv.B["qkv"], seg.scale, words, c_direct, K, (0, 512, 640, 768))
            lora.expand_silu_mul_tiled(tg, lv.Bg, lv.Bu, seg.scale, words, y, a_direct, K)
        else:
            lora.expand_add(tq, lv.B["qkv"], seg.scale, words, c_direct)
            lora.expand_silu_mul(tg, lv.Bg, lv.Bu, seg.scale, words, y, a_direct)
        assert torch.equal(c_layer.view(torch.int16), c_direct.view(torch.int16)) and not torch.equal(c_layer, c0), f"{m} rows: LoraLayer ran another q/k/v form"
        assert torch.equal(a_layer.view(torch.int16), a_direct.view(torch.int16)) and bool(a_layer.any()), f"{m} rows: LoraLayer ran another gate/up form"

    out = {}
    for name, p in (("segmented", seg), ("default", pool()), ("none", None)):
        adm = [(0, model.rows(24, 101), 0), (1, model.rows(17, 102), 0)]
        for d in model.decoders(True, p):
            d.prefill_many(adm)
        torch.cuda.synchronize()
        out[name] = [rows.cpu().numpy() for _, rows, _ in adm]
    assert np.array_equal(out["segmented"][1].view(np.uint16), out["default"][1].view(np.uint16)), "the slot without an adapter differs from the default pool's"
    assert np.isfinite(out["segmented"][0].astype(np.float32)).all() and not np.array_equal(out["segmented"][0], out["none"][0])
