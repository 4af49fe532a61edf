"""The LoRA kernels through the C ABI (tce_lora_shrink_f16, tce_lora_expand_add_f16) on the designed operands of tests/lora_cases.py, at the smallest shapes that can
break them (lora_cases.GPU_SHAPES says why each size is there).

Every launch pair runs on a C with leading dimension N + 16, an x with leading dimension K + 8, one guard row behind C and behind t, and C's untouched memory poisoned
with a pattern that includes -0.0 and NaN payloads:

* `exact` cases equal lora_reference bit for bit; `bounded` cases stay inside lora_cases.bound (every element; the worst ratio is recorded);
* rows whose word is -1, n_adapters, -7 or 2^31 - 1 hold the poison pattern in C and keep its bits, and so do the padding columns and the guard rows of C and t;
* a row's bits (t and C) do not depend on the other rows' words, the row's index in the launch, or `rows`;
* the same results under torch.cuda.graph; a replay picks up a row_adapter word and an adapter rewritten between replays.
"""
import numpy as np
import pytest

import lora_cases as lc
from conftest import record_parity

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = np.array([0x8000, 0x7E01, 0xFDFF, 0x7C00, 0x8001, 0x7FFF, 0xFC00, 0x3C00], np.uint16)  # -0.0, NaN payloads, +inf, a subnormal, NaN, -inf, 1.0
T_POISON = 0x7FC12345  # an fp32 NaN payload: t where nothing was written


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


class _Device:
    """A case on the device: x with ldx = K + 8, the pool, and per run a fresh poisoned C (ldc = N + 16, one guard row) and t (one guard row)."""

    def __init__(self, dev, case):
        self.dev, self.case = dev, case
        rows, K = case["x"].shape
        self.rows, self.K, self.N, self.R = rows, K, case["C"].shape[1], case["A"].shape[1]
        xh = np.tile(POISON, (rows * (K + 8) + 7) // 8)[:rows * (K + 8)].reshape(rows, K + 8).copy()
        xh[:, :K] = case["x"].view(np.uint16)
        self.x_full = torch.from_numpy(xh.view(np.float16)).to(dev)
        self.A, self.B = torch.from_numpy(case["A"]).to(dev), torch.from_numpy(case["B"]).to(dev)
        self.scale = torch.from_numpy(case["scale"]).to(dev)

    def fresh(self, on=None):
        """on: bool [rows], the rows whose word names an adapter of the pool; every OTHER row of C is the poison pattern too (-0.0, NaN payloads, infinities), so a
        kernel that rewrote such a row -- as fp16(float(C) + 0), say -- would lose bits the comparison with `before` sees"""
        rows, N, R = self.rows, self.N, self.R
        ch = np.tile(POISON, ((rows + 1) * (N + 16) + 7) // 8)[:(rows + 1) * (N + 16)].reshape(rows + 1, N + 16).copy()
        keep = np.ones(rows, bool) if on is None else np.asarray(on, bool)
        ch[:rows, :N][keep] = self.case["C"].view(np.uint16)[keep]
        return ch, torch.from_numpy(ch.view(np.float16)).to(self.dev), torch.full((rows + 1, R), float("nan"), dtype=torch.float32, device=self.dev).view(torch.int32).fill_(T_POISON).view(torch.float32)

    def launch(self, words_t, c_full, t_full):
        from tinychatengine_amd.lora import expand_add, shrink
        shrink(self.x_full[:, :self.K], self.A, words_t, t_full, rows=self.rows)
        expand_add(t_full, self.B, self.scale, words_t, c_full[:self.rows, :self.N], rows=self.rows)

    def run(self, words):
        """-> (C fp16 [rows][N] as numpy, t fp32 [rows][R] as int32 bits); asserts that padding columns, guard rows and unwritten t rows kept their bits"""
        words_t = torch.from_numpy(np.asarray(words).astype(np.int64).astype(np.int32)).to(self.dev)
        on = (np.asarray(words) >= 0) & (np.asarray(words) < self.A.shape[0])
        before, c_full, t_full = self.fresh(on)
        assert on.all() or {0x8000, 0x7E01, 0xFDFF} <= set(before[:self.rows, :self.N][~on].reshape(-1).tolist()), "the untouched rows must hold -0.0 and NaN payloads"
        self.launch(words_t, c_full, t_full)
        torch.cuda.synchronize()
        after = c_full.cpu().numpy().view(np.uint16)
        tb = t_full.cpu().numpy().view(np.int32)
        assert np.array_equal(after[self.rows], before[self.rows]) and np.array_equal(after[:, self.N:], before[:, self.N:]), "memory behind C's rows was written"
        assert np.all(tb[self.rows] == T_POISON), "memory behind t was written"
        assert np.all(tb[:self.rows][~on] == T_POISON), "t of a row without an adapter was written"
        assert np.array_equal(after[:self.rows, :self.N][~on], before[:self.rows, :self.N][~on]), "a row without an adapter lost its bits"
        return after[:self.rows, :self.N].copy().view(np.float16), tb[:self.rows].copy()


@pytest.mark.parametrize("shape", lc.GPU_SHAPES, ids=lambda s: "rows{}-K{}-N{}-R{}-n{}".format(*s[:5]))
def test_kernels_on_designed_cases(dev, shape):
    rows, K, N, R, n, names = shape
    pats = lc.patterns(rows, n)
    exact, bounded = lc.exact_case(21, rows, K, N, R, n), lc.bounded_case(22, rows, K, N, R, n)
    de, db = _Device(dev, exact), _Device(dev, bounded)
    for name in names:
        words = pats[name]
        on = (words >= 0) & (words < n)  # (the other rows hold the poison pattern and were compared with it in run())
        got, _ = de.run(words)
        ref = lc.reference(exact, words)
        assert np.array_equal(got[on].view(np.uint16), ref[on].view(np.uint16)), f"exact / {name}: {int((got[on].view(np.uint16) != ref[on].view(np.uint16)).sum())} elements differ from lora_reference"
        got, _ = db.run(words)
        b = lc.bound(bounded, words)[on]
        err = np.abs(got[on].astype(np.float64) - lc.reference64(bounded, words)[on])
        ratio = float((err / np.maximum(b, 1e-300)).max()) if b.any() else 0.0
        print(f"lora bounded rows={rows} K={K} N={N} R={R} n={n} {name}: worst |err| / bound = {ratio:.4f}")
        record_parity(f"lora bounded rows={rows} K={K} N={N} R={R} n={n} {name}", {"worst_ratio": ratio, "n": int(err.size)})
        assert np.all(err <= b), f"bounded / {name}: worst |err| / bound = {ratio}"


def test_a_rows_bits_do_not_depend_on_its_neighbours_its_index_or_rows(dev):
    """Row 5 of a 17-row bounded case (K 2056: a ragged last step of the 64 lanes; R 48, N 1032, four adapters) on adapter 2: in its launch with every other row on
    another adapter, on the same adapter (it then shares passes of four), on none; alone as rows = 1; as the last row of a second block; among 130 rows."""
    rows, K, N, R, n = 17, 2056, 1032, 48, 4
    case = lc.bounded_case(31, rows, K, N, R, n)
    base_words = np.arange(rows) % n
    base_words[5] = 2
    want_c, want_t = _Device(dev, case).run(base_words)
    want_c, want_t = want_c[5].view(np.uint16), want_t[5]
    assert np.any(want_c != case["C"][5].view(np.uint16))

    def moved(index, total, words):
        c = {k: v for k, v in case.items()}
        src = np.arange(total) % rows
        src[index] = 5
        c["x"], c["C"] = case["x"][src].copy(), case["C"][src].copy()
        w = np.asarray(words).copy()
        w[index] = 2
        gc, gt = _Device(dev, c).run(w)
        return gc[index].view(np.uint16), gt[index]

    for what, (index, total, words) in {"same adapter everywhere": (5, rows, np.full(rows, 2)), "no other adapter": (5, rows, np.full(rows, -1)),
                                        "alone": (0, 1, np.array([2])), "last of a second block": (16, rows, base_words[::-1]),
                                        "among 130 rows": (129, 130, np.arange(130) % n), "among 130 rows of its adapter": (77, 130, np.full(130, 2))}.items():
        gc, gt = moved(index, total, words)
        assert np.array_equal(gt, want_t), f"{what}: t differs"
        assert np.array_equal(gc, want_c), f"{what}: C differs"


def test_graph_replay_follows_the_words_and_the_pool(dev):
    rows, K, N, R, n = 17, 520, 1032, 48, 4
    case = lc.bounded_case(41, rows, K, N, R, n)
    d = _Device(dev, case)
    pats = lc.patterns(rows, n)
    eager = {name: d.run(pats[name])[0].view(np.uint16) for name in ("different", "mixed")}
    words_t = torch.from_numpy(pats["different"].astype(np.int32)).to(dev)
    _, c0, t_full = d.fresh()
    c_full = c0.clone()
    d.launch(words_t, c_full, t_full)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c_full.copy_(c0)
        d.launch(words_t, c_full, t_full)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(c_full[:rows, :N].cpu().numpy().view(np.uint16), eager["different"]), "graph replay differs from the eager run"
    # another set of words, written on the device between replays
    words_t.copy_(torch.from_numpy(pats["mixed"].astype(np.int64).astype(np.int32)))
    g.replay()
    torch.cuda.synchronize()
    on = (pats["mixed"] >= 0) & (pats["mixed"] < n)  # (run() poisons the other rows; here they hold the case's C and must keep it)
    c0_bits = c0[:rows, :N].cpu().numpy().view(np.uint16)
    got = c_full[:rows, :N].cpu().numpy().view(np.uint16)
    assert np.array_equal(got[on], eager["mixed"][on]) and np.array_equal(got[~on], c0_bits[~on]), "the replay did not pick up the new row_adapter words"
    # an adapter reloaded between replays: adapter 0 takes adapter 3's contents
    d.A[0].copy_(d.A[3])
    d.B[0].copy_(d.B[3])
    d.scale[0:1].copy_(d.scale[3:4])
    g.replay()
    torch.cuda.synchronize()
    swapped = {k: v.copy() for k, v in case.items() if k != "kind"}
    swapped["A"][0], swapped["B"][0], swapped["scale"][0] = case["A"][3], case["B"][3], case["scale"][3]
    want = _Device(dev, swapped).run(pats["mixed"])[0].view(np.uint16)
    got = c_full[:rows, :N].cpu().numpy().view(np.uint16)
    assert np.array_equal(got[on], want[on]) and np.array_equal(got[~on], c0_bits[~on]), "the replay did not pick up the reloaded adapter"
    assert not np.array_equal(got[on], eager["mixed"][on])
