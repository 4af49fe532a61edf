"""tce_lora_expand_silu_mul_f16 (tinychatengine_amd/csrc/lora.hip) on the designed operands of tests/lora_gate_up_cases.py.  The contract needs no tolerance: C is
BIT-IDENTICAL to the composition of kernels the suite already holds, on the SAME t (one tce_lora_shrink_f16 with gate's and up's A stacked):

    1  tce_lora_expand_add_f16 on a copy of y with the block-structured B' [2R][2N] (gate's rows in the even columns, up's in the odd, zeros elsewhere)
    2  de-interleave
    3  tce_silu_mul_half

Every launch runs on a y with leading dimension 2N + 16 and a C with leading dimension N + 16 and one guard row, the padding and the guard rows holding canaries; y
is only read.  y carries -0.0 and values near +-65504 (rows on an adapter then overflow to infinities in g or u: the same bits in both forms).

* rows 1 / 3 / 4 / 5 / 17 / 130, K 8 / 2056, N 8 / 520 / 1032, R 8 / 24 / 64 / 96, 1 / 4 / 64 adapters; the word patterns of lora_cases.patterns plus one with -7 and
  n_adapters in every block of four;
* a row without an adapter equals tce_silu_mul_half on the plain launch's columns; exact cases: a row on an adapter equals tce_silu_mul_half on the float64 g and u;
* a row's bits do not depend on its index in the launch, on `rows` or on its neighbours' words;
* a graph replay follows rewritten words and a reloaded adapter;
* the base gate_up linear + this launch with every word on -1 equals the TCE_W4_SILU_MUL_PAIRS launch of the same linear at M = 1 and 4;
* the entry point's refusals (tests/test_lora_gate_up_host.py's, here beside a device).
"""
import ctypes as C

import numpy as np
import pytest

import lora_cases as lc
import lora_gate_up_cases as gc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = np.array([0x7E01, 0xFDFF, 0x7C00, 0x8001, 0x7FFF, 0xFC00, 0x3C00, 0x8000], np.uint16)  # NaN payloads, infinities, a subnormal, 1.0, -0.0
SPECIAL = np.array([0x8000, 0x7BFF, 0xFBFF, 0x7BFE, 0xFBF0, 0x0000, 0x8001, 0x7800], np.uint16)  # -0.0, +-65504, their neighbours, +0, a subnormal, 32768

# (rows, K, N, R, n_adapters): every size of the list above at least once; 130 rows: 33 blocks, the last of two rows; N 520 / 1032: one full workgroup of 512 columns
# and one lane more / two and one lane more; R 24 / 96: an odd number of 8-row steps under the loop's unroll of 2, and the largest R (2R = TCE_LORA_MAX_RANK)
GPU_SHAPES = [(1, 8, 8, 8, 1), (3, 2056, 520, 24, 4), (4, 8, 1032, 64, 4), (5, 8, 520, 96, 64), (17, 2056, 1032, 96, 4), (130, 8, 520, 8, 4), (130, 2056, 1032, 24, 1)]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _with_specials(case):
    """the case with -0.0, +-65504 and their neighbours written over the first 8 columns of every row of y (4 gate / up pairs)"""
    c = dict(case)
    y = case["y"].copy()
    y.view(np.uint16)[:, :8] = SPECIAL
    c["y"] = y
    return c


class _Device:
    """A case on the device: the pool, B' for the composition, x; per run a y with ldy = 2N + 16 and a C with ldc = N + 16 and a guard row, canaries in the padding."""

    def __init__(self, dev, case):
        self.dev, self.case = dev, case
        self.rows, self.K = case["x"].shape
        self.n, self.R, self.N = case["Bg"].shape
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.x, self.A, self.Bg, self.Bu, self.scale = up(case["x"]), up(case["A"]), up(case["Bg"]), up(case["Bu"]), up(case["scale"])
        self.Bblock = up(gc.block_structured(case)["B"])
        yh = np.tile(CANARY, ((self.rows + 1) * (2 * self.N + 16) + 7) // 8)[:(self.rows + 1) * (2 * self.N + 16)].reshape(self.rows + 1, 2 * self.N + 16).copy()
        yh[:self.rows, :2 * self.N] = case["y"].view(np.uint16)
        self.y_bits = yh
        self.y_full = up(yh.view(np.float16))
        self.t = torch.empty((self.rows, 2 * self.R), dtype=torch.float32, device=dev)

    def fresh_c(self):
        ch = np.tile(CANARY, ((self.rows + 1) * (self.N + 16) + 7) // 8)[:(self.rows + 1) * (self.N + 16)].reshape(self.rows + 1, self.N + 16).copy()
        return ch, torch.from_numpy(ch.view(np.float16)).to(self.dev)

    def launch(self, words_t, c_full):
        from tinychatengine_amd.lora import expand_silu_mul, shrink
        shrink(self.x, self.A, words_t, self.t)
        expand_silu_mul(self.t, self.Bg, self.Bu, self.scale, words_t, self.y_full[:self.rows, :2 * self.N], c_full[:self.rows, :self.N], rows=self.rows)

    def words(self, words):
        return torch.from_numpy(np.asarray(words).astype(np.int64).astype(np.int32)).to(self.dev)

    def run(self, words):
        """-> C fp16 [rows][N] as uint16 bits; asserts that y, C's padding columns and C's guard row kept their bits and that every row of C was written"""
        before, c_full = self.fresh_c()
        self.launch(self.words(words), c_full)
        torch.cuda.synchronize()
        after = c_full.cpu().numpy().view(np.uint16)
        assert np.array_equal(self.y_full.cpu().numpy().view(np.uint16), self.y_bits), "y was written"
        assert np.array_equal(after[self.rows], before[self.rows]) and np.array_equal(after[:, self.N:], before[:, self.N:]), "memory behind C's rows was written"
        return after[:self.rows, :self.N].copy()

    def silu_mul(self, g, u):
        """tce_silu_mul_half on numpy fp16 [rows][N] -> bits"""
        from tinychatengine_amd import capi
        from tinychatengine_amd.linear import _stream
        gt, ut = torch.from_numpy(np.ascontiguousarray(g)).to(self.dev), torch.from_numpy(np.ascontiguousarray(u)).to(self.dev)
        capi.check(capi.lib().tce_silu_mul_half(gt.data_ptr(), ut.data_ptr(), gt.numel(), _stream()))
        return gt.cpu().numpy().view(np.uint16)

    def composition(self, words):
        """the three existing kernels on the SAME t (the shrink is launched again: same kernel, same operands) -> bits [rows][N]"""
        from tinychatengine_amd.lora import expand_add, shrink
        wt = self.words(words)
        yc = self.y_full[:self.rows, :2 * self.N].clone(memory_format=torch.contiguous_format)  # (a copy even where the slice counts as contiguous: one row)
        shrink(self.x, self.A, wt, self.t)
        expand_add(self.t, self.Bblock, self.scale, wt, yc)
        y2 = yc.cpu().numpy()
        return self.silu_mul(y2[:, 0::2], y2[:, 1::2])


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "rows{}-K{}-N{}-R{}-n{}".format(*s))
def test_bit_identical_to_expand_add_deinterleave_silu_mul(dev, shape):
    rows, K, N, R, n = shape
    pats = gc.words_patterns(rows, n)
    for kind, seed in (("exact", 61), ("bounded", 62)):
        case = gc.gate_up_case(kind, seed, *shape)
        if kind == "bounded":
            case = _with_specials(case)
        d = _Device(dev, case)
        plain = d.silu_mul(case["y"][:, 0::2], case["y"][:, 1::2])
        changed = False
        for name, words in pats.items():
            on = (words >= 0) & (words < n)
            got = d.run(words)
            want = d.composition(words)
            assert np.array_equal(got, want), f"{kind} / {name}: {int((got != want).sum())} elements differ from expand_add + de-interleave + silu_mul"
            assert np.array_equal(got[~on], plain[~on]), f"{kind} / {name}: a row without an adapter is not tce_silu_mul_half of the plain launch's columns"
            changed = changed or bool(on.any() and np.any(got[on] != plain[on]))
            if kind == "exact" and on.any():  # an anchor outside the kernels under comparison: g and u by the float64 definition
                g64, u64 = lc.reference(gc.segment(case, "gate"), words), lc.reference(gc.segment(case, "up"), words)
                assert np.array_equal(got[on], d.silu_mul(g64, u64)[on]), f"exact / {name}: differs from SiLU * mul of the float64 g and u"
        assert changed, "the adapters changed nothing"


def test_a_rows_bits_do_not_depend_on_its_neighbours_its_index_or_rows(dev):
    """Row 5 of a 17-row bounded case on adapter 2: among rows on other adapters, on its own adapter (it then shares passes of four), on none; alone as rows = 1; as
    the last row of a second block; among 130 rows."""
    rows, K, N, R, n = 17, 520, 1032, 24, 4
    case = gc.gate_up_case("bounded", 71, rows, K, N, R, n)
    base_words = np.arange(rows) % n
    base_words[5] = 2
    want = _Device(dev, case).run(base_words)[5]
    plain5 = _Device(dev, case).run(np.full(rows, -1))[5]
    assert np.any(want != plain5)

    def moved(index, total, words):
        c = dict(case)
        src = np.arange(total) % rows
        src[index] = 5
        c["x"], c["y"] = case["x"][src].copy(), case["y"][src].copy()
        w = np.asarray(words).copy()
        w[index] = 2
        return _Device(dev, c).run(w)[index]

    for what, (index, total, words) in {"same adapter everywhere": (5, rows, np.full(rows, 2)), "no other adapter": (5, rows, np.full(rows, -1)),
                                        "alone": (0, 1, np.array([2])), "last of a second block": (16, rows, base_words[::-1]),
                                        "three of a block on its adapter": (6, rows, np.array([0, 1, 3, 0, 2, 2, 0, -1] + [1] * 9)),
                                        "among 130 rows": (129, 130, np.arange(130) % n), "among 130 rows of its adapter": (77, 130, np.full(130, 2))}.items():
        assert np.array_equal(moved(index, total, words), want), f"{what}: C differs"
    # and without an adapter: the row's bits are the plain ones wherever it sits
    c = dict(case)
    src = np.arange(130) % rows
    src[129] = 5
    c["x"], c["y"] = case["x"][src].copy(), case["y"][src].copy()
    w = np.arange(130) % n
    w[129] = n
    assert np.array_equal(_Device(dev, c).run(w)[129], plain5)


def test_graph_replay_follows_the_words_and_the_pool(dev):
    rows, K, N, R, n = 17, 520, 1032, 24, 4
    case = gc.gate_up_case("bounded", 81, rows, K, N, R, n)
    d = _Device(dev, case)
    pats = gc.words_patterns(rows, n)
    eager = {name: d.run(pats[name]) for name in ("different", "outside")}
    words_t = d.words(pats["different"])
    _, c_full = d.fresh_c()
    d.launch(words_t, c_full)  # warm-up outside the capture
    torch.cuda.synchronize()
    c_full.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.launch(words_t, c_full)
    g.replay()
    torch.cuda.synchronize()
    got = lambda: c_full[:rows, :N].cpu().numpy().view(np.uint16)
    assert np.array_equal(got(), eager["different"]), "graph replay differs from the eager run"
    words_t.copy_(d.words(pats["outside"]))  # another set of words, written on the device between replays
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(got(), eager["outside"]) and not np.array_equal(eager["outside"], eager["different"]), "the replay did not pick up the new row_adapter words"
    # an adapter reloaded between replays: adapter 0 takes adapter 3's contents
    d.A[0].copy_(d.A[3])
    d.Bg[0].copy_(d.Bg[3])
    d.Bu[0].copy_(d.Bu[3])
    d.scale[0:1].copy_(d.scale[3:4])
    g.replay()
    torch.cuda.synchronize()
    swapped = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    for k in ("A", "Bg", "Bu", "scale"):
        swapped[k][0] = case[k][3]
    want = _Device(dev, swapped).run(pats["outside"])
    assert np.array_equal(got(), want) and not np.array_equal(want, eager["outside"]), "the replay did not pick up the reloaded adapter"


@pytest.mark.parametrize("M", [1, 4])
def test_unadapted_rows_equal_the_fused_pair_launch(dev, M):
    """The tiny model's gate_up linear (hidden 512 -> 2 * 1408): the plain launch + this launch with every word on -1 against the TCE_W4_SILU_MUL_PAIRS launch."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import Linear_half_int4, _stream
    from tinychatengine_amd.lora import expand_silu_mul
    hidden, ffn, R, n = 512, 1408, 8, 2
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda a, b: torch.empty(a, b, device=dev).normal_(0.0, b ** -0.5, generator=g)
    gate_up = Linear_half_int4.interleave(Linear_half_int4.from_float(rnd(ffn, hidden), 128), Linear_half_int4.from_float(rnd(ffn, hidden), 128))
    gate_up.prepack()
    x = torch.empty((M, hidden), device=dev).normal_(0, 1, generator=g).half()
    fused, y, out = (torch.empty((M, w), dtype=torch.float16, device=dev) for w in (ffn, 2 * ffn, ffn))
    capi.check(capi.w4a16_forward(gate_up.desc(x, fused, flags=capi.TCE_W4_SILU_MUL_PAIRS), _stream()))
    capi.check(capi.w4a16_forward(gate_up.desc(x, y), _stream()))
    z = lambda *s, dt=torch.float16: torch.zeros(s, dtype=dt, device=dev)
    words = torch.full((M,), -1, dtype=torch.int32, device=dev)
    expand_silu_mul(z(M, 2 * R, dt=torch.float32), z(n, R, ffn), z(n, R, ffn), z(n, dt=torch.float32), words, y, out)
    torch.cuda.synchronize()
    print(f"M={M}: pair launch {capi.describe_dispatch(gate_up.desc(x, fused, flags=capi.TCE_W4_SILU_MUL_PAIRS))} / plain launch {capi.describe_dispatch(gate_up.desc(x, y))}")
    assert torch.equal(out.view(torch.int16), fused.view(torch.int16)), "the plain gate_up launch + the unadapted expand differs from the fused pair launch"


def test_entry_point_refusals(dev):
    """tests/test_lora_gate_up_host.py's table of refusals beside a device, and the Python wrapper's own overlap refusal on real tensors"""
    import test_lora_gate_up_host as host
    from tinychatengine_amd import capi
    from tinychatengine_amd.lora import expand_silu_mul
    host.entry_point_refusals()
    z = lambda *s, dt=torch.float16: torch.zeros(s, dtype=dt, device=dev)
    y = z(4, 32)
    with pytest.raises(RuntimeError):
        expand_silu_mul(z(4, 16, dt=torch.float32), z(2, 8, 16), z(2, 8, 16), z(2, dt=torch.float32), torch.zeros(4, dtype=torch.int32, device=dev), y, y[:, :16])
    assert "overlaps" in capi.last_error()
