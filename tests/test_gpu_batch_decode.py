"""The batched decode step (tce_attention_decode_step_batch_f16, tinychatengine_amd/batch_decode.py): B independent sequences per attention launch.

Contract: every active row's output and appended cache rows are BIT-IDENTICAL to tce_attention_decode_step_pos_f16 run on that sequence's slot with its
position word and the same pos_bound; a row whose position is < 0 or > pos_bound writes a zero output row and touches neither its caches nor its counters.
Then the float64 checks: the attention outputs within the single step's tolerance, whole decoder blocks over staggered sequences within 2 %."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _tables(n, seed):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, (n, HD // 2))
    cos = np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)
    return cos, sin


def _bits(t):
    return t.contiguous().view(torch.int16)


def _setup(dev, batch, heads, kv_heads, bound, rope, seed, max_keys=None):
    from tinychatengine_amd.batch_decode import BatchDecodeAttention
    max_keys = bound + 9 if max_keys is None else max_keys
    g = torch.Generator(device=dev).manual_seed(seed)
    tc = ts = None
    if rope:
        cos, sin = _tables(max_keys, seed)
        tc, ts = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    A = BatchDecodeAttention(batch, heads, max_keys, dev, tc, ts, kv_heads=kv_heads)
    R = BatchDecodeAttention(batch, heads, max_keys, dev, tc, ts, kv_heads=kv_heads)  # the single-step yardstick, slot by slot
    A.k_cache.copy_((torch.randn(A.k_cache.shape, generator=g, device=dev) * 0.8).half())
    A.v_cache.copy_((torch.randn(A.v_cache.shape, generator=g, device=dev) * 0.8).half())
    R.k_cache.copy_(A.k_cache)
    R.v_cache.copy_(A.v_cache)
    qkv = (torch.randn((batch, (heads + 2 * kv_heads) * HD), generator=g, device=dev) * 0.9).half()
    return A, R, qkv, g


def _ragged(rng, batch, bound):
    pos = rng.integers(0, bound + 1, batch)
    pos[0] = 0
    if batch > 1:
        pos[-1] = bound
    if batch > 2:
        pos[1] = bound  # two rows at the bound
    return pos.astype(np.int32)


def _single(R, qkv, pos_t, bound):
    out = torch.empty((R.batch, R.heads * HD), dtype=torch.float16, device=qkv.device)
    for b in range(R.batch):
        R.slot(b).step(qkv[b], bound, out=out[b], pos_device=pos_t[b:b + 1])
    return out


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("heads,kv_heads", [(32, 8), (8, 8), (4, 1)])
def test_batch_step_is_bit_identical_to_the_single_step(dev, heads, kv_heads, rope):
    for batch in (1, 3, 8, 16):
        for bound in (63, 319, 320, 1023, 2047, 4095):
            rng = np.random.default_rng(batch * 10000 + bound)
            A, R, qkv, _ = _setup(dev, batch, heads, kv_heads, bound, rope, seed=batch + bound)
            pos_t = torch.from_numpy(_ragged(rng, batch, bound)).to(dev)
            out = A.step(qkv, pos_t, bound)
            want = _single(R, qkv, pos_t, bound)
            torch.cuda.synchronize()
            what = f"B={batch} bound={bound} pos={pos_t.tolist()}"
            assert torch.equal(_bits(out), _bits(want)), f"{what}: outputs differ"
            assert torch.equal(_bits(A.k_cache), _bits(R.k_cache)) and torch.equal(_bits(A.v_cache), _bits(R.v_cache)), f"{what}: caches differ"
            del A, R


def _rope16(x, c, s):
    """RotaryPosEmb_cuda_forward in binary16: hfma(x, cos, hmul(rot, sin)) (an fp64 x * cos + t is exact, then one rounding: the fused form)."""
    half = x.shape[-1] // 2
    rot = np.concatenate([-x[:, half:], x[:, :half]], axis=1)
    t = (rot.astype(np.float64) * s.astype(np.float64)).astype(np.float16)
    return (x.astype(np.float64) * c.astype(np.float64) + t.astype(np.float64)).astype(np.float16)


@pytest.mark.parametrize("heads,kv_heads,bound", [(32, 8, 320), (32, 8, 1023), (8, 8, 2047), (4, 1, 4095)])
def test_batch_step_against_float64(dev, heads, kv_heads, bound):
    batch = 3
    rng = np.random.default_rng(bound)
    A, _, qkv, _ = _setup(dev, batch, heads, kv_heads, bound, True, seed=7 + bound)
    K0, V0 = A.k_cache.cpu().numpy(), A.v_cache.cpu().numpy()
    pos = _ragged(rng, batch, bound)
    out = A.step(qkv, torch.from_numpy(pos).to(dev), bound).float().cpu().numpy().reshape(batch, heads, HD)
    x = qkv.cpu().numpy()
    cos, sin = A.cos.cpu().numpy(), A.sin.cpu().numpy()
    alpha = float(np.float16(1.0 / np.sqrt(HD)))
    rep = heads // kv_heads
    for b in range(batch):
        p = int(pos[b])
        q = _rope16(x[b, :heads * HD].reshape(heads, HD), cos[p], sin[p]).astype(np.float64)
        k = _rope16(x[b, heads * HD:(heads + kv_heads) * HD].reshape(kv_heads, HD), cos[p], sin[p]).astype(np.float64)
        v = x[b, (heads + kv_heads) * HD:].reshape(kv_heads, HD).astype(np.float64)
        Kc = K0[b, :, :p + 1].astype(np.float64)
        Vc = V0[b, :, :p + 1].astype(np.float64)
        Kc[:, p], Vc[:, p] = k, v
        sc = alpha * np.einsum("hd,hkd->hk", q, np.repeat(Kc, rep, axis=0))
        w = np.exp(sc - sc.max(axis=1, keepdims=True))
        ref = np.einsum("hk,hkd->hd", w / w.sum(axis=1, keepdims=True), np.repeat(Vc, rep, axis=0))
        tol = 2e-3 * np.abs(ref).max(axis=1, keepdims=True) + 2.0 ** -10 * np.abs(ref)
        err = np.abs(out[b] - ref)
        assert np.isfinite(out[b]).all() and np.all(err <= tol), f"row {b} pos {p}: worst |err|/tol = {(err / tol).max():.3f}"


@pytest.mark.parametrize("bound", [63, 1023])
def test_inactive_rows_write_zeros_and_touch_nothing(dev, bound):
    heads, kv_heads, batch = 32, 8, 6
    A, R, qkv, _ = _setup(dev, batch, heads, kv_heads, bound, True, seed=31 + bound)
    pos = np.array([5, -1, bound, -7, bound + 1, 0], np.int32)
    inactive = [1, 3, 4]
    pos_t = torch.from_numpy(pos).to(dev)
    K0, V0 = A.k_cache.clone(), A.v_cache.clone()
    A.workspace.fill_(0)
    out = A.step(qkv, pos_t, bound)
    torch.cuda.synchronize()
    sw = A.slot_workspace_bytes
    for b in range(batch):
        if b in inactive:
            assert torch.count_nonzero(out[b]) == 0 and not torch.isnan(out[b]).any(), f"row {b}: inactive row not zero"
            assert torch.equal(_bits(A.k_cache[b]), _bits(K0[b])) and torch.equal(_bits(A.v_cache[b]), _bits(V0[b])), f"row {b}: inactive caches written"
            assert torch.count_nonzero(A.workspace[b * sw:(b + 1) * sw]) == 0, f"row {b}: inactive workspace touched"
        else:
            assert torch.count_nonzero(A.workspace[b * sw:b * sw + 256]) == 0, f"row {b}: a counter was left non-zero"
    # the active rows of the same launch are the single step's, bit for bit (inactive slots' references are not run: their rows must stay as they were)
    want = torch.zeros_like(out)
    for b in range(batch):
        if b not in inactive:
            R.slot(b).step(qkv[b], bound, out=want[b], pos_device=pos_t[b:b + 1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(A.k_cache), _bits(R.k_cache)) and torch.equal(_bits(A.v_cache), _bits(R.v_cache))
    # and the next launch, every row active, too
    pos_t.copy_(torch.tensor([6, 1, bound - 1, 0, bound, 2], dtype=torch.int32))
    out = A.step(qkv, pos_t, bound)
    want = _single(R, qkv, pos_t, bound)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(A.k_cache), _bits(R.k_cache)) and torch.equal(_bits(A.v_cache), _bits(R.v_cache))


@pytest.mark.parametrize("heads,kv_heads,bound", [(32, 8, 1023), (4, 1, 319)])
def test_poisoned_cache_rows_stay_put_and_do_not_leak(dev, heads, kv_heads, bound):
    """Every cache row at or beyond a sequence's position holds NaN / Inf bits: only the B appended rows may change, and every output is finite and the
    single step's."""
    batch = 4
    A, R, qkv, _ = _setup(dev, batch, heads, kv_heads, bound, True, seed=5 + bound)
    pos = np.array([0, bound // 3, bound, 17], np.int32)
    poison = torch.tensor([0x7C00, 0x7E00, -1024, 0x7D55], dtype=torch.int16, device=dev)  # +Inf, NaN, -Inf, a signalling-style NaN
    for c in (A.k_cache, A.v_cache):
        bits = c.view(torch.int16)
        for b in range(batch):
            tail = bits[b, :, int(pos[b]):]
            tail.copy_(poison.repeat(tail.numel() // 4 + 1)[:tail.numel()].view(tail.shape))
    R.k_cache.copy_(A.k_cache)
    R.v_cache.copy_(A.v_cache)
    K0, V0 = _bits(A.k_cache).clone(), _bits(A.v_cache).clone()
    pos_t = torch.from_numpy(pos).to(dev)
    out = A.step(qkv, pos_t, bound)
    want = _single(R, qkv, pos_t, bound)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all(), "a poisoned row leaked into an output"
    assert torch.equal(_bits(out), _bits(want))
    for c, c0 in ((A.k_cache, K0), (A.v_cache, V0)):
        changed = (_bits(c) != c0).any(dim=-1)  # [batch][kv_heads][max_keys]
        for b in range(batch):
            rows = changed[b].any(dim=0).nonzero().flatten().tolist()
            assert set(rows) <= {int(pos[b])}, f"slot {b}: rows {rows[:8]} changed, only {int(pos[b])} may"


def test_two_hundred_launches_reset_their_counters(dev):
    heads, kv_heads, batch, bound = 32, 8, 4, 1023
    A, R, qkv, g = _setup(dev, batch, heads, kv_heads, bound, True, seed=200)
    rng = np.random.default_rng(200)
    pos_t = torch.zeros(batch, dtype=torch.int32, device=dev)
    for it in range(200):
        pos = rng.integers(0, bound + 1, batch).astype(np.int32)
        if it % 5 == 0:
            pos[it % batch] = rng.integers(0, 64)  # short contexts beside long ones (one live chunk next to eight)
        pos_t.copy_(torch.from_numpy(pos))
        qkv.copy_((torch.randn(qkv.shape, generator=g, device=dev) * 0.9).half())
        out = A.step(qkv, pos_t, bound)
        want = _single(R, qkv, pos_t, bound)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)), f"launch {it}: outputs differ (pos {pos.tolist()})"
    assert torch.equal(_bits(A.k_cache), _bits(R.k_cache)) and torch.equal(_bits(A.v_cache), _bits(R.v_cache))
    assert torch.count_nonzero(A.workspace.view(batch, -1)[:, :256]) == 0


def _blocks(dev, hidden, heads, kv_heads, ffn, layers, max_keys, seed):
    from tinychatengine_amd.decoder_block import DecoderBlock
    cos, sin = _tables(max_keys, seed)
    tc, ts = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    return [DecoderBlock(hidden, heads, ffn, max_keys, dev, tc, ts, seed=seed + i, kv_heads=kv_heads) for i in range(layers)], cos, sin


def test_captured_batched_step_replays_bit_identically(dev):
    from tinychatengine_amd.batch_decode import BatchedDecoder
    hidden, heads, kv_heads, ffn, batch, bound = 512, 4, 1, 1408, 4, 63
    blocks, _, _ = _blocks(dev, hidden, heads, kv_heads, ffn, 2, bound + 1, 40)
    dec_e = [BatchedDecoder(b, batch) for b in blocks]
    dec_g = [BatchedDecoder(b, batch) for b in blocks]
    g = torch.Generator(device=dev).manual_seed(3)
    for de, dg in zip(dec_e, dec_g):
        for c in ("k_cache", "v_cache"):
            getattr(de.attention, c).copy_((torch.randn(getattr(de.attention, c).shape, generator=g, device=dev) * 0.5).half())
            getattr(dg.attention, c).copy_(getattr(de.attention, c))
    h0 = (torch.randn((batch, hidden), generator=g, device=dev)).half()
    h_e, h_g = h0.clone(), h0.clone()
    start = torch.tensor([3, 20, -100, 50], dtype=torch.int32, device=dev)  # slot 2 stays retired through every replay
    pos_e, pos_g = start.clone(), start.clone()
    for d, h, p in ((dec_e, h_e, pos_e), (dec_g, h_g, pos_g)):  # token 0 eagerly on both (the warm-up before the capture)
        for layer in d:
            layer.step(h, p, bound)
        p.add_(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for layer in dec_g:
            layer.step(h_g, pos_g, bound)
        pos_g.add_(1)
    for t in range(4):
        graph.replay()
        for layer in dec_e:
            layer.step(h_e, pos_e, bound)
        pos_e.add_(1)
        torch.cuda.synchronize()
        assert torch.equal(pos_e, pos_g)
        assert torch.equal(_bits(h_e), _bits(h_g)), f"token {t + 1}: replay differs from the eager step"
        for de, dg in zip(dec_e, dec_g):
            assert torch.equal(_bits(de.attention.k_cache), _bits(dg.attention.k_cache)) and torch.equal(_bits(de.attention.v_cache), _bits(dg.attention.v_cache))


def _rmsnorm(x, gamma, eps):
    return x / np.sqrt(np.mean(x * x) + eps) * gamma


def _rope(v, cos, sin):
    half = v.shape[-1] // 2
    rot = np.concatenate([-v[:, half:], v[:, :half]], axis=1)
    return v * cos[None, :] + rot * sin[None, :]


class _Ref:
    """float64 Int4llamaDecoderLayer over the dequantized weights, one sequence's history (its own caches per layer)."""

    def __init__(self, W, G, heads, kv_heads, cos, sin):
        self.W, self.G, self.heads, self.kv_heads, self.cos, self.sin = W, G, heads, kv_heads, cos, sin
        self.K = [np.zeros((kv_heads, 0, HD)) for _ in W]
        self.V = [np.zeros((kv_heads, 0, HD)) for _ in W]

    def token(self, x, pos):
        h = x.astype(np.float64)
        c, s = self.cos[pos].astype(np.float64), self.sin[pos].astype(np.float64)
        heads, kvh, rep = self.heads, self.kv_heads, self.heads // self.kv_heads
        alpha = float(np.float16(1.0 / np.sqrt(HD)))
        for li, W in enumerate(self.W):
            qkv = W["qkv"] @ _rmsnorm(h, self.G[li][0], 1e-6)
            q = qkv[:heads * HD].reshape(heads, HD)
            k = qkv[heads * HD:(heads + kvh) * HD].reshape(kvh, HD)
            v = qkv[(heads + kvh) * HD:].reshape(kvh, HD)
            q, k = _rope(q, c, s), _rope(k, c, s)
            assert self.K[li].shape[1] == pos
            self.K[li] = np.concatenate([self.K[li], k[:, None, :]], axis=1)
            self.V[li] = np.concatenate([self.V[li], v[:, None, :]], axis=1)
            sc = alpha * np.einsum("hd,hkd->hk", q, np.repeat(self.K[li], rep, axis=0))
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            h = h + W["o"] @ np.einsum("hk,hkd->hd", p, np.repeat(self.V[li], rep, axis=0)).reshape(-1)
            hn = _rmsnorm(h, self.G[li][1], 1e-6)
            gate, up = W["gate"] @ hn, W["up"] @ hn
            h = h + W["down"] @ (gate / (1.0 + np.exp(-gate)) * up)
        return h


@pytest.mark.parametrize("hidden,heads,kv_heads,ffn,layers", [(512, 4, 1, 1408, 2), (1024, 8, 4, 512, 1), (512, 4, 4, 1408, 2), (4096, 32, 8, 14336, 1)])
def test_batched_blocks_against_float64(dev, hidden, heads, kv_heads, ffn, layers):
    """Four slots: sequences admitted at staggered steps through prefill(slot, ...), one retired mid-run (position -1), the others decoding; every live
    sequence's residual row against a float64 evaluation of its own history."""
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.decoder_block import dequantize
    batch, max_keys = 4, 64
    blocks, cos, sin = _blocks(dev, hidden, heads, kv_heads, ffn, layers, max_keys, 70 + hidden)
    decs = [BatchedDecoder(b, batch) for b in blocks]
    W = [{k: dequantize(getattr(b, k)) for k in ("qkv", "o", "gate", "up", "down")} for b in blocks]
    G = [(b.gamma1.cpu().numpy().astype(np.float64), b.gamma2.cpu().numpy().astype(np.float64)) for b in blocks]
    rng = np.random.default_rng(hidden + ffn)
    refs = [None] * batch
    pos = np.full(batch, -1, np.int32)
    pos_t = torch.from_numpy(pos).to(dev)
    hidden_rows = torch.zeros((batch, hidden), dtype=torch.float16, device=dev)
    admit = {0: [(0, 5), (3, 2)], 2: [(1, 3)], 4: [(2, 4)]}  # step -> [(slot, prompt rows)]
    retire = {5: 0}
    bound = max_keys - 1

    def check(got, ref, what):
        tol = 2e-2 * np.abs(ref).max()
        err = np.abs(got.astype(np.float64) - ref).max()
        assert err <= tol, f"{what}: max |err| {err:.4f} vs tol {tol:.4f}"

    for t in range(9):
        for slot, m in admit.get(t, []):
            refs[slot] = _Ref(W, G, heads, kv_heads, cos, sin)
            x = rng.standard_normal((m, hidden)).astype(np.float16)
            rows = torch.from_numpy(x).to(dev)
            for d in decs:
                d.prefill(slot, rows, 0)
            torch.cuda.synchronize()
            got = rows.cpu().numpy()
            for r in range(m):
                check(got[r], refs[slot].token(x[r], r), f"step {t} slot {slot} prompt row {r}")
            pos[slot] = m
        if t in retire:
            refs[retire[t]] = None
            pos[retire[t]] = -1
        x = rng.standard_normal((batch, hidden)).astype(np.float16)
        hidden_rows.copy_(torch.from_numpy(x))
        pos_t.copy_(torch.from_numpy(pos))
        for d in decs:
            d.step(hidden_rows, pos_t, bound)
        torch.cuda.synchronize()
        got = hidden_rows.cpu().numpy()
        for b in range(batch):
            if refs[b] is not None:
                check(got[b], refs[b].token(x[b], int(pos[b])), f"step {t} slot {b} pos {pos[b]}")
                pos[b] += 1
