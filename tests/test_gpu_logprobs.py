"""Log-probabilities on the device (csrc/sampling.hip: the LSE forms of the sampler's kernels, logprobs_partials_kernel / logprobs_merge_kernel;
tinychatengine_amd/generate.py: Sampler(logprobs=True), BatchedGenerator.logprobs / score; speculative.py).

ACCURACY: logprob = x_t - LSE(x) on the raw fp16 logits; for rows with every |x_i| <= 64, |device - logprob_reference (float64)| <= 2^-16 -- expf / logf are
accurate to a few ulp, the sums are 16 + 6 + 3 + 8 additions deep in the order the kernels fix, and the two last subtractions round at magnitudes < 256.
IDENTITY (bitwise): tce_sample_logprobs_f16 leaves token, log, ring, counters, position and debug record as tce_sample_f16 does; its value equals tce_logprobs_f16's
on the same row with the chosen token as target; values do not depend on slot, batch size, or eager versus graph; the speculative generator returns the values of
plain decoding for the same tokens."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BOUND = 2.0 ** -16
NAN_PATTERN = 0x7FC01234  # what an untouched out_logprob word holds in the kernel-level tests
SHAPES = [(1, 8), (7, 8), (4096, 4096), (4097, 4104), (12328, 12352)]  # one thread; one piece; one chunk exactly; one element into a second chunk; three chunks plus 40


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _gauss(rng, vocab, ld, sigma=4.0):
    """A row [ld]: Gaussian logits, and the largest fp16 values in the columns past the vocabulary (they must take no part)."""
    x = np.full(ld, 60000.0, np.float16)
    x[:vocab] = (rng.standard_normal(vocab) * sigma).clip(-64, 64).astype(np.float16)
    return x


def _device_logprobs(dev, logits: np.ndarray, vocab: int, targets, partials_fill: int = 0xFF):
    """tce_logprobs_f16 on logits [rows][ld] -> (logprob, lse) fp32 [rows]; the outputs and the partials start as garbage."""
    from tinychatengine_amd import capi
    rows, ld = logits.shape
    lg = torch.from_numpy(logits).to(dev)
    tg = torch.tensor(list(targets), dtype=torch.int32, device=dev)
    out = torch.full((rows,), 123.0, dtype=torch.float32, device=dev)
    lse = torch.full((rows,), 123.0, dtype=torch.float32, device=dev)
    partials = torch.full((int(capi.lib().tce_logprobs_workspace_bytes(rows, vocab)),), partials_fill, dtype=torch.uint8, device=dev)  # (need not be zeroed)
    capi.check(capi.logprobs_f16(lg.data_ptr(), ld, vocab, rows, tg.data_ptr(), out.data_ptr(), lse.data_ptr(), partials.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def _lse64(row16: np.ndarray) -> float:
    x = row16.astype(np.float64)
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


# =====================================================================================================================================================
# scoring: tce_logprobs_f16 against float64
# =====================================================================================================================================================
@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_logprobs_f16_against_float64(dev, vocab, ld):
    """Targets at index 0, vocab - 1, 4095, 4096, the maximum and the minimum of Gaussian rows; rows that are all equal; a 60.0 spike on a chunk edge; one whole chunk
    of -inf beside finite chunks (a finite result); "no target" (-1: 0.0, the LSE still written) and targets outside the vocabulary (NaN); all -inf, one NaN, one
    +inf (NaN, no fault)."""
    from tinychatengine_amd.generate import logprob_reference
    rng = np.random.default_rng(vocab)
    rows, targets, finite = [], [], []

    def add(row, t, is_finite=True):
        rows.append(row)
        targets.append(int(t))
        finite.append(is_finite)

    g = _gauss(rng, vocab, ld)
    for t in sorted({0, vocab - 1, 4095, 4096, int(np.argmax(g[:vocab])), int(np.argmin(g[:vocab]))}):
        if t < vocab:
            add(g, t)
    g16 = _gauss(rng, vocab, ld, sigma=16.0)
    add(g16, int(np.argmin(g16[:vocab])))
    add(g16, int(np.argmax(g16[:vocab])))
    flat = np.full(ld, 60000.0, np.float16)
    flat[:vocab] = 3.25
    add(flat, 0)
    add(flat, vocab - 1)
    for edge in sorted({min(4095, vocab - 1), min(4096, vocab - 1)}):  # a spike on a chunk edge (either side of it where the vocabulary reaches)
        sp = _gauss(rng, vocab, ld, sigma=1.0)
        sp[edge] = 60.0
        add(sp, edge)
        add(sp, 0)
    if vocab > 4096:  # a whole chunk of -inf: the first, and the last (partial) one
        for lo, hi in ((0, 4096), ((vocab - 1) // 4096 * 4096, vocab)):
            h = g.copy()
            h[lo:hi] = -np.inf
            live = 4096 if lo == 0 else 0
            add(h, live)
            add(h, lo, is_finite=False)  # a -inf target: -inf exactly
    add(g, -1)                           # "no target"
    for t in (vocab, -2, 1 << 30):       # outside the vocabulary (index `vocab` lies inside the row where ld > vocab: still NaN)
        add(g, t, is_finite=False)
    ninf = np.full(ld, -np.inf, np.float16)
    add(ninf, 0, is_finite=False)
    for bad in (np.nan, np.inf):
        h = g.copy()
        h[vocab // 2] = bad
        add(h, 0, is_finite=False)
        if vocab > 1:
            add(h, vocab // 2, is_finite=False)
    logits = np.stack(rows)
    got, lse = _device_logprobs(dev, logits, vocab, targets)
    worst = 0.0
    for r, (row, t, fin) in enumerate(zip(rows, targets, finite)):
        want = logprob_reference(row[:vocab], t)
        what = f"vocab {vocab} row {r} target {t}"
        if t == -1:
            assert got[r] == 0.0 and abs(float(lse[r]) - _lse64(row[:vocab])) <= BOUND, what
        elif np.isnan(want):
            assert np.isnan(got[r]), f"{what}: {got[r]!r}, NaN expected"
        elif not fin:
            assert got[r] == want == -np.inf, what
        else:
            assert np.abs(row[:vocab].astype(np.float32)).max() <= 64 or np.isinf(row[:vocab]).any()
            err = abs(float(got[r]) - want)
            worst = max(worst, err)
            assert err <= BOUND, f"{what}: device {got[r]!r}, float64 {want!r}, |difference| {err:.3e} > 2^-16"
            assert abs(float(lse[r]) - _lse64(row[:vocab])) <= BOUND, what
    print(f"vocab {vocab}: worst |device - float64| = {worst:.3e} = {worst / BOUND:.2f} of 2^-16 over {sum(finite)} rows")
    # a row's value does not depend on the rows beside it, the number of rows, or what the workspace held
    one, one_lse = _device_logprobs(dev, logits[2:3].copy(), vocab, targets[2:3], partials_fill=0x00)
    assert _bits(one)[0] == _bits(got)[2] and _bits(one_lse)[0] == _bits(lse)[2]


# =====================================================================================================================================================
# the sampler: tce_sample_logprobs_f16 beside tce_sample_f16
# =====================================================================================================================================================
def _row_words(row) -> np.ndarray:
    return np.frombuffer(bytes(row), dtype=np.int32).copy()


def _make_row(params, seed, max_new, ring=(), generated=0):
    from tinychatengine_amd.generate import make_row
    r = make_row(params, seed, max_new, ring)
    r.generated = generated
    return r


def _pair_step(dev, vocab, logits: np.ndarray, rows, pos, log_stride, uniforms=None, pos_bound=63):
    """One call of tce_sample_f16 and one of tce_sample_logprobs_f16 on the same inputs (batch = len(rows)).  Asserts that token, log, ring, counters, position and
    debug record are the same bits and returns the logprob side: tokens, out_logprob [batch][log_stride], last_lse [batch]."""
    from tinychatengine_amd.generate import Sampler
    B = len(rows)
    lg = torch.from_numpy(logits).to(dev)
    state = {}
    for on in (False, True):
        s = Sampler(B, vocab, log_stride, dev, top_k_bound=8, stop_ids=[vocab + 5], debug=True, logprobs=on)
        s.rows.copy_(torch.from_numpy(np.stack([_row_words(r) for r in rows])))
        s.next_token.fill_(-7)
        if uniforms is not None:
            s.uniform_override = torch.tensor(uniforms, dtype=torch.float32, device=dev)
        if on:
            s.out_logprob.copy_(torch.from_numpy(np.full((B, log_stride), NAN_PATTERN, np.int32).view(np.float32)))
            s.last_lse.copy_(torch.from_numpy(np.full(B, NAN_PATTERN, np.int32).view(np.float32)))
            s.partials.fill_(0xFF)
        p = torch.tensor(pos, dtype=torch.int32, device=dev)
        s.step(lg, p, pos_bound)
        torch.cuda.synchronize()
        state[on] = {"token": s.next_token.cpu().numpy(), "log": s.out_log.cpu().numpy(), "rows": s.rows.cpu().numpy(), "pos": p.cpu().numpy(),
                     "debug": s.debug.cpu().numpy(), "logprob": s.out_logprob.cpu().numpy() if on else None, "lse": s.last_lse.cpu().numpy() if on else None}
    for k in ("token", "log", "rows", "pos", "debug"):
        assert np.array_equal(state[False][k], state[True][k]), f"tce_sample_logprobs_f16 changes `{k}`"
    return state[True]


def _check_pair(dev, vocab, ld, logits, rows, pos, log_stride, what, uniforms=None, expect_nan=(), pos_bound=63):
    """_pair_step, then per row: an inactive row's words untouched; an active row's value at [generated] within 2^-16 of float64 (or NaN where the row is degenerate),
    bit-equal to tce_logprobs_f16 on the same row with the chosen token as target, every other word untouched."""
    from tinychatengine_amd.generate import logprob_reference
    st = _pair_step(dev, vocab, logits, rows, pos, log_stride, uniforms, pos_bound)
    active = [b for b in range(len(rows)) if 0 <= pos[b] <= pos_bound]
    assert len(active) < len(rows), "every case keeps an inactive row"
    scored, scored_lse = _device_logprobs(dev, logits, vocab, [int(st["token"][b]) if b in active else -1 for b in range(len(rows))])
    lp_bits, lse_bits = _bits(st["logprob"]), _bits(st["lse"])
    for b in range(len(rows)):
        if b not in active:
            assert (lp_bits[b] == NAN_PATTERN).all() and lse_bits[b] == NAN_PATTERN and st["token"][b] == -7, f"{what}: the inactive row {b} was written"
            continue
        g, tok = int(rows[b].generated), int(st["token"][b])
        assert 0 <= tok < vocab and st["log"][b, g] == tok
        others = np.delete(lp_bits[b], g)
        assert (others == NAN_PATTERN).all(), f"{what} row {b}: a word beside index {g} was written"
        got = st["logprob"][b, g]
        if b in expect_nan:
            assert np.isnan(got) and np.isnan(scored[b]), f"{what} row {b}: {got!r} / {scored[b]!r}, NaN expected"
        else:
            assert lp_bits[b, g] == _bits(scored)[b] and lse_bits[b] == _bits(scored_lse)[b], f"{what} row {b}: the sampler's value and tce_logprobs_f16's differ"
            want = logprob_reference(logits[b, :vocab], tok)
            assert abs(float(got) - want) <= BOUND, f"{what} row {b} token {tok}: device {got!r}, float64 {want!r}"
    return st


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_sample_logprobs_identity_and_values(dev, vocab, ld):
    """Batch 3, row 1 inactive (its out_logprob pre-filled with a NaN pattern that must stay).  Greedy rows with the maximum at index 0, vocab - 1, 4095, 4096; sampled
    rows; penalties on with repeated ids in the ring (the value is still the RAW logits'); all-equal rows; a 60.0 spike on a chunk edge; a whole chunk of -inf;
    generated = log_stride - 1; the degenerate rows."""
    from tinychatengine_amd.generate import SamplingParams
    rng = np.random.default_rng(100 + vocab)
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    sampled = SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.0)
    LOG = 6

    def three(r0, r2):
        return np.stack([r0, _gauss(rng, vocab, ld), r2])

    # greedy: the maximum where the targets of the issue lie
    spots = [t for t in (0, vocab - 1, 4095, 4096) if t < vocab]
    for i in range(0, len(spots), 2):
        pair = (spots + spots)[i:i + 2]
        rows16 = []
        for t in pair:
            x = _gauss(rng, vocab, ld)
            x[t] = 30.0
            rows16.append(x)
        st = _check_pair(dev, vocab, ld, three(*rows16), [_make_row(greedy, 1, LOG, generated=g) for g in (0, 3, 2)], [5, -1, 9], LOG, f"greedy max at {pair}")
        assert [int(st["token"][0]), int(st["token"][2])] == pair
    # the inactive row by the other rule: a position past pos_bound
    x = three(_gauss(rng, vocab, ld), _gauss(rng, vocab, ld))
    _check_pair(dev, vocab, ld, x, [_make_row(greedy, 1, LOG) for _ in range(3)], [0, 64, 63], LOG, "pos > pos_bound")
    # sampled, several uniforms
    for u in (0.0, 0.37, 0.93):
        _check_pair(dev, vocab, ld, x, [_make_row(sampled, 7 + b, LOG, generated=b) for b in range(3)], [3, -1, 4], LOG, f"sampled u={u}", uniforms=[u, u, u])
    # penalties on, the ring full of the rows' top tokens (repeated): another token may be chosen, the value is that of the raw logits
    top = np.argsort(-x[0, :vocab].astype(np.float32), kind="stable")[:3].tolist()
    ring = (top * 22)[:64]
    pen = SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.3, alpha_frequency=0.2, alpha_presence=0.1)
    pen_greedy = SamplingParams(temp=0.0, repeat_penalty=1.5, alpha_frequency=0.5, alpha_presence=0.5)
    st = _check_pair(dev, vocab, ld, np.stack([x[0], x[1], x[0]]), [_make_row(pen, 3, LOG, ring), _make_row(pen, 3, LOG, ring), _make_row(pen_greedy, 3, LOG, ring)],
                     [7, -1, 7], LOG, "penalties", uniforms=[0.5, 0.5, 0.5])
    if vocab >= 4096:
        assert int(st["token"][2]) not in top, "the penalties did not move the greedy choice: the case tests nothing"
    # all equal; a 60.0 spike on a chunk edge
    flat = np.full(ld, 60000.0, np.float16)
    flat[:vocab] = -2.5
    sp = _gauss(rng, vocab, ld, sigma=1.0)
    sp[min(4095, vocab - 1)] = 60.0
    sp[min(4096, vocab - 1)] = 60.0
    st = _check_pair(dev, vocab, ld, three(flat, sp), [_make_row(greedy, 1, LOG) for _ in range(3)], [1, -1, 2], LOG, "flat / spike")
    assert int(st["token"][0]) == 0 and int(st["token"][2]) == min(4095, vocab - 1)
    # generated = log_stride - 1: the last word of the row is written and the row retires
    st = _check_pair(dev, vocab, ld, x, [_make_row(sampled, 5, LOG, generated=LOG - 1) for _ in range(3)], [2, -1, 2], LOG, "gen = log_stride - 1", uniforms=[0.2] * 3)
    assert st["pos"].tolist() == [-1, -1, -1]
    # one whole chunk of -inf beside finite chunks: a finite result
    if vocab > 4096:
        h0, h2 = _gauss(rng, vocab, ld), _gauss(rng, vocab, ld)
        h0[:4096] = -np.inf
        h2[(vocab - 1) // 4096 * 4096:vocab] = -np.inf
        st = _check_pair(dev, vocab, ld, three(h0, h2), [_make_row(sampled, 9, LOG) for _ in range(3)], [2, -1, 2], LOG, "a chunk of -inf", uniforms=[0.6] * 3)
        assert np.isfinite(st["logprob"][[0, 2], 0]).all()
    # degenerate rows: NaN, and nothing faults; the sampler's own outputs still equal tce_sample_f16's
    ninf = np.full(ld, -np.inf, np.float16)
    nan_row, inf_row = _gauss(rng, vocab, ld), _gauss(rng, vocab, ld)
    nan_row[vocab // 2], inf_row[vocab // 2] = np.nan, np.inf
    _check_pair(dev, vocab, ld, three(ninf, nan_row), [_make_row(greedy, 1, LOG) for _ in range(3)], [2, -1, 2], LOG, "-inf / NaN", expect_nan=(0, 2))
    _check_pair(dev, vocab, ld, three(inf_row, ninf), [_make_row(greedy, 1, LOG) for _ in range(3)], [2, -1, 2], LOG, "+inf / -inf", expect_nan=(0, 2))


# =====================================================================================================================================================
# the generators
# =====================================================================================================================================================
def _small(dev):
    import test_gpu_generate as G
    assert (G.VOCAB, G.MAX_KEYS, G.PAGE_KEYS, G.BATCH, G.NUM_PAGES) == (4096, 64, 16, 4, 12)
    return G, G._model(dev, G.SMALL)


def _generator(G, m, graph=True, stop_ids=(), logprobs=True, free_order=None, kv_dtype="fp16", max_new=24):
    from tinychatengine_amd.generate import BatchedGenerator
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    alloc = PageAllocator(G.NUM_PAGES, G.PAGE_KEYS, G.BATCH, G.MAX_KEYS // G.PAGE_KEYS, m.dev, free_order=free_order)
    kw = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-1) if kv_dtype != "fp16" else {}
    decs = [PagedBatchedDecoder(b, alloc, **kw) for b in m.blocks]
    return BatchedGenerator(decs, m.final_gamma, m.lm_head, m.table, max_new=max_new, stop_ids=stop_ids, graph=graph, logprobs=logprobs)


def _schedule(gen, prompts, layout, after_step=None):
    """Four sequences in the slots layout[q], staggered admissions; sequence 0 (greedy) may retire on a stop id; its slot is then released and sequence 4 admitted into
    it.  Sequences 0 and 2 greedy, the others sampled, a seed each.  after_step(gen, slots just advanced or admitted): called behind every admission and every run(1).
    Returns {sequence: (tokens, logprobs or None)}."""
    from tinychatengine_amd.generate import SamplingParams
    greedy, sampled = SamplingParams(temp=0.0, repeat_penalty=1.0), SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.1)
    params = {0: greedy, 1: sampled, 2: greedy, 3: sampled, 4: sampled}
    out = {}

    def take(q, slot):
        out[q] = (gen.tokens(slot), gen.logprobs(slot) if gen.sampler.logprobs else None)

    def admit(qs):
        gen.admit([(layout[q], prompts[q], params[q], 900 + q, 24 if q != 3 else 9) for q in qs])
        if after_step:
            after_step(gen, [layout[q] for q in qs])

    def run(n):
        for _ in range(n):
            live = gen.book.live()
            gen.run(1)
            gen.allocator.check_invariants()
            if after_step:
                after_step(gen, live)

    admit([0, 3])
    run(2)
    admit([1])
    run(2)
    admit([2])
    run(10)
    take(0, layout[0])
    gen.release(layout[0])
    layout = {**layout, 4: layout[0]}
    admit([4])
    run(6)
    for q in (1, 2, 3, 4):
        take(q, layout[q])
    return out


def test_generator_logprobs_graph_eager_slots_and_float64(dev):
    """SMALL model on 16-key pages, four slots, staggered admissions, one sequence retiring on a stop id and its slot readmitted; greedy and sampled sequences.
    logprobs=True changes no token (graph, against logprobs=False); every value of the eager run lies within 2^-16 of float64 on the logits of its step; the graph run's
    values are the eager run's bits, and the same bits with the slots permuted and another page order."""
    from tinychatengine_amd.generate import logprob_reference
    G, m = _small(dev)
    rng = np.random.default_rng(2024)
    ident = {q: q for q in range(4)}
    stop = None
    for _ in range(8):  # discovery: a token of sequence 0's own at index 4 .. 9, which no other sequence of the schedule produces
        prompts = {q: rng.integers(0, G.VOCAB, n).tolist() for q, n in {0: 20, 1: 3, 2: 4, 3: 2, 4: 6}.items()}
        disc = _schedule(_generator(G, m), prompts, ident)
        seq0, others = disc[0][0], set().union(*[set(disc[q][0]) for q in (1, 2, 3, 4)])
        found = [i for i in range(4, 10) if seq0[i] not in seq0[:i] and seq0[i] not in others]
        if found:
            stop_at, stop = found[0], seq0[found[0]]
            break
    assert stop is not None, "no prompt set gave sequence 0 a token of its own at index 4 .. 9"

    gen = _generator(G, m, stop_ids=[stop])
    assert gen.launches_per_token == 7 * len(m.blocks) + 5
    a = _schedule(gen, prompts, ident)
    assert a[0][0] == seq0[:stop_at + 1] and len(a[3][0]) == 9 and all(len(a[q][0]) == len(a[q][1]) for q in a)
    for q in (1, 2, 3, 4):
        assert a[q][0] == disc[q][0] and np.array_equal(_bits(a[q][1]), _bits(disc[q][1]))
    assert np.array_equal(_bits(a[0][1]), _bits(disc[0][1][:stop_at + 1]))
    off = _schedule(_generator(G, m, stop_ids=[stop], logprobs=False), prompts, ident)
    assert {q: t for q, (t, _) in off.items()} == {q: t for q, (t, _) in a.items()}, "logprobs=True changes the tokens"

    # eager: behind every step, the new token of every advanced slot against float64 on that step's logits
    seen = {"n": 0, "worst": 0.0}

    def check(g, slots):
        logits = g.logits.cpu().numpy()
        for s in slots:
            toks, lps = g.tokens(s), g.logprobs(s)
            row = logits[s, :G.VOCAB]
            assert np.abs(row.astype(np.float32)).max() <= 64
            err = abs(float(lps[-1]) - logprob_reference(row, toks[-1]))
            seen["n"], seen["worst"] = seen["n"] + 1, max(seen["worst"], err)
            assert err <= BOUND, f"slot {s} token {len(toks) - 1}: |device - float64| = {err:.3e}"

    e = _schedule(_generator(G, m, graph=False, stop_ids=[stop]), prompts, ident, after_step=check)
    print(f"eager run: {seen['n']} values, worst |device - float64| = {seen['worst']:.3e} = {seen['worst'] / BOUND:.2f} of 2^-16")
    assert seen["n"] == sum(len(e[q][0]) for q in e) >= 50  # every token of every sequence was checked
    for q in a:
        assert e[q][0] == a[q][0] and np.array_equal(_bits(e[q][1]), _bits(a[q][1])), f"sequence {q}: graph replay and eager steps disagree"
        assert np.isfinite(a[q][1]).all() and (a[q][1] <= 0).all()
    c = _schedule(_generator(G, m, stop_ids=[stop], free_order=np.random.default_rng(2).permutation(G.NUM_PAGES).tolist()), prompts, {0: 3, 1: 0, 2: 1, 3: 2})
    for q in a:
        assert c[q][0] == a[q][0] and np.array_equal(_bits(c[q][1]), _bits(a[q][1])), f"sequence {q}: a value depends on its slot"
    with pytest.raises(ValueError):
        _generator(G, m, logprobs=False).logprobs(0)


def _spec_generator(G, m, T, logprobs, script=True, max_new=24):
    from tinychatengine_amd.paged_kv import PageAllocator
    from tinychatengine_amd.speculative import SpeculativeDecoder, SpeculativeGenerator
    alloc = PageAllocator(G.NUM_PAGES, G.PAGE_KEYS, G.BATCH, G.MAX_KEYS // G.PAGE_KEYS, m.dev)
    return SpeculativeGenerator([SpeculativeDecoder(b, alloc, T) for b in m.blocks], m.final_gamma, m.lm_head, m.table, max_new=max_new, script=script, logprobs=logprobs)


def test_speculative_logprobs_equal_plain_decoding(dev):
    """T = 4, scripted drafts: the plain sequences corrupted at chosen token indices (as tests/test_gpu_speculative.py does).  Plain decoding = the same generator with
    an empty script (every step emits one token from row 0), so both sides run the linears at M = B T; where the linears' rows do not depend on their index (checked,
    not assumed) accepted rows t >= 1 give the plain tokens and then the values must be the plain values, bit for bit.  Rejected rows write nothing: every word
    behind a sequence's last token still holds NaN.  logprobs=True changes no token and no step's count.  And T = 1 equals the BatchedGenerator."""
    import test_gpu_speculative as S
    from tinychatengine_amd.generate import SamplingParams
    G, m = _small(dev)
    T = 4
    rng = np.random.default_rng(77)
    greedy, sampled = SamplingParams(temp=0.0, repeat_penalty=1.0), SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.1)
    adm = [(0, rng.integers(0, G.VOCAB, 5).tolist(), greedy, 11, 20), (1, rng.integers(0, G.VOCAB, 3).tolist(), sampled, 12, 14), (3, rng.integers(0, G.VOCAB, 9).tolist(), greedy, 13, 9)]
    plain_gen = _spec_generator(G, m, T, True)
    assert plain_gen.launches_per_token == 7 * len(m.blocks) + 7
    plain_gen.admit(adm)
    for _ in range(19):
        plain_gen.run(1)
    plain = {s: (plain_gen.tokens(s), plain_gen.logprobs(s)) for s in (0, 1, 3)}
    assert [len(plain[s][0]) for s in (0, 1, 3)] == [20, 14, 9] and all(np.isfinite(plain[s][1]).all() and len(plain[s][1]) == len(plain[s][0]) for s in plain)
    corrupted = {0: {3, 4, 9, 15}, 1: set(), 3: {1, 2, 3, 4, 5, 6, 7, 8}}
    runs = {}
    for on in (True, False):
        gen = _spec_generator(G, m, T, on)
        for s, prompt, *_ in adm:
            gen.set_script(s, [-1] * len(prompt) + [(t + 1) % G.VOCAB if i in corrupted[s] else t for i, t in enumerate(plain[s][0])])
        gen.admit(adm)
        retired = []
        while len(retired) < 3:
            retired += gen.run(1)
            assert gen._steps <= 20
        gen.allocator.check_invariants()
        runs[on] = gen
    on, off = runs[True], runs[False]
    assert np.array_equal(on.emitted_per_step(), off.emitted_per_step()) and on.emitted_per_step().max() == T
    for s in (0, 1, 3):
        assert on.tokens(s) == off.tokens(s), "logprobs=True changes the speculative run's tokens"
        n = len(on.tokens(s))
        row = on.sampler.out_logprob[s].cpu().numpy()
        assert np.isfinite(row[:n]).all() and np.isnan(row[n:]).all(), f"slot {s}: a rejected row wrote a value, or an emitted token has none"
    if S._rows_do_not_depend_on_their_index(m):
        for s in (0, 1, 3):
            assert on.tokens(s) == plain[s][0]
            assert np.array_equal(_bits(on.logprobs(s)), _bits(plain[s][1])), f"slot {s}: the speculative run's values differ from plain decoding's"
    # T = 1: the verifier's three launches against the sampler's two, same M
    one, base = _spec_generator(G, m, 1, True, script=False, max_new=12), _generator(G, m, max_new=12)
    adm1 = [(0, adm[0][1], sampled, 21, 12), (2, adm[1][1], greedy, 22, 12)]
    one.admit(adm1)
    base.admit(adm1)
    one.run(11)
    base.run(11)
    for s in (0, 2):
        assert one.tokens(s) == base.tokens(s) and len(one.tokens(s)) == 12
        assert np.array_equal(_bits(one.logprobs(s)), _bits(base.logprobs(s)))


# =====================================================================================================================================================
# score()
# =====================================================================================================================================================
def _check_scores(gen, prompts, values, vocab):
    from tinychatengine_amd.generate import logprob_reference
    logits = np.concatenate([c.cpu().numpy() for c in gen.score_logits])
    work = [p for p in prompts if len(p) >= 2]
    assert logits.shape[0] == sum(len(p) for p in work)
    assert np.abs(logits[:, :vocab].astype(np.float32)).max() <= 64
    r0, worst = 0, 0.0
    for p, v in zip(prompts, values):
        assert v.dtype == np.float32 and v.size == len(p) - 1
        if len(p) < 2:
            continue
        for i in range(len(p) - 1):
            err = abs(float(v[i]) - logprob_reference(logits[r0 + i, :vocab], p[i + 1]))
            worst = max(worst, err)
            assert err <= BOUND, f"prompt of {len(p)} tokens, token {i + 1}: |device - float64| = {err:.3e}"
        r0 += len(p)
    return worst


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_score_against_float64_on_the_logits_it_produced(dev, kv_dtype):
    """Prompts of 1, 2, 17 and 40 tokens in one call, chunk_rows 256 (one chunk of 59 rows) and 8 (seven chunks and three rows): every value within 2^-16 of float64
    on the logits the call produced (the two runs are not required bit-equal: lm_head may take another form at another M); the 1-token prompt gives an empty
    result; every page and slot is back afterwards."""
    from tinychatengine_amd.generate import perplexity
    G, m = _small(dev)
    gen = _generator(G, m, logprobs=False, kv_dtype=kv_dtype)
    gen.score_keep_logits = True
    rng = np.random.default_rng(31)
    prompts = [rng.integers(0, G.VOCAB, n).tolist() for n in (1, 2, 17, 40)]
    results = {}
    for chunk_rows in (256, 8):
        values = gen.score(prompts, chunk_rows=chunk_rows)
        assert len(gen.score_logits) == (1 if chunk_rows == 256 else 8) and gen.score_logits[-1].shape[0] == (59 if chunk_rows == 256 else 3)
        worst = _check_scores(gen, prompts, values, G.VOCAB)
        print(f"{kv_dtype} chunk_rows {chunk_rows}: worst |device - float64| = {worst:.3e} = {worst / BOUND:.2f} of 2^-16")
        gen.allocator.check_invariants()
        assert gen.allocator.pages_in_use() == 0 and gen.free_slots() == [0, 1, 2, 3]
        results[chunk_rows] = values
    for a, b in zip(results[256], results[8]):
        assert a.size == b.size and (a.size == 0 or np.abs(a - b).max() < 0.05)  # the same model, the same prompts: close, whatever the form of lm_head
    ppl = perplexity(results[256])
    assert np.isfinite(ppl) and ppl > 1.0


def test_score_beside_live_sequences_and_when_the_pool_is_short(dev):
    """score() between two runs of a live sequence changes none of its tokens; PagePoolExhausted and too few free slots leave pages, slots and the live sequence as
    they were."""
    from tinychatengine_amd.generate import SamplingParams
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    G, m = _small(dev)
    rng = np.random.default_rng(8)
    prompt = rng.integers(0, G.VOCAB, 40).tolist()  # three pages
    sampled = SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.1)
    alone = _generator(G, m)
    alone.admit(1, prompt, sampled, 5, 20)
    alone.run(19)
    gen = _generator(G, m)
    gen.score_keep_logits = True
    gen.admit(1, prompt, sampled, 5, 20)
    gen.run(6)
    scored = [rng.integers(0, G.VOCAB, n).tolist() for n in (17, 40, 9)]
    values = gen.score(scored)
    _check_scores(gen, scored, values, G.VOCAB)
    assert gen.free_slots() == [0, 2, 3] and gen.allocator.pages_in_use() == len(gen.allocator.pages[1]) == 3
    state = (list(gen.allocator.free), [list(p) for p in gen.allocator.pages], list(gen.allocator.refcount))
    with pytest.raises(PagePoolExhausted):
        gen.score([rng.integers(0, G.VOCAB, 60).tolist() for _ in range(3)])  # 3 x 4 pages, 9 free
    with pytest.raises(ValueError):
        gen.score([[1, 2]] * 4)  # four prompts, three free slots
    assert (list(gen.allocator.free), [list(p) for p in gen.allocator.pages], list(gen.allocator.refcount)) == state
    gen.allocator.check_invariants()
    gen.run(13)
    assert gen.tokens(1) == alone.tokens(1) and len(gen.tokens(1)) == 20
    assert np.array_equal(_bits(gen.logprobs(1)), _bits(alone.logprobs(1)))
    gen.allocator.check_invariants()
