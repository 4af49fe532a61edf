"""Speculative decoding on the device (tinychatengine_amd/speculative.py; csrc/attention_fast.hip, csrc/sampling.hip).

(a) tce_attention_decode_step_paged_rows_f16 / _fp8: row (b, t) and the appended pool rows are BIT-IDENTICAL to t + 1 successive calls of the single-row paged step
    with the same bound; every other pool byte is unchanged; table words that must not be followed point at a page of NaNs.
(b) tce_draft_ngram against ngram_draft_reference.
(c) tce_sample_verify_f16 against verify_reference: tokens, ring, counters, log, history, positions, emitted.
(d) SpeculativeGenerator (one captured graph) against HostDrivenSpeculativeLoop token for token, with scripted drafts corrupted at chosen indices; T = 1 against
    BatchedGenerator.
(e) one run with real n-gram drafts.
There is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128
NAN16 = [0x7E00, 0x7D55, -512 + 1, 0x7FFF]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _raw(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.uint8)


# =====================================================================================================================================================
# (a) the rows step
# =====================================================================================================================================================
def _rope_tables(n, seed, dev):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, (n, HD // 2))
    cos = np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)
    return torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)


# (max_keys, [(base position slot 0, base position slot 2)]): 64 keys = one chunk, 16 keys per wave -- 0, 1, 14 (page and block edge), 61 (rows run out of the bound);
# 512 keys with bound 511 = chunks of 128, 32 keys per wave -- 30 (wave edge), 126 (the new rows fall into two chunks' workgroups), 125, 510
ROWS_SHAPES = [(64, [(0, 14), (1, 61), (14, 0), (61, 1)]), (512, [(30, 126), (125, 510), (126, 30), (510, 125)])]


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("heads,kv_heads", [(4, 1), (4, 4)])
def test_rows_step_equals_successive_single_steps(dev, heads, kv_heads, rope, kv_dtype):
    from tinychatengine_amd import capi
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention
    B, page_keys = 3, 16
    fp8 = kv_dtype == "fp8_e4m3"
    scales = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-2) if fp8 else {}
    for max_keys, bases in ROWS_SHAPES:
        bound = max_keys - 1
        assert capi.describe_attention_paged(B, heads, kv_heads, bound, page_keys)["keys-per-chunk"] == (64 if max_keys == 64 else 128)
        cos, sin = _rope_tables(max_keys, max_keys, dev) if rope else (None, None)
        stride = max_keys // page_keys
        for T in (1, 2, 4, 8):
            for case, (p0, p2) in enumerate(bases):
                what = f"{kv_dtype} heads={heads}/{kv_heads} rope={rope} keys={max_keys} T={T} bases=({p0}, {p2})"
                g = torch.Generator(device=dev).manual_seed(max_keys + 10 * T + case)
                num_pages = B * stride + 3
                alloc = PageAllocator(num_pages, page_keys, B, stride, dev, free_order=np.random.default_rng(T + case).permutation(num_pages).tolist())
                R = PagedRowsDecodeAttention(alloc, heads, kv_heads, dev, cos, sin, rows_per_seq=T, **scales)
                S = PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, cos, sin, **scales)
                if fp8:
                    fill = torch.randint(0, 256, R.k_pool.shape, generator=g, device=dev, dtype=torch.int32)
                    fill = torch.where((fill & 0x7F) == 0x7F, fill - 1, fill).to(torch.uint8)  # (no NaN bytes among the cached rows)
                    R.k_pool.copy_(fill)
                    R.v_pool.copy_(fill.flip(0))
                else:
                    R.k_pool.copy_((torch.randn(R.k_pool.shape, generator=g, device=dev) * 0.8).half())
                    R.v_pool.copy_((torch.randn(R.v_pool.shape, generator=g, device=dev) * 0.8).half())
                # active prefixes: slot 0 full (as far as the bound lets it), slot 1 inactive, slot 2 one row short (n_b < T); rows past the bound keep their
                # position and are inactive by the position rule
                n_act = [T, 0, max(1, T - 1)]
                pos = np.full((B, T), -1, np.int32)
                for b, p in ((0, p0), (2, p2)):
                    pos[b, :n_act[b]] = p + np.arange(n_act[b])
                    alloc.reserve(b, min(p + n_act[b] - 1, bound))
                # a page of NaNs behind every table word that must not be followed
                canary = alloc.free[0]
                for pool in (R.k_pool, R.v_pool):
                    if fp8:
                        pool[canary].fill_(0x7F)
                    else:
                        v = pool.view(torch.int16)[canary]
                        v.copy_(torch.tensor(NAN16, dtype=torch.int16, device=dev).repeat(v.numel() // 4).view(v.shape))
                table = torch.full_like(alloc.table, canary)
                for b, ps in enumerate(alloc.pages):
                    if ps:
                        table[b, :len(ps)] = torch.tensor(ps, dtype=torch.int32, device=dev)
                alloc.table.copy_(table)
                S.k_pool.copy_(R.k_pool)
                S.v_pool.copy_(R.v_pool)
                k0, v0 = R.k_pool.clone(), R.v_pool.clone()
                qkv = (torch.randn((B * T, (heads + 2 * kv_heads) * HD), generator=g, device=dev) * 0.9).half()
                pos_t = torch.from_numpy(pos.reshape(-1)).to(dev)
                # the yardstick first: T successive single-row steps, each after a table check
                want = torch.empty((B, T, heads * HD), dtype=torch.float16, device=dev)
                for t in range(T):
                    pt = torch.from_numpy(pos[:, t].copy()).to(dev)
                    assert S.table_violations(pt, bound) == 0, f"{what}: the block table is not sound: no launch"
                    want[:, t] = S.step(qkv.view(B, T, -1)[:, t].contiguous(), pt, bound)
                out = torch.full((B * T, heads * HD), 3.0, dtype=torch.float16, device=dev)
                R.step(qkv, pos_t, bound, out=out)
                torch.cuda.synchronize()
                assert not torch.isnan(out.float()).any(), f"{what}: the canary leaked into an output"
                assert torch.equal(_raw(out).view(B, T, -1), _raw(want).view(B, T, -1)), f"{what}: output rows differ"
                assert torch.equal(_raw(R.k_pool), _raw(S.k_pool)) and torch.equal(_raw(R.v_pool), _raw(S.v_pool)), f"{what}: the pools differ from the single steps'"
                # the single steps' pools = the start + the appended rows; checked here so that "every other byte unchanged" does not rest on them alone
                changed = (_raw(R.k_pool) != _raw(k0)).any(-1) | (_raw(R.v_pool) != _raw(v0)).any(-1)  # [page][head][row]
                allowed = torch.zeros_like(changed)
                for b in (0, 2):
                    for t in range(T):
                        p = int(pos[b, t])
                        if 0 <= p <= bound:
                            allowed[alloc.pages[b][p // page_keys], :, p % page_keys] = True
                assert not (changed & ~allowed).any(), f"{what}: a pool row other than the appended ones changed"
                assert not changed[canary].any()
                del R, S, alloc


def test_rows_step_refusals(dev):
    from tinychatengine_amd import capi
    from tinychatengine_amd.paged_kv import PageAllocator
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention
    alloc = PageAllocator(8, 16, 2, 4, dev)
    with pytest.raises(ValueError):
        PagedRowsDecodeAttention(alloc, 4, 1, dev, rows_per_seq=9)
    R = PagedRowsDecodeAttention(alloc, 4, 1, dev, rows_per_seq=8)
    R.rows_per_seq = 9  # past the Python check: the library refuses before any launch
    qkv = torch.zeros((18, 6 * HD), dtype=torch.float16, device=dev)
    pos = torch.full((18,), -1, dtype=torch.int32, device=dev)
    with pytest.raises(Exception, match="rows_per_seq"):
        R.step(qkv, pos, 63)


# =====================================================================================================================================================
# (b) drafts
# =====================================================================================================================================================
def _device_drafts(dev, hist, pos, bound, T, n, script=None):
    from tinychatengine_amd.speculative import draft_ngram
    B = len(pos)
    h = torch.from_numpy(np.asarray(hist, np.int32)).to(dev)
    sc = torch.from_numpy(np.asarray(script, np.int32)).to(dev) if script is not None else None
    tok = torch.full((B * T,), 77, dtype=torch.int32, device=dev)
    rp = torch.full((B * T,), 77, dtype=torch.int32, device=dev)
    draft_ngram(h, sc, torch.from_numpy(np.asarray(pos, np.int32)).to(dev), bound, T, n, tok, rp)
    return tok.cpu().numpy().reshape(B, T), rp.cpu().numpy().reshape(B, T)


def test_draft_ngram_equals_the_reference(dev):
    from tinychatengine_amd.speculative import ngram_draft_reference
    stride = 72
    designed = [([1, 2, 3, 4, 5, 6], 5), ([7, 7, 7], 1), ([7, 7, 7], 2), ([1, 2, 30, 31, 1, 2, 40, 41, 1, 2], 9), ([5, 9, 9], 2), ([1, 2, 30, 31, 32, 1, 2], 6),
                ([1, 2, 30, 31, 32, 1, 2], -1), ([3] * 70, 63), ([3] * 70, 64)]
    rng = np.random.default_rng(5)
    for _ in range(40):  # a vocabulary of 4: matches are dense
        designed.append((rng.integers(0, 4, 70).tolist(), int(rng.integers(0, 66))))
    hist = np.full((len(designed), stride), 9999, np.int32)  # (what lies behind a sequence's position is not its history)
    pos = []
    for i, (h, p) in enumerate(designed):
        hist[i, :len(h)] = h
        pos.append(p)
    script = np.full_like(hist, -1)
    script[:, 3:40] = rng.integers(0, 50, (len(designed), 37))
    script[::3, 8] = -1
    for bound in (63, 7, 6):
        for T in (1, 4, 8):
            for n in (1, 2, 3, 4):
                for sc in (None, script):
                    tok, rp = _device_drafts(dev, hist, pos, bound, T, n, sc)
                    for i, p in enumerate(pos):
                        wt, wp = ngram_draft_reference(hist[i], p, n, T, bound, script=None if sc is None else sc[i])
                        assert tok[i].tolist() == wt.tolist() and rp[i].tolist() == wp.tolist(), f"sequence {i} p={p} bound={bound} T={T} n={n} script={sc is not None}"


# =====================================================================================================================================================
# (c) the verifier
# =====================================================================================================================================================
def _verify_case(dev, vocab, params, cases, stop_ids=(), log_stride=16, T=4, sampled=False):
    """cases: per sequence a dict(p, n, targets [n] (the token each row's logits favour), drafts [n - 1], max_new, generated, active).  Builds designed logits, runs
    the device verifier and verify_reference from the same state, and compares everything."""
    from tinychatengine_amd.generate import Sampler, make_row, ring_window, sample_reference
    from tinychatengine_amd.speculative import Verifier, verify_reference
    from tinychatengine_amd import capi
    B = len(cases)
    ld = (vocab + 7) // 8 * 8
    rng = np.random.default_rng(vocab + B)
    smp = Sampler(B, vocab, log_stride, dev, top_k_bound=8, stop_ids=stop_ids)
    ver = Verifier(smp, T)
    hist_stride = 80
    logits = np.zeros((B * T, ld), np.float16)
    row_token, row_pos = np.zeros((B, T), np.int32), np.full((B, T), -1, np.int32)
    history = rng.integers(0, vocab, (B, hist_stride)).astype(np.int32)
    pos = np.array([c["p"] if c.get("active", True) else -1 for c in cases], np.int32)
    uniforms = np.zeros((B, T), np.float32)
    prompts = []
    for b, c in enumerate(cases):
        prompt = rng.integers(0, vocab, 5).tolist()
        prompts.append(prompt)
        smp.set_row(b, params, seed=1000 + b, max_new=c["max_new"], prompt_ids=prompt)
        n = c["n"]
        row_token[b, 0] = history[b, c["p"]]
        row_token[b, 1:n] = c["drafts"]
        if c.get("active", True):
            row_pos[b, :n] = c["p"] + np.arange(n)
        for t in range(T):
            row = rng.uniform(-1.0, 1.0, ld).astype(np.float16)
            if t < n:
                for rank, tok in enumerate(c["targets"][t]):  # large gaps: the favoured token, then runners-up 2.0 apart (the penalty cases need the second)
                    row[tok] = np.float16(12.0 - 2.0 * rank)
            logits[b * T + t] = row
    rows_t = smp.rows.clone()
    # counters a sequence in mid-flight has: `generated` tokens behind it
    for b, c in enumerate(cases):
        if c.get("generated", 0):
            smp.rows[b, 10] = c["generated"]
    if sampled:  # a uniform at the midpoint of a chosen candidate's CDF interval, row by row along the accepted chain
        for b, c in enumerate(cases):
            r = make_row(params, 1000 + b, c["max_new"], prompts[b])
            ring, pushed = np.array(list(r.ring), np.int32), int(r.ring_pushed)
            for t in range(c["n"]):
                ref = sample_reference(logits[b * T + t, :vocab], ring_window(ring, pushed, params.repeat_last_n), params, 0.0)
                cdf = np.cumsum(ref["final_p"], dtype=np.float32)
                pick = (b + t) % ref["n"]
                uniforms[b, t] = (cdf[pick] + (cdf[pick - 1] if pick else 0.0)) / 2
                y = int(ref["ids"][pick])
                if t + 1 < c["n"] and c.get("follow", True):
                    row_token[b, t + 1] = y if t + 1 not in c.get("wrong", ()) else (y + 1) % vocab
                ring[pushed % 64] = y
                pushed += 1
        ver.uniform_override = torch.from_numpy(uniforms.reshape(-1)).to(dev)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lg, rt, rp, hs, ps = d(logits), d(row_token.reshape(-1)), d(row_pos.reshape(-1)), d(history), d(pos)
    next0 = smp.next_token.clone()
    ver.step(lg, rt, rp, hs, ps, 63)
    torch.cuda.synchronize()
    got_pos, got_hist, got_emit, got_next = ps.cpu().numpy(), hs.cpu().numpy(), ver.emitted.cpu().numpy(), smp.next_token.cpu().numpy()
    got_log = smp.out_log.cpu().numpy()
    emitted = []
    for b, c in enumerate(cases):
        r0 = capi.SampleRow.from_buffer_copy(rows_t[b].cpu().numpy().tobytes())
        r1 = smp.row(b)
        g0 = c.get("generated", 0)
        what = f"vocab {vocab} sequence {b} ({c.get('name', '')})"
        if not c.get("active", True):
            assert got_emit[b] == 0 and got_pos[b] == -1 and list(r1.ring) == list(r0.ring) and r1.generated == g0 and r1.ring_pushed == r0.ring_pushed, what
            assert np.array_equal(got_hist[b], history[b]) and got_next[b] == next0[b].item() and (got_log[b] == -1).all(), what
            emitted.append(0)
            continue
        n = c["n"]
        v = verify_reference(logits[b * T:b * T + n, :vocab], row_token[b, 1:n], np.array(list(r0.ring), np.int32), r0.ring_pushed, g0, params, 1000 + b, stop_ids,
                             c["max_new"], uniforms=uniforms[b] if sampled else None, log_stride=log_stride)
        e = len(v["tokens"])
        assert got_emit[b] == e, f"{what}: emitted {got_emit[b]}, the reference {e}"
        assert got_log[b, g0:g0 + e].tolist() == v["tokens"] and (got_log[b, g0 + e:] == -1).all() and (got_log[b, :g0] == -1).all(), what
        assert list(r1.ring) == v["ring"].tolist() and r1.ring_pushed == v["pushed"] and r1.generated == v["generated"], what
        assert got_next[b] == v["tokens"][-1] and got_pos[b] == (-1 if v["retired"] else c["p"] + e), what
        want_hist = history[b].copy()
        want_hist[c["p"] + 1:c["p"] + 1 + e] = v["tokens"]
        assert np.array_equal(got_hist[b], want_hist), what
        if "emits" in c:
            assert e == c["emits"], f"{what}: the case was designed to emit {c['emits']}, it emitted {e}"
        emitted.append(e)
    return emitted


@pytest.mark.parametrize("vocab", [4096, 4097])
def test_verify_greedy_chains(dev, vocab):
    from tinychatengine_amd.generate import SamplingParams
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    tg = [[100], [200], [300], [vocab - 1]]  # y_t, known from the gaps
    y = [t[0] for t in tg]
    cases = [dict(name="all drafts right", p=10, n=4, targets=tg, drafts=y[:3], max_new=16, emits=4),
             dict(name="wrong at t = 1", p=0, n=4, targets=tg, drafts=[5, y[1], y[2]], max_new=16, emits=1),
             dict(name="wrong at t = 2", p=30, n=4, targets=tg, drafts=[y[0], 5, y[2]], max_new=16, emits=2),
             dict(name="wrong at t = 3", p=59, n=4, targets=tg, drafts=[y[0], y[1], 5], max_new=16, emits=3),
             dict(name="a stop id in mid-chain", p=20, n=4, targets=[[100], [777], [300], [400]], drafts=[100, 777, 300], max_new=16, emits=2),
             dict(name="the budget in mid-chain", p=21, n=4, targets=tg, drafts=y[:3], max_new=7, generated=4, emits=3),
             dict(name="ragged: two rows", p=22, n=2, targets=tg[:2], drafts=y[:1], max_new=16, emits=2),
             dict(name="ragged: one row", p=63, n=1, targets=tg[:1], drafts=[], max_new=16, emits=1),
             dict(name="inactive", p=5, n=4, targets=tg, drafts=y[:3], max_new=16, active=False),
             dict(name="the log's end in mid-chain", p=23, n=4, targets=tg, drafts=y[:3], max_new=16, generated=14, emits=2)]
    assert _verify_case(dev, vocab, greedy, cases, stop_ids=(777,)) == [4, 1, 2, 3, 2, 3, 2, 1, 0, 2]


@pytest.mark.parametrize("vocab", [4096, 4097])
def test_verify_penalties_use_the_virtual_window(dev, vocab):
    """Row t's favourite is the token row t - 1 emits: only the window WITH the accepted drafts pushed penalises it (12 / 1.5 = 8 < 10), so the runner-up wins.  A
    verifier that sampled every row with the ring as it stands would emit the favourite."""
    from tinychatengine_amd.generate import SamplingParams
    pen = SamplingParams(temp=0.0, repeat_penalty=1.5, alpha_frequency=0.25, alpha_presence=0.25, repeat_last_n=64)
    a, b, c, d = 50, 60, 70, vocab - 1
    targets = [[a, b], [a, b], [b, c], [c, d]]  # emits a, then b (a penalised), then c (b penalised), then d
    cases = [dict(name="chain through the window", p=12, n=4, targets=targets, drafts=[a, b, c], max_new=16, emits=4),
             dict(name="the draft ignores the penalty", p=13, n=4, targets=targets, drafts=[a, a, c], max_new=16, emits=2)]
    _verify_case(dev, vocab, pen, cases)


@pytest.mark.parametrize("vocab", [4096, 4097])
def test_verify_sampled_rows(dev, vocab):
    """temp > 0, top-k 8, top-p, penalties on: uniforms at the midpoints of CDF intervals pick a known candidate per row; drafts follow the picks, or miss at a chosen
    row."""
    from tinychatengine_amd.generate import SamplingParams
    sp = SamplingParams(temp=0.9, top_k=8, top_p=0.97, repeat_penalty=1.2, repeat_last_n=16)
    close = lambda base: [base, base + 1, base + 2, base + 3]  # 12, 10, 8, 6: four candidates with weight
    tg = [close(100), close(200), close(300), close(vocab - 4)]
    cases = [dict(name="all drafts follow", p=3, n=4, targets=tg, drafts=[0, 0, 0], max_new=16, emits=4),
             dict(name="the draft misses at row 2", p=40, n=4, targets=tg, drafts=[0, 0, 0], wrong=(2,), max_new=16, emits=2),
             dict(name="three rows", p=41, n=3, targets=tg[:3], drafts=[0, 0], max_new=16, emits=3)]
    _verify_case(dev, vocab, sp, cases, sampled=True)


def test_verify_refusals(dev):
    from tinychatengine_amd.generate import Sampler
    from tinychatengine_amd.speculative import Verifier
    smp = Sampler(2, 4096, 8, dev)
    with pytest.raises(ValueError):
        Verifier(smp, 9)
    ver = Verifier(smp, 4)
    z = lambda n, fill=0: torch.full((n,), fill, dtype=torch.int32, device=dev)
    lg = torch.zeros((8, 4096), dtype=torch.float16, device=dev)
    hist = torch.zeros((2, 60), dtype=torch.int32, device=dev)
    with pytest.raises(Exception, match="hist_stride"):
        ver.step(lg, z(8), z(8, -1), hist, z(2, -1), 63)
    smp.tfs_z = 0.5
    with pytest.raises(Exception, match="not built"):
        ver.step(lg, z(8), z(8, -1), torch.zeros((2, 64), dtype=torch.int32, device=dev), z(2, -1), 63)


# =====================================================================================================================================================
# (d), (e) end to end
# =====================================================================================================================================================
VOCAB, MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES = 4096, 64, 16, 4, 12  # (test_gpu_generate.py's: fewer pages than 4 slots x 4)


def _small(dev):
    import test_gpu_generate as G
    assert (G.VOCAB, G.MAX_KEYS, G.PAGE_KEYS, G.BATCH, G.NUM_PAGES) == (VOCAB, MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES)
    return G._model(dev, G.SMALL)


def _spec_decoders(m, T, kv_dtype, free_order=None):
    from tinychatengine_amd.paged_kv import PageAllocator
    from tinychatengine_amd.speculative import SpeculativeDecoder
    alloc = PageAllocator(NUM_PAGES, PAGE_KEYS, BATCH, MAX_KEYS // PAGE_KEYS, m.dev, free_order=free_order)
    kw = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-1) if kv_dtype != "fp16" else {}
    return [SpeculativeDecoder(b, alloc, T, **kw) for b in m.blocks]


def _spec_generator(m, T, kv_dtype, script, ngram=2, stop_ids=(), free_order=None, max_new=24):
    from tinychatengine_amd.speculative import SpeculativeGenerator
    return SpeculativeGenerator(_spec_decoders(m, T, kv_dtype, free_order), m.final_gamma, m.lm_head, m.table, max_new=max_new, ngram=ngram, stop_ids=stop_ids, script=script)


def _spec_host(m, T, kv_dtype, ngram=2, stop_ids=(), free_order=None):
    from tinychatengine_amd.speculative import HostDrivenSpeculativeLoop
    return HostDrivenSpeculativeLoop(_spec_decoders(m, T, kv_dtype, free_order), m.final_gamma, m.lm_head, m.table, ngram=ngram, stop_ids=stop_ids)


def _rows_do_not_depend_on_their_index(m):
    """w4a16_forward on the model's linears at M = 16 with the rows permuted gives the permuted bits?"""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import _stream
    g = torch.Generator(device=m.dev).manual_seed(3)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(16)).to(m.dev)
    blk = m.blocks[0]
    for lin in (m.lm_head, blk.qkv, blk.o, blk.gate, blk.up, blk.down):
        x = torch.randn((16, lin.in_features), generator=g, device=m.dev).half()
        y1 = torch.empty((16, lin.out_features), dtype=torch.float16, device=m.dev)
        y2 = torch.empty_like(y1)
        capi.check(capi.w4a16_forward(lin.desc(x, y1), _stream()))
        capi.check(capi.w4a16_forward(lin.desc(x[perm].contiguous(), y2), _stream()))
        torch.cuda.synchronize()
        if not torch.equal(_raw(y2), _raw(y1[perm])):
            return False
    return True


def _expected_emitted(total: int, corrupted: set, T: int) -> list[int]:
    """Tokens per step of a sequence whose plain run produces `total` tokens (the first at admission) when every draft is the plain token except those for the token
    indices in `corrupted`."""
    g, steps = 1, []
    while g < total:
        e = 0
        for t in range(T):
            e += 1
            if g + e >= total:          # the sequence retires with this token
                break
            if g + t in corrupted:      # row t + 1 was fed a wrong guess for token g + t
                break
        steps.append(e)
        g += e
    return steps


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_scripted_graph_run_equals_the_host_loop_and_plain_decoding(dev, kv_dtype):
    from tinychatengine_amd.generate import SamplingParams
    m = _small(dev)
    T = 4
    rng = np.random.default_rng(77)
    greedy, sampled = SamplingParams(temp=0.0, repeat_penalty=1.0), SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.1)
    adm = [(0, rng.integers(0, VOCAB, 5).tolist(), greedy, 11, 20), (1, rng.integers(0, VOCAB, 3).tolist(), sampled, 12, 14), (3, rng.integers(0, VOCAB, 9).tolist(), greedy, 13, 9)]
    later = (3, rng.integers(0, VOCAB, 6).tolist(), sampled, 14, 8)
    order = np.random.default_rng(13).permutation(NUM_PAGES).tolist()

    # discovery: an all -1 script, so every row 0 is a plain token and a step emits exactly one
    disc = _spec_generator(m, T, kv_dtype, script=True, free_order=order)
    assert disc.launches_per_token == 7 * len(m.blocks) + 4 + 3
    assert disc.admit(adm) == []
    retired = []
    for _ in range(19):
        retired += disc.run(1)
        disc.allocator.check_invariants()
    assert sorted(retired) == [0, 1, 3]
    plain = {s: disc.tokens(s) for s, *_ in adm}
    assert [len(plain[s]) for s in (0, 1, 3)] == [20, 14, 9]
    em = disc.emitted_per_step()
    assert em.shape == (19, BATCH) and set(np.unique(em)) <= {0, 1} and em[:, 0].sum() == 19 and em[:, 2].sum() == 0
    disc.release(3)
    disc.admit(*later)
    for _ in range(7):
        disc.run(1)
    plain["later"] = disc.tokens(3)
    assert len(plain["later"]) == 8
    del disc

    # the scripts: the plain sequences, corrupted at chosen token indices
    corrupted = {0: {3, 4, 9, 15}, 1: set(), 3: {1, 2, 3, 4, 5, 6, 7, 8}, "later": {5}}

    def script_for(prompt, seq, bad):
        row = [-1] * len(prompt) + [(t + 1) % VOCAB if i in bad else t for i, t in enumerate(seq)]
        return row

    gen = _spec_generator(m, T, kv_dtype, script=True, free_order=order)
    host = _spec_host(m, T, kv_dtype, free_order=order)
    host.script = [None] * BATCH
    for s, prompt, *_ in adm:
        gen.set_script(s, script_for(prompt, plain[s], corrupted[s]))
        host.script[s] = script_for(prompt, plain[s], corrupted[s]) + [-1] * 80
    assert gen.admit(adm) == []
    host.admit(adm)

    def both_step():
        r = gen.run(1)
        host.step()
        gen.allocator.check_invariants()
        for s in range(BATCH):
            if host.state[s] is not None:
                assert gen.tokens(s) == host.tokens(s), f"slot {s}: the graph run and the host-driven loop disagree"
        assert gen.emitted_per_step()[-1].tolist() == host.emitted[-1]
        return r

    retired = []
    while len(retired) < 3:
        retired += both_step()
        assert len(host.emitted) <= 20
    em = gen.emitted_per_step()
    for s in (0, 1, 3):
        want = _expected_emitted(len(plain[s]), corrupted[s], T)
        got = [int(e) for e in em[:, s] if e]
        assert got == want, f"slot {s}: emitted per step {got}, the corruption pattern gives {want}"
    assert [int(e) for e in em[:, 1] if e] == [4, 4, 4, 1]  # nothing corrupted: 13 tokens behind the first in four steps
    assert em[:, 2].sum() == 0

    # a slot retires, its pages come back and are reused
    released = gen.release(3)
    host.release(3)
    assert released
    gen.set_script(3, script_for(later[1], plain["later"], corrupted["later"]))
    host.script[3] = script_for(later[1], plain["later"], corrupted["later"]) + [-1] * 80
    gen.admit(*later)
    host.admit([later])
    assert set(gen.allocator.pages[3]) & set(released), "the new sequence reuses none of the released pages"
    steps0 = len(host.emitted)
    while 3 not in retired[3:]:
        retired += both_step()
        assert len(host.emitted) <= steps0 + 8
    assert [int(e) for e in gen.emitted_per_step()[steps0:, 3] if e] == _expected_emitted(8, corrupted["later"], T)
    assert gen.embed_violations() == 0
    gen.allocator.check_invariants()
    host.allocator.check_invariants()

    # losslessness against plain decoding needs a row's logits not to depend on its index in the M = B T launch: checked, not assumed
    if _rows_do_not_depend_on_their_index(m):
        for s in (0, 1):
            assert gen.tokens(s) == plain[s], f"slot {s}: the scripted run differs from plain decoding"
        assert gen.tokens(3) == plain["later"]


def test_one_row_per_sequence_equals_the_batched_generator(dev):
    from tinychatengine_amd.generate import SamplingParams
    m = _small(dev)
    rng = np.random.default_rng(5)
    sampled = SamplingParams(temp=0.7, top_k=10, top_p=0.9, repeat_penalty=1.15)
    adm = [(0, rng.integers(0, VOCAB, 7).tolist(), sampled, 21, 12), (2, rng.integers(0, VOCAB, 2).tolist(), SamplingParams(temp=0.0), 22, 12)]
    plain = m.generator(max_new=12)
    spec = _spec_generator(m, 1, "fp16", script=False, max_new=12)
    assert spec.launches_per_token == plain.launches_per_token + 2  # the draft launch and the verifier's third
    plain.admit(adm)
    spec.admit(adm)
    plain.run(11)
    spec.run(11)
    for s in (0, 2):
        assert len(plain.tokens(s)) == 12 and spec.tokens(s) == plain.tokens(s)
    assert spec.book.live() == plain.book.live() == []


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_ngram_drafts_graph_run_equals_the_host_loop(dev, kv_dtype):
    """Prompts that repeat a short pattern, real prompt-lookup drafts.  What gets accepted depends on the synthetic weights; the graph run and the host-driven loop
    must agree on every token and on every step's count."""
    from tinychatengine_amd.generate import SamplingParams
    m = _small(dev)
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    adm = [(0, [11, 12, 13] * 4, greedy, 1, 16), (1, [900, 901] * 5 + [900], greedy, 2, 16), (2, [5] * 6, SamplingParams(temp=0.8, top_k=4), 3, 10)]
    gen = _spec_generator(m, 4, kv_dtype, script=False, ngram=2)
    host = _spec_host(m, 4, kv_dtype, ngram=2)
    gen.admit(adm)
    host.admit(adm)
    retired = []
    while len(retired) < 3:
        retired += gen.run(1)
        host.step()
        assert gen.emitted_per_step()[-1].tolist() == host.emitted[-1]
        for s in range(3):
            assert gen.tokens(s) == host.tokens(s)
        assert len(host.emitted) <= 16
    gen.allocator.check_invariants()
    assert [len(gen.tokens(s)) for s in range(3)] == [16, 16, 10]
