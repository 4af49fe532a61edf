"""tce_sample_f16 and tce_embed_rows_f16 on the device (csrc/sampling.hip, tinychatengine_amd/generate.py: Sampler, embed_rows).

The sampler is held to the reference's own results (tests/golden/sampling_golden.npz, under the rules of tests/sampling_rules.py) and, candidates and n being
equal, token for token to the numpy restatement sample_reference on the same u.  Everything else here is exact: inactive rows against canaries, 200 calls on one
workspace against a host simulation, a row's result whatever its neighbours and slot, retirement at the right token, refusals without a launch."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


def _row_words(row) -> np.ndarray:
    return np.frombuffer(bytes(row), dtype=np.int32).copy()


def _set_rows(sampler, rows) -> None:
    sampler.rows.copy_(torch.from_numpy(np.stack([_row_words(r) for r in rows])))


def _debug(sampler) -> dict:
    d = sampler.debug.cpu().numpy()
    return {"n": d[:, 0], "k": d[:, 1], "u": d[:, 2].copy().view(np.float32), "choice": d[:, 3], "ids": d[:, 4:260], "logit": d[:, 260:516].copy().view(np.float32),
            "p": d[:, 516:772].copy().view(np.float32), "final_p": d[:, 772:1028].copy().view(np.float32)}


def _row(params, seed=0, max_new=8, ring=None, pushed=0, generated=0):
    from tinychatengine_amd.generate import make_row
    r = make_row(params, seed, max_new)
    if ring is not None:
        for i, t in enumerate(ring):
            r.ring[i] = int(t)
    r.ring_pushed, r.generated = pushed, generated
    return r


def _params(name):
    from tinychatengine_amd.generate import SamplingParams
    k, top_p, temp, sigma, rp, af, ap, rows, seed = R.CONFIGS[name]
    return SamplingParams(temp=temp, top_k=k, top_p=top_p, repeat_penalty=rp, alpha_frequency=af, alpha_presence=ap, repeat_last_n=64)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_device_sampler_against_the_references_own_code(dev, fixture, name):
    """Every row of the configuration through tce_sample_f16 at B = 16 (vocab 128256): greedy id, candidates, p, n, final p under the fixture's rules; where the
    candidates and n equal sample_reference's, the token equals sample_reference's on the same u; then every draw point of every row."""
    from tinychatengine_amd.generate import Sampler, draw_reference, sample_reference
    k, top_p, temp, sigma, rp, af, ap, rows, seed = R.CONFIGS[name]
    params = _params(name)
    inputs = R.config_inputs(name, fixture)
    B, V = 16, R.VOCAB
    logits_all = torch.from_numpy(np.stack([lg for lg, _ in inputs])).to(dev)
    s = Sampler(B, V, 4, dev, top_k_bound=max(k, 1), debug=True)
    s.uniform_override = torch.full((B,), 0.5, dtype=torch.float32, device=dev)
    pristine = [_row(params, seed=r, max_new=4, ring=inputs[r][1]) for r in range(rows)]
    refs = [None] * rows
    worst_p = worst_fp = 0.0
    draws = []  # (row, u, accepted positions)
    for r0 in range(0, rows, B):
        idx = list(range(r0, min(r0 + B, rows)))
        pad = idx + [idx[-1]] * (B - len(idx))
        _set_rows(s, [pristine[r] for r in pad])
        pos = torch.tensor([5] * len(idx) + [-1] * (B - len(idx)), dtype=torch.int32, device=dev)
        s.step(logits_all[pad].contiguous(), pos, 63)
        torch.cuda.synchronize()
        d, tok = _debug(s), s.next_token.cpu().numpy()
        for j, r in enumerate(idx):
            what = f"{name} row {r}"
            logits, recent = inputs[r]
            if temp <= 0:
                assert int(tok[j]) == int(fixture[name + "/greedy"][r]), f"{what}: greedy id"
                continue
            x = R.penalised(logits, recent, rp, af, ap)
            kk, n = int(d["k"][j]), int(d["n"][j])
            assert kk == k
            R.check_candidates(what, x, d["ids"][j][:kk], d["logit"][j][:kk], fixture[name + "/ids"][r], fixture[name + "/logit"][r])
            worst_p = max(worst_p, R.check_p(what + " p", d["p"][j][:kk], fixture[name + "/p"][r], k))
            lo, hi = R.n_band(fixture[name + "/p"][r], top_p, k)
            assert lo <= n <= hi, f"{what}: n = {n} outside [{lo}, {hi}]"
            n_ref = int(fixture[name + "/n"][r])
            if n == n_ref:
                worst_fp = max(worst_fp, R.check_p(what + " final p", d["final_p"][j][:n], fixture[name + "/final_p"][r][:n_ref], k))
                draws += [(r, u, ok) for u, ok in R.draw_points(fixture[name + "/final_p"][r][:n_ref], k, seed * 1000 + r)]
            ref = sample_reference(logits, recent, params, 0.5)
            if np.array_equal(ref["ids"], d["ids"][j][:kk]) and ref["n"] == n:
                refs[r] = ref
                assert int(tok[j]) == ref["token"] and int(d["choice"][j]) == ref["choice"], f"{what}: token {tok[j]}, sample_reference draws {ref['token']}"
    if temp > 0:  # the greedy id of the sampled configurations: the same rows with temp = 0
        g = type(params)(**{**params.__dict__, "temp": 0.0})
        for r0 in range(0, rows, B):
            idx = list(range(r0, min(r0 + B, rows)))
            pad = idx + [idx[-1]] * (B - len(idx))
            _set_rows(s, [_row(g, seed=r, max_new=4, ring=inputs[r][1]) for r in pad])
            s.step(logits_all[pad].contiguous(), torch.full((B,), 5, dtype=torch.int32, device=dev), 63)
            tok = s.next_token.cpu().numpy()
            assert tok[:len(idx)].tolist() == fixture[name + "/greedy"][idx].tolist(), f"{name} rows {r0}..: greedy ids"
    print(f"{name}: worst relative error of p {worst_p:.2e}, of the final p {worst_fp:.2e} (tolerance {R.tol(k):.2e}); {len(draws)} draw points")
    for c0 in range(0, len(draws), B):
        chunk = draws[c0:c0 + B]
        pad = chunk + [chunk[-1]] * (B - len(chunk))
        rws = [r for r, _, _ in pad]
        _set_rows(s, [pristine[r] for r in rws])
        s.uniform_override.copy_(torch.tensor([float(u) for _, u, _ in pad], dtype=torch.float32))
        s.step(logits_all[rws].contiguous(), torch.full((B,), 5, dtype=torch.int32, device=dev), 63)
        choice = s.debug[:, 3].cpu().numpy()
        for j, (r, u, ok) in enumerate(chunk):
            assert int(choice[j]) in ok, f"{name} row {r}: u = {u!r} drew position {choice[j]}, accepted {sorted(ok)}"
            if refs[r] is not None:  # candidates and n equal sample_reference's: the same position, exactly
                assert int(choice[j]) == draw_reference(refs[r]["final_p"], u), f"{name} row {r}: u = {u!r}: position {choice[j]}, sample_reference draws another"


def _random_case(rng, B, vocab, bound):
    """B rows with mixed settings: greedy rows, k from 1 to the bound, penalties on and off, rings at every fill level, windows shorter than the ring."""
    from tinychatengine_amd.generate import SamplingParams
    ld = (vocab + 7) // 8 * 8 + 8
    logits = (rng.standard_normal((B, ld), dtype=np.float32) * np.float32(2.5)).astype(np.float16)
    logits[:, vocab:] = 60000.0  # columns past the vocabulary hold the largest values: they must never be candidates
    rows, meta = [], []
    for b in range(B):
        kind = (b + int(rng.integers(0, 4))) % 4
        p = SamplingParams(temp=0.0 if kind == 0 else float(rng.uniform(0.5, 1.5)), top_k=int(rng.integers(1, bound + 1)), top_p=[0.95, 0.9, 1.0, 0.5][kind],
                           repeat_penalty=[1.1, 1.0, 1.3, 1.1][kind], alpha_frequency=[0.0, 0.0, 0.3, 0.0][kind], alpha_presence=[0.0, 0.0, 0.2, 0.0][kind],
                           repeat_last_n=[64, 64, 17, 0][kind])
        pushed = int(rng.integers(0, 150))
        ring = np.zeros(64, np.int32)
        strongest = np.argsort(-logits[b, :vocab].astype(np.float32), kind="stable")[:20]
        for t in range(pushed):
            ring[t % 64] = int(strongest[rng.integers(0, 20)]) if rng.random() < 0.5 else int(rng.integers(0, vocab))
        gen = int(rng.integers(0, 5))
        seed = int(rng.integers(0, 2 ** 63))
        rows.append(_row(p, seed=seed, max_new=100, ring=ring, pushed=pushed, generated=gen))
        meta.append((p, ring, pushed, gen, seed))
    return logits, ld, rows, meta


def _check_against_sample_reference(what, logits_row, vocab, p, ring, pushed, u, d, j, tok):
    from tinychatengine_amd.generate import ring_window, sample_reference
    ref = sample_reference(logits_row[:vocab], ring_window(ring, pushed, p.repeat_last_n), p, u)
    kk, n = int(d["k"][j]), int(d["n"][j])
    assert kk == ref["ids"].size and d["ids"][j][:kk].tolist() == ref["ids"].tolist(), f"{what}: candidate ids"
    assert np.array_equal(d["logit"][j][:kk].view(np.uint32), ref["logits"].view(np.uint32)), f"{what}: candidate logits"
    if p.temp > 0:
        R.check_p(what + " p", d["p"][j][:kk], ref["p"], max(kk, 1))
        assert n == ref["n"], f"{what}: n = {n}, sample_reference keeps {ref['n']}"
        R.check_p(what + " final p", d["final_p"][j][:n], ref["final_p"], max(kk, 1))
    assert int(tok) == ref["token"], f"{what}: token {tok}, sample_reference draws {ref['token']}"
    return ref


@pytest.mark.parametrize("vocab", [128256, 32000, 50272])
@pytest.mark.parametrize("B", [1, 3, 8, 16])
def test_batches_and_vocabularies_against_sample_reference(dev, B, vocab):
    """Vocabularies that are and are not multiples of the 4096-logit chunk, vocab < ld with large values behind it, the generator's own uniform: candidates, n and
    token equal sample_reference's, and the tail has updated token, log, ring, counters and position."""
    from tinychatengine_amd.generate import Sampler, uniform
    rng = np.random.default_rng(B * 1000003 + vocab)
    bound = 64
    logits, ld, rows, meta = _random_case(rng, B, vocab, bound)
    s = Sampler(B, vocab, 128, dev, top_k_bound=bound, debug=True)
    _set_rows(s, rows)
    pos0 = rng.integers(0, 60, B).astype(np.int32)
    pos = torch.from_numpy(pos0).to(dev)
    s.step(torch.from_numpy(logits).to(dev), pos, 63)
    torch.cuda.synchronize()
    d, tok, log = _debug(s), s.next_token.cpu().numpy(), s.out_log.cpu().numpy()
    for b, (p, ring, pushed, gen, seed) in enumerate(meta):
        u = uniform(seed, gen)
        if p.temp > 0:
            assert d["u"][b].view(np.uint32) == np.float32(u).view(np.uint32), f"row {b}: the device's uniform is not Philox4x32-10(seed, token index)"
        _check_against_sample_reference(f"B {B} vocab {vocab} row {b}", logits[b], vocab, p, ring, pushed, u, d, b, tok[b])
        after = s.row(b)
        assert after.generated == gen + 1 and after.ring_pushed == pushed + 1 and after.ring[pushed % 64] == tok[b] and log[b, gen] == tok[b]
        want_ring = ring.copy()
        want_ring[pushed % 64] = tok[b]
        assert list(after.ring) == want_ring.tolist()
    assert pos.cpu().numpy().tolist() == (pos0 + 1).tolist()


def test_inactive_rows_touch_nothing(dev):
    from tinychatengine_amd.generate import Sampler
    rng = np.random.default_rng(11)
    B, vocab = 8, 32000
    logits, ld, rows, meta = _random_case(rng, B, vocab, 40)
    s = Sampler(B, vocab, 16, dev, top_k_bound=40, debug=True)
    _set_rows(s, rows)
    s.next_token.fill_(-777)
    s.out_log.fill_(-555)
    s.debug.fill_(-333)
    pos0 = np.array([3, 0, -1, 63, 64, 9, -5, 1000], np.int32)  # bound 63: rows 2, 4, 6, 7 are inactive
    pos = torch.from_numpy(pos0).to(dev)
    before = s.rows.cpu().numpy().copy()
    s.step(torch.from_numpy(logits).to(dev), pos, 63)
    torch.cuda.synchronize()
    after, tok, log, dbg, p1 = s.rows.cpu().numpy(), s.next_token.cpu().numpy(), s.out_log.cpu().numpy(), s.debug.cpu().numpy(), pos.cpu().numpy()
    for b in range(B):
        if b in (2, 4, 6, 7):
            assert np.array_equal(after[b], before[b]) and tok[b] == -777 and (log[b] == -555).all() and (dbg[b] == -333).all() and p1[b] == pos0[b], f"inactive row {b} was touched"
        else:
            assert tok[b] >= 0 and not np.array_equal(after[b], before[b]) and p1[b] == pos0[b] + 1 and (log[b] != -555).sum() == 1


def test_two_hundred_calls_on_one_workspace(dev):
    """The workspace is zeroed once; call 200 behaves as call 1: every token of three sequences equals a host simulation with sample_reference that keeps its own
    rings and counters (the logits change every call; the generator advances with the token index)."""
    from tinychatengine_amd.generate import Sampler, SamplingParams, ring_window, sample_reference, uniform
    rng = np.random.default_rng(200)
    B, vocab, calls = 3, 50272, 200
    ps = [SamplingParams(), SamplingParams(temp=0.0), SamplingParams(top_k=7, top_p=0.8, temp=1.2, repeat_penalty=1.2, alpha_frequency=0.1, alpha_presence=0.1, repeat_last_n=32)]
    seeds = [11, 22, 33]
    s = Sampler(B, vocab, 256, dev, top_k_bound=40)
    _set_rows(s, [_row(p, seed=sd, max_new=256) for p, sd in zip(ps, seeds)])
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    base = (rng.standard_normal((8, B, vocab), dtype=np.float32) * np.float32(2.5)).astype(np.float16)
    base_t = torch.from_numpy(base).to(dev)
    for c in range(calls):
        s.step(base_t[c % 8], pos, 1000)
    torch.cuda.synchronize()
    log = s.out_log.cpu().numpy()
    assert pos.cpu().numpy().tolist() == [calls] * B and s.generated().tolist() == [calls] * B
    for b in range(B):
        ring, pushed = np.zeros(64, np.int32), 0
        for c in range(calls):
            ref = sample_reference(base[c % 8, b], ring_window(ring, pushed, ps[b].repeat_last_n), ps[b], uniform(seeds[b], c))
            assert log[b, c] == ref["token"], f"sequence {b}, call {c}: token {log[b, c]}, the host simulation draws {ref['token']}"
            ring[pushed % 64] = ref["token"]
            pushed += 1


def test_a_rows_result_does_not_depend_on_neighbours_or_slot(dev):
    from tinychatengine_amd.generate import Sampler, SamplingParams
    rng = np.random.default_rng(3)
    vocab = 128256
    row_logits = (rng.standard_normal(vocab, dtype=np.float32) * np.float32(2.5)).astype(np.float16)
    ring = rng.integers(0, vocab, 64).astype(np.int32)
    mine = lambda: _row(SamplingParams(top_k=50), seed=987654321012345, max_new=50, ring=ring, pushed=70, generated=6)
    results = []
    for B, slot in [(1, 0), (8, 5), (16, 15), (16, 0)]:
        logits = (rng.standard_normal((B, vocab), dtype=np.float32) * np.float32(3.0)).astype(np.float16)
        logits[slot] = row_logits
        _, _, rows, _ = _random_case(rng, B, 32000, 50)
        rows[slot] = mine()
        s = Sampler(B, vocab, 64, dev, top_k_bound=50, debug=True)
        _set_rows(s, rows)
        pos = torch.full((B,), 7, dtype=torch.int32, device=dev)
        if B == 16 and slot == 0:
            pos[3:9] = -1  # ... and beside retired rows
        s.step(torch.from_numpy(logits).to(dev), pos, 63)
        torch.cuda.synchronize()
        results.append((s.debug[slot].cpu().numpy().tobytes(), int(s.next_token[slot].item()), s.rows[slot].cpu().numpy().tobytes(), s.out_log[slot].cpu().numpy().tobytes()))
    assert all(r == results[0] for r in results[1:])


def test_stop_ids_and_the_budget_retire_a_row_at_the_right_token(dev):
    from tinychatengine_amd.generate import Sampler, SamplingParams
    B, vocab = 5, 32000
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    logits = np.zeros((B, vocab), np.float16)
    for b, t in enumerate([100, 200, 300, 31999, 400]):
        logits[b, t] = 5.0
    s = Sampler(B, vocab, 8, dev, top_k_bound=40, stop_ids=[7, 200, 31999])
    _set_rows(s, [_row(greedy, max_new=8), _row(greedy, max_new=8), _row(greedy, max_new=3, generated=2), _row(greedy, max_new=8), _row(greedy, max_new=3, generated=1)])
    pos = torch.tensor([10, 11, 12, 13, 14], dtype=torch.int32, device=dev)
    s.step(torch.from_numpy(logits).to(dev), pos, 63)
    assert s.next_token.cpu().numpy().tolist() == [100, 200, 300, 31999, 400]
    assert pos.cpu().numpy().tolist() == [11, -1, -1, -1, 15]  # an ordinary token; a stop id; the budget's last token; the last id of the vocabulary as a stop id; budget left
    assert s.generated().tolist() == [1, 1, 3, 1, 2]
    log = s.out_log.cpu().numpy()
    assert [log[0, 0], log[1, 0], log[2, 2], log[3, 0], log[4, 1]] == [100, 200, 300, 31999, 400]  # the retiring token is still delivered
    s.step(torch.from_numpy(logits).to(dev), pos, 63)  # retired rows stay retired and silent
    assert pos.cpu().numpy().tolist() == [12, -1, -1, -1, -1] and s.generated().tolist() == [2, 1, 3, 1, 3]


def test_unsupported_settings_are_refused_with_no_launch(dev):
    from tinychatengine_amd import capi
    from tinychatengine_amd.generate import Sampler, SamplingParams
    B, vocab = 2, 32000
    logits = torch.zeros((B, vocab), dtype=torch.float16, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    for kw in (dict(tfs_z=0.95), dict(typical_p=0.9), dict(mirostat=1), dict(top_k_bound=0), dict(top_k_bound=257)):
        s = Sampler(B, vocab, 8, dev, **{"top_k_bound": 40, **kw})
        s.next_token.fill_(-9)
        with pytest.raises(capi.TceError) as e:
            s.step(logits, pos, 63)
        assert e.value.code == capi.TCE_ERR_UNSUPPORTED_SHAPE
        torch.cuda.synchronize()
        assert s.next_token.cpu().numpy().tolist() == [-9, -9] and pos.cpu().numpy().tolist() == [0, 0] and s.generated().tolist() == [0, 0]
    s = Sampler(B, vocab, 8, dev, top_k_bound=40)
    with pytest.raises(ValueError):
        s.set_row(0, SamplingParams(top_k=0), 1, 4)  # "the whole vocabulary" is not built
    with pytest.raises(ValueError):
        s.set_row(0, SamplingParams(top_k=41), 1, 4)


def test_embed_rows(dev):
    from tinychatengine_amd.generate import embed_rows
    rng = np.random.default_rng(8)
    vocab, hidden, B = 1000, 512, 8
    table = torch.from_numpy(rng.standard_normal((vocab, hidden)).astype(np.float16)).to(dev)
    out = torch.full((B, hidden), 7.0, dtype=torch.float16, device=dev)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    token = torch.tensor([0, 999, 5, 1000, -1, 17, 17, 400], dtype=torch.int32, device=dev)
    pos = torch.tensor([0, 63, -1, 5, 6, 64, 7, 8], dtype=torch.int32, device=dev)  # rows 2 and 5 inactive; rows 3 and 4 carry ids outside the table
    embed_rows(table, token, out, pos, 63, ws)
    torch.cuda.synchronize()
    got, tab = out.cpu().numpy().view(np.uint16), table.cpu().numpy().view(np.uint16)
    seven = np.array([7.0], np.float16).view(np.uint16)[0]
    for b, t in enumerate([0, 999, None, "zero", "zero", None, 17, 400]):
        if t is None:
            assert (got[b] == seven).all(), f"inactive row {b} was written"
        elif t == "zero":
            assert (got[b] == 0).all(), f"row {b}: an id outside the table was followed"
        else:
            assert np.array_equal(got[b], tab[t]), f"row {b}"
    assert int(ws.cpu().numpy().view(np.uint32)[0]) == 2
