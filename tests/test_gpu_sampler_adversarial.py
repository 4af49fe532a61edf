"""The designed sampler cases (tests/sampler_cases.py) on the device: tce_sample_f16, tce_sample_logprobs_f16, tce_sample_constrained_f16 and the verifier's three
forms (csrc/sampling.hip) against the independent reference of the case table.

Cases of one (vocab, top_k_bound) share a call of B <= 16 with inactive rows among them.  Every call runs in four forms -- plain, logprobs, constraints with the row
unconstrained, constraints with a one-state automaton that allows every id -- which must leave bit-identical debug blocks, tokens, rows, logs and positions; the plain
form's are then held to the reference: ids, logit bits, n, choice and token exactly, p and final p bit for bit (exact cases) or within the case's tolerance of
float64 (toleranced cases), the tail (log, ring, counters, position) exactly, the emitted token's logprob within test_gpu_logprobs.py's bound of logprob_reference."""
import dataclasses
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as S  # noqa: E402

F32 = np.float32
LOGPROB_BOUND = 2.0 ** -16  # tests/test_gpu_logprobs.py: BOUND
FORMS = ("plain", "logprobs", "unconstrained", "allow_all")
LOG = 16
POS, POS_BOUND = 5, 63


def _groups() -> dict:
    g: dict = {}
    for c in S.cases():
        g.setdefault((c.vocab, c.bound), []).append(c)
    return g


GROUPS = _groups()
WORST: dict = {}  # family -> [worst p, its tolerance, worst final p, its tolerance]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _bits(a) -> np.ndarray:
    return np.asarray(a, F32).view(np.uint32)


def _params(c):
    from tinychatengine_amd.generate import SamplingParams
    return SamplingParams(**dataclasses.asdict(c.prm))


def _row(c, seed, generated=0):
    from tinychatengine_amd.generate import make_row
    r = make_row(_params(c), seed, LOG)
    for i, t in enumerate(c.ring.tolist()):
        r.ring[i] = int(t)
    r.ring_pushed, r.generated = int(c.pushed), generated
    return r


def _words(row) -> np.ndarray:
    return np.frombuffer(bytes(row), dtype=np.int32).copy()


def _debug(words: np.ndarray) -> dict:
    d = words
    return {"n": d[:, 0], "k": d[:, 1], "u": d[:, 2].copy().view(F32), "choice": d[:, 3], "ids": d[:, 4:260], "logit": d[:, 260:516].copy().view(F32),
            "p": d[:, 516:772].copy().view(F32), "final_p": d[:, 772:1028].copy().view(F32)}


def _sampler(dev, B, vocab, bound, form):
    """A Sampler in one of the four forms; allow_all: every row names a one-state automaton whose mask allows every id of the vocabulary and whose default loops."""
    from tinychatengine_amd.constrain import constraint_row
    from tinychatengine_amd.generate import Sampler
    s = Sampler(B, vocab, LOG, dev, top_k_bound=bound, debug=True, logprobs=form == "logprobs", constraints=form in ("unconstrained", "allow_all"))
    if form == "allow_all":
        words = (vocab + 31) // 32
        mask = np.full((1, words), 0xFFFFFFFF, np.uint32)
        if vocab % 32:
            mask[0, -1] = (1 << (vocab % 32)) - 1
        idx = s.table.register_packed({"mask": mask, "edge_begin": np.array([0, 0], np.int32), "edge_token": np.array([0], np.int32), "edge_next": np.array([0], np.int32),
                                       "default_next": np.array([0], np.int32), "states": 1, "mask_words": words, "start": 0})
        cr = torch.from_numpy(_words(constraint_row(idx, 0, ())))
        for b in range(B):
            s.crows[b].copy_(cr)
    return s


def _layout(cs, with_inactive: bool):
    """[(case, active)] of a call: the cases in order, an inactive copy of the first case at slot 1 and of the last at the end."""
    rows = [(c, True) for c in cs]
    if with_inactive:
        rows.insert(1, (cs[0], False))
        rows.append((cs[-1], False))
    assert len(rows) <= 16
    return rows


def _step(dev, layout, vocab, bound, form):
    B = len(layout)
    s = _sampler(dev, B, vocab, bound, form)
    logits = torch.from_numpy(np.stack([S.padded(c) for c, _ in layout])).to(dev)
    s.rows.copy_(torch.from_numpy(np.stack([_words(_row(c, 100 + b)) for b, (c, _) in enumerate(layout)])))
    s.uniform_override = torch.tensor([float(F32(c.u)) for c, _ in layout], dtype=torch.float32, device=dev)
    s.next_token.fill_(-7)
    pos0 = np.array([POS if a else (-1 if b % 2 else POS_BOUND + 1) for b, (_, a) in enumerate(layout)], np.int32)
    pos = torch.from_numpy(pos0).to(dev)
    before = s.rows.cpu().numpy().copy()
    s.step(logits, pos, POS_BOUND)
    torch.cuda.synchronize()
    out = {"debug": s.debug.cpu().numpy(), "token": s.next_token.cpu().numpy(), "rows": s.rows.cpu().numpy(), "log": s.out_log.cpu().numpy(), "pos": pos.cpu().numpy(),
           "before": before, "pos0": pos0}
    if form == "logprobs":
        out["logprob"] = s.out_logprob.cpu().numpy()
    if form in ("unconstrained", "allow_all"):
        assert s.violations() == 0, f"{form}: the device counted a constraint violation"
    return out


def _note(c, wp, tp, wf, tf) -> None:
    w = WORST.setdefault(c.family, [0.0, 0.0, 0.0, 0.0])
    if wp >= w[0]:
        w[0], w[1] = wp, tp
    if wf >= w[2]:
        w[2], w[3] = wf, tf


def _check_tail(c, b, st, what) -> int:
    """The tail, whatever the case: exactly one token of the vocabulary, in the log, in the ring, counted, the position moved on."""
    from tinychatengine_amd import capi
    tok = int(st["token"][b])
    after, before = capi.SampleRow.from_buffer_copy(st["rows"][b].tobytes()), capi.SampleRow.from_buffer_copy(st["before"][b].tobytes())
    assert 0 <= tok < c.vocab, f"{what}: token {tok} outside the vocabulary"
    assert after.generated == 1 and after.ring_pushed == before.ring_pushed + 1 and st["pos"][b] == POS + 1, f"{what}: the row did not advance exactly once"
    want_ring = list(before.ring)
    want_ring[before.ring_pushed % 64] = tok
    assert list(after.ring) == want_ring and st["log"][b, 0] == tok and (st["log"][b, 1:] == -1).all(), f"{what}: ring / log"
    return tok


def _check_row(c, b, st, lp) -> None:
    """Row b of a call's plain-form state against the reference of its case."""
    from tinychatengine_amd.generate import logprob_reference
    what = f"{c.name} (row {b})"
    d = _debug(st["debug"])
    tok = _check_tail(c, b, st, what)
    if c.kind == "undefined":
        print(f"{what}: the device emits {tok} (k = {d['k'][b]}, n = {d['n'][b]}, choice = {d['choice'][b]}, ids {d['ids'][b][:d['k'][b]].tolist()})")
        return
    if not S.defined(c):  # the greedy row with +inf logits: the first +inf id
        assert tok == c.expect["token"] and d["ids"][b][0] == tok, f"{what}: greedy token {tok}, max_element picks {c.expect['token']}"
        return
    ref = S.ref_of(c)
    kk, n = int(d["k"][b]), int(d["n"][b])
    assert kk == ref["ids"].size, f"{what}: {kk} candidates, the reference has {ref['ids'].size}"
    assert d["ids"][b][:kk].tolist() == ref["ids"].tolist(), f"{what}: candidate ids {d['ids'][b][:kk].tolist()[:12]} ..., the reference {ref['ids'].tolist()[:12]} ..."
    assert (d["ids"][b][kk:] == -1).all()
    assert np.array_equal(_bits(d["logit"][b][:kk]), _bits(ref["logits"])), f"{what}: candidate logits {d['logit'][b][:kk][:8]}, the reference {ref['logits'][:8]}"
    print(f"{what}: n {n} / {ref['n']}, choice {d['choice'][b]} / {ref['choice']}, token {tok} / {ref['token']}", end="")
    if c.kind != "greedy":
        assert _bits(d["u"][b]) == _bits(F32(c.u)), f"{what}: the uniform is not the override"
        wp, wf = S.rel_err(d["p"][b][:kk], ref["p"]), (S.rel_err(d["final_p"][b][:n], ref["final_p"]) if n == ref["n"] else float("nan"))
        tp, tf = S.tol_p(c), S.tol_final(c, ref)
        print(f"; p {wp:.2e} (tol {tp:.2e}), final p {wf:.2e} (tol {tf:.2e})", end="")
        assert n == ref["n"], f"{what}: n = {n}, the reference keeps {ref['n']}"
        if c.kind == "exact":
            assert np.array_equal(_bits(d["p"][b][:kk]), _bits(ref["p"])), f"{what}: p is not the exact {ref['p'].astype(F32)[:8]}: {d['p'][b][:kk][:8]}"
            assert np.array_equal(_bits(d["final_p"][b][:n]), _bits(ref["final_p"])), f"{what}: final p is not the exact {ref['final_p'].astype(F32)[:8]}: {d['final_p'][b][:n][:8]}"
        else:
            assert wp <= tp, f"{what}: p off by {wp:.3e} > {tp:.3e}"
            assert wf <= tf, f"{what}: final p off by {wf:.3e} > {tf:.3e}"
            _note(c, wp, tp, wf, tf)
        assert (d["final_p"][b][n:] == 0).all() and (d["p"][b][kk:] == 0).all()
    print()
    assert int(d["choice"][b]) == ref["choice"] and tok == ref["token"], f"{what}: position {d['choice'][b]} = token {tok}, the reference draws position {ref['choice']} = token {ref['token']}"
    want = logprob_reference(c.logits, tok)
    assert abs(float(lp[b, 0]) - want) <= LOGPROB_BOUND, f"{what}: logprob {lp[b, 0]!r}, float64 {want!r}"
    if c.vocab == 1:
        assert float(lp[b, 0]) == 0.0, f"{what}: the only token's logprob is {lp[b, 0]!r}, not 0.0"


def _batches(key) -> list:
    cs = GROUPS[key]
    if key[0] > 8200:
        return [(cs, False)]  # 2^20 at B = 1, 128256 at B = 3: single calls
    return [(cs[i:i + 12], True) for i in range(0, len(cs), 12)]


@pytest.mark.parametrize("key", list(GROUPS), ids=lambda k: f"vocab{k[0]}_bound{k[1]}")
def test_designed_cases_in_four_forms(dev, key):
    vocab, bound = key
    for cs, with_inactive in _batches(key):
        layout = _layout(cs, with_inactive)
        st = {form: _step(dev, layout, vocab, bound, form) for form in FORMS}
        bad = [b for b, (c, a) in enumerate(layout) if a and c.kind == "undefined"]  # +inf / NaN in a sampled row: only the three properties, in every form
        for form in FORMS[1:]:
            for k in ("debug", "token", "rows", "log", "pos"):
                mine, theirs = np.delete(st["plain"][k], bad, axis=0), np.delete(st[form][k], bad, axis=0)
                assert np.array_equal(mine, theirs), f"vocab {vocab}: the `{form}` form's `{k}` differs from the plain form's (kept rows {np.nonzero((mine != theirs).reshape(mine.shape[0], -1).any(axis=1))[0].tolist()})"
            for b in bad:
                _check_tail(layout[b][0], b, st[form], f"{layout[b][0].name} (row {b}, form {form})")
        p = st["plain"]
        for b, (c, active) in enumerate(layout):
            if not active:
                assert np.array_equal(p["rows"][b], p["before"][b]) and p["token"][b] == -7 and (p["log"][b] == -1).all() and (p["debug"][b] == 0).all() and p["pos"][b] == p["pos0"][b], \
                    f"vocab {vocab}: the inactive row {b} was touched"
                continue
            _check_row(c, b, p, st["logprobs"]["logprob"])
        if bad:  # the neighbours of a +inf / NaN row: the same bits as in a call in which that row is inactive
            calm = [(c, a and b not in bad) for b, (c, a) in enumerate(layout)]
            q = _step(dev, calm, vocab, bound, "plain")
            for b, (c, a) in enumerate(layout):
                if b not in bad:
                    for k in ("debug", "token", "rows", "log", "pos"):
                        assert np.array_equal(p[k][b], q[k][b]), f"vocab {vocab} row {b} ({c.name}): `{k}` depends on the +inf / NaN rows beside it"
    for fam, (wp, tp, wf, tf) in sorted(WORST.items()):
        print(f"worst so far, {fam}: p {wp:.2e} (tolerance {tp:.2e}), final p {wf:.2e} (tolerance {tf:.2e})")


# ---- the verifier: T = 4, row 0 a designed case, rows 1 .. 3 the same logits behind a window that has taken the drafts ----
def _decisive_u(c, window, t):
    """A uniform for a virtual row behind row 0: the midpoint of a CDF interval of the reference's final distribution that is wider than four tolerances."""
    r = S.reference(c.logits, window, c.prm, 0.0, c.bound)
    if c.prm.temp <= 0:
        return 0.0
    assert c.kind == "exact" or r["d_top_p"] > 4 * S.tol_p(c), f"{c.name}: behind the drafts top_p lies {r['d_top_p']:.2e} from a cumulative sum"
    cdf = np.concatenate([[0.0], np.cumsum(r["final_p"])])
    width = np.diff(cdf)
    wide = np.nonzero(width > 4 * S.tol_final(c, r))[0]
    assert wide.size, f"{c.name}: no interval wide enough"
    i = int(wide[t % wide.size])
    return float(F32((cdf[i] + cdf[i + 1]) / 2))


def _host_chain(c, drafts_follow_until, T):
    """The tokens a sequence emits, the uniforms of its rows and the drafts it is fed: drafts equal the chain's tokens up to row `drafts_follow_until`, the next one
    misses.  Rows behind the miss get the uniform of the window the DEVICE samples them with (the drafts pushed)."""
    ring, pushed = c.ring.copy(), int(c.pushed)
    us, tokens, drafts = [], [], []
    alive = True
    for t in range(T):
        w = S.window_of(ring, pushed, c.prm.repeat_last_n)
        u = float(F32(c.u)) if t == 0 else _decisive_u(c, w, t)
        y = S.reference(c.logits, w, c.prm, u, c.bound)["token"]
        us.append(u)
        if alive:
            tokens.append(y)
        if t + 1 < T:
            follow = t < drafts_follow_until
            dft = y if follow else (y + 1) % c.vocab
            drafts.append(dft)
            alive = alive and follow
            ring[pushed % 64] = dft  # what virtual row t + 1 sees behind the ring: the draft
            pushed += 1
    return tokens, us, drafts


def _verify(dev, seqs, vocab, bound, form, T=4):
    from tinychatengine_amd.speculative import Verifier
    B = len(seqs)
    s = _sampler(dev, B, vocab, bound, form)
    ver = Verifier(s, T, debug=True)
    hist_stride = 80
    rng = np.random.default_rng(4)
    history = rng.integers(0, vocab, (B, hist_stride)).astype(np.int32)
    logits = np.stack([S.padded(c) for c, _, _ in seqs for _ in range(T)])
    row_token, row_pos = np.zeros((B, T), np.int32), np.full((B, T), -1, np.int32)
    uniforms = np.zeros((B, T), F32)
    pos0 = np.zeros(B, np.int32)
    for b, (c, active, chain) in enumerate(seqs):
        p = 3 + 2 * b
        pos0[b] = p if active else -1
        row_token[b, 0] = history[b, p]
        row_token[b, 1:] = chain[2]
        uniforms[b] = chain[1]
        if active:
            row_pos[b] = p + np.arange(T)
    s.rows.copy_(torch.from_numpy(np.stack([_words(_row(c, 500 + b)) for b, (c, _, _) in enumerate(seqs)])))
    ver.uniform_override = torch.from_numpy(uniforms.reshape(-1)).to(dev)
    before = s.rows.cpu().numpy().copy()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lg, rt, rp, hs, ps = d(logits), d(row_token.reshape(-1)), d(row_pos.reshape(-1)), d(history), d(pos0)
    s.next_token.fill_(-7)
    ver.step(lg, rt, rp, hs, ps, POS_BOUND)
    torch.cuda.synchronize()
    out = {"debug": ver.debug.cpu().numpy(), "token": s.next_token.cpu().numpy(), "rows": s.rows.cpu().numpy(), "log": s.out_log.cpu().numpy(), "pos": ps.cpu().numpy(),
           "emitted": ver.emitted.cpu().numpy(), "history": hs.cpu().numpy(), "before": before, "pos0": pos0, "history0": history}
    if form == "logprobs":
        out["logprob"] = s.out_logprob.cpu().numpy()
    if form in ("unconstrained", "allow_all"):
        assert s.violations() == 0
    return out


def test_verifier_chains_of_designed_cases(dev):
    """Sequences of vocab 8197: every third follows all drafts, the others miss at row 1 or 2; one inactive sequence.  Tokens, emitted, log, ring, counters, history
    and positions against a host chain of the new reference; the four forms bit-identical; the emitted tokens' logprobs within the bound."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.generate import logprob_reference
    vocab, bound, T = 8197, 40, 4
    cs = [c for c in GROUPS[(vocab, bound)] if S.defined(c)][:15]
    seqs = [(c, True, _host_chain(c, [3, 1, 2][i % 3], T)) for i, c in enumerate(cs)]
    seqs.insert(2, (cs[0], False, _host_chain(cs[0], 3, T)))
    assert len(seqs) <= 16 and any(c.family == "penalties" for c, _, _ in seqs) and any(c.kind == "exact" for c, _, _ in seqs)
    st = {form: _verify(dev, seqs, vocab, bound, form, T) for form in FORMS}
    for form in FORMS[1:]:
        for k in ("debug", "token", "rows", "log", "pos", "emitted", "history"):
            assert np.array_equal(st["plain"][k], st[form][k]), f"verifier: the `{form}` form's `{k}` differs from the plain form's"
    p, lp = st["plain"], st["logprobs"]["logprob"]
    dbg = _debug(p["debug"])
    for b, (c, active, (tokens, us, drafts)) in enumerate(seqs):
        what = f"verifier sequence {b} ({c.name})"
        after, before = capi.SampleRow.from_buffer_copy(p["rows"][b].tobytes()), capi.SampleRow.from_buffer_copy(p["before"][b].tobytes())
        if not active:
            assert p["emitted"][b] == 0 and p["pos"][b] == -1 and np.array_equal(p["rows"][b], p["before"][b]) and p["token"][b] == -7 and (p["log"][b] == -1).all() \
                and np.array_equal(p["history"][b], p["history0"][b]), f"{what}: an inactive sequence was touched"
            continue
        e = len(tokens)
        print(f"{what}: emitted {p['emitted'][b]} / {e}, tokens {p['log'][b, :4].tolist()} / {tokens}")
        ref0 = S.ref_of(c)  # row 0 is the designed case itself
        y0 = b * T
        assert dbg["ids"][y0][:dbg["k"][y0]].tolist() == ref0["ids"].tolist() and int(dbg["n"][y0]) == ref0["n"] and int(dbg["choice"][y0]) == ref0["choice"], f"{what}: row 0"
        assert p["emitted"][b] == e, f"{what}: emitted {p['emitted'][b]}, the host chain {e}"
        assert p["log"][b, :e].tolist() == tokens and (p["log"][b, e:] == -1).all(), f"{what}: tokens {p['log'][b, :e].tolist()}, the host chain {tokens}"
        want_ring = list(before.ring)
        for i, y in enumerate(tokens):
            want_ring[(before.ring_pushed + i) % 64] = y
        assert list(after.ring) == want_ring and after.ring_pushed == before.ring_pushed + e and after.generated == e, f"{what}: ring / counters"
        assert p["token"][b] == tokens[-1] and p["pos"][b] == p["pos0"][b] + e, f"{what}: next token / position"
        want_hist = p["history0"][b].copy()
        want_hist[p["pos0"][b] + 1:p["pos0"][b] + 1 + e] = tokens
        assert np.array_equal(p["history"][b], want_hist), f"{what}: history"
        for i, y in enumerate(tokens):
            want = logprob_reference(c.logits, y)
            assert abs(float(lp[b, i]) - want) <= LOGPROB_BOUND, f"{what} token {i}: logprob {lp[b, i]!r}, float64 {want!r}"
    assert sorted({int(v) for v in p["emitted"]}) == [0, 2, 3, 4]
