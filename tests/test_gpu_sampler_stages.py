"""tce_sample_stages_f16 on the device (csrc/sampling.hip: the STG = true forms of sample_draw_kernel; generate.Sampler(stages=True)): tail-free and typical
sampling per slot between top-k and top-p.

The identity rule is held in bytes against the existing entry points; every designed case (tests/stage_cases.py) against its own float64 reference; the five fixture
configurations against the reference's own results (tests/golden/sampler_stages_golden.npz) under the rules of tests/stage_rules.py; a row against itself among
fifteen others; and a slot that changes hands between two replays of one captured graph."""
import dataclasses
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402
import stage_cases as SC  # noqa: E402
import stage_rules as SR  # noqa: E402

VOCAB = 8200  # three chunks, the last partial
POS_BOUND = 63


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _words(struct) -> np.ndarray:
    return np.frombuffer(bytes(struct), dtype=np.int32).copy()


def _row(params, seed=0, max_new=8, ring=None, pushed=0, generated=0):
    from tinychatengine_amd.generate import make_row
    r = make_row(params, seed, max_new)
    if ring is not None:
        for i, t in enumerate(ring):
            r.ring[i] = int(t)
    r.ring_pushed, r.generated = pushed, generated
    return r


def _set(sampler, rows, pairs=None, crows=None):
    sampler.rows.copy_(torch.from_numpy(np.stack([_words(r) for r in rows])))
    if pairs is not None:
        sampler.srows.copy_(torch.tensor(pairs, dtype=torch.float32))
    if crows is not None:
        sampler.crows.copy_(torch.from_numpy(np.stack([_words(c) for c in crows])))


def _debug(sampler) -> dict:
    d = sampler.debug.cpu().numpy()
    out = {"n": d[:, 0], "k": d[:, 1], "u": d[:, 2].copy().view(np.float32), "choice": d[:, 3], "ids": d[:, 4:260], "logit": d[:, 260:516].copy().view(np.float32),
           "p": d[:, 516:772].copy().view(np.float32), "final_p": d[:, 772:1028].copy().view(np.float32)}
    if sampler.sdebug is not None:
        s = sampler.sdebug.cpu().numpy()
        out.update({"n_tfs": s[:, 0], "n_typ": s[:, 1], "order": s[:, 2:258], "p_top": s[:, 258:514].copy().view(np.float32)})
    return out


def _result(d: dict, j: int, tok: int) -> dict:
    """Row j of the two debug records with generate._chain's keys."""
    kk, n, n2 = int(d["k"][j]), int(d["n"][j]), int(d["n_typ"][j])
    order = d["order"][j][:n2].astype(np.int64)
    assert (d["order"][j][n2:] == -1).all() and ((order >= 0) & (order < kk)).all() and len(set(order.tolist())) == n2, "order is not a partial permutation of the candidates"
    ids = d["ids"][j][:kk]
    return {"ids": ids, "logits": d["logit"][j][:kk], "p": d["p"][j][:kk], "n_tfs": int(d["n_tfs"][j]), "n_typ": n2, "order": order, "final_ids": ids[order],
            "p_top": d["p_top"][j][:n2], "n": n, "final_p": d["final_p"][j][:n], "choice": int(d["choice"][j]), "token": int(tok)}


def _mixed_logits(rng, rows, vocab=VOCAB):
    ld = (vocab + 7) // 8 * 8 + 8
    x = (rng.standard_normal((rows, ld), dtype=np.float32) * np.float32(2.5)).astype(np.float16)
    x[:, vocab:] = 60000.0  # columns past the vocabulary hold the largest values: they must never be candidates
    return x


@pytest.mark.parametrize("form", ["plain", "logprobs", "constrained", "constrained_logprobs"])
def test_identity_rule_in_bytes(dev, form):
    """B = 5: one inactive row, one greedy row, three sampled rows, every slot at (1.0, 1.0): token, log, rows, position and debug record (log-probability and LSE;
    constraint rows and the violations word) equal the underlying entry point's, byte for byte."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    from tinychatengine_amd.generate import Sampler, SamplingParams, ring_window, sample_reference
    B = 5
    rng = np.random.default_rng(17)
    logits = torch.from_numpy(_mixed_logits(rng, B)).to(dev)
    ring = rng.integers(0, VOCAB, 64).astype(np.int32)
    ps = [SamplingParams(), SamplingParams(temp=0.0), SamplingParams(temp=0.7, top_k=40, top_p=0.9, repeat_penalty=1.2, alpha_frequency=0.1),
          SamplingParams(temp=1.3, top_k=17, top_p=1.0, repeat_penalty=1.0), SamplingParams(temp=0.8, top_k=3, top_p=0.5, alpha_presence=0.2)]
    rows = [_row(p, seed=b + 1, ring=ring, pushed=70 + b, generated=b) for b, p in enumerate(ps)]
    lp, con = "logprobs" in form, "constrained" in form
    out = []
    for stages in (False, True):
        s = Sampler(B, VOCAB, 16, dev, top_k_bound=40, debug=True, logprobs=lp, constraints=con, stages=stages)
        crows = None
        if con:
            a = s.table.register(TokenAutomaton.any_of(VOCAB, range(0, VOCAB, 3)))
            crows = [constraint_row(), constraint_row(a, 0), constraint_row(a, 0), constraint_row(-1, 0, [(5, 2.0), (4096, -1.0)]), constraint_row(a, 0, [(9, 30.0)])]
        _set(s, rows, [(1.0, 1.0)] * B if stages else None, crows)
        pos = torch.tensor([-1, 0, 63, 9, 17], dtype=torch.int32, device=dev)
        s.step(logits, pos, POS_BOUND)
        torch.cuda.synchronize()
        got = {"token": s.next_token, "log": s.out_log, "rows": s.rows, "pos": pos, "debug": s.debug}
        if lp:
            got.update({"logprob": s.out_logprob, "lse": s.last_lse})
        if con:
            got.update({"crows": s.crows, "violations": s.violations_word})
        out.append({k: v.cpu().numpy().tobytes() for k, v in got.items()})
        if stages:
            d = _debug(s)
            assert d["n_tfs"][1:].tolist() == d["k"][1:].tolist() == d["n_typ"][1:].tolist() and (d["order"][2, :40] == np.arange(40)).all()
            # the greedy row's record is generate._chain's: one candidate, n_tfs = n_typ = 1, the identity order, no p_top
            ref = sample_reference(logits[1, :VOCAB].cpu().numpy(), ring_window(ring, 71, ps[1].repeat_last_n), ps[1], 0.0)
            assert (int(d["n_tfs"][1]), int(d["n_typ"][1])) == (ref["n_tfs"], ref["n_typ"]) == (1, 1) and d["order"][1, 0] == ref["order"][0] == 0
            assert (d["order"][1, 1:] == -1).all() and (d["p_top"][1] == 0).all()
            if not con:  # (constrained, row 1 runs under the automaton: another token)
                assert int(d["ids"][1, 0]) == ref["token"]
    assert np.frombuffer(out[0]["pos"], np.int32).tolist() == [-1, 1, 64, 10, 18]  # the inactive row stays, every other row advances once
    for key in out[0]:
        assert out[0][key] == out[1][key], f"{form}: {key} differs from the underlying entry point's"


def _check_case(c, ref, res, what):
    kk = ref["ids"].size
    assert res["ids"].tolist() == ref["ids"].tolist(), f"{what}: candidate ids"
    assert np.array_equal(np.asarray(res["logits"], np.float32).view(np.uint32), ref["logits"].view(np.uint32)), f"{what}: candidate logits"
    for key in ("n_tfs", "n_typ", "n", "choice", "token"):
        assert int(res[key]) == int(ref[key]), f"{what}: {key} = {res[key]}, the reference gives {ref[key]}"
    assert res["order"].tolist() == ref["order"].tolist() and res["final_ids"].tolist() == ref["final_ids"].tolist(), f"{what}: order {res['order'].tolist()}"
    worst = 0.0
    for key in ("p", "p_top", "final_p"):
        a, b = np.asarray(res[key], np.float64), np.asarray(ref[key], np.float64)
        assert a.shape == b.shape, f"{what}: {key} has {a.size} entries, the reference {b.size}"
        if c.kind == "exact":
            assert np.array_equal(np.asarray(res[key], np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)), f"{what}: {key} bits"
        else:
            nz = b > 0
            err = float((np.abs(a[nz] - b[nz]) / b[nz]).max()) if nz.any() else 0.0
            worst = max(worst, err)
            assert err <= R.tol(kk) and np.all(a[~nz] == 0), f"{what}: {key} relative error {err:.3e} > {R.tol(kk):.3e}"
    return worst


def _run_cases(dev, cases, vocab, bound, constrained=False):
    """The cases of one (vocab, top_k_bound) in launches of at most 16 rows: every row its own (tfs_z, typical_p), parameters, ring and u."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    from tinychatengine_amd.generate import Sampler, SamplingParams
    ld = (vocab + 7) // 8 * 8
    for c0 in range(0, len(cases), 16):
        chunk = cases[c0:c0 + 16]
        B = len(chunk)
        s = Sampler(B, vocab, 8, dev, top_k_bound=bound, debug=True, stages=True, constraints=constrained)
        logits = np.full((B, ld), 60000.0, np.float16)
        rows, pairs, crows = [], [], []
        for j, c in enumerate(chunk):
            logits[j, :vocab] = c.logits
            rows.append(_row(SamplingParams(**dataclasses.asdict(c.prm)), max_new=8, ring=c.ring, pushed=c.pushed))
            pairs.append((c.prm.tfs_z, c.prm.typical_p))
            if constrained:
                crows.append(constraint_row(s.table.register(TokenAutomaton.any_of(vocab, c.allowed)), 0) if c.allowed is not None else constraint_row())
        _set(s, rows, pairs, crows if constrained else None)
        s.uniform_override = torch.tensor([c.u for c in chunk], dtype=torch.float32, device=dev)
        pos = torch.full((B,), 5, dtype=torch.int32, device=dev)
        s.step(torch.from_numpy(logits).to(dev), pos, POS_BOUND)
        torch.cuda.synchronize()
        d, tok = _debug(s), s.next_token.cpu().numpy()
        assert pos.cpu().numpy().tolist() == [6] * B and s.generated().tolist() == [1] * B and s.violations() == 0
        for j, c in enumerate(chunk):
            worst = _check_case(c, SC.ref_of(c), _result(d, j, tok[j]), c.name)
            print(f"{c.name}: n_tfs {d['n_tfs'][j]} n_typ {d['n_typ'][j]} n {d['n'][j]} token {tok[j]} worst relative error {worst:.2e}")


def test_designed_cases_share_launches_with_their_own_values_per_row(dev):
    small = [c for c in SC.cases() if c.vocab == VOCAB and c.allowed is None]
    assert len({(c.prm.tfs_z, c.prm.typical_p) for c in small[:16]}) >= 8  # one launch carries many different pairs
    _run_cases(dev, small, VOCAB, 64)


def test_designed_cases_under_a_mask(dev):
    """Fewer allowed tokens than k: the constrained form of the stages kernel, the masked case beside unmasked ones."""
    cs = [c for c in SC.cases() if c.allowed is not None] + [SC.by_name(n) for n in ("typical_non_maximal_first", "top_p_cuts_again", "equal8_both")]
    assert cs[0].allowed is not None
    _run_cases(dev, cs, VOCAB, 64, constrained=True)


def test_designed_case_with_ids_near_2_20(dev):
    cs = [c for c in SC.cases() if c.vocab == 1 << 20]
    assert cs
    _run_cases(dev, cs, 1 << 20, cs[0].bound)


@pytest.fixture(scope="module")
def fixture():
    return SR.load_fixture()


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_device_stages_against_the_references_own_code(dev, fixture, name):
    """The first 40 rows of the configuration through tce_sample_stages_f16 at B = 16 (vocab 128256) under the rules of stage_rules.py, then every draw point of every
    decided row."""
    from tinychatengine_amd.generate import Sampler
    k, sigma, z, typ, nrows, seed = SR.CONFIGS[name]
    rows = min(nrows, 40)
    params = SR.params_of(name)
    inputs = SR.config_inputs(name, fixture)[:rows]
    B, V = 16, SR.VOCAB
    logits_all = torch.from_numpy(np.stack([lg for lg, _ in inputs])).to(dev)
    s = Sampler(B, V, 4, dev, top_k_bound=k, debug=True, stages=True)
    s.uniform_override = torch.full((B,), 0.5, dtype=torch.float32, device=dev)
    pristine = [_row(params, seed=r, max_new=4, ring=inputs[r][1]) for r in range(rows)]
    draws, decided, worst = [], 0, 0.0
    for r0 in range(0, rows, B):
        idx = list(range(r0, min(r0 + B, rows)))
        pad = idx + [idx[-1]] * (B - len(idx))
        _set(s, [pristine[r] for r in pad], [(z, typ)] * B)
        pos = torch.tensor([5] * len(idx) + [-1] * (B - len(idx)), dtype=torch.int32, device=dev)
        s.step(logits_all[pad].contiguous(), pos, POS_BOUND)
        torch.cuda.synchronize()
        d, tok = _debug(s), s.next_token.cpu().numpy()
        assert pos.cpu().numpy()[:len(idx)].tolist() == [6] * len(idx) and s.generated()[:len(idx)].tolist() == [1] * len(idx)  # every row advances once
        for j, r in enumerate(idx):
            logits, recent = inputs[r]
            x = R.penalised(logits, recent, SR.REPEAT_PENALTY, 0.0, 0.0)
            res = SR.check_row(f"{name} row {r}", name, r, fixture, x, _result(d, j, tok[j]))
            decided += res["decided"]
            worst = max(worst, res["worst"])
            draws += [(r, u, ok) for u, ok in res["draws"]]
    print(f"{name}: {decided} of {rows} rows decided, worst relative error {worst:.2e} (tolerance {R.tol(k):.2e}); {len(draws)} draw points")
    for c0 in range(0, len(draws), B):
        chunk = draws[c0:c0 + B]
        pad = chunk + [chunk[-1]] * (B - len(chunk))
        rws = [r for r, _, _ in pad]
        _set(s, [pristine[r] for r in rws], [(z, typ)] * B)
        s.uniform_override.copy_(torch.tensor([float(u) for _, u, _ in pad], dtype=torch.float32))
        s.step(logits_all[rws].contiguous(), torch.full((B,), 5, dtype=torch.int32, device=dev), POS_BOUND)
        choice = s.debug[:, 3].cpu().numpy()
        for j, (r, u, ok) in enumerate(chunk):
            assert int(choice[j]) in ok, f"{name} row {r}: u = {u!r} drew position {choice[j]}, accepted {sorted(ok)}"


def test_a_row_alone_equals_the_same_row_among_fifteen_others(dev):
    from tinychatengine_amd.generate import Sampler, SamplingParams
    rng = np.random.default_rng(23)
    logits = _mixed_logits(rng, 16)
    ring = rng.integers(0, VOCAB, 64).astype(np.int32)
    pairs = [(float(rng.uniform(0.3, 1.0)), float(rng.uniform(0.2, 1.0))) for _ in range(16)]
    rows = [_row(SamplingParams(temp=0.9, top_k=int(rng.integers(3, 41)), top_p=0.9, repeat_penalty=1.1), seed=100 + b, ring=ring, pushed=64 + b, generated=b) for b in range(16)]
    big = Sampler(16, VOCAB, 32, dev, top_k_bound=40, debug=True, stages=True)
    _set(big, rows, pairs)
    big.step(torch.from_numpy(logits).to(dev), torch.full((16,), 7, dtype=torch.int32, device=dev), POS_BOUND)
    for b in (0, 6, 15):
        one = Sampler(1, VOCAB, 32, dev, top_k_bound=40, debug=True, stages=True)
        _set(one, [rows[b]], [pairs[b]])
        one.step(torch.from_numpy(logits[b:b + 1].copy()).to(dev), torch.full((1,), 7, dtype=torch.int32, device=dev), POS_BOUND)
        torch.cuda.synchronize()
        for name in ("next_token", "rows", "debug", "sdebug", "out_log"):
            assert torch.equal(getattr(one, name)[0], getattr(big, name)[b]), f"row {b}: {name} depends on the neighbours"
        assert int(one.sdebug[0, 1]) >= 1


def test_a_slot_changes_hands_between_two_replays_of_one_graph(dev):
    """One captured graph of Sampler.step; between two replays slot 1 goes from (0.5, 0.2) to (1.0, 1.0) by set_row's stream-ordered copies, nothing is captured
    again, and each replay equals the same call made eagerly on a fresh sampler."""
    from tinychatengine_amd.generate import Sampler, SamplingParams
    rng = np.random.default_rng(31)
    logits = torch.from_numpy(_mixed_logits(rng, 3)).to(dev)
    prompt = rng.integers(0, VOCAB, 9).tolist()
    tight, off = SamplingParams(temp=0.9, top_k=40, top_p=0.95, tfs_z=0.5, typical_p=0.2), SamplingParams(temp=0.9, top_k=40, top_p=0.95)
    other = SamplingParams(temp=0.8, top_k=20, tfs_z=0.9, typical_p=0.7)

    def admit(s, mine):
        for b, p in enumerate((other, mine, off)):
            s.set_row(b, p, seed=50 + b, max_new=8, prompt_ids=prompt)

    def state(s, pos):
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (s.next_token, s.out_log, s.rows, s.srows, s.debug, s.sdebug, pos)]

    eager = []
    for mine in (tight, off):
        s = Sampler(3, VOCAB, 8, dev, top_k_bound=40, debug=True, stages=True)
        admit(s, mine)
        pos = torch.full((3,), 4, dtype=torch.int32, device=dev)
        s.step(logits, pos, POS_BOUND)
        eager.append(state(s, pos))
    g = Sampler(3, VOCAB, 8, dev, top_k_bound=40, debug=True, stages=True)
    pos = torch.full((3,), -1, dtype=torch.int32, device=dev)
    g.step(logits, pos, POS_BOUND)  # warm-up: every row inactive
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(logits, pos, POS_BOUND)
    for i, mine in enumerate((tight, off)):
        admit(g, mine)
        g.out_log.fill_(-1)
        pos.fill_(4)
        graph.replay()
        assert state(g, pos) == eager[i], f"replay {i}: differs from the eager call"
    d = _debug(g)
    assert d["n_typ"][1] == d["k"][1] == 40  # the slot now runs no stage
    assert eager[0][0] != eager[1][0] or eager[0][5] != eager[1][5]  # (the two settings do differ in what the slot's record shows)


def test_sampler_without_stages_refuses_non_default_params(dev):
    from tinychatengine_amd.generate import Sampler, SamplingParams
    s = Sampler(2, VOCAB, 8, dev, top_k_bound=40)
    before = s.rows.clone()
    with pytest.raises(ValueError, match="not built"):
        s.set_row(0, SamplingParams(tfs_z=0.5), seed=1, max_new=4)
    with pytest.raises(ValueError, match="not built"):
        s.set_row(0, SamplingParams(typical_p=0.5), seed=1, max_new=4)
    assert torch.equal(s.rows, before) and s.srows is None
