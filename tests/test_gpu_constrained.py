"""tce_sample_constrained_f16 on the device (csrc/sampling.hip CON = true forms; tinychatengine_amd/constrain.py, generate.Sampler(constraints=True)).

Batch 4; vocabularies 100 (ld 104) and 4096 + 40 (two chunks, the second partial), the columns behind the vocabulary holding the row's largest values.  Rule 7 is held
bit for bit against tce_sample_f16 / tce_sample_logprobs_f16; masks and bias against constrain.constrained_reference on fp16 logits quantised to quarter steps (ties
everywhere) under the rules of tests/sampling_rules.py -- candidate ids and n equal, sorted logits bit-equal, probabilities within tol(k), the token equal on the same
u --; state, retirement and rule 6 exactly.
("The only allowed token is vocab - 1" and "an id of the partial last chunk in the UPPER half of its mask word" are two cases: 99 & 31 = 3 and 4135 & 31 = 7 lie
in lower halves, so the upper half is covered by 83 and 4117.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402

B = 4
VOCABS = [100, 4096 + 40]
POS_BOUND = 63


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _logits(rng, vocab, rows=B):
    """fp16 in quarter steps (many ties), [rows][ld] with ld = 104 for vocab 100 and 4136 for 4136; columns past the vocabulary hold 60000."""
    ld = (vocab + 7) // 8 * 8
    x = (np.round(rng.standard_normal((rows, ld)) * 2.5 * 4) / 4).astype(np.float16)
    x[:, vocab:] = 60000.0
    return x


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


def _set(sampler, rows, crows=None):
    sampler.rows.copy_(torch.from_numpy(np.stack([_words(r) for r in rows])))
    if crows is not None:
        sampler.crows.copy_(torch.from_numpy(np.stack([_words(c) for c in crows])))


def _debug(sampler) -> dict:
    d = sampler.debug.cpu().numpy()
    return {"n": d[:, 0], "k": d[:, 1], "choice": d[:, 3], "ids": d[:, 4:260], "logit": d[:, 260:516].copy().view(np.float32), "p": d[:, 516:772].copy().view(np.float32),
            "final_p": d[:, 772:1028].copy().view(np.float32)}


def _sampler(dev, vocab, **kw):
    from tinychatengine_amd.generate import Sampler
    return Sampler(B, vocab, 16, dev, **{"top_k_bound": 40, "debug": True, "constraints": True, **kw})


def _params(sampled, **kw):
    from tinychatengine_amd.generate import SamplingParams
    return SamplingParams(**{"temp": 0.8 if sampled else 0.0, "top_k": 40, "top_p": 0.9, "repeat_penalty": 1.0, "repeat_last_n": 64, **kw})


def _check_p(what, got, ref, k):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaNs differ"
    ok = ~np.isnan(ref) & (ref != 0)
    assert np.array_equal(got[~np.isnan(ref) & (ref == 0)], ref[~np.isnan(ref) & (ref == 0)]), f"{what}: zeros differ"
    if ok.any():
        R.check_p(what, got[ok], ref[ok], k)


def _check_against_reference(what, ref, d, j, tok):
    kk, n = int(d["k"][j]), int(d["n"][j])
    print(f"{what}: k {kk} n {n} token {tok} | reference k {ref['ids'].size} n {ref['n']} token {ref['token']}")
    assert kk == ref["ids"].size and d["ids"][j][:kk].tolist() == ref["ids"].tolist(), f"{what}: candidate ids {d['ids'][j][:kk].tolist()}, the reference's {ref['ids'].tolist()}"
    assert np.array_equal(d["logit"][j][:kk].view(np.uint32), ref["logits"].view(np.uint32)), f"{what}: candidate logits"
    if ref["p"].size == kk and kk > 0 and ref["final_p"].size == ref["n"] and not (ref["p"] == 0).all():
        _check_p(what + " p", d["p"][j][:kk], ref["p"], max(kk, 1))
        assert n == ref["n"], f"{what}: n = {n}, the reference keeps {ref['n']}"
        _check_p(what + " final p", d["final_p"][j][:n], ref["final_p"], max(kk, 1))
    assert int(tok) == ref["token"], f"{what}: token {tok}, the reference draws {ref['token']}"


def _run_cases(dev, vocab, cases, u=0.37):
    """cases: dicts with logits (fp16 [ld]), params, and optionally allowed (ids; None: unconstrained), packed (a hand-packed automaton instead of any_of(allowed)),
    bias (pairs for the reference), raw_bias (pairs written into the device row as they are), ring / pushed.  Four per launch; every case against constrained_reference."""
    from tinychatengine_amd.constrain import TokenAutomaton, constrained_reference, constraint_row
    from tinychatengine_amd.generate import ring_window
    for c0 in range(0, len(cases), B):
        chunk = cases[c0:c0 + B]
        chunk = chunk + [chunk[0]] * (B - len(chunk))
        s = _sampler(dev, vocab)
        s.uniform_override = torch.full((B,), u, dtype=torch.float32, device=dev)
        rows, crows = [], []
        for c in chunk:
            ring, pushed = c.get("ring", np.zeros(64, np.int32)), c.get("pushed", 0)
            rows.append(_row(c["params"], max_new=8, ring=ring, pushed=pushed))
            fsm = -1
            if c.get("packed") is not None:
                fsm = s.table.register_packed(c["packed"])
            elif c.get("allowed") is not None:
                fsm = s.table.register(TokenAutomaton.any_of(vocab, c["allowed"]))
            crows.append(constraint_row(fsm, 0, c.get("raw_bias", c.get("bias", []))))
        _set(s, rows, crows)
        pos = torch.full((B,), 5, dtype=torch.int32, device=dev)
        s.step(torch.from_numpy(np.stack([c["logits"] for c in chunk])).to(dev), pos, POS_BOUND)
        torch.cuda.synchronize()
        d, tok = _debug(s), s.next_token.cpu().numpy()
        assert s.violations() == 0 and pos.cpu().numpy().tolist() == [6] * B
        for j, c in enumerate(chunk):
            ring, pushed = c.get("ring", np.zeros(64, np.int32)), c.get("pushed", 0)
            ref = constrained_reference(c["logits"][:vocab], ring_window(ring, pushed, c["params"].repeat_last_n), c["params"], u, c.get("allowed"), c.get("bias"))
            _check_against_reference(f"vocab {vocab} {c['name']}", ref, d, j, tok[j])
            after = s.row(j)
            assert after.generated == 1 and after.ring[pushed % 64] == tok[j] and s.constraint_row(j).state == 0


@pytest.mark.parametrize("logprobs", [False, True])
@pytest.mark.parametrize("vocab", VOCABS)
def test_rule_7_bit_for_bit_against_the_unconstrained_entry_points(dev, vocab, logprobs):
    """Rows 0, 1: fsm = -1; rows 2, 3: a one-state automaton that allows everything.  Token, log, ring, counters, position, debug record (and log-probability, LSE)
    equal tce_sample_f16's / tce_sample_logprobs_f16's bytes; the automaton rows stay in state 0."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    from tinychatengine_amd.generate import Sampler
    rng = np.random.default_rng(vocab + logprobs)
    logits = torch.from_numpy(_logits(rng, vocab)).to(dev)
    ring = rng.integers(0, vocab, 64).astype(np.int32)
    ps = [_params(False, repeat_penalty=1.1), _params(True, repeat_penalty=1.2, alpha_frequency=0.1), _params(True), _params(False, repeat_penalty=1.3, alpha_presence=0.2)]
    rows = [_row(p, seed=b + 1, ring=ring, pushed=70 + b, generated=b) for b, p in enumerate(ps)]
    out = []
    for constrained in (False, True):
        s = Sampler(B, vocab, 16, dev, top_k_bound=40, debug=True, logprobs=logprobs, constraints=constrained)
        crows = None
        if constrained:
            a = s.table.register(TokenAutomaton.any_of(vocab, range(vocab)))
            crows = [constraint_row(), constraint_row(), constraint_row(a, 0), constraint_row(a, 0)]
        _set(s, rows, crows)
        pos = torch.tensor([3, 0, 63, 9], dtype=torch.int32, device=dev)
        s.step(logits, pos, POS_BOUND)
        torch.cuda.synchronize()
        got = [s.next_token.cpu().numpy().tobytes(), s.out_log.cpu().numpy().tobytes(), s.rows.cpu().numpy().tobytes(), pos.cpu().numpy().tobytes(), s.debug.cpu().numpy().tobytes()]
        if logprobs:
            got += [s.out_logprob.cpu().numpy().tobytes(), s.last_lse.cpu().numpy().tobytes()]
        if constrained:
            assert s.violations() == 0 and [s.constraint_row(b).state for b in range(B)] == [0] * B
        out.append(got)
    for name, x, y in zip(["token", "log", "rows", "pos", "debug", "logprob", "lse"], out[0], out[1]):
        assert x == y, f"{name} differs from the unconstrained entry point's"


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("vocab", VOCABS)
def test_masks_against_constrained_reference(dev, vocab, sampled):
    from tinychatengine_amd.constrain import TokenAutomaton
    rng = np.random.default_rng(7 * vocab + sampled)
    lg = _logits(rng, vocab, 8)
    p = _params(sampled)
    upper = 83 if vocab == 100 else 4117
    three = [3, 40, 97] if vocab == 100 else [17, 4095, 4100]
    everything = TokenAutomaton.any_of(vocab, range(vocab)).pack()
    everything["mask"][:] = 0xFFFFFFFF  # bits at and beyond the vocabulary: ignored
    ninf = lg[4].copy()
    ninf_ids = [5, 50, 99] if vocab == 100 else [5, 4090, 4130]
    ninf[ninf_ids] = -np.inf
    ring = rng.permutation(vocab)[:64].astype(np.int32)
    cases = [dict(name="one allowed token", logits=lg[0], params=p, allowed=[three[1]]),
             dict(name="3 allowed tokens, k 40", logits=lg[1], params=p, allowed=three),
             dict(name="only vocab - 1", logits=lg[2], params=p, allowed=[vocab - 1]),
             dict(name="only an id in the upper half of a word of the last chunk", logits=lg[3], params=p, allowed=[upper]),
             dict(name="mask bits at and beyond the vocabulary", logits=lg[5], params=p, allowed=None, packed=everything),
             dict(name="all allowed tokens at -inf", logits=ninf, params=p, allowed=ninf_ids),
             dict(name="the allowed set is the 64 penalised ids", logits=lg[6], params=_params(sampled, repeat_penalty=1.3, alpha_frequency=0.2, alpha_presence=0.1), allowed=ring.tolist(),
                  ring=ring, pushed=64),
             dict(name="unconstrained beside constrained rows", logits=lg[7], params=p, allowed=None)]
    _run_cases(dev, vocab, cases)


@pytest.mark.parametrize("vocab", VOCABS)
def test_bias_against_constrained_reference(dev, vocab):
    rng = np.random.default_rng(13 * vocab)
    lg = _logits(rng, vocab, 8)
    far = vocab - 2
    flip = lg[0].copy()
    top = int(np.argmax(flip[:vocab].astype(np.float32)))
    loser = (top + 37) % vocab
    pen = lg[1].copy()
    pen[far] = 2.25  # biased to 2.25 - 5.5 = -3.25, then * 1.3 (the negative branch of the repetition penalty)
    ring = np.zeros(64, np.int32)
    ring[:4] = [far, 1, far, 2]
    sixteen = [(int(i), float(v)) for i, v in zip(range(far - 20, far - 4), rng.uniform(-3, 3, 16))]  # 16 pairs in one chunk (the last)
    cases = [dict(name="bias flips the argmax", logits=flip, params=_params(False), bias=[(loser, 100.0)]),
             dict(name="bias flips the argmax (sampled)", logits=flip, params=_params(True), bias=[(loser, 100.0)]),
             dict(name="biased and penalised", logits=pen, params=_params(True, repeat_penalty=1.3, alpha_frequency=0.25, alpha_presence=0.5), bias=[(far, -5.5)], ring=ring, pushed=4),
             dict(name="biased and penalised (greedy)", logits=pen, params=_params(False, repeat_penalty=1.3), bias=[(far, 30.0)], ring=ring, pushed=4),
             dict(name="the same id twice", logits=lg[2], params=_params(True), bias=[(7, 1.1), (far, 0.7), (7, 2.3)]),
             dict(name="ids outside the vocabulary in the device row", logits=lg[3], params=_params(True), bias=[(3, 1.5)],
                  raw_bias=[(vocab, 500.0), (3, 1.5), (vocab + 1, 500.0), (-1, 500.0), (1 << 30, 500.0)]),
             dict(name="16 pairs in one chunk", logits=lg[4], params=_params(True), bias=sixteen),
             dict(name="bias under a mask", logits=lg[5], params=_params(True), bias=[(far, 4.0), (2, -4.0)], allowed=[2, 9, far])]
    _run_cases(dev, vocab, cases)
    assert int(np.argmax(flip[:vocab].astype(np.float32))) != loser  # (the case is a flip)


def _peaked(vocab, tokens):
    ld = (vocab + 7) // 8 * 8
    x = np.zeros((len(tokens), ld), np.float16)
    for b, t in enumerate(tokens):
        x[b, t] = 9.0
    return x


def test_a_chain_automaton_yields_exactly_its_tokens(dev):
    """Six states, state i allows only token chain[i] -- never the row's favourite --: six steps, the state word read back after each, then retirement."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    vocab, chain = 4136, [4100, 3, 4135, 77, 4096, 4095]
    a = TokenAutomaton(vocab, 6)
    for i, t in enumerate(chain):
        a.allow(i, t, i + 1 if i < 5 else -1)
    s = _sampler(dev, vocab)
    fsm = s.table.register(a)
    _set(s, [_row(_params(b % 2 == 1), seed=b, max_new=16) for b in range(B)], [constraint_row(fsm, 0)] * 2 + [constraint_row(fsm, 2), constraint_row()])
    logits = torch.from_numpy(_logits(np.random.default_rng(1), vocab)).to(dev)
    pos = torch.tensor([0, 10, 20, 30], dtype=torch.int32, device=dev)
    for step in range(6):
        s.step(logits, pos, POS_BOUND)
        states, p1 = [s.constraint_row(b).state for b in range(B)], pos.cpu().numpy().tolist()
        assert states[:2] == [min(step + 1, 5)] * 2 and p1[:2] == ([step + 1, 11 + step] if step < 5 else [-1, -1]), f"step {step}: states {states}, positions {p1}"
        assert states[2] == min(step + 3, 5) and p1[2] == (21 + step if step < 3 else -1) and p1[3] == 31 + step
    log = s.out_log.cpu().numpy()
    assert log[0, :6].tolist() == chain and log[1, :6].tolist() == chain and log[2, :4].tolist() == chain[2:] and (log[:3, 6] == -1).all() and s.violations() == 0
    assert s.generated().tolist() == [6, 6, 4, 6]


def test_edges_defaults_stop_ids_inactive_rows_and_mixed_slots(dev):
    """Automaton X: state 0 has 300 edges (tokens 10, 20, ..., next 1 + j % 3) and 50 default tokens (next 4).  Launch 1: rows at the first, middle and last edge and
    at a default token.  Launch 2: X, another automaton and an unconstrained slot in one launch, a stop id inside the automaton, and an inactive row."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    vocab = 4136
    X = TokenAutomaton(vocab, 5)
    edge_tokens = [10 * (j + 1) for j in range(300)]
    for j, t in enumerate(edge_tokens):
        X.allow(0, t, 1 + j % 3)
    X.allow_default(0, range(4001, 4101, 2), 4)
    for st in range(1, 5):
        X.allow_default(st, [st, 4135], st)
    Y = TokenAutomaton.from_sequences(vocab, [[4001, 8], [4001, 9]])
    s = _sampler(dev, vocab, stop_ids=[1500])
    x, y = s.table.register(X), s.table.register(Y)
    greedy = _params(False)
    want = [edge_tokens[0], edge_tokens[150], edge_tokens[299], 4051]
    _set(s, [_row(greedy, max_new=16)] * B, [constraint_row(x, 0)] * B)
    pos = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=dev)
    s.step(torch.from_numpy(_peaked(vocab, want)).to(dev), pos, POS_BOUND)
    assert s.next_token.cpu().numpy().tolist() == want and pos.cpu().numpy().tolist() == [2, 3, 4, 5]
    assert [s.constraint_row(b).state for b in range(B)] == [1, 1 + 150 % 3, 1 + 299 % 3, 4]
    # 1500 = edge 149 of X (next 1 + 149 % 3 = 3) is a stop id: the row retires AND the state advances; Y's first token; an unconstrained row; an inactive row
    _set(s, [_row(greedy, max_new=16)] * B, [constraint_row(x, 0), constraint_row(y, 0), constraint_row(), constraint_row(x, 0)])
    before = s.crows.cpu().numpy().copy()
    pos = torch.tensor([7, 8, 9, -1], dtype=torch.int32, device=dev)
    s.next_token.fill_(-7)
    s.step(torch.from_numpy(_peaked(vocab, [1500, 5, 5, 10])).to(dev), pos, POS_BOUND)  # (Y allows only 4001: logit 0 against the row's favourite 5)
    assert s.next_token.cpu().numpy().tolist() == [1500, 4001, 5, -7] and pos.cpu().numpy().tolist() == [-1, 9, 10, -1]
    after = s.crows.cpu().numpy()
    assert [int(after[b, 1]) for b in range(B)] == [3, 1, 0, 0] and np.array_equal(after[3], before[3]) and np.array_equal(after[2], before[2])
    assert s.violations() == 0


def test_rule_6_invalid_rows_retire_and_write_nothing_else(dev):
    """A state out of range, fsm >= n_fsm, a hand-packed state that allows nothing, a next of `states`: each row retires, token / log / ring / counters / constraint
    row / debug record keep their canaries, violations += 1 each."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    vocab = 4136
    s = _sampler(dev, vocab)
    ok = s.table.register(TokenAutomaton.any_of(vocab, [5, 6]))
    empty = TokenAutomaton(vocab, 2).allow_default(0, [5], 1).allow_default(1, [6], 1).pack()
    empty["mask"][1, :] = 0
    empty["mask"][1, -1] = 0xFFFFFF00  # (only bits at and beyond the vocabulary: 4136 = 129 * 32 + 8)
    bad_next = TokenAutomaton(vocab, 2).allow(0, 5, 1).allow_default(1, [6], 1).pack()
    bad_next["edge_next"][0] = 2
    e, n = s.table.register_packed(empty), s.table.register_packed(bad_next)
    crows = [constraint_row(ok, 1), constraint_row(capi.TCE_FSM_MAX, 0), constraint_row(e, 1), constraint_row(n, 0)]
    _set(s, [_row(_params(b % 2 == 0), seed=b, max_new=16, pushed=3, generated=2) for b in range(B)], crows)
    s.next_token.fill_(-7)
    s.out_log.fill_(-5)
    s.debug.fill_(-3)
    rows0, crows0 = s.rows.cpu().numpy().copy(), s.crows.cpu().numpy().copy()
    pos = torch.tensor([4, 5, 6, 7], dtype=torch.int32, device=dev)
    s.step(torch.from_numpy(_logits(np.random.default_rng(6), vocab)).to(dev), pos, POS_BOUND)
    torch.cuda.synchronize()
    assert pos.cpu().numpy().tolist() == [-1] * B and s.violations() == 4
    assert (s.next_token.cpu().numpy() == -7).all() and (s.out_log.cpu().numpy() == -5).all() and (s.debug.cpu().numpy() == -3).all()
    assert np.array_equal(s.rows.cpu().numpy(), rows0) and np.array_equal(s.crows.cpu().numpy(), crows0)
    pos.fill_(3)  # a second call counts again; the negative state
    s.crows[0, 1] = -1
    s.step(torch.from_numpy(_logits(np.random.default_rng(6), vocab)).to(dev), pos, POS_BOUND)
    assert pos.cpu().numpy().tolist() == [-1] * B and s.violations() == 8 and (s.next_token.cpu().numpy() == -7).all()


def test_refusals_before_any_launch(dev):
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import _stream
    vocab = 100
    s = _sampler(dev, vocab)
    logits = torch.zeros((B, 104), dtype=torch.float16, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    s.next_token.fill_(-9)
    call = s.call(logits.data_ptr(), 104, pos.data_ptr(), POS_BOUND)

    def refused(con, code, c=call):
        rc = capi.sample_constrained_f16(c, con, None, _stream())
        assert rc == code, f"rc {rc}, expected {code}"
        with pytest.raises(capi.TceError) as e:
            capi.check(rc)
        assert e.value.code == code

    def con(**kw):
        c = s.constraint()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    refused(None, capi.TCE_ERR_BAD_ARG)
    refused(con(rows=None), capi.TCE_ERR_BAD_ARG)
    refused(con(violations=None), capi.TCE_ERR_BAD_ARG)
    refused(con(n_fsm=-1), capi.TCE_ERR_BAD_ARG)
    refused(con(n_fsm=capi.TCE_FSM_MAX + 1), capi.TCE_ERR_BAD_ARG)
    refused(con(fsms=None), capi.TCE_ERR_BAD_ARG)
    refused(con(fsms=s.table.fsms.data_ptr() + 4), capi.TCE_ERR_UNSUPPORTED_SHAPE)
    refused(con(rows=s.crows.data_ptr() + 2), capi.TCE_ERR_UNSUPPORTED_SHAPE)
    bad = s.call(logits.data_ptr(), 104, pos.data_ptr(), POS_BOUND)
    bad.tfs_z = 0.9
    refused(s.constraint(), capi.TCE_ERR_UNSUPPORTED_SHAPE, bad)  # tce_sample_f16's own refusals come first
    assert capi.sample_constrained_f16(call, con(fsms=None, n_fsm=0), None, _stream()) == capi.TCE_OK  # no automaton at all is a valid table
    torch.cuda.synchronize()
    assert s.violations() == 0


def test_python_refusals(dev):
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import Sampler, SamplingParams
    s = _sampler(dev, 100)
    p = SamplingParams()
    a = s.table.register(TokenAutomaton.any_of(100, [1, 2]))
    with pytest.raises(ValueError):
        s.table.register(TokenAutomaton.any_of(101, [1, 2]))  # another vocabulary
    for bias in ([(i, 1.0) for i in range(17)], {3: float("inf")}, {3: float("nan")}, {100: 1.0}, {-1: 1.0}):
        with pytest.raises(ValueError):
            s.set_row(0, p, 1, 4, automaton=a, logit_bias=bias)
    with pytest.raises(ValueError):
        s.set_row(0, p, 1, 4, automaton=a + 1)  # not registered
    s.set_row(1, p, 1, 4, automaton=a, logit_bias={5: 1.0})
    assert s.constraint_row(1).fsm == a and s.constraint_row(1).n_bias == 1
    with pytest.raises(ValueError):
        s.table.unregister(a)  # slot 1's row names it
    s.set_row(1, p, 1, 4)
    s.table.unregister(a)
    with pytest.raises(ValueError):
        Sampler(B, 100, 16, dev).set_row(0, p, 1, 4, logit_bias={5: 1.0})  # built without constraints=True
