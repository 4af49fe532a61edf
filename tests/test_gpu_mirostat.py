"""tce_sample_mirostat_f16 on the device (csrc/sampling.hip: the MIRO = true forms of sample_draw_kernel; generate.Sampler(mirostat_rows=True)): mirostat v1 and v2
per slot over the row's top-k candidates, with mu read and written by the launch that emits the token.

The fixture configurations are held against the reference's own results (tests/golden/mirostat_golden.npz) under the rules of tests/mirostat_rules.py; every designed
case (tests/mirostat_cases.py) against its own float64 restatement; a mixed batch against tce_sample_stages_f16 in bytes for its mode-0 rows; the constraint and
logprob blocks; and the rows on which mu must not move."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirostat_cases as MC  # noqa: E402
import mirostat_rules as MR  # noqa: E402
import sampling_rules as R  # noqa: E402

POS_BOUND = 63


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return MR.load_fixture()


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


def _mrow(mode, mu, tau=5.0, eta=0.1, m=100):
    from tinychatengine_amd import capi
    return capi.MirostatRow(mode=mode, m=m, tau=tau, eta=eta, mu=mu)


def _set(sampler, rows, mrows, pairs=None, crows=None):
    sampler.rows.copy_(torch.from_numpy(np.stack([_words(r) for r in rows])))
    sampler.mrows.copy_(torch.from_numpy(np.stack([_words(r) for r in mrows])))
    if pairs is not None:
        sampler.srows.copy_(torch.tensor(pairs, dtype=torch.float32))
    if crows is not None:
        sampler.crows.copy_(torch.from_numpy(np.stack([_words(c) for c in crows])))


def _debug(sampler) -> dict:
    d = sampler.debug.cpu().numpy()
    out = {"n": d[:, 0], "k": d[:, 1], "u": d[:, 2].copy().view(np.float32), "choice": d[:, 3], "ids": d[:, 4:260], "logit": d[:, 260:516].copy().view(np.float32),
           "p": d[:, 516:772].copy().view(np.float32), "final_p": d[:, 772:1028].copy().view(np.float32)}
    m = sampler.mdebug.cpu().numpy()
    f = lambda j: m[:, j].copy().view(np.float32)
    out.update({"mode": m[:, 0], "kk": m[:, 1], "s_hat": f(2), "k_f": f(3), "kept": m[:, 4], "mu_in": f(5), "mu_out": f(6), "surprise": f(7), "m_choice": m[:, 8], "m_final_p": f(9)})
    return out


def _mu(sampler) -> np.ndarray:
    return sampler.mrows.cpu().numpy()[:, 4].copy().view(np.float32)


def _result(d: dict, j: int, tok: int, mu_after) -> dict:
    """Row j of the debug records with mirostat_rules.check_row's keys; the two records and the stored mu must tell one story."""
    kk, n = int(d["k"][j]), int(d["n"][j])
    assert int(d["kk"][j]) == kk and int(d["kept"][j]) == n and int(d["m_choice"][j]) == int(d["choice"][j])
    assert np.float32(d["mu_out"][j]).view(np.uint32) == np.float32(mu_after).view(np.uint32), "the stored mu is not the record's mu_out"
    assert np.float32(d["m_final_p"][j]).view(np.uint32) == np.float32(d["final_p"][j][int(d["choice"][j])]).view(np.uint32)
    assert (d["final_p"][j][n:] == 0).all() and (d["ids"][j][kk:] == -1).all()
    return {"ids": d["ids"][j][:kk], "logits": d["logit"][j][:kk], "p": d["p"][j][:kk], "kept": n, "final_p": d["final_p"][j][:n], "choice": int(d["choice"][j]),
            "token": int(tok), "mu_out": d["mu_out"][j], "mu_in": d["mu_in"][j], "s_hat": d["s_hat"][j], "k_f": d["k_f"][j], "surprise": d["surprise"][j], "mode": int(d["mode"][j])}


@pytest.mark.parametrize("name", list(MR.CONFIGS))
def test_fixture_rows_against_the_reference(dev, fixture, name):
    """Every row of a configuration in ONE launch: row r starts from the mu the reference's row r started from and draws on the midpoint of X's interval."""
    from tinychatengine_amd.generate import Sampler
    mode, vocab, k, sigma, temp, tau, eta, rows, seed = MR.CONFIGS[name]
    ins = MR.config_inputs(name, fixture)
    prm = MR.params_of(name)
    ld = (vocab + 7) // 8 * 8 + 8
    x = np.full((rows, ld), 60000.0, np.float16)  # columns past the vocabulary hold the largest values: they must never be candidates
    for r, (logits, _) in enumerate(ins):
        x[r, :vocab] = logits
    s = Sampler(rows, vocab, 4, dev, top_k_bound=k, debug=True, mirostat_rows=True)
    _set(s, [_row(prm, seed=r, ring=rec, pushed=64) for r, (_, rec) in enumerate(ins)], [_mrow(mode, float(fixture[name + "/mu_in"][r]), tau, eta) for r in range(rows)])
    s.uniform_override = torch.tensor([float(MR.row_u(name, r, fixture)[0]) for r in range(rows)], dtype=torch.float32, device=dev)
    pos = torch.full((rows,), 5, dtype=torch.int32, device=dev)
    s.step(torch.from_numpy(x).to(dev), pos, POS_BOUND)
    torch.cuda.synchronize()
    d, tok, mu, gen = _debug(s), s.next_token.cpu().numpy(), _mu(s), s.generated()
    assert pos.cpu().numpy().tolist() == [6] * rows and gen.tolist() == [1] * rows  # every row advances once, decided or not
    decided, worst = 0, 0.0
    for r, (logits, rec) in enumerate(ins):
        got = _result(d, r, tok[r], mu[r])
        assert got["mode"] == mode and np.float32(got["mu_in"]).view(np.uint32) == fixture[name + "/mu_in"][r].view(np.uint32)
        res = MR.check_row(f"{name} row {r}", name, r, fixture, R.penalised(logits, rec, MR.REPEAT_PENALTY, 0.0, 0.0), got)
        decided += res["decided"]
        worst = max(worst, res["worst"])
    print(f"{name}: {decided} of {rows} rows decided, worst relative error of a p {worst:.3e} (tol {R.tol(k):.3e})")
    assert decided >= (1 - MR.MAX_UNDECIDED) * rows


@pytest.mark.parametrize("name", [c.name for c in MC.cases()])
def test_designed_cases(dev, name):
    from tinychatengine_amd.generate import Sampler, SamplingParams
    c = MC.by_name(name)
    ref = MC.ref_of(c)
    prm = SamplingParams(**{f: getattr(c.prm, f) for f in ("temp", "top_k", "top_p", "repeat_penalty", "alpha_frequency", "alpha_presence", "repeat_last_n")})
    s = Sampler(1, c.vocab, 4, dev, top_k_bound=c.bound, debug=True, mirostat_rows=True)
    _set(s, [_row(prm, ring=c.ring, pushed=c.pushed)], [_mrow(c.prm.mirostat, c.mu, c.prm.mirostat_tau, c.prm.mirostat_eta, c.prm.m)])
    s.uniform_override = torch.tensor([c.u], dtype=torch.float32, device=dev)
    pos = torch.tensor([3], dtype=torch.int32, device=dev)
    s.step(torch.from_numpy(MC.padded(c)[None, :]).to(dev), pos, POS_BOUND)
    torch.cuda.synchronize()
    d = _debug(s)
    got = _result(d, 0, int(s.next_token[0]), _mu(s)[0])
    assert int(pos[0]) == 4 and int(s.out_log[0, 0]) == got["token"] == ref["token"], f"{name}: token {got['token']}, the float64 restatement gives {ref['token']}"
    assert got["ids"].tolist() == ref["ids"].tolist() and np.array_equal(np.asarray(got["logits"], np.float32).view(np.uint32), ref["logits"].view(np.uint32))
    assert np.float32(got["mu_in"]).view(np.uint32) == np.float32(c.mu).view(np.uint32)
    if c.prm.temp <= 0:  # greedy: nothing of the rule runs, mu keeps its bits
        assert got["mode"] == 0 and got["kept"] == 1 and np.float32(got["mu_out"]).view(np.uint32) == np.float32(c.mu).view(np.uint32)
        return
    assert got["mode"] == c.prm.mirostat and got["kept"] == ref["kept"] and got["choice"] == ref["choice"], f"{name}: kept {got['kept']} / choice {got['choice']}"
    t = R.tol(c.bound)
    assert np.abs(np.asarray(got["p"], np.float64) / ref["p"] - 1).max() <= t and np.abs(np.asarray(got["final_p"], np.float64) / ref["final_p"] - 1).max() <= t
    err, bound = abs(float(got["mu_out"]) - ref["mu_out"]), MC.mu_bound(c, ref)
    print(f"{name}: kept {got['kept']}, s_hat {got['s_hat']}, k_f {got['k_f']}, mu {c.mu} -> {got['mu_out']} (error {err:.3e}, bound {bound:.3e})")
    assert err <= bound
    if c.prm.mirostat == 1:
        if math.isnan(ref["k_f"]):
            assert math.isnan(float(got["k_f"]))
        elif math.isinf(ref["k_f"]):
            assert math.isinf(float(got["k_f"])) and got["k_f"] > 0
        else:
            v = MR.v1_decided(ref["p"], c.mu, c.vocab, c.prm.m, c.bound)[2]
            if "delta_k" in v:
                assert abs(float(got["k_f"]) - ref["k_f"]) <= v["delta_k"] * ref["k_f"]


def _mixed_logits(rng, rows, vocab):
    ld = (vocab + 7) // 8 * 8 + 8
    x = (rng.standard_normal((rows, ld), dtype=np.float32) * np.float32(2.5)).astype(np.float16)
    x[:, vocab:] = 60000.0
    return x


def _mixed_setup() -> dict:
    """The mixed batch's inputs, and for its mirostat rows the numpy rule's result with the assertion that the row is DECIDED (from the float64 rules on the
    reference's p, never from the device's result): needs no GPU."""
    from tinychatengine_amd.generate import SamplingParams, ring_window, sample_reference
    B, V = 8, 8200
    rng = np.random.default_rng(23)
    host = _mixed_logits(rng, B, V)
    ring = rng.integers(0, V, 64).astype(np.int32)
    ps = [SamplingParams(), SamplingParams(temp=0.0), SamplingParams(temp=0.7, top_k=40, top_p=0.9, repeat_penalty=1.2, tfs_z=0.9, typical_p=0.8),
          SamplingParams(temp=0.9, top_k=30, repeat_penalty=1.1, mirostat=1, mirostat_tau=3.0), SamplingParams(temp=0.8, top_k=40, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.2),
          SamplingParams(temp=1.3, top_k=17, top_p=1.0, repeat_penalty=1.0), SamplingParams(temp=0.8, top_k=3, top_p=0.5, alpha_presence=0.2),
          SamplingParams(temp=0.8, top_k=40, repeat_penalty=1.0, mirostat=2)]
    st = {"B": B, "V": V, "host": host, "ring": ring, "ps": ps, "modes": [2, 2, 0, 1, 2, 0, 7, 2], "mus": [3.25, 4.5, 5.75, 6.0, 4.0, -1.5, 9.0, 10.0], "miro": [3, 4, 7],
          "us": [0.5, 0.5, 0.3, 0.4, 0.6, 0.7, 0.2, 0.0], "refs": {}}
    for b in st["miro"]:
        ref = sample_reference(host[b, :V], ring_window(ring, 70 + b, ps[b].repeat_last_n), ps[b], st["us"][b], mu=st["mus"][b])
        ok = MR.v1_decided(ref["p"], st["mus"][b], V, MR.M, 40)[0] if ps[b].mirostat == 1 else MR.v2_decided(ref["p"], st["mus"][b], 40)[0]
        cdf = np.cumsum(ref["final_p"], dtype=np.float32).astype(np.float64)
        assert ok and (ref["kept"] == 1 or np.abs(cdf[:-1] - st["us"][b]).min() > 2 * R.tol(40)), f"row {b} of the mixed batch is not decided (move its mu or u)"
        st["refs"][b] = ref
    return st


@pytest.mark.parametrize("form", ["plain", "logprobs", "constrained_logprobs"])
def test_mixed_batch_and_the_mode_0_rows_in_bytes(dev, form):
    """B = 8 in one launch: inactive, greedy (mode 2 set), mode 0 with stages, mode 1, mode 2, mode 0 plain, a mode outside {0, 1, 2}, mode 2 on a stop token.  The rows
    that run no mirostat are tce_sample_stages_f16's rows byte for byte -- token, log, row, position, debug and stage records (logprob, LSE, constraint rows) -- and
    their mu keeps its bits; the mirostat rows emit the numpy rule's token and move mu, the one that draws a stop id included."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    from tinychatengine_amd.generate import Sampler
    st = _mixed_setup()
    B, V, host, ring, ps, modes, mus, miro, us = (st[k] for k in ("B", "V", "host", "ring", "ps", "modes", "mus", "miro", "us"))
    logits = torch.from_numpy(host).to(dev)
    lp, con = "logprobs" in form, "constrained" in form
    stop = int(np.argmax(host[7, :V].astype(np.float32)))  # row 7 draws its best candidate (u = 0, no penalty): the call's stop id
    rows = [_row(p, seed=b + 1, ring=ring, pushed=70 + b, generated=b) for b, p in enumerate(ps)]
    out = []
    for mirostat in (False, True):
        s = Sampler(B, V, 16, dev, top_k_bound=40, stop_ids=[stop], debug=True, logprobs=lp, constraints=con, stages=True, mirostat_rows=mirostat)
        s.rows.copy_(torch.from_numpy(np.stack([_words(r) for r in rows])))
        s.srows.copy_(torch.tensor([(p.tfs_z, p.typical_p) for p in ps], dtype=torch.float32))
        if mirostat:
            s.mrows.copy_(torch.from_numpy(np.stack([_words(_mrow(modes[b], mus[b], ps[b].mirostat_tau, ps[b].mirostat_eta)) for b in range(B)])))
        if con:  # the rows that run no mirostat carry automata and biases; the mirostat rows are unconstrained rows of a constrained call
            a = s.table.register(TokenAutomaton.any_of(V, range(0, V, 3)))
            crows = [constraint_row(), constraint_row(a, 0), constraint_row(a, 0), constraint_row(), constraint_row(), constraint_row(-1, 0, [(4096, -1.0)]),
                     constraint_row(a, 0, [(9, 30.0)]), constraint_row()]
            s.crows.copy_(torch.from_numpy(np.stack([_words(c) for c in crows])))
        s.uniform_override = torch.tensor(us, dtype=torch.float32, device=dev)
        pos = torch.tensor([-1, 0, 63, 9, 17, 4, 30, 12], dtype=torch.int32, device=dev)
        s.step(logits, pos, POS_BOUND)
        torch.cuda.synchronize()
        got = {"token": s.next_token, "log": s.out_log, "rows": s.rows, "pos": pos, "debug": s.debug, "sdebug": s.sdebug}
        if lp:
            got.update({"logprob": s.out_logprob, "lse": s.last_lse})
        if con:
            got.update({"crows": s.crows})
        out.append({k: v.cpu().numpy() for k, v in got.items()})
        if mirostat:
            d, mu_after, tok = _debug(s), _mu(s), s.next_token.cpu().numpy()
            assert int(s.violations()) == 0
    plain, mixed = out
    assert mixed["pos"].tolist() == [-1, 1, 64, 10, 18, 5, 31, -1]  # the inactive row stays, row 7 retires on its stop id, every other row advances once
    same = [b for b in range(B) if b not in miro]
    for key in plain:
        assert plain[key][same].tobytes() == mixed[key][same].tobytes(), f"{form}: {key} of the rows that run no mirostat differs from tce_sample_stages_f16's"
    for b in same:
        assert np.float32(mu_after[b]).view(np.uint32) == np.float32(mus[b]).view(np.uint32), f"row {b}: mu moved"
    assert d["mode"][[1, 2, 5, 6]].tolist() == [0, 0, 0, 0] and d["mode"][miro].tolist() == [1, 2, 2]
    for b in miro:
        got, ref = _result(d, b, tok[b], mu_after[b]), st["refs"][b]
        assert got["ids"].tolist() == ref["ids"].tolist() and got["kept"] == ref["kept"] and got["token"] == ref["token"], f"row {b}"
        bound = 2 * MR.dmu(40, float(ref["surprise"]), ps[b].mirostat_tau, ps[b].mirostat_eta, float(ref["mu_out"]))  # (two fp32 implementations, each within dmu of the exact value)
        assert abs(float(got["mu_out"]) - float(ref["mu_out"])) <= bound and mu_after[b] != np.float32(mus[b]), f"row {b}"
        assert mixed["log"][b, b] == tok[b] and mixed["rows"][b, 10] == b + 1  # the log at `generated`, the counter
    assert tok[7] == stop and mu_after[7] != np.float32(mus[7])  # a stop token is an emitted token: mu moved
    if lp:  # a mirostat row's log-probability is the model's: tce_logprobs_f16's for the same token, bit for bit
        from tinychatengine_amd import capi
        from tinychatengine_amd.linear import _stream
        target = torch.from_numpy(tok.astype(np.int32)).to(dev)
        val, lse = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
        part = torch.empty(int(capi.lib().tce_logprobs_workspace_bytes(B, V)), dtype=torch.uint8, device=dev)
        capi.check(capi.logprobs_f16(logits.data_ptr(), logits.shape[1], V, B, target.data_ptr(), val.data_ptr(), lse.data_ptr(), part.data_ptr(), _stream()))
        torch.cuda.synchronize()
        for b in miro:
            assert mixed["logprob"][b, b].tobytes() == val[b].cpu().numpy().tobytes() and mixed["lse"][b].tobytes() == lse[b].cpu().numpy().tobytes(), f"row {b}"


def test_rule_6_row_emits_nothing_and_keeps_mu(dev):
    """A constrained mirostat row in an invalid state (rule 6): no token, no log entry, no counter, the row retires, one violation -- and mu keeps its bits.  Its
    neighbour, a constrained mirostat row in a valid state, emits an allowed token and moves mu."""
    from tinychatengine_amd.constrain import TokenAutomaton, constraint_row
    from tinychatengine_amd.generate import Sampler, SamplingParams
    B, V = 2, 4097
    rng = np.random.default_rng(29)
    logits = torch.from_numpy(_mixed_logits(rng, B, V)).to(dev)
    prm = SamplingParams(temp=0.8, top_k=40, mirostat=2)
    s = Sampler(B, V, 8, dev, top_k_bound=40, debug=True, constraints=True, logprobs=True, mirostat_rows=True)
    a = s.table.register(TokenAutomaton.any_of(V, range(1, V, 2)))
    _set(s, [_row(prm, seed=1), _row(prm, seed=2)], [_mrow(2, 6.5), _mrow(2, 6.5)], crows=[constraint_row(a, 99), constraint_row(a, 0)])
    before = s.rows.cpu().numpy().copy()
    pos = torch.tensor([7, 7], dtype=torch.int32, device=dev)
    s.step(logits, pos, POS_BOUND)
    torch.cuda.synchronize()
    assert pos.cpu().numpy().tolist() == [-1, 8] and s.violations() == 1
    assert s.rows.cpu().numpy()[0].tobytes() == before[0].tobytes() and int(s.out_log[0, 0]) == -1 and (s.mdebug.cpu().numpy()[0] == 0).all()
    mu = _mu(s)
    assert np.float32(mu[0]).view(np.uint32) == np.float32(6.5).view(np.uint32) and mu[1] != np.float32(6.5)
    assert int(s.next_token[1]) % 2 == 1 and int(s.generated()[1]) == 1


def test_set_row_writes_the_slots_row_and_a_sampler_without_the_flag_refuses(dev):
    from tinychatengine_amd.generate import Sampler, SamplingParams
    s = Sampler(3, 300, 8, dev, top_k_bound=40, mirostat_rows=True)
    assert s.stages and s.mirostat_rows and [s.mirostat_row(b).mode for b in range(3)] == [0, 0, 0]
    s.set_row(1, SamplingParams(mirostat=2, mirostat_tau=3.5, mirostat_eta=0.25, tfs_z=0.9), 5, 4)
    r = s.mirostat_row(1)
    assert (r.mode, r.m, r.tau, r.eta, r.mu) == (2, 100, 3.5, 0.25, 7.0) and s.mirostat_row(0).mode == s.mirostat_row(2).mode == 0
    s.set_row(1, SamplingParams(), 5, 4)  # the next request of the slot: off again
    assert s.mirostat_row(1).mode == 0
    with pytest.raises(ValueError):
        s.set_row(0, SamplingParams(mirostat=3), 5, 4)
    for kw in (dict(), dict(stages=True)):
        with pytest.raises(ValueError, match="not built"):
            Sampler(1, 300, 8, dev, **kw).set_row(0, SamplingParams(mirostat=1), 5, 4)
    # the constructor's `mirostat` is the CALL's field: refused by the entry point, flag or not
    bad = Sampler(1, 300, 8, dev, mirostat=2, mirostat_rows=True)
    bad.set_row(0, SamplingParams(), 5, 4)
    with pytest.raises(Exception, match="not built"):
        bad.step(torch.zeros((1, 304), dtype=torch.float16, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), POS_BOUND)
