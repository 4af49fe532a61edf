"""tce_sample_verify_mirostat_f16 (speculative.Verifier over a Sampler(mirostat_rows=True)): B = 4 sequences of T = 4 rows with scripted drafts -- all accepted (mode
2), rejected at row 1 (mode 1), none (mode 2), all accepted (mode 0 with stages) -- must leave exactly what successive tce_sample_mirostat_f16 calls leave: emitted
tokens, rows (ring, counters), positions, `emitted`, history and the stored mu, bit for bit; with log-probabilities and with an automaton, one case each."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VOCAB, B, T, POS_BOUND, HIST = 8200, 4, 4, 63, 80
P0 = [10, 0, 30, 21]  # the sequences' positions


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _params():
    from tinychatengine_amd.generate import SamplingParams
    return [SamplingParams(temp=0.9, top_k=16, repeat_penalty=1.2, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.3), SamplingParams(temp=0.8, top_k=40, mirostat=1, mirostat_tau=4.0),
            SamplingParams(temp=1.1, top_k=8, repeat_penalty=1.0, mirostat=2, mirostat_tau=2.0), SamplingParams(temp=0.8, top_k=40, top_p=0.9, tfs_z=0.95, typical_p=0.8)]


def _sampler(dev, form):
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import Sampler
    s = Sampler(B, VOCAB, 16, dev, top_k_bound=40, mirostat_rows=True, logprobs=form == "logprobs", constraints=form == "automaton")
    rng = np.random.default_rng(3)
    fsm = s.table.register(TokenAutomaton.any_of(VOCAB, range(1, VOCAB, 2))) if form == "automaton" else None  # odd ids only
    for b, p in enumerate(_params()):
        s.set_row(b, p, seed=900 + b, max_new=12, prompt_ids=rng.integers(0, VOCAB, 6).tolist(), **({"automaton": fsm if b != 2 else None} if form == "automaton" else {}))
    return s


def _serial(dev, form, logits, steps):
    """steps[b] successive tce_sample_mirostat_f16 calls for sequence b on its rows (b, 0), (b, 1), ...: the sampler afterwards, the positions, the tokens."""
    s = _sampler(dev, form)
    pos = torch.tensor(P0, dtype=torch.int32, device=dev)
    tokens = [[] for _ in range(B)]
    for t in range(max(steps)):
        live = [b for b in range(B) if t < steps[b]]
        step_pos = torch.tensor([P0[b] + t if b in live else -1 for b in range(B)], dtype=torch.int32, device=dev)
        s.step(logits.view(B, T, -1)[:, t].contiguous(), step_pos, POS_BOUND)
        tok = s.next_token.cpu().numpy()
        for b in live:
            tokens[b].append(int(tok[b]))
            pos[b] = step_pos[b]
    return s, pos, tokens


@pytest.mark.parametrize("form", ["plain", "logprobs", "automaton"])
def test_verifier_equals_successive_mirostat_calls(dev, form):
    from tinychatengine_amd.speculative import Verifier
    rng = np.random.default_rng(41)
    ld = (VOCAB + 7) // 8 * 8
    x = (rng.standard_normal((B * T, ld), dtype=np.float32) * np.float32(2.5)).astype(np.float16)
    logits = torch.from_numpy(x).to(dev)
    _, _, y = _serial(dev, form, logits, [T] * B)  # discovery: what the plain loop samples from rows (b, 0 .. T - 1) when every row is reached
    assert all(len(t) == T for t in y)
    drafts = {0: y[0][:3], 1: [(y[1][0] + 2) % VOCAB, y[1][1], y[1][2]], 2: [], 3: y[3][:3]}  # all accepted; rejected at row 1; no draft at all; all accepted
    emits = [4, 1, 1, 4]
    want, want_pos, want_tok = _serial(dev, form, logits, emits)
    assert [t for t in want_tok] == [y[b][:emits[b]] for b in range(B)]

    s = _sampler(dev, form)
    ver = Verifier(s, T)
    history = rng.integers(0, VOCAB, (B, HIST)).astype(np.int32)
    row_token, row_pos = np.zeros((B, T), np.int32), np.full((B, T), -1, np.int32)
    for b in range(B):
        n = 1 + len(drafts[b])
        row_token[b, 0] = history[b, P0[b]]
        row_token[b, 1:n] = drafts[b]
        row_pos[b, :n] = P0[b] + np.arange(n)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rt, rp, hs, ps = d(row_token.reshape(-1)), d(row_pos.reshape(-1)), d(history), d(np.array(P0, np.int32))
    ver.step(logits, rt, rp, hs, ps, POS_BOUND)
    torch.cuda.synchronize()
    assert ver.emitted.cpu().numpy().tolist() == emits
    assert ps.cpu().numpy().tolist() == want_pos.cpu().numpy().tolist() == [P0[b] + emits[b] for b in range(B)]
    assert torch.equal(s.out_log, want.out_log), "emitted tokens"
    assert torch.equal(s.rows, want.rows), "rows: ring and counters"
    assert torch.equal(s.next_token, want.next_token) and torch.equal(s.srows, want.srows)
    assert torch.equal(s.mrows, want.mrows), "mirostat rows: the stored mu"
    mu = s.mrows.cpu().numpy()[:, 4].copy().view(np.float32)
    assert all(mu[b] != np.float32(2.0) * np.float32(_params()[b].mirostat_tau) for b in (0, 1, 2)) and mu[3] == np.float32(10.0)  # mu moved where mirostat ran
    got_hist = hs.cpu().numpy()
    for b in range(B):
        h = history[b].copy()
        h[P0[b] + 1:P0[b] + 1 + emits[b]] = y[b][:emits[b]]
        assert np.array_equal(got_hist[b], h), f"sequence {b}: history"
    if form == "logprobs":
        a, w = s.out_logprob.cpu().numpy(), want.out_logprob.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(w)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), w[~np.isnan(w)].view(np.uint32)), "log-probabilities"
        assert torch.equal(s.last_lse.view(torch.int32), want.last_lse.view(torch.int32))
    if form == "automaton":
        assert torch.equal(s.crows, want.crows) and s.violations() == want.violations() == 0
        assert all(t % 2 == 1 for b in (0, 1) for t in y[b])
