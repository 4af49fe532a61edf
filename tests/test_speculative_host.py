"""The host side of speculative decoding (tinychatengine_amd/speculative.py), no GPU: the acceptance rule is lossless, the n-gram drafts on designed histories, and
the slot book's reservation."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tinychatengine_amd.generate import RING, SamplingParams, ring_window, sample_reference, uniform  # noqa: E402
from tinychatengine_amd.paged_kv import PageAllocator, PagePoolExhausted  # noqa: E402
from tinychatengine_amd.speculative import SpecSlotBook, ngram_draft_reference, verify_reference  # noqa: E402

VOCAB = 48


def _logits(context, salt: int) -> np.ndarray:
    """A deterministic 'model': the fp16 logits row that follows `context` (a function of the whole context, as a causal model's is)."""
    h = salt
    for t in context:
        h = (h * 1000003 + int(t) + 1) % (2 ** 61 - 1)
    return np.random.default_rng(h).normal(0.0, 2.0, VOCAB).astype(np.float16)


def _plain(prompt, params, seed, stop_ids, max_new, salt):
    """One token at a time, as BatchedGenerator does: window of the ring, uniform keyed (seed, index), push, stop."""
    ring, pushed = np.zeros(RING, np.int32), 0
    for t in prompt:
        ring[pushed % RING] = t
        pushed += 1
    seq, out = list(prompt), []
    while True:
        y = sample_reference(_logits(seq, salt), ring_window(ring, pushed, params.repeat_last_n), params, uniform(seed, len(out)))["token"]
        out.append(y)
        seq.append(y)
        ring[pushed % RING] = y
        pushed += 1
        if y in stop_ids or len(out) >= max_new:
            return out


def test_the_chain_emits_what_plain_sampling_emits():
    """300 seeded trials: greedy and sampled, penalties on, stop ids and budgets that fall inside a chain, drafts corrupted at random, ragged draft counts.  The
    speculative loop feeds rows (next token, drafts...), gets each row's logits from the same 'model' on the context the row would see, and lets verify_reference
    decide; its output must be the plain loop's, token for token, and every emitted count from 1 to 4 must occur."""
    rng = np.random.default_rng(2024)
    counts = set()
    for trial in range(300):
        greedy = trial % 3 == 0
        params = SamplingParams(temp=0.0 if greedy else 0.9, top_k=int(rng.integers(1, 12)), top_p=float(rng.choice([0.8, 0.95, 1.0])),
                                repeat_penalty=float(rng.choice([1.0, 1.3])), alpha_frequency=float(rng.choice([0.0, 0.2])), alpha_presence=float(rng.choice([0.0, 0.1])),
                                repeat_last_n=int(rng.choice([0, 5, 64])))
        seed, salt, T = int(rng.integers(0, 2 ** 62)), int(rng.integers(1, 2 ** 30)), 4
        prompt = rng.integers(0, VOCAB, int(rng.integers(1, 6))).tolist()
        max_new = int(rng.integers(1, 14))
        probe = _plain(prompt, params, seed, (), max_new, salt)
        stop_ids = (int(probe[int(rng.integers(0, len(probe)))]),) if trial % 2 else ()
        want = _plain(prompt, params, seed, stop_ids, max_new, salt)

        ring, pushed = np.zeros(RING, np.int32), 0
        for t in prompt:
            ring[pushed % RING] = t
            pushed += 1
        # admission: the first token, a chain of one row
        v = verify_reference([_logits(prompt, salt)], [], ring, pushed, 0, params, seed, stop_ids, max_new)
        out, seq = list(v["tokens"]), prompt + v["tokens"]
        while not v["retired"]:
            ring, pushed, generated = v["ring"], v["pushed"], v["generated"]
            # drafts: the plain continuation (known here), ragged in number and corrupted at random
            n = int(rng.integers(1, T + 1))
            drafts = []
            for t in range(n - 1):
                d = probe[len(out) + t] if len(out) + t < len(probe) else int(rng.integers(0, VOCAB))
                if rng.random() < 0.3:
                    d = int(rng.integers(0, VOCAB))
                drafts.append(int(d))
            rows = [_logits(seq + drafts[:t], salt) for t in range(n)]  # row t sees the sequence plus drafts 1 .. t
            v = verify_reference(rows, drafts, ring, pushed, generated, params, seed, stop_ids, max_new)
            assert 1 <= len(v["tokens"]) <= n and v["generated"] == generated + len(v["tokens"])
            counts.add(len(v["tokens"]))
            out += v["tokens"]
            seq += v["tokens"]
        assert out == want, f"trial {trial}: the chain's tokens differ from plain sampling"
    assert counts == {1, 2, 3, 4}


def test_uniform_hook_and_log_stride():
    p = SamplingParams(temp=1.0, top_k=4, top_p=1.0, repeat_penalty=1.0)
    row = np.zeros(VOCAB, np.float16)
    row[[3, 9]] = 8.0  # two candidates of equal weight, the rest far below
    ring = np.zeros(RING, np.int32)
    v = verify_reference([row, row], [9], ring, 0, 0, p, 0, (), 10, uniforms=[0.75, 0.25])
    assert v["tokens"] == [9, 3] and v["accepted"] == 1 and not v["retired"]
    v = verify_reference([row, row], [9], ring, 0, 0, p, 0, (), 10, uniforms=[0.75, 0.25], log_stride=1)
    assert v["tokens"] == [9] and v["retired"]


# ---- drafts ----
def _draft(history, p, n=2, T=4, bound=63, script=None):
    tok, pos = ngram_draft_reference(history, p, n, T, bound, script=script)
    return tok.tolist(), pos.tolist()


def test_ngram_no_match():
    assert _draft([1, 2, 3, 4, 5, 6], 5) == ([6, 0, 0, 0], [5, -1, -1, -1])


def test_ngram_position_shorter_than_the_ngram():
    assert _draft([7, 7, 7], 1, n=2) == ([7, 0, 0, 0], [1, -1, -1, -1])  # p < n: no drafts, though the token repeats
    assert _draft([7, 7, 7], 2, n=2) == ([7, 7, 0, 0], [2, 3, -1, -1])   # p == n: (7, 7) ends at i = 1 too; what follows it is index 2


def test_ngram_most_recent_of_two_matches():
    #        0  1  2  3  4  5  6  7  8  9
    hist = [1, 2, 30, 31, 1, 2, 40, 41, 1, 2]
    assert _draft(hist, 9) == ([2, 40, 41, 1], [9, 10, 11, 12])  # i* = 5, not 1
    assert _draft(hist, 9, T=8)[0] == [2, 40, 41, 1, 2, 0, 0, 0]  # i* + t <= p ends the prefix at t = 4


def test_ngram_match_ending_right_in_front_yields_one_draft():
    hist = [5, 9, 9]
    assert _draft(hist, 2, n=1) == ([9, 9, 0, 0], [2, 3, -1, -1])  # i* = p - 1: only history[p] itself follows it


def test_ngram_truncation_at_the_bound():
    hist = [1, 2, 30, 31, 32, 1, 2]
    assert _draft(hist, 6, bound=63) == ([2, 30, 31, 32], [6, 7, 8, 9])
    assert _draft(hist, 6, bound=7) == ([2, 30, 0, 0], [6, 7, -1, -1])
    assert _draft(hist, 6, bound=6) == ([2, 0, 0, 0], [6, -1, -1, -1])
    assert _draft(hist, 6, bound=5) == ([0, 0, 0, 0], [-1, -1, -1, -1])  # the sequence itself is past the bound: inactive
    assert _draft(hist, -1) == ([0, 0, 0, 0], [-1, -1, -1, -1])


def test_script_hook_replaces_the_lookup():
    hist = [1, 2, 30, 31, 32, 1, 2]
    script = [-1] * 7 + [70, 71, -1, 73]
    assert _draft(hist, 6, script=script) == ([2, 70, 71, 0], [6, 7, 8, -1])  # -1 ends the prefix; what lies behind it is not used
    assert _draft(hist, 6, script=[-1] * 16) == ([2, 0, 0, 0], [6, -1, -1, -1])
    assert _draft(hist, 6, script=script, bound=7) == ([2, 70, 0, 0], [6, 7, -1, -1])


def test_refusals():
    with pytest.raises(ValueError):
        ngram_draft_reference([1, 2], 1, 2, 9, 63)
    with pytest.raises(ValueError):
        ngram_draft_reference([1, 2], 1, 5, 4, 63)
    with pytest.raises(ValueError):
        SpecSlotBook(2, 64, 0)


# ---- the slot book ----
def test_slot_book_reserves_for_every_row_whatever_the_budget():
    book = SpecSlotBook(3, 64, 4)
    book.admit(0, 10, 2)   # one token left: the replay still writes rows 10 .. 13
    book.admit(2, 60, 40)
    assert book.wanted(1) == [(0, 13), (2, 63)]
    assert book.wanted(3) == [(0, 21), (2, 63)]  # clipped at the cache's last key
    alloc = PageAllocator(8, 16, 3, 4, "cpu")
    alloc.reserve_many([(0, 9), (2, 59)])  # admission: 1 + 4 pages
    assert alloc.pages_in_use() == 5
    book.reserve(alloc, 1)
    assert alloc.pages_in_use() == 5  # positions 13 and 63 lie in pages the slots hold
    book.reserve(alloc, 3)
    assert alloc.pages_in_use() == 6 and len(alloc.pages[0]) == 2
    alloc.check_invariants()


def test_slot_book_reservation_is_all_or_nothing():
    book = SpecSlotBook(2, 64, 8)
    book.admit(0, 15, 40)
    book.admit(1, 15, 40)
    alloc = PageAllocator(3, 16, 2, 4, "cpu")
    alloc.reserve_many([(0, 14), (1, 14)])
    before = ([list(p) for p in alloc.pages], list(alloc.free), alloc.table.clone())
    with pytest.raises(PagePoolExhausted):
        book.reserve(alloc, 1)  # both slots need a second page for rows 15 .. 22; one page is free
    assert [list(p) for p in alloc.pages] == before[0] and alloc.free == before[1] and torch.equal(alloc.table, before[2])
    alloc.check_invariants()
    book.update([-1, 15], [3, 1])  # slot 0 retired
    assert book.wanted(1) == [(1, 22)]
    book.reserve(alloc, 1)
    assert len(alloc.pages[1]) == 2
