"""tinychatengine_amd/constrain.py without a device: the ctypes mirrors' layout, the automaton builder's refusals and packing, the three constructors, and
constrained_reference (rules 1-3 of tce_sample_constrained_f16) against sample_reference and against hand-made rows."""
import ctypes as C

import numpy as np
import pytest

from tinychatengine_amd import capi
from tinychatengine_amd.constrain import DONE, TokenAutomaton, biased_logits, check_bias, constrained_reference
from tinychatengine_amd.generate import SamplingParams, sample_reference


def test_struct_sizes_and_offsets():
    assert C.sizeof(capi.Fsm) == 56 and C.sizeof(capi.ConstraintRow) == 144 and C.sizeof(capi.Constraint) == 32
    assert [getattr(capi.Fsm, f).offset for f in ("mask", "edge_begin", "edge_token", "edge_next", "default_next", "states", "mask_words", "start", "reserved0")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert [getattr(capi.ConstraintRow, f).offset for f in ("fsm", "state", "n_bias", "reserved0", "bias_id", "bias_val")] == [0, 4, 8, 12, 16, 80]
    assert [getattr(capi.Constraint, f).offset for f in ("fsms", "n_fsm", "reserved0", "rows", "violations")] == [0, 8, 12, 16, 24]
    assert (capi.TCE_FSM_DONE, capi.TCE_FSM_MAX, capi.TCE_BIAS_MAX) == (-1, 64, 16)


def test_builder_refusals():
    with pytest.raises(ValueError):
        TokenAutomaton(0, 1)
    with pytest.raises(ValueError):
        TokenAutomaton(10, 0)
    with pytest.raises(ValueError):
        TokenAutomaton(10, 2, start=2)
    with pytest.raises(ValueError):
        TokenAutomaton(10, 2).allow(2, 1, 0)  # no such state
    with pytest.raises(ValueError, match="allows no token"):
        TokenAutomaton(10, 2).allow(0, 1, 1).check()  # state 1 is empty
    with pytest.raises(ValueError, match="no next state"):
        TokenAutomaton(10, 1).allow(0, 1, 0).allow(0, 2).check()  # token 2: allowed, no edge, no default
    with pytest.raises(ValueError, match="next 1 outside"):
        TokenAutomaton(10, 1).allow(0, 1, 1).check()
    with pytest.raises(ValueError, match="next -2 outside"):
        TokenAutomaton(10, 1).allow_default(0, [1], -2).check()
    with pytest.raises(ValueError, match="outside the vocabulary"):
        TokenAutomaton(10, 1).allow(0, 10, 0).check()
    with pytest.raises(ValueError, match="outside the vocabulary"):
        TokenAutomaton(10, 1).allow_default(0, [-1], 0).check()
    with pytest.raises(ValueError, match="already has the default"):
        TokenAutomaton(10, 2).allow_default(0, [1], 0).allow_default(0, [2], 1)
    with pytest.raises(ValueError):
        TokenAutomaton(10, 1).pack()  # pack() checks
    with pytest.raises(ValueError):
        TokenAutomaton.from_sequences(10, [])
    with pytest.raises(ValueError):
        TokenAutomaton.from_sequences(10, [[1], []])
    TokenAutomaton(10, 1).allow(0, 1, DONE).allow(0, 2).allow_default(0, [3], 0).check()  # (a default makes token 2 complete)


def test_pack_layout():
    a = TokenAutomaton(70, 3, start=1)  # 70 is no multiple of 32: three mask words
    a.allow(0, 69, 2).allow(0, 3, 1).allow(0, 33, DONE).allow_default(0, [0, 31, 32, 64], 0)
    a.allow_default(1, range(70), 1)
    a.allow(2, 5, 0)
    p = a.pack()
    assert (p["states"], p["mask_words"], p["start"]) == (3, 3, 1)
    assert p["mask"].dtype == np.uint32 and p["mask"].shape == (3, 3)
    assert p["mask"][0].tolist() == [(1 << 0) | (1 << 3) | (1 << 31), (1 << 0) | (1 << 1), (1 << 0) | (1 << 5)]
    assert p["mask"][1].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x3F] and p["mask"][2].tolist() == [1 << 5, 0, 0]
    assert p["edge_begin"].tolist() == [0, 3, 3, 4]
    assert p["edge_token"].tolist() == [3, 33, 69, 5] and p["edge_next"].tolist() == [1, DONE, 2, 0]  # ascending within a state, whatever the order of allow()
    assert p["default_next"].tolist() == [0, 1, DONE]
    assert all(p[k].dtype == np.int32 for k in ("edge_begin", "edge_token", "edge_next", "default_next"))
    for s in range(3):
        for t in range(70):
            assert bool((p["mask"][s, t >> 5] >> (t & 31)) & 1) == (a.next_state(s, t) is not None)
    one = TokenAutomaton.any_of(40, [1, 39]).pack()
    assert one["mask"].tolist() == [[2, 1 << 7]] and one["edge_begin"].tolist() == [0, 0] and one["edge_token"].size == 1 and one["default_next"].tolist() == [0]


def _walk(a, seq):
    s, out = a.start, []
    for t in seq:
        s = a.next_state(s, t)
        out.append(s)
        if s is None or s == DONE:
            break
    return out


def test_from_sequences_shared_prefixes_and_a_prefix_of_another():
    a = TokenAutomaton.from_sequences(50, [[7, 8, 9], [7, 8, 10], [7, 11], [12]])
    assert a.states == 3  # the root, "7", "7 8": leaves are DONE
    assert sorted(a.allowed[0]) == [7, 12] and _walk(a, [12]) == [DONE]
    assert _walk(a, [7, 8, 9])[-1] == DONE and _walk(a, [7, 8, 10])[-1] == DONE and _walk(a, [7, 11])[-1] == DONE
    s7 = a.next_state(0, 7)
    assert sorted(a.allowed[s7]) == [8, 11] and sorted(a.allowed[a.next_state(s7, 8)]) == [9, 10]
    assert _walk(a, [7, 9])[-1] is None and _walk(a, [8]) == [None]
    # [1, 2] is a prefix of [1, 2, 3]: the shorter sequence does NOT end -- its last token leads to the state that allows only the continuation
    b = TokenAutomaton.from_sequences(50, [[1, 2], [1, 2, 3], [4]])
    w = _walk(b, [1, 2])
    assert w[-1] not in (None, DONE) and sorted(b.allowed[w[-1]]) == [3] and _walk(b, [1, 2, 3])[-1] == DONE
    assert _walk(TokenAutomaton.from_sequences(50, [[1, 2, 3], [1, 2]]), [1, 2, 3])[-1] == DONE


def test_from_char_dfa_digits():
    """[0-9]+ as a 3-state DFA -- 0: nothing read, 1: digits read (accepting), 2: the trap every other character leads to -- over 12 strings."""
    strings = ["<eos>", "0", "7", "42", "123", "a", "4a", "a4", "", " ", "9", "00"]
    digits = "0123456789"
    tr = {}
    for s in (0, 1):
        for ch in digits:
            tr[(s, ch)] = 1
        for ch in "a ":
            tr[(s, ch)] = 2
    for ch in digits + "a ":
        tr[(2, ch)] = 2
    a = TokenAutomaton.from_char_dfa(strings, tr, 0, [1], eos_id=0)
    numeric = [1, 2, 3, 4, 10, 11]
    assert a.states == 2 and a.start == 0  # the trap is dropped: no token sequence finishes from it
    assert sorted(a.allowed[0]) == numeric and sorted(a.allowed[1]) == [0] + numeric  # <eos> only in the accepting state; "4a", "a4", "" and " " nowhere
    assert all(a.next_state(0, t) == 1 and a.next_state(1, t) == 1 for t in numeric) and a.next_state(1, 0) == DONE and a.next_state(0, 0) is None
    p = a.pack()
    assert p["default_next"].tolist() == [1, 1] and p["edge_token"].tolist() == [0] and p["edge_next"].tolist() == [DONE]  # the frequent next is the default
    with pytest.raises(ValueError):
        TokenAutomaton.from_char_dfa(["<eos>", "a"], tr, 0, [1], eos_id=0)  # nothing leads to an accepting state
    with pytest.raises(ValueError):
        TokenAutomaton.from_char_dfa(strings, tr, 0, [1], eos_id=12)


def _row(seed, vocab=300):
    rng = np.random.default_rng(seed)
    return (np.round(rng.standard_normal(vocab) * 2.5 * 4) / 4).astype(np.float16)  # quarter steps: ties everywhere


@pytest.mark.parametrize("params", [SamplingParams(temp=0.0), SamplingParams(), SamplingParams(top_k=7, top_p=0.8, temp=1.2, repeat_penalty=1.3, alpha_frequency=0.1, alpha_presence=0.2)])
def test_constrained_reference_is_sample_reference_when_everything_is_allowed(params):
    for seed in range(5):
        x = _row(seed)
        recent = np.random.default_rng(100 + seed).integers(0, 300, 64)
        want = sample_reference(x, recent, params, 0.61)
        for allowed, bias in ((None, None), (range(300), []), (list(range(300)) + [300, -1, 5000], None)):
            got = constrained_reference(x, recent, params, 0.61, allowed, bias)
            assert got.keys() == want.keys()
            for k in want:
                assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])) and np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, k


def test_constrained_reference_rules_on_hand_made_rows():
    x = np.array([1.0, 5.0, 3.0, 3.0, -2.0, 4.0, 3.0, 0.5], np.float16)
    g, s = SamplingParams(temp=0.0, repeat_penalty=1.0), SamplingParams(temp=1.0, top_k=3, top_p=1.0, repeat_penalty=1.0)
    # rule 2: a masked token is no candidate whatever its logit; ties go to the lowest allowed id
    assert constrained_reference(x, [], g, 0.0, [0, 2, 3, 6])["token"] == 2
    assert constrained_reference(x, [], g, 0.0, [6, 3])["token"] == 3
    r = constrained_reference(x, [], s, 0.0, [0, 3, 6, 4, 7])
    assert r["ids"].tolist() == [3, 6, 0] and r["logits"].tolist() == [3.0, 3.0, 1.0] and r["n"] == 3 and r["token"] == 3
    # rule 3: fewer allowed tokens than k: k becomes their number
    r = constrained_reference(x, [], s, 0.999, [4, 7])
    assert r["ids"].tolist() == [7, 4] and r["p"].size == 2 and r["token"] == 4
    e = np.exp(np.float32(-2.5))
    assert np.allclose(r["p"], [1 / (1 + e), e / (1 + e)], rtol=1e-6)
    # an allowed token at -inf IS a candidate
    y = x.copy()
    y[[2, 4]] = -np.inf
    assert constrained_reference(y, [], g, 0.0, [4, 2])["token"] == 2
    r = constrained_reference(y, [], s, 0.5, [2, 4, 7])
    assert r["ids"].tolist() == [7, 2, 4] and r["p"].tolist() == [1.0, 0.0, 0.0]
    # rule 1: one fp32 add per pair, before the penalties; twice the same id adds twice, in order; ids outside the row are ignored; at most 16 pairs
    assert constrained_reference(x, [], g, 0.0, None, [(4, 7.5)])["token"] == 4
    b = biased_logits(x, [(0, 0.1), (9, 50.0), (-1, 50.0), (0, 1e8), (0, -1e8)])
    assert b[0] == np.float32(np.float32(np.float32(np.float32(1.0) + np.float32(0.1)) + np.float32(1e8)) + np.float32(-1e8)) and b[0] == 0.0 and b[1:].tolist() == x[1:].tolist()
    assert biased_logits(x, [(7, 1.0)] * 20)[7] == 16.5
    pen = SamplingParams(temp=0.0, repeat_penalty=2.0, alpha_frequency=0.5, alpha_presence=0.25)
    r = constrained_reference(x, [4, 4, 1], pen, 0.0, [4, 0], [(4, 3.0), (0, -0.5)])  # id 4: (-2 + 3) = 1 -> / 2 -> - (2 * 0.5 + 0.25) = -0.75; id 0: 0.5
    assert r["token"] == 0 and r["logits"].tolist() == [0.5]
    r = constrained_reference(x, [4, 4, 1], pen, 0.0, [4], [(4, -1.0)])  # (-2 - 1) = -3 -> * 2 (the negative branch) -> -6 - 1.25
    assert r["logits"].tolist() == [-7.25]
    # rule 6 has no reference result
    with pytest.raises(ValueError):
        constrained_reference(x, [], g, 0.0, [8, 100])


def test_check_bias():
    assert check_bias(None, 10) == [] and check_bias({3: 1.5}, 10) == [(3, 1.5)] and check_bias([(3, 1.0), (3, 2.0)], 10) == [(3, 1.0), (3, 2.0)]
    for bad in ([(i % 10, 1.0) for i in range(17)], {3: float("inf")}, [(3, float("nan"))], {10: 1.0}, {-1: 0.0}):
        with pytest.raises(ValueError):
            check_bias(bad, 10)
