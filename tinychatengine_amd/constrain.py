"""Constrained decoding: token automata, masks and logit bias for the device-side sampler (include/tce_matmul.h: tce_sample_constrained_f16; csrc/sampling.hip).

Which tokens a sequence may draw next is a TOKEN AUTOMATON: per state a set of allowed tokens (a bit mask over the vocabulary) and, per allowed token, the next state
(an edge, or the state's default) or DONE (the token is emitted, then the sequence retires).  The automaton lives on the device and advances in the sampler's tail, so
a captured graph replay stays one token per live slot with no host round trip.

    TokenAutomaton          the host-side builder: allow / allow_default / check / pack; any_of, from_sequences, from_char_dfa
    constrained_reference   rules 1-3 of tce_sample_constrained_f16 in numpy, on generate.py's own penalties and chain: the CPU-side yardstick
    AutomatonTable          the device side: TCE_FSM_MAX descriptors (tce_fsm) and the arrays they point to; register / unregister

No tokenizer and no regex or JSON-schema compiler: a caller brings the vocabulary's strings and a character DFA (from_char_dfa), or token sequences.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .generate import SamplingParams, _chain, _penalise

DONE = capi.TCE_FSM_DONE


class TokenAutomaton:
    """states x vocab: allow(state, token, next) adds an edge; allow_default(state, tokens, next) allows `tokens` in `state` and sets the state's default -- the next
    state of every allowed token that has no edge (one default per state).  allow(state, token) without a next relies on that default.  next = DONE (-1): the token
    is emitted, then the sequence retires.  start: the state a freshly admitted sequence is in."""

    def __init__(self, vocab: int, states: int, start: int = 0):
        if int(vocab) < 1 or int(states) < 1 or not 0 <= int(start) < int(states):
            raise ValueError("TokenAutomaton: vocab >= 1, states >= 1, 0 <= start < states")
        self.vocab, self.states, self.start = int(vocab), int(states), int(start)
        self.edges: list[dict[int, int]] = [{} for _ in range(self.states)]
        self.allowed: list[set[int]] = [set() for _ in range(self.states)]
        self.default: list[int | None] = [None] * self.states

    def _state(self, state: int) -> int:
        if not 0 <= int(state) < self.states:
            raise ValueError(f"state {state} of {self.states}")
        return int(state)

    def allow(self, state: int, token: int, next: int | None = None) -> "TokenAutomaton":
        s = self._state(state)
        self.allowed[s].add(int(token))
        if next is not None:
            self.edges[s][int(token)] = int(next)
        return self

    def allow_default(self, state: int, tokens, next: int) -> "TokenAutomaton":
        s = self._state(state)
        if self.default[s] is not None and self.default[s] != int(next):
            raise ValueError(f"state {s} already has the default {self.default[s]}")
        self.default[s] = int(next)
        self.allowed[s].update(int(t) for t in tokens)
        return self

    def check(self) -> "TokenAutomaton":
        """Refuses a state with no allowed token, an allowed token without a next state, a next outside [-1, states) and tokens outside the vocabulary."""
        for s in range(self.states):
            if not self.allowed[s]:
                raise ValueError(f"state {s} allows no token")
            bad = [t for t in self.allowed[s] if not 0 <= t < self.vocab]
            if bad:
                raise ValueError(f"state {s}: token {bad[0]} lies outside the vocabulary ({self.vocab})")
            if self.default[s] is None:
                loose = [t for t in self.allowed[s] if t not in self.edges[s]]
                if loose:
                    raise ValueError(f"state {s}: token {min(loose)} is allowed but has no next state")
            for nx in list(self.edges[s].values()) + ([] if self.default[s] is None else [self.default[s]]):
                if not DONE <= nx < self.states:
                    raise ValueError(f"state {s}: next {nx} outside [-1, {self.states})")
        return self

    def next_state(self, state: int, token: int) -> int | None:
        """The transition the device takes (None: the token is not allowed)."""
        if int(token) not in self.allowed[state]:
            return None
        return self.edges[state].get(int(token), self.default[state])

    def pack(self) -> dict:
        """The five arrays of struct tce_fsm: mask uint32 [states][mask_words] (bit t & 31 of word t >> 5; mask_words = ceil(vocab / 32)), edge_begin int32
        [states + 1], edge_token / edge_next int32 [edges] (ascending tokens within a state; one unused entry when there is no edge, so that no array is empty),
        default_next int32 [states] (DONE where the state has none: no allowed token reaches it)."""
        self.check()
        words = (self.vocab + 31) // 32
        mask = np.zeros((self.states, words), np.uint32)
        begin, tok, nxt = [0], [], []
        for s in range(self.states):
            ids = np.fromiter(self.allowed[s], np.int64, len(self.allowed[s]))
            np.bitwise_or.at(mask[s], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
            for t in sorted(self.edges[s]):
                tok.append(t)
                nxt.append(self.edges[s][t])
            begin.append(len(tok))
        return {"mask": mask, "edge_begin": np.asarray(begin, np.int32), "edge_token": np.asarray(tok or [0], np.int32), "edge_next": np.asarray(nxt or [DONE], np.int32),
                "default_next": np.asarray([DONE if d is None else d for d in self.default], np.int32), "states": self.states, "mask_words": words, "start": self.start}

    # ---- constructors ----
    @staticmethod
    def any_of(vocab: int, ids) -> "TokenAutomaton":
        """One looping state that allows exactly `ids`: "only these ids" -- or, with the complement, "ban these ids"."""
        return TokenAutomaton(vocab, 1).allow_default(0, ids, 0).check()

    @staticmethod
    def from_sequences(vocab: int, seqs) -> "TokenAutomaton":
        """A trie over token sequences (a choice, a tool name): state = a proper prefix, a sequence's last token goes to DONE.  A sequence that is a PREFIX OF ANOTHER
        does not end there: its last token leads to the state that allows only the longer sequence's continuation (the automaton cannot express "stop or go on"
        without a token for it; append an end token to both sequences to get that)."""
        seqs = [[int(t) for t in s] for s in seqs]
        if not seqs or any(not s for s in seqs):
            raise ValueError("from_sequences: at least one sequence, none empty")
        children: list[dict[int, int]] = [{}]
        for s in seqs:
            node = 0
            for t in s:
                if t not in children[node]:
                    children.append({})
                    children[node][t] = len(children) - 1
                node = children[node][t]
        inner = [n for n in range(len(children)) if children[n]]  # leaves are DONE, not states
        index = {n: i for i, n in enumerate(inner)}
        a = TokenAutomaton(vocab, len(inner), 0)
        for n in inner:
            for t, c in children[n].items():
                a.allow(index[n], t, index[c] if children[c] else DONE)
        return a.check()

    @staticmethod
    def from_char_dfa(vocab_strings, transitions: dict, start: int, accepting, eos_id: int) -> "TokenAutomaton":
        """The index construction of Willard & Louf ("Efficient guided generation for large language models", 2023; the Outlines library): every token's string is walked
        through the character DFA `transitions` {(state, char): state} from every state; a token whose walk survives is allowed there and leads to the walk's end.
        eos_id is allowed, with next DONE, exactly in the accepting states.  Tokens with an empty string are never allowed.  DFA states from which no accepting
        state can be reached through tokens are dropped together with the tokens that lead into them (a sequence could never finish there); the remaining states
        are renumbered in ascending order.  Per state the most frequent next state becomes the default and the other tokens get edges."""
        strings = [str(s) for s in vocab_strings]
        vocab, eos_id, accepting = len(strings), int(eos_id), {int(s) for s in accepting}
        if not 0 <= eos_id < vocab:
            raise ValueError("from_char_dfa: eos_id outside the vocabulary")
        n = 1 + max([int(start)] + list(accepting) + [int(s) for s, _ in transitions] + [int(v) for v in transitions.values()])
        moves: list[dict[int, int]] = [{} for _ in range(n)]
        for s in range(n):
            for t, text in enumerate(strings):
                if t == eos_id or not text:
                    continue
                cur = s
                for ch in text:
                    cur = transitions.get((cur, ch))
                    if cur is None:
                        break
                if cur is not None:
                    moves[s][t] = int(cur)
        live, grew = set(accepting), True
        while grew:
            grew = False
            for s in range(n):
                if s not in live and any(nx in live for nx in moves[s].values()):
                    live.add(s)
                    grew = True
        if int(start) not in live:
            raise ValueError("from_char_dfa: no token sequence leads from the start state to an accepting state")
        keep = sorted(live)
        index = {s: i for i, s in enumerate(keep)}
        a = TokenAutomaton(vocab, len(keep), index[int(start)])
        for s in keep:
            nexts = [index[nx] for nx in moves[s].values() if nx in live]
            default = max(set(nexts), key=lambda v: (nexts.count(v), -v)) if nexts else None
            for t, nx in moves[s].items():
                if nx not in live:
                    continue
                if index[nx] == default:
                    a.allow_default(index[s], [t], default)
                else:
                    a.allow(index[s], t, index[nx])
            if s in accepting:
                a.allow(index[s], eos_id, DONE)
        return a.check()


def check_bias(logit_bias, vocab: int) -> list[tuple[int, float]]:
    """logit_bias as [(id, value)] (a dict {id: value} or a sequence of pairs, in order; an id may occur twice): refuses more than TCE_BIAS_MAX pairs, a non-finite
    value and an id outside the vocabulary."""
    if logit_bias is None:
        return []
    pairs = [(int(i), float(np.float32(v))) for i, v in (logit_bias.items() if isinstance(logit_bias, dict) else logit_bias)]
    if len(pairs) > capi.TCE_BIAS_MAX:
        raise ValueError(f"logit_bias: {len(pairs)} pairs (at most {capi.TCE_BIAS_MAX})")
    for i, v in pairs:
        if not np.isfinite(v):
            raise ValueError(f"logit_bias: a non-finite value for id {i}")
        if not 0 <= i < vocab:
            raise ValueError(f"logit_bias: id {i} lies outside the vocabulary ({vocab})")
    return pairs


def biased_logits(logits_f16_row: np.ndarray, bias) -> np.ndarray:
    """Rule 1: fp32 logits with the first TCE_BIAS_MAX (id, value) pairs added, one fp32 add each, in index order; ids outside the row are ignored."""
    assert logits_f16_row.dtype == np.float16 and logits_f16_row.ndim == 1
    x = logits_f16_row.astype(np.float32)
    for i, v in list(bias or [])[:capi.TCE_BIAS_MAX]:
        if 0 <= int(i) < x.size:
            x[int(i)] = np.float32(x[int(i)] + np.float32(v))
    return x


def constrained_reference(logits_f16_row: np.ndarray, recent, params: SamplingParams, u, allowed=None, bias=None) -> dict:
    """One row through rules 1-3 of tce_sample_constrained_f16: the bias, then generate.py's penalties on the biased values, then sample_reference's chain over the
    `allowed` ids only (None: every id; ids outside the row are ignored) -- the ids keep their values for penalties and ties.  Returns sample_reference's dict.
    An empty allowed set is rule 6 (nothing is emitted): ValueError."""
    x = _penalise(biased_logits(logits_f16_row, bias), recent, params)
    if allowed is None:
        cand = np.arange(x.size)
    else:
        cand = np.unique(np.asarray(list(allowed), dtype=np.int64).reshape(-1))
        cand = cand[(cand >= 0) & (cand < x.size)]
    if cand.size == 0:
        raise ValueError("constrained_reference: no allowed token inside the vocabulary (rule 6: the row emits nothing)")
    with np.errstate(invalid="ignore"):  # (allowed tokens that are all -inf: expf(-inf - -inf) is NaN here as on the device)
        return _chain(x, cand, params, u)


def constraint_row(fsm: int = -1, state: int = 0, bias=()) -> capi.ConstraintRow:
    r = capi.ConstraintRow(fsm=int(fsm), state=int(state), n_bias=len(bias))
    for j, (i, v) in enumerate(bias):
        r.bias_id[j], r.bias_val[j] = int(i), float(v)
    return r


class AutomatonTable:
    """The device side: TCE_FSM_MAX descriptors (struct tce_fsm) in one device array whose pointer a captured graph keeps, and the arrays they point to.  A free
    entry is all zeros (states = 0), so a row that names it is invalid by the device's rule 6, never followed.  register / unregister write one entry each,
    stream-ordered.  `users` {slot: index} is kept by the Sampler that owns the rows: an entry a row still names cannot be unregistered."""

    def __init__(self, vocab: int, device):
        import torch
        self.vocab, self.device = int(vocab), device
        self.words = C.sizeof(capi.Fsm) // 4
        self.fsms = torch.zeros((capi.TCE_FSM_MAX, self.words), dtype=torch.int32, device=device)
        self.entries: list[dict | None] = [None] * capi.TCE_FSM_MAX
        self.users: dict[int, int] = {}

    def register(self, a: TokenAutomaton) -> int:
        """Uploads the automaton's arrays and writes one descriptor; returns its index (what a row's `fsm` word names)."""
        if a.vocab != self.vocab:
            raise ValueError(f"an automaton over a vocabulary of {a.vocab}, the table's is {self.vocab}")
        return self.register_packed(a.pack(), a)

    def register_packed(self, p: dict, a: TokenAutomaton | None = None) -> int:
        """register for arrays in pack()'s layout that did not go through TokenAutomaton.check (tests of the device's own refusals)."""
        import torch
        free = [i for i, e in enumerate(self.entries) if e is None]
        if not free:
            raise ValueError(f"all {capi.TCE_FSM_MAX} automata are in use (unregister one)")
        dev = {k: torch.from_numpy(np.ascontiguousarray(p[k]).view(np.int32)).to(self.device) for k in ("mask", "edge_begin", "edge_token", "edge_next", "default_next")}
        d = capi.Fsm(mask=dev["mask"].data_ptr(), edge_begin=dev["edge_begin"].data_ptr(), edge_token=dev["edge_token"].data_ptr(), edge_next=dev["edge_next"].data_ptr(),
                     default_next=dev["default_next"].data_ptr(), states=p["states"], mask_words=p["mask_words"], start=p["start"])
        self.fsms[free[0]].copy_(torch.from_numpy(np.frombuffer(bytes(d), dtype=np.int32).copy()))
        self.entries[free[0]] = {"arrays": dev, "start": p["start"], "states": p["states"], "automaton": a}
        return free[0]

    def unregister(self, index: int) -> None:
        if self.entries[index] is None:
            raise ValueError(f"automaton {index} is not registered")
        named = [s for s, i in self.users.items() if i == index]
        if named:
            raise ValueError(f"automaton {index} is still named by the row of slot {named[0]}")
        self.fsms[index].zero_()  # (stream-ordered: launches already enqueued still see the entry and its arrays' memory, which the caching allocator reuses in stream order)
        self.entries[index] = None

    def start(self, index: int) -> int:
        if not 0 <= int(index) < capi.TCE_FSM_MAX or self.entries[index] is None:
            raise ValueError(f"automaton {index} is not registered")
        return self.entries[index]["start"]
