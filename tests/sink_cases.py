"""Attention sinks beside the sliding window (include/tce_matmul.h, "ATTENTION SINKS"): the float64 reference of the definition, and designed cases for it.

    sink_reference_f64   the definition, evaluated in float64 on what the pools hold, with the two binary16 rotations of q made by oracle.rope_half
    window_reference_f64 the same row with the sinks ignored (what a windowed step without sinks computes): what the tests show the sink rows are NOT
    compact_case         a designed attention_cases family laid out for a binding row: the family's keys 0 .. S - 1 become the sinks, its keys S .. S + W - 1 the
                         window -- with the sink keys re-rotated so that the family's scores are what the row sees

Everything here is host code (numpy); the GPU tests share it with tests/test_sink_host.py."""
import numpy as np

import attention_cases as ac

HD = ac.HD
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        from oracle.oracle import Oracle
        _oracle = Oracle()
    return _oracle


def rotate_half(x, cos, sin, row):
    """RotaryPosEmb_cuda_forward's binary16 statement on x fp16 [heads][hd] with cos / sin row `row` (oracle.rope_half: the statement the kernels restate)."""
    x = np.ascontiguousarray(x, np.float16)
    q, _ = oracle().rope_half(x[:, None, :], x[:, None, :], cos, sin, int(row))
    return q[:, 0]


def binds(p, W, S):
    return p >= S + W


def weighed_keys(p, W, S):
    """(sink keys, window keys) of a row at position p: a row that does not bind has no sink keys and the window 0 .. p."""
    if not binds(p, W, S):
        return np.arange(0), np.arange(p + 1)
    return np.arange(S), np.arange(p - W + 1, p + 1)


def sink_reference_f64(q_raw, cos, sin, K_pool_rows, V_pool_rows, p, W, S):
    """The definition in float64.  q_raw fp16 [heads][hd] (the projection's row, not rotated), cos / sin fp16 [positions][hd] or None, K_pool_rows / V_pool_rows fp16
    [heads][>= p + 1][hd]: what the pools hold for keys 0 .. p, repeated per QUERY head (the own key included, as the step appends it).  Keys 0 .. S - 1 are scored
    with q rotated by row S + W - 1, keys lo .. p with q rotated by row p, one softmax over the S + W scores; a row that does not bind: keys 0 .. p, q rotated by
    row p.  attention_cases.reference_f64's clamp rule: a score outside binary16's range becomes -65504 and still takes part."""
    q_raw = np.ascontiguousarray(q_raw, np.float16)
    sk, wk = weighed_keys(p, W, S)
    q_p = rotate_half(q_raw, cos, sin, p) if cos is not None else q_raw
    q_s = rotate_half(q_raw, cos, sin, S + W - 1) if cos is not None and len(sk) else q_raw
    K = np.asarray(K_pool_rows, np.float16).astype(np.float64)
    V = np.asarray(V_pool_rows, np.float16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.concatenate([ac.ALPHA * np.einsum("hd,hkd->hk", q_s.astype(np.float64), K[:, sk]), ac.ALPHA * np.einsum("hd,hkd->hk", q_p.astype(np.float64), K[:, wk])], axis=1)
        s = np.where(np.abs(s) <= ac.HALF_MAX, s, -ac.HALF_MAX)
    s = s - s.max(axis=1, keepdims=True)
    w = np.exp(s)
    w /= w.sum(axis=1, keepdims=True)
    return np.einsum("hk,hkd->hd", w, np.concatenate([V[:, sk], V[:, wk]], axis=1))


def window_reference_f64(q_raw, cos, sin, K_pool_rows, V_pool_rows, p, W):
    """The windowed row WITHOUT sinks: keys max(0, p - W + 1) .. p, q rotated by row p."""
    q_raw = np.ascontiguousarray(q_raw, np.float16)
    q_p = rotate_half(q_raw, cos, sin, p) if cos is not None else q_raw
    lo = max(0, p - W + 1)
    K, V = np.asarray(K_pool_rows, np.float16)[:, lo:p + 1], np.asarray(V_pool_rows, np.float16)[:, lo:p + 1]
    return ac.reference_f64(q_p, K, V)


def _rot64(x, cos_row, sin_row, inverse=False):
    """x [..][hd] rotated by the table row's angles (the pairs (j, j + hd / 2)) in float64; inverse: by minus the angles."""
    c, s = cos_row.astype(np.float64)[: HD // 2], sin_row.astype(np.float64)[: HD // 2]
    if inverse:
        s = -s
    lo, hi = x[..., : HD // 2].astype(np.float64), x[..., HD // 2:].astype(np.float64)
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=-1)


class SinkCase:
    """One row of a sink launch: q_raw fp16 [heads][hd], K / V fp16 [kv_heads][p + 1][hd] as the POOLS hold them (key p: the own row as the step appends it, i.e. the
    rotated k of the q/k/v row and its v), k_raw fp16 [kv_heads][hd] the own row's key before its rotation."""

    def __init__(self, case, q_raw, K, V, k_raw, p, W, S, planted):
        self.case, self.q_raw, self.K, self.V, self.k_raw, self.p, self.W, self.S, self.planted = case, q_raw, K, V, k_raw, p, W, S, planted
        self.heads, self.kv_heads, self.rep = case.heads, case.kv_heads, case.rep

    def qkv_row(self):
        return np.concatenate([self.q_raw.reshape(-1), self.k_raw.reshape(-1), self.V[:, self.p].reshape(-1)])

    def repeated(self):
        return np.repeat(self.K, self.rep, axis=0), np.repeat(self.V, self.rep, axis=0)

    def reference(self, cos, sin, K=None, V=None):
        Kr, Vr = self.repeated() if K is None else (np.repeat(K, self.rep, axis=0), np.repeat(V, self.rep, axis=0))
        return sink_reference_f64(self.q_raw, cos, sin, Kr, Vr, self.p, self.W, self.S)

    def window_only(self, cos, sin):
        Kr, Vr = self.repeated()
        return window_reference_f64(self.q_raw, cos, sin, Kr, Vr, self.p, self.W)


def compact_case(family, heads, kv_heads, p, W, S, cos, sin, seed, e4m3=False, ke=None, ve=0, step=100.0, plant=True, own=None):
    """A designed family for the row at position p (cos / sin: the launch's tables, fp16 numpy).  The family is made for the n keys the row weighs (S + W if it binds,
    else p + 1), as the ROTATED q (row p) and the pool's keys; then
      * the family's keys 0 .. S - 1 go to pool rows 0 .. S - 1 RE-ROTATED by (row S + W - 1) - (row p) in float64, so that q rotated by row S + W - 1 scores them
        as the family's q scores the family's keys (a rotation of both sides of a dot product) -- up to the binary16 rounding of the stored key;
      * its keys S .. S + W - 1 go to pool rows lo .. p;
      * pool rows S .. lo - 1 are Gaussian, and (plant) rows S and lo - 1 hold a DOMINANT key: 60 nats along the pilot under both rotations would be the largest
        score of the row if it were weighed.  It must weigh nothing.
      * q_raw is the family's q un-rotated by row p (attention_cases.unrotate), the own key k_raw likewise.
    e4m3: the pools' contents are rounded to the grid (ke / ve), the dominant plants too.  own: make_case's (`sink_own`: the FAMILY's index of the peak -- S - 1 is
    the last sink, S is pool key lo).
    The float64 reference is always evaluated on what the case HOLDS (sink_reference_f64), so none of the roundings above loosens a check."""
    b = binds(p, W, S)
    n = S + W if b else p + 1
    kw = dict(e4m3=True, ke=ke, ve=ve, step=step) if e4m3 else {}
    case = ac.make_case(family, n, heads, kv_heads, seed=seed, own=own, **kw)
    rng = np.random.default_rng([seed, p, W, S, 77])
    lo = p - W + 1 if b else 0
    K = (rng.standard_normal((kv_heads, p + 1, HD)) * 0.5).astype(np.float16)
    V = (rng.standard_normal((kv_heads, p + 1, HD)) * 0.8).astype(np.float16)
    planted = []
    if b:
        Ks = case.K[:, :S]
        if cos is not None:
            Ks = _rot64(_rot64(Ks, cos[p], sin[p], inverse=True), cos[S + W - 1], sin[S + W - 1]).astype(np.float16)
        K[:, :S], V[:, :S] = Ks, case.V[:, :S]
        K[:, lo:], V[:, lo:] = case.K[:, S:], case.V[:, S:]
        if plant and family not in ac.OUT_OF_RANGE + ("flat", "subnormal_v"):
            # the pilot direction of each kv head, from the family's rotated q: a key 60 / alpha along it (and its image under the sinks' rotation: rows S .. lo - 1
            # would be scored with row p if the lower cut were wrong, with row S + W - 1 if the sink count were)
            d = case.q[0].reshape(kv_heads, case.rep, HD)[:, 0].astype(np.float64) / case.a[0].reshape(kv_heads, case.rep)[:, 0][:, None]
            big = 60.0 * d / (ac.ALPHA * (d * d).sum(axis=1, keepdims=True))
            for key in sorted({S, lo - 1}):
                if S <= key < lo:
                    K[:, key] = big.astype(np.float16)
                    planted.append(key)
    else:
        K[:, :], V[:, :] = case.K, case.V
    if e4m3:
        K, V = ac.on_e4m3_grid(K, case.ke), ac.on_e4m3_grid(V, case.ve)
    if cos is not None:
        q_raw = ac.unrotate(case.q[0], cos[p], sin[p])
        k_raw = ac.unrotate(K[:, p], cos[p], sin[p])
        K[:, p] = rotate_half(k_raw, cos, sin, p)  # what the step will append: the binary16 rotation of the raw row
        if e4m3:
            K[:, p] = ac.on_e4m3_grid(K[:, p], case.ke)
    else:
        q_raw, k_raw = case.q[0].copy(), K[:, p].copy()
    return SinkCase(case, q_raw, K, V, k_raw, p, W, S, planted)
