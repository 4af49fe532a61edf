"""Tail-free and typical sampling per slot, everything that needs no GPU: the new structs' layout, SamplingParams.check in both modes, the new entry points' refusals
before any HIP call, generate._chain against the reference's own results (tests/golden/sampler_stages_golden.npz under the rules of tests/stage_rules.py) and against
every designed case (tests/stage_cases.py), the decidedness cap of every configuration and case, and _chain with (1.0, 1.0) unchanged on the existing fixture."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402
import stage_cases as SC  # noqa: E402
import stage_rules as SR  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return SR.load_fixture()


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_at_most_a_tenth_of_a_configuration_is_undecided(fixture, name):
    """From the fixture alone, before anything of the package runs."""
    rows, by_tfs, by_typ = SR.undecided_counts(name, fixture)
    undecided = sum(1 for r in range(rows) if not all(SR.row_decided(name, r, fixture)))
    print(f"{name}: {rows} rows, undecided by tail-free {by_tfs}, by typical {by_typ}, rows {undecided}")
    assert rows <= 60 and undecided <= SR.MAX_UNDECIDED * rows


def test_struct_sizes_and_the_abi_number():
    from tinychatengine_amd import capi
    assert C.sizeof(capi.StageRow) == 8 and C.sizeof(capi.StageDebug) == 8 + 256 * 4 * 2 == 2056 and C.sizeof(capi.SampleStages) == 16
    assert capi.StageDebug.order.offset == 8 and capi.StageDebug.p_top.offset == 8 + 1024
    assert C.sizeof(capi.SampleRow) == 304 and C.sizeof(capi.SampleCall) == 120  # additive: the existing structs did not move
    from tinychatengine_amd import build as B
    B.build()
    assert capi.lib().tce_version() == capi.TCE_ABI_VERSION == 113


def test_sampling_params_check_in_both_modes():
    from tinychatengine_amd.generate import SamplingParams
    SamplingParams().check(40)
    SamplingParams().check(40, stages=True)
    for kw in (dict(tfs_z=0.95), dict(typical_p=0.9), dict(tfs_z=0.5, typical_p=0.2), dict(tfs_z=2.0)):
        with pytest.raises(ValueError, match="not built"):
            SamplingParams(**kw).check(40)
        SamplingParams(**kw).check(40, stages=True)
    for kw in (dict(mirostat=1), dict(mirostat=2), dict(tfs_z=float("nan")), dict(typical_p=float("nan"))):
        with pytest.raises(ValueError):
            SamplingParams(**kw).check(40, stages=True)
    with pytest.raises(ValueError):
        SamplingParams(top_k=41, tfs_z=0.5).check(40, stages=True)  # the other refusals stay


def test_stage_entry_points_refuse_bad_arguments_before_any_hip_call():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    L = capi.lib()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 15) & ~15

    def call(**kw):
        c = capi.SampleCall(logits=p, ld=128256, vocab=128256, batch=2, top_k_bound=40, rows=p, pos_device=p, pos_bound=63, log_stride=8, next_token=p, out_log=p,
                            workspace=p, n_stop=0, mirostat=0, tfs_z=1.0, typical_p=1.0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def vcall(**kw):
        return capi.SampleVerifyCall(s=call(**kw), rows_per_seq=4, hist_stride=128, row_token=p, row_pos=p, history=p, emitted=p)

    st = lambda rows=p, debug=None: capi.SampleStages(rows=rows, debug=debug)
    for fn, mk in ((capi.sample_stages_f16, call), (capi.sample_verify_stages_f16, vcall)):
        # the stages block's own
        assert fn(mk(), None, None, None, None) == capi.TCE_ERR_BAD_ARG and "tce_sample_stages" in capi.last_error()
        assert fn(mk(), st(rows=None), None, None, None) == capi.TCE_ERR_BAD_ARG
        assert fn(mk(), st(rows=p + 2), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
        assert fn(mk(), st(debug=p + 1), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
        # everything the underlying entry point refuses -- the CALL's tfs_z / typical_p / mirostat included
        for kw in (dict(tfs_z=0.95), dict(typical_p=0.9), dict(mirostat=1), dict(mirostat=2), dict(top_k_bound=257), dict(top_k_bound=0)):
            assert fn(mk(**kw), st(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE, kw
        assert "not built" in capi.last_error() or "top_k_bound" in capi.last_error()
        for field in ("logits", "rows", "pos_device", "next_token", "out_log", "workspace"):
            assert fn(mk(**{field: None}), st(), None, None, None) == capi.TCE_ERR_BAD_ARG, field
        assert fn(mk(logits=p + 2), st(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
        # the constrained and logprob blocks' own, for a non-NULL block
        assert fn(mk(), st(), capi.Constraint(fsms=None, n_fsm=0, rows=None, violations=p), None, None) == capi.TCE_ERR_BAD_ARG
        assert fn(mk(), st(), capi.Constraint(fsms=None, n_fsm=capi.TCE_FSM_MAX + 1, rows=p, violations=p), None, None) == capi.TCE_ERR_BAD_ARG
        assert fn(mk(), st(), None, capi.LogprobOut(out_logprob=None, last_lse=None, partials=p), None) == capi.TCE_ERR_BAD_ARG
        assert fn(mk(), st(), None, capi.LogprobOut(out_logprob=p, last_lse=None, partials=p + 4), None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert L.tce_sample_stages_f16(None, None, None, None, None) == capi.TCE_ERR_BAD_ARG
    assert L.tce_sample_verify_stages_f16(None, None, None, None, None) == capi.TCE_ERR_BAD_ARG
    v = vcall()
    v.rows_per_seq = capi.TCE_SPEC_MAX_ROWS + 1
    assert capi.sample_verify_stages_f16(v, st(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    # the existing entry points go on refusing the call's fields
    assert capi.sample_f16(call(tfs_z=0.95), None) == capi.TCE_ERR_UNSUPPORTED_SHAPE and capi.sample_f16(call(typical_p=0.9), None) == capi.TCE_ERR_UNSUPPORTED_SHAPE


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_chain_against_the_references_own_stages(fixture, name):
    from tinychatengine_amd.generate import draw_reference, sample_reference
    k, sigma, z, typ, rows, seed = SR.CONFIGS[name]
    params = SR.params_of(name)
    decided, worst, points = 0, 0.0, 0
    for r, (logits, recent) in enumerate(SR.config_inputs(name, fixture)):
        x = R.penalised(logits, recent, SR.REPEAT_PENALTY, 0.0, 0.0)
        got = sample_reference(logits, recent, params, 0.5)
        assert int(got["token"]) == int(got["final_ids"][got["choice"]])
        res = SR.check_row(f"{name} row {r}", name, r, fixture, x, got)
        decided += res["decided"]
        worst = max(worst, res["worst"])
        for u, ok in res["draws"]:
            points += 1
            assert draw_reference(got["final_p"], u) in ok, f"{name} row {r}: u = {u!r}"
    print(f"{name}: {decided} of {rows} rows decided, worst relative error {worst:.2e} (tolerance {R.tol(k):.2e}), {points} draw points")
    assert decided >= (1 - SR.MAX_UNDECIDED) * rows


def _params(c):
    from tinychatengine_amd.generate import SamplingParams
    return SamplingParams(**dataclasses.asdict(c.prm))


@pytest.mark.parametrize("name", [c.name for c in SC.cases()])
def test_designed_case(name):
    """The case's own float64 reference says what its design claims (expect), a toleranced case is decided by construction, and generate._chain (through
    constrain.constrained_reference, which adds the mask) returns the reference's cuts, order, n, choice and token exactly and its p within tol(k)."""
    from tinychatengine_amd.constrain import constrained_reference
    c = SC.by_name(name)
    ref = SC.ref_of(c)
    for key, want in c.expect.items():
        have = ref[key].tolist() if hasattr(ref[key], "tolist") else ref[key]
        assert have == want, f"{name}: the design says {key} = {want}, the reference gives {have}"
    if c.kind == "toleranced":
        margins = SC.decided(c, ref)
        print(name, {k: (ref[k] if k in ref else None) for k in ("S", "d_tfs", "d_typ", "gap_s", "d_top_p", "d_u")})
        assert all(margins.values()), f"{name}: not decided by construction: {margins}"
    with np.errstate(all="ignore"):
        got = constrained_reference(c.logits, c.window, _params(c), c.u, allowed=None if c.allowed is None else np.array(c.allowed))
    kk = ref["ids"].size
    assert got["ids"].tolist() == ref["ids"].tolist() and np.array_equal(got["logits"].view(np.uint32), ref["logits"].view(np.uint32))
    for key in ("n_tfs", "n_typ", "n", "choice", "token"):
        assert int(got[key]) == int(ref[key]), f"{name}: {key} = {got[key]}, the reference gives {ref[key]}"
    assert got["order"].tolist() == ref["order"].tolist() and got["final_ids"].tolist() == ref["final_ids"].tolist()
    for key in ("p", "p_top", "final_p"):
        a, b = np.asarray(got[key], np.float64), np.asarray(ref[key], np.float64)
        assert a.shape == b.shape
        if c.kind == "exact":
            assert np.array_equal(np.asarray(got[key], np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)), f"{name}: {key} bits"
        else:
            nz = b > 0
            assert np.all(np.abs(a[nz] - b[nz]) / b[nz] <= R.tol(kk)) and np.all(a[~nz] == 0), f"{name}: {key}"


def test_the_penalty_case_differs_from_its_twin():
    """In the cases' own reference and in generate._chain: the penalty, not the logits, decides which candidates stand behind typical's cut."""
    from tinychatengine_amd.generate import sample_reference
    a, b = SC.ref_of(SC.by_name("penalty_moves_across_the_cut")), SC.ref_of(SC.by_name("penalty_off_twin"))
    assert a["final_ids"].tolist() != b["final_ids"].tolist() and a["n_typ"] != b["n_typ"]
    ca, cb = (sample_reference(c.logits, c.window, _params(c), c.u) for c in (SC.by_name("penalty_moves_across_the_cut"), SC.by_name("penalty_off_twin")))
    assert ca["final_ids"].tolist() == a["final_ids"].tolist() != cb["final_ids"].tolist() == b["final_ids"].tolist() and (ca["n_typ"], cb["n_typ"]) == (a["n_typ"], b["n_typ"])


def test_chain_with_both_stages_off_is_what_it_was():
    """On the existing fixture's rows, _chain at (1.0, 1.0) returns every key it returned before with the values the chain without the stages computes, written out here
    from the module's own unchanged pieces; the new keys say "nothing happened"."""
    from tinychatengine_amd import generate as G
    fx = R.load_fixture()
    for name in ("defaults", "k64_hot", "top_p_off", "greedy"):
        k, top_p, temp, sigma, rp, af, ap, rows, seed = R.CONFIGS[name]
        params = G.SamplingParams(temp=temp, top_k=k, top_p=top_p, repeat_penalty=rp, alpha_frequency=af, alpha_presence=ap)
        for r, (logits, recent) in enumerate(R.config_inputs(name, fx)[:12]):
            got = G.sample_reference(logits, recent, params, 0.37)
            if temp <= 0:
                assert got["token"] == int(fx[name + "/greedy"][r]) and got["n_tfs"] == got["n_typ"] == 1
                continue
            l = got["logits"]
            p = G._softmax_sorted(l)
            n = G.top_p_cut(p, top_p)
            fp = G._softmax_sorted((l[:n] / np.float32(temp)).astype(np.float32))
            choice = G.draw_reference(fp, 0.37)
            assert np.array_equal(got["p"].view(np.uint32), p.view(np.uint32)) and got["n"] == n and np.array_equal(got["final_p"].view(np.uint32), fp.view(np.uint32))
            assert got["choice"] == choice and got["token"] == int(got["ids"][choice])
            assert got["n_tfs"] == got["n_typ"] == k and got["order"].tolist() == list(range(k)) and got["final_ids"].tolist() == got["ids"].tolist()
            assert np.array_equal(got["p_top"].view(np.uint32), p.view(np.uint32))
            R.check_candidates(f"{name} row {r}", R.penalised(logits, recent, rp, af, ap), got["ids"], got["logits"], fx[name + "/ids"][r], fx[name + "/logit"][r])
            assert got["n"] == int(fx[name + "/n"][r]) or R.n_band(fx[name + "/p"][r], top_p, k)[0] != R.n_band(fx[name + "/p"][r], top_p, k)[1]


def test_sampler_without_stages_refuses_non_default_params_at_set_row():
    """set_row's check happens before anything is written or launched: a Sampler object is not even needed to see which mode refuses."""
    from tinychatengine_amd.generate import SamplingParams
    with pytest.raises(ValueError):
        SamplingParams(tfs_z=0.5, typical_p=0.2).check(40, stages=False)
