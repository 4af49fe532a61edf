"""Mirostat on the host (no GPU): generate.mirostat_reference -- the numpy fp32 restatement of tce_sample_mirostat_f16's rule -- against the reference's own results
(tests/golden/mirostat_golden.npz) under the rules of tests/mirostat_rules.py and against the float64 restatement of every designed case (tests/mirostat_cases.py); the
undecided cap from the fixture alone; the refusals of SamplingParams.check and of the entry point before any HIP call."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirostat_cases as MC  # noqa: E402
import mirostat_rules as MR  # noqa: E402
import sampling_rules as R  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return MR.load_fixture()


def test_the_fixture_holds_the_configurations_the_rule_is_judged_on():
    c = MR.CONFIGS
    for mode in (1, 2):
        for k in (40, 256):
            assert sum(1 for v in c.values() if v[0] == mode and v[1] == 128256 and v[2] == k) >= 2, (mode, k)  # sharp and flat
        assert any(v[0] == mode and v[1] <= v[2] for v in c.values()), f"mode {mode}: no configuration with vocab <= k (the reference's unmodified chain)"
    for name, v in c.items():  # and the package takes every configuration's parameters
        p = MR.params_of(name)
        p.check(v[2], mirostat_rows=True)
        assert (p.mirostat, p.mirostat_tau, p.mirostat_eta, p.top_k) == (v[0], v[5], v[6], v[2])


@pytest.mark.parametrize("name", list(MR.CONFIGS))
def test_undecided_rows_stay_under_the_cap(fixture, name):
    """From the fixture alone, before anything of the package runs."""
    rows, undecided = MR.undecided_count(name, fixture)
    print(f"{name}: {rows} rows, undecided {undecided}")
    assert rows <= 60 and undecided <= MR.MAX_UNDECIDED * rows


@pytest.mark.parametrize("name", list(MR.CONFIGS))
def test_numpy_rule_against_the_reference(fixture, name):
    from tinychatengine_amd.generate import sample_reference
    prm = MR.params_of(name)
    decided, worst = 0, 0.0
    for r, (logits, recent) in enumerate(MR.config_inputs(name, fixture)):
        x = R.penalised(logits, recent, MR.REPEAT_PENALTY, 0.0, 0.0)
        u, _ = MR.row_u(name, r, fixture)
        got = sample_reference(logits, recent, prm, u, mu=fixture[name + "/mu_in"][r])
        res = MR.check_row(f"{name} row {r}", name, r, fixture, x, got)
        decided += res["decided"]
        worst = max(worst, res["worst"])
    print(f"{name}: {decided} decided rows, worst relative error of a p {worst:.3e} (tol {R.tol(MR.CONFIGS[name][2]):.3e})")
    assert decided >= (1 - MR.MAX_UNDECIDED) * MR.CONFIGS[name][7]


def test_mu_is_carried_as_the_reference_carries_it(fixture):
    """Row r + 1 of a configuration starts from the mu row r ended on, and row 0 from 2 * tau (LLaMA3Generate.cc:163): the fixture's own chain."""
    for name, (mode, vocab, k, sigma, temp, tau, eta, rows, seed) in MR.CONFIGS.items():
        mu_in, mu_out = fixture[name + "/mu_in"], fixture[name + "/mu_out"]
        assert mu_in[0] == np.float32(2.0) * np.float32(tau) and np.array_equal(mu_in[1:].view(np.uint32), mu_out[:-1].view(np.uint32)), name


def _params_of_case(c):
    from tinychatengine_amd.generate import SamplingParams
    prm = SamplingParams(**{f: getattr(c.prm, f) for f in ("temp", "top_k", "top_p", "repeat_penalty", "alpha_frequency", "alpha_presence", "repeat_last_n", "mirostat",
                                                           "mirostat_tau", "mirostat_eta")})
    prm.top_k = min(prm.top_k, c.bound)
    return prm


def _case_result(c):
    from tinychatengine_amd.generate import mirostat_reference, sample_reference
    prm = _params_of_case(c)
    if c.prm.temp <= 0:
        return sample_reference(c.logits, c.window, prm, c.u, mu=c.mu)
    ref = MC.ref_of(c)
    got = mirostat_reference(ref["logits"], prm, c.mu, c.u, c.vocab, m=c.prm.m)
    got["token"] = int(ref["ids"][got["choice"]])
    return got


@pytest.mark.parametrize("name", [c.name for c in MC.cases()])
def test_designed_cases(name):
    """The float64 restatement holds what the design fixes and is decided; the numpy fp32 rule agrees with it."""
    c = MC.by_name(name)
    ref = MC.ref_of(c)
    for key in ("kept", "token"):
        if key in c.expect:
            assert ref[key] == c.expect[key], f"{name}: the design fixes {key} = {c.expect[key]}, the float64 restatement gives {ref[key]}"
    if c.expect.get("nan"):
        assert math.isnan(ref["k_f"])
    if c.expect.get("inf"):
        assert math.isinf(ref["k_f"]) and ref["k_f"] > 0
    assert ref["decided"], f"{name}: the cut is not decided (move mu or the seed)"
    assert ref["d_u"] > 2 * R.tol(c.bound), f"{name}: u lies within the tolerance of an edge of the final CDF"
    got = _case_result(c)
    assert int(got["token"]) == ref["token"]
    if c.prm.temp <= 0:
        return
    assert int(got["kept"]) == ref["kept"] and int(got["choice"]) == ref["choice"]
    t = R.tol(c.bound)
    assert np.abs(np.asarray(got["p"], np.float64) / ref["p"] - 1).max() <= t and np.abs(np.asarray(got["final_p"], np.float64) / ref["final_p"] - 1).max() <= t
    assert abs(float(got["mu_out"]) - ref["mu_out"]) <= MC.mu_bound(c, ref)
    if c.prm.mirostat == 1:
        if math.isnan(ref["k_f"]):
            assert math.isnan(float(got["k_f"]))
        elif math.isinf(ref["k_f"]):
            assert math.isinf(float(got["k_f"]))


def test_equal_logits_fall_on_one_side_of_the_cut():
    """Six equal logits around the v2 cut: bit-equal p and surprise in the numpy rule, so all six stay or all six go."""
    from tinychatengine_amd.generate import mirostat_reference
    kept = {}
    for name in ("equal_logits_inside_v2", "equal_logits_outside_v2"):
        c = MC.by_name(name)
        ref = MC.ref_of(c)
        got = mirostat_reference(ref["logits"], _params_of_case(c), c.mu, c.u, c.vocab, m=c.prm.m)
        assert len(set(np.asarray(got["p"][4:10]).view(np.uint32).tolist())) == 1 and len(set(ref["logits"][4:10].tolist())) == 1
        kept[name] = (int(got["kept"]), ref["kept"])
    assert kept == {"equal_logits_inside_v2": (10, 10), "equal_logits_outside_v2": (4, 4)}


def test_sampling_params_check_with_and_without_the_flag():
    from tinychatengine_amd.generate import SamplingParams
    assert (SamplingParams().mirostat_tau, SamplingParams().mirostat_eta) == (5.0, 0.1)  # the reference's defaults (Generate.h:70-71)
    for mode in (1, 2):
        for kw in (dict(), dict(stages=True)):
            with pytest.raises(ValueError, match="not built"):
                SamplingParams(mirostat=mode).check(40, **kw)
        SamplingParams(mirostat=mode).check(40, stages=True, mirostat_rows=True)
        SamplingParams(mirostat=mode, tfs_z=0.9).check(40, mirostat_rows=True)  # the flag implies stages, as in Sampler
        SamplingParams(mirostat=mode, mirostat_tau=0.0, mirostat_eta=0.0, tfs_z=0.9).check(40, stages=True, mirostat_rows=True)
    SamplingParams().check(40, stages=True, mirostat_rows=True)
    for kw in (dict(mirostat=3), dict(mirostat=-1), dict(mirostat=1, mirostat_tau=float("nan")), dict(mirostat=2, mirostat_tau=float("inf")),
               dict(mirostat=1, mirostat_eta=float("nan")), dict(mirostat=2, mirostat_eta=-0.1), dict(mirostat=1, top_k=41), dict(mirostat=2, top_k=0),
               dict(mirostat=1, tfs_z=float("nan"))):
        with pytest.raises(ValueError):
            SamplingParams(**kw).check(40, stages=True, mirostat_rows=True)


def test_struct_sizes():
    from tinychatengine_amd import capi
    from tinychatengine_amd.generate import SamplingParams, make_mirostat_row
    assert C.sizeof(capi.MirostatRow) == 20 and C.sizeof(capi.MirostatDebug) == 40 and C.sizeof(capi.SampleMirostat) == 16
    assert C.sizeof(capi.SampleRow) == 304 and C.sizeof(capi.SampleCall) == 120 and C.sizeof(capi.StageRow) == 8  # additive: the existing structs did not move
    r = make_mirostat_row(SamplingParams(mirostat=2, mirostat_tau=3.5, mirostat_eta=0.25))
    assert (r.mode, r.m, r.tau, r.eta, r.mu) == (2, 100, 3.5, 0.25, 7.0)


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
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

    st = lambda rows=p, debug=None: capi.SampleStages(rows=rows, debug=debug)
    mi = lambda rows=p, debug=None: capi.SampleMirostat(rows=rows, debug=debug)
    fn = capi.sample_mirostat_f16
    assert fn(call(), st(), None, None, None, None) == capi.TCE_ERR_BAD_ARG and "tce_sample_mirostat" in capi.last_error()
    assert fn(call(), st(), mi(rows=None), None, None, None) == capi.TCE_ERR_BAD_ARG
    assert fn(call(), st(), mi(rows=p + 2), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert fn(call(), st(), mi(debug=p + 1), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert fn(call(), None, mi(), None, None, None) == capi.TCE_ERR_BAD_ARG and "tce_sample_stages" in capi.last_error()  # the stage block is required
    assert fn(call(), st(rows=None), mi(), None, None, None) == capi.TCE_ERR_BAD_ARG
    # the CALL's mirostat stays refused here too: the mode lives per row
    for kw in (dict(mirostat=1), dict(mirostat=2), dict(tfs_z=0.95), dict(typical_p=0.9), dict(top_k_bound=257), dict(top_k_bound=0)):
        assert fn(call(**kw), st(), mi(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE, kw
    for field in ("logits", "rows", "pos_device", "next_token", "out_log", "workspace"):
        assert fn(call(**{field: None}), st(), mi(), None, None, None) == capi.TCE_ERR_BAD_ARG, field
    assert fn(call(), st(), mi(), capi.Constraint(fsms=None, n_fsm=0, rows=None, violations=p), None, None) == capi.TCE_ERR_BAD_ARG
    assert fn(call(), st(), mi(), None, capi.LogprobOut(out_logprob=None, last_lse=None, partials=p), None) == capi.TCE_ERR_BAD_ARG
    assert L.tce_sample_mirostat_f16(None, None, None, None, None, None) == capi.TCE_ERR_BAD_ARG
    # the verifier form: the verifier's refusals, then the same two blocks
    vcall = lambda **kw: capi.SampleVerifyCall(s=call(**kw), rows_per_seq=4, hist_stride=128, row_token=p, row_pos=p, history=p, emitted=p)
    vfn = capi.sample_verify_mirostat_f16
    assert vfn(vcall(), st(), None, None, None, None) == capi.TCE_ERR_BAD_ARG and "tce_sample_mirostat" in capi.last_error()
    assert vfn(vcall(), None, mi(), None, None, None) == capi.TCE_ERR_BAD_ARG
    assert vfn(vcall(), st(), mi(rows=p + 2), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert vfn(vcall(mirostat=2), st(), mi(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "not built" in capi.last_error()
    v = vcall()
    v.rows_per_seq = capi.TCE_SPEC_MAX_ROWS + 1
    assert vfn(v, st(), mi(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert L.tce_sample_verify_mirostat_f16(None, None, None, None, None, None) == capi.TCE_ERR_BAD_ARG
    base, mine = L.tce_sample_verify_workspace_bytes(3, 4, 128256), L.tce_sample_verify_mirostat_workspace_bytes(3, 4, 128256)
    assert base > 0 and mine == base + 3 * 4 * 2064  # the verifier's, then kk, mu and the sorted candidates per virtual row
    assert L.tce_sample_verify_mirostat_workspace_bytes(3, capi.TCE_SPEC_MAX_ROWS + 1, 128256) == 0 and L.tce_sample_verify_mirostat_workspace_bytes(0, 4, 128256) == 0
    # the existing entry points go on refusing the call's field
    assert capi.sample_stages_f16(call(mirostat=2), st(), None, None, None) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "not built" in capi.last_error()
    assert capi.sample_f16(call(mirostat=1), None) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "not built" in capi.last_error()
    assert L.tce_version() == capi.TCE_ABI_VERSION == 113  # additive within the ABI number, as every added sampler entry point has been
