"""Pins the column-physics oracle (oracle/column_oracle.c) bit for bit to the reference's own column step, recorded case by
case (tests/golden/ref_column_v1.npz), and to every known-answer value the reference's own tests hold for this path, the
survey's 17-digit probe table and the recorded outputs of the reference's own header-only leaf functions
(tests/golden/ref_leaf_v1.json).  Where oracle/_ref is built, both recordings are also recomputed live."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "column_known_answers.json")))


def run_case(case):
    pk = dict(case["params"])
    params = O.column_params(**pk)
    inp = case["inputs"]
    state = {k: np.array([inp[k]], dtype=np.float64) for k in O.STATE}
    forcing = {k: np.array([inp[k]], dtype=np.float64) for k in O.FORCING}
    newice = np.array([inp["newice"]], dtype=np.float64)
    diag = O.column_step(params, case["dt"], state, forcing, newice, want_diag=True)
    got = {k: float(v[0]) for k, v in diag.items()}
    got.update({k: float(v[0]) for k, v in state.items()})
    got["newice"] = float(newice[0])
    return got


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_known_answers(case):
    got = run_case(case)
    for key, (want, rtol) in case["expect"].items():
        # Catch2 Approx(x).epsilon(e): |got - want| <= e * |want| (plus its tiny default margin)
        assert abs(got[key] - want) <= rtol * abs(want) + 1e-300 + (1e-12 if want == 0.0 and rtol > 0 else 0.0), \
            (case["name"], key, got[key], want)


def test_config_defaults_match_reference():
    # physics/test/NextsimPhysics_test.cpp:21-45 exercises min_conc/min_thick/I_0 overrides;
    # defaults: NextsimPhysics.cpp:76-82, ThermoIce0.cpp:30-31, HiblerConcentration.cpp:28-29
    p = O.column_params()
    assert (p.drag_ocean_q, p.drag_ocean_t, p.drag_ice_t) == (1.5e-3, 0.83e-3, 1.3e-3)
    assert (p.ocean_albedo, p.i0, p.min_conc, p.min_thick) == (0.07, 0.17, 1e-12, 0.01)
    assert (p.ks, p.flooding, p.h0, p.phi_m) == (0.3096, 1, 0.25, 0.5)
    assert (p.ccsm_ice_albedo, p.ccsm_snow_albedo) == (0.538, 0.8256)
    assert (p.albedo_kind, p.freezing_kind) == (0, 0)
    q = O.column_params(min_conc=2e-12, min_thick=0.02, i0=0.18)
    assert (q.min_conc, q.min_thick, q.i0) == (2e-12, 0.02, 0.18)


def test_no_ice_branch():
    # intent of the stale physics/test/ThermoIce0_test.cpp:41-43: no ice in => hi = hs = 0 and
    # T = -mu * s_ice (ThermoIce0.cpp:45-51)
    case = dict(GOLD["cases"][0])
    case = json.loads(json.dumps(case))
    case["inputs"].update(hice=0.0, cice=0.0, hsnow=0.0, sst=5.0, tair=10.0)
    got = run_case(case)
    assert got["hice"] == 0.0 and got["hsnow"] == 0.0 and got["cice"] == 0.0
    assert got["tice0"] == -0.055 * 5


def test_against_reference_leaf_build():
    """LinearFreezing.hpp / UnescoFreezing.hpp / constants.hpp of the reference, compiled by oracle/ref_leaf_driver.cpp:
    their outputs are recorded in tests/golden/ref_leaf_v1.json (tools/gen_ref_leaf_golden.py), and where oracle/_ref is
    built the live library must still produce the recording.  Bit-exact agreement is required (same expressions, same libm)."""
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_leaf_v1.json")))
    h = lambda xs: [float.fromhex(x) for x in xs]
    sss, linear, unesco = h(gold["sss"]), h(gold["freezing_linear"]), h(gold["freezing_unesco"])
    consts = h(c["value"] for c in gold["constants"])
    assert sss == [float(s) for s in np.random.default_rng(7).uniform(0, 45, 200)] + [0.0, 32.0, 35.0]
    L = O.lib()
    for s, fl, fu in zip(sss, linear, unesco):
        assert L.oracle_freezing_point(0, s) == fl, s
        assert L.oracle_freezing_point(1, s) == fu, s
    want = [5.670374419e-8, 2100., 0.996, 2.0334, 333.55e3, 917., 330., 5., 273.15, 1004.64, 287.058,
            1860., 2500.79e3, 461.5, 4186.84, 333.55e3, 0.055, 1025., 273.15, 273.15]
    assert consts == want
    R = O.ref_leaf()
    if R is not None:
        for s, fl, fu in zip(sss, linear, unesco):
            assert R.ref_freezing_linear(s) == fl and R.ref_freezing_unesco(s) == fu, s
        for k, w in enumerate(want):
            assert R.ref_constant(k) == w, k


def test_newice_carry_over_quirk():
    # SURVEY.md A.7 quirk 1 (NextsimPhysics.cpp:244-253): m_newice is only assigned inside
    # `if (t1 < tf)` and is re-used by lateralGrowth on later steps.
    params = O.column_params(freezing="unesco")
    inp = GOLD["cases"][1]["inputs"]
    state = {k: np.array([inp[k]]) for k in O.STATE}
    forcing = {k: np.array([inp[k]]) for k in O.FORCING}
    newice = np.zeros(1)
    O.column_step(params, 86400.0, state, forcing, newice)
    first = newice[0]
    assert first > 0
    forcing["sst"][:] = 5.0  # warm ocean: no new ice can form, value must persist
    forcing["tair"][:] = 10.0
    O.column_step(params, 600.0, state, forcing, newice)
    assert newice[0] == first


def test_dev1_cfg_grid():
    # BASELINE config 1: 10x10 identical elements, one iterate(1); x-major linear index i*nx+j
    # (core/src/DevGridIO.cpp:107-109) is irrelevant for identical elements but the loop runs all 100.
    case = [c for c in GOLD["cases"] if c["name"] == "dev1_cfg"][0]
    n = 100
    params = O.column_params()
    state = {k: np.full(n, case["inputs"][k]) for k in O.STATE}
    forcing = {k: np.full(n, case["inputs"][k]) for k in O.FORCING}
    newice = np.zeros(n)
    O.column_step(params, 1.0, state, forcing, newice)
    for key, (want, rtol) in case["expect"].items():
        assert np.all(np.abs(state[key] - want) <= rtol * abs(want))
    assert np.all(forcing["sst"] == -1.0)


# ---- the reference's own column physics, recorded case by case (tests/golden/ref_column_v1.npz,
#      tools/gen_ref_column_golden.py, oracle/ref_column_driver.cpp)

RC_META, RC = O.ref_column_fixture()
RC_GROUPS = [(g["set"], g["group"]) for g in RC_META["groups"]]


def rc_params(name, **override):
    """the recorded set's ColumnParams, with single fields replaced"""
    p = O.column_params(**O.ref_column_set_params(RC_META, name))
    for k, v in override.items():
        setattr(p, k, v)
    return p


def rc_run_oracle(name, group, params=None):
    """The oracle over one recorded group, step by step from the recorded inputs: final state, newice, last-step diagnostics,
    and for chains the state + newice after every step (planes as the fixture's record)."""
    g = next(x for x in RC_META["groups"] if (x["set"], x["group"]) == (name, group))
    ikey = g["inputs"] + "in/"  # the random draw and the chain are shared by every set
    state = {k: RC[ikey + k].copy() for k in O.STATE}
    newice = np.zeros(state["hice"].size)
    rec, diag = [], None
    for s in range(g["nsteps"]):
        forcing = {k: np.ascontiguousarray(RC[ikey + k][s] if g["nsteps"] > 1 else RC[ikey + k]) for k in O.FORCING}
        diag = O.column_step(params or rc_params(name), g["dt"], state, forcing, newice, want_diag=True)
        rec.append(np.stack([state[k].copy() for k in O.STATE] + [newice.copy()]))
    return state, newice, diag, np.stack(rec)


def bits_differ(got, want):
    """entries whose float64 bit patterns differ, NaN matching NaN whatever its payload"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return (got.view(np.int64) != want.view(np.int64)) & ~both_nan


def rc_mismatches(name, group, params=None):
    key = "%s/%s/" % (name, group)
    state, newice, diag, rec = rc_run_oracle(name, group, params)
    out = {k: bits_differ(state[k], RC[key + "out/" + k]) for k in O.STATE}
    out["newice"] = bits_differ(newice, RC[key + "out/newice"])
    out.update({"diag " + k: bits_differ(diag[k], RC[key + "out/diag"][i]) for i, k in enumerate(O.DIAG)})
    if key + "out/record" in RC:
        out["record"] = bits_differ(rec, RC[key + "out/record"])
    return out


@pytest.mark.parametrize("name,group", RC_GROUPS, ids=["%s-%s" % g for g in RC_GROUPS])
def test_oracle_matches_reference_column_build(name, group):
    """The oracle reproduces the reference's own column step bit for bit on every recorded case: state, newice, all 15
    diagnostics (every one has a reference counterpart, oracle/ref_column_driver.cpp) and, for chains, every step.  Both
    sides evaluate the same expressions in the same order with the same libm and contraction off; there are no exceptions."""
    bad = {k: int(v.sum()) for k, v in rc_mismatches(name, group).items() if v.any()}
    assert not bad, bad


# every ColumnParams value of the all_params set differs from its default, and resetting any single one of them changes what
# the oracle computes on the recorded cases: the fixture checks the wiring of each parameter (ALL of them: the h0 latch in
# the reference is why each set was recorded in its own process, tools/gen_ref_column_golden.py)
RC_PARAMS = ["drag_ocean_q", "drag_ocean_t", "drag_ice_t", "ocean_albedo", "i0", "min_conc", "min_thick", "ks", "h0", "phi_m",
             "ccsm_ice_albedo", "ccsm_snow_albedo"]


@pytest.mark.parametrize("field", RC_PARAMS)
def test_reference_column_fixture_pins_each_parameter(field):
    default = getattr(O.column_params(), field)
    assert getattr(rc_params("all_params"), field) != default
    changed = False
    for name, group in RC_GROUPS:
        if name == "all_params":
            changed |= any(v.any() for v in rc_mismatches(name, group, rc_params(name, **{field: default})).values())
    assert changed, field


def test_reference_column_fixture_reaches_the_branches():
    """The recorded cases take the branches the column step has, not only its middle."""
    meta_sets = RC_META["sets"]
    assert set(meta_sets) == {"default", "unesco_ccsm", "smu2_noflood", "all_params"} and "h0" in RC_META["h0_latch"]
    assert (meta_sets["unesco_ccsm"]["freezing_kind"], meta_sets["unesco_ccsm"]["albedo_kind"]) == (1, 2)
    assert (meta_sets["smu2_noflood"]["albedo_kind"], meta_sets["smu2_noflood"]["flooding"]) == (1, 0)
    for name in meta_sets:
        k = name + "/edge/"
        cin, cout = RC[k + "in/cice"], RC[k + "out/cice"]
        d = dict(zip(O.DIAG, RC[k + "out/diag"]))
        assert np.any((cin == 0) & (RC[k + "out/newice"] > 0)), name  # new ice in open water
        assert np.any((cin > 0) & (cin < 1) & (cout == 0)), name  # melts away / cut below min_conc, min_thick
        assert np.any((cin > 0) & (cout > cin)), name  # lateral growth
        assert np.any(RC[k + "out/hsnow"] > 0) and np.any(np.isnan(RC[k + "out/hice"])), name
        if meta_sets[name]["flooding"]:
            assert np.any(d["hifroms"] > 0), name  # snow-ice from flooding
        else:
            assert not np.any(d["hifroms"] > 0), name
    for dt in ("1", "86400"):
        assert np.any(RC["default/edge_dt%s/out/cice" % dt] != RC["default/edge_dt%s/in/cice" % dt])
    # the chain carries m_newice over a step that forms none (NextsimPhysics.cpp:244-253 assigns it only when t1 < tf)
    for name in meta_sets:
        ni = RC[name + "/chain/out/record"][:, 4]
        assert np.any((ni[1:] == ni[:-1]) & (ni[1:] > 0)), name


def test_reference_column_build_reproduces_fixture():
    """Where oracle/_ref/libref_column.so is built, the live reference still produces the recording (each set in its own
    process, as recorded)."""
    if O.ref_column() is None:
        return  # the fixture checks above run everywhere; this one needs the reference's sources at build time
    tool = os.path.join(O.ROOT, "tools", "gen_ref_column_golden.py")
    r = subprocess.run([sys.executable, tool, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
