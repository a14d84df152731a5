"""Pins the column-physics oracle (oracle/column_oracle.c) against every known-answer value the
reference's own tests hold for this path, the survey's 17-digit probe table, and the recorded outputs of
the reference's own header-only leaf functions (tests/golden/ref_leaf_v1.json; live as well where oracle/_ref is built)."""
import json
import os

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
