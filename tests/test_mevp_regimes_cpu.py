"""The mEVP sub-iteration at every seam and regime, without a GPU: the vectorised restatement tests/mevp_ref.py against the committed
outputs of the pure-Python restatement on its 6 x 5 case; every case of tests/mevp_cases.py held to the condition it is there for, to its
margins and to its conditioning, on the reference alone; and oracle/dyn_oracle.c held to the restatement on every case -- helpers and one
sub-iteration, row ranges included -- under the bound the device is held to in tests/test_gpu_mevp_regimes.py.

The condition of each kind, from the reference's diag (Gauss points and nodes of the sea, at 70 x 9):

  plastic     Delta / delta_min >= 100 at >= 90 % of the Gauss points; alpha != beta
  transition  1.1 <= Delta / delta_min <= 10 at >= 50 % of the points
  viscous     Delta / delta_min <= 1.001 at every point
  rest        u = v = u0 = v0 = 0 and S != 0; |v_o - v| == 0 at >= 5 % of the interior nodes and > 0 at others
  params      plastic; every parameter differs from its default, and resetting any ONE of them moves the reference by more than 100 times
              the comparison bound in at least one output array (test_params_kind_feels_every_parameter)
  clamps      a share > 0 of h < 0, a < 0 and a > 1 at the Gauss points (the strength) and of a < 0, a > 1, h < h_min at the nodes
  icefree     every trigger of the ice-free rule decides alone at >= 1 node; ice-free nodes on both sides of the seams after columns 57
              and 63 and on the first and last node row that moves
  ad_floor    alpha_e == alpha_min everywhere
  ad_spread   max alpha_e / min alpha_e > 2; alpha_e > alpha_min at >= 30 % of the elements; beta_n taken from an element's offer (not
              from alpha_min) at >= 10 % of the nodes
  ad_icefree  icefree, and: ice-free centre nodes with alpha_e == alpha_min, ice-free nodes with beta_n == alpha_min, at least one node
              with ice whose beta_n exceeds 5 alpha_min AND 1.5 times the largest alpha_e around it (a light node beside a strong element)
  drift       Delta / delta_min <= 3 everywhere on ice that moves at 0.1 m/s

Margins: every threshold decision -- the three triggers of the ice-free rule, the clamps of h and a at the Gauss points and of a and h at
the nodes, alpha_e against alpha_min, the offer beta_n takes against the next one -- lies at least 1e-6 (relative) off its threshold, but
for entries exactly ON it (the zeros of a patch of zeros, equal in every arithmetic)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mevp_cases as B  # noqa: E402
import mevp_ref as R  # noqa: E402
import oracle_lib as O  # noqa: E402


def test_restatement_reproduces_the_6x5_fixture():
    """tests/golden/dyn_independent_v3.npz holds what the loops of tests/dyn_independent.py give on their 6 x 5 case (clamps, a node
    under h_min, ice-free nodes, hx != hy); mevp_ref gives the same to 1e-12 of each array's largest value, the bound the oracle is held
    to there -- uniform and adaptive, every element's alpha included.  The fixture is read, the loops are not run"""
    import dyn_independent as D

    fix = np.load(os.path.join(HERE, "golden", "dyn_independent_v3.npz"))
    I, W, c = (lambda k: fix["in_" + k]), (lambda k: fix["out_" + k]), D.CASE
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    worst = {}
    for pre, extra in (("", {}), ("ad_", D.ADAPTIVE)):
        p, diag = R.par(**dict(D.PARAMS, **extra)), {}
        prep = R.prepare(p, I("H"), I("A"), I("ua"), I("va"), I("uo"), I("vo"))
        S, u, v = R.iterate(p, c["hx"], c["hy"], c["dt"], list(I("S")), I("u"), I("v"), I("u0"), I("v0"), prep, diag=diag)
        got = {pre + "s11": S[0], pre + "s12": S[1], pre + "s22": S[2], pre + "u_new": u, pre + "v_new": v}
        if extra:
            got["ad_alpha"] = diag["alpha_e"]
        else:
            got.update(pg=prep["pg"], cgh=prep["cgh"], cga=prep["cga"], tax=prep["tax"], tay=prep["tay"])
        worst.update({k: rel(x, W(k)) for k, x in got.items()})
    print("largest |difference| / largest value: " + ", ".join("%s %.2g" % kv for kv in worst.items()))
    assert len(worst) == 16 and max(worst.values()) < 1e-12, worst


def conditioning(case, ref, wide):
    """per output array the largest |float64 - longdouble| / comparison bound; for the ice-free kinds the nodes with ice once more under
    the floor of their own maximum, as the device test compares them"""
    a, b = B.outputs(ref), B.outputs(wide)
    assert all(x.dtype == np.longdouble for x in b.values())
    worst = {k: float(np.max(np.abs(a[k] - b[k]) / B.tolerance(k, a[k]))) for k in B.OUTPUTS}
    if case["kind"] in ("icefree", "ad_icefree"):
        ice = ~B.ice_free_nodes(case, ref)
        for k in ("u", "v"):
            worst[k + " (ice)"] = float(np.max((np.abs(a[k] - b[k]) / B.tolerance(k, a[k], a[k][ice]))[ice]))
    return worst


@pytest.mark.parametrize("key", B.ALL_CASES, ids=B.case_id)
def test_case_holds_its_condition_margins_and_conditioning(key):
    """every (kind, shape, mask) of tests/test_gpu_mevp_regimes.py on the reference alone: (a) at 70 x 9 the condition of the kind's row
    in the table above; (b) the margins; (c) the float64 reference agrees with its own evaluation in longdouble within a quarter of the
    bound the device is held to, so an error above that bound is the kernel's.  drift is the exception to (c) by construction: its strain
    rate is a difference of nearly equal velocities, whose error of about zeta 2^-53 |u| / h is not small against 1e-12 of the stress;
    its stress must MISS the quarter (or it would need no bound of its own) and its velocity hold it"""
    case, ref = B.built(key)
    kind, nx, ny = key[:3]
    if (nx, ny) == (70, 9):
        s = B.check_condition(case, ref)
        print("shares: " + ", ".join("%s %.4g" % kv for kv in s.items()))
    B.assert_margins(case, ref, B.case_id(key))
    worst = conditioning(case, ref, B.reference(case, np.longdouble))
    print("float64 against longdouble, worst |difference| / bound: " + ", ".join("%s %.4f" % kv for kv in worst.items()))
    if kind == "drift":
        assert max(worst[k] for k in ("s11", "s22")) > 0.25 and max(worst[k] for k in ("u", "v")) <= 0.25, worst
    else:
        assert max(worst.values()) <= 0.25, worst


def test_params_kind_feels_every_parameter():
    """params: with any ONE of its parameters (hy too) back at the default, the reference moves by more than 100 times the comparison
    bound in at least one output array -- a literal in place of that parameter cannot pass the device test"""
    key = B.KIND_CASES[B.KINDS.index("params")]
    case, ref = B.built(key)
    want = B.outputs(ref)
    base, moved = R.par(), {}
    for name in list(B.PARAMS) + ["hy"]:
        if name == "hy":
            other = B.reference(case, hy=case["hx"])
        else:
            other = B.reference(case, par=R.par(**dict(case["par"], **{name: base[name]})))
        got = B.outputs(other)
        moved[name] = max(float(np.max(np.abs(got[k] - want[k]) / B.tolerance(k, want[k]))) for k in B.OUTPUTS)
    print("largest move / bound with one parameter at its default: " + ", ".join("%s %.3g" % kv for kv in moved.items()))
    assert len(moved) == 13 and min(moved.values()) > 100.0, moved


def test_drift_bound_is_the_recorded_one():
    """drift: the device is compared with the longdouble evaluation rounded to float64, under 4 times the distance of the float64
    reference from it, per array.  The distances are measured here and kept in tests/golden/mevp_drift_bounds.json, which the device test
    reads; this test writes the file where it is missing (or NSDG_RECORD_DRIFT_BOUNDS is set) and otherwise holds the file to a fresh
    measurement within a factor 2 (exp of another libm may round the ice strength another way)"""
    key = B.KIND_CASES[B.KINDS.index("drift")]
    case, ref = B.built(key)
    dist = B.drift_distances(ref, B.reference(case, np.longdouble))
    want = B.outputs(ref)
    print("drift: distance float64 - longdouble per array, as a share of the largest value, and in units of the ordinary bound's floor")
    for k in B.OUTPUTS:
        top = float(np.max(np.abs(want[k])))
        print("  %s %.3e (%.3e of %.4g; %.2f floors); bound %.3e" % (k, dist[k], dist[k] / top, top, dist[k] / float(np.min(B.tolerance(k, want[k]))), B.DRIFT_FACTOR * dist[k]))
    if not os.path.exists(B.DRIFT_JSON) or os.environ.get("NSDG_RECORD_DRIFT_BOUNDS"):
        with open(B.DRIFT_JSON, "w") as f:
            json.dump(dict(case=B.case_id(key), seed=B.SEED, factor=B.DRIFT_FACTOR, distance=dist), f, indent=1, sort_keys=True)
            f.write("\n")
    rec = json.load(open(B.DRIFT_JSON))["distance"]
    for k in B.OUTPUTS:
        assert 0.5 * rec[k] <= dist[k] <= 2.0 * rec[k] and dist[k] > 0.0, (k, rec[k], dist[k])
    bounds = B.drift_bounds()
    # the bound stays a statement about round-off: under 1e-9 of the stress scale and 1e-12 of the velocity scale
    assert max(bounds[k] for k in ("s11", "s12", "s22")) < 1e-9 * np.max(np.abs(want["s11"])) and max(bounds["u"], bounds["v"]) < 1e-12 * np.max(np.abs(want["u"]))


# ---- the oracle against the restatement ---------------------------------------------------------------------------------------------------
def assert_close(got, want, rtol, atol, what):
    err, lim = np.abs(got - want), atol + rtol * np.abs(want)
    assert np.all(err <= lim), "%s: worst |difference| / bound %.3g" % (what, float(np.max(err / lim)))
    return float(np.max(err / np.maximum(lim, 1e-300)))


def oracle_iterate(case, k0=0, j0=0, j1=None):
    """the case through oracle/dyn_oracle.c: dict(pg, cgh, cga, tax, tay, S, u, v, alpha_e) with the row ranges of nsdg_mevp_iterate;
    land as tests/land_ref.py states it (land nodes zeroed after the sub-iteration)"""
    c, nx, ny = case["c"], case["c"]["nx"], case["c"]["ny"]
    j1 = ny if j1 is None else j1
    po = O.mevp_params(**case["par"])
    ln = B.land_of(case)
    ua, va = (np.ascontiguousarray(np.where(ln, 0.0, c[k]) if ln is not None else c[k]) for k in ("ua", "va"))
    out = dict(pg=O.ice_strength(nx, ny, po, c["H"], c["A"]), cgh=O.dg_to_cg(nx, ny, c["H"]), cga=O.dg_to_cg(nx, ny, c["A"]))
    out["tax"], out["tay"] = O.wind_stress(po, ua, va)
    s = [x.copy() for x in c["S"]]
    alpha_e = np.zeros((ny, nx)) if po.aevp_c > 0 else None
    O.mevp_stress(nx, ny, k0, j1, case["hx"], case["hy"], po, c["u"], c["v"], out["pg"], *s, dt=case["dt"], cgh=out["cgh"], cga=out["cga"], alpha_e=alpha_e)
    un, vn = c["u"].copy(), c["v"].copy()
    O.mevp_velocity(nx, ny, j0, j1, case["hx"], case["hy"], case["dt"], po, s, (c["u"], c["v"]), (un, vn), (c["u0"], c["v0"]), (out["tax"], out["tay"]),
                    (c["uo"], c["vo"]), out["cgh"], out["cga"], alpha_e=alpha_e)
    if ln is not None:
        g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == ny else 0)
        un[g0:g1][ln[g0:g1]] = 0.0
        vn[g0:g1][ln[g0:g1]] = 0.0
    out.update(S=s, u=un, v=vn, alpha_e=alpha_e)
    return out


def compare_outputs(case, got, ref, what, wide=None):
    """the device test's comparison of one sub-iteration (tests/test_gpu_mevp_regimes.py::check_against_reference restated for numpy
    results): returns the largest |difference| / bound"""
    a, w = B.outputs(got), B.outputs(ref)
    worst = 0.0
    if case["kind"] == "drift":
        bounds, w = B.drift_bounds(), {k: x.astype(np.float64) for k, x in B.outputs(wide).items()}
        for k in B.OUTPUTS:
            worst = max(worst, assert_close(a[k], w[k], 0.0, bounds[k], "%s %s" % (what, k)))
        return worst
    for k in B.OUTPUTS:
        rel, floor = B.VELOCITY_TOL if k in ("u", "v") else B.STRESS_TOL
        worst = max(worst, assert_close(a[k], w[k], rel, floor * np.max(np.abs(w[k])), "%s %s" % (what, k)))
    if case["kind"] in ("icefree", "ad_icefree"):
        ice = ~B.ice_free_nodes(case, ref)
        for k in ("u", "v"):
            worst = max(worst, assert_close(a[k][ice], w[k][ice], B.VELOCITY_TOL[0], B.VELOCITY_TOL[1] * np.max(np.abs(w[k][ice])), "%s %s (ice)" % (what, k)))
    return worst


@pytest.mark.parametrize("key", B.ALL_CASES, ids=B.case_id)
def test_oracle_agrees_with_the_restatement(key):
    """oracle/dyn_oracle.c on every case: the helpers under the bounds of tests/test_gpu_parity.py::test_mevp_helpers_match_oracle, one
    sub-iteration under those of test_mevp_single_iteration_matches_oracle (drift: under its recorded bound, against the longdouble
    evaluation), every element's alpha to 1e-12"""
    case, ref = B.built(key)
    got = oracle_iterate(case)
    prep = ref["prep"]
    assert_close(got["pg"], prep["pg"], 1e-12, 1e-10, "ice strength")
    for k in ("cgh", "cga"):
        assert_close(got[k], prep[k], 1e-13, 1e-14, k)
    for k in ("tax", "tay"):
        assert_close(got[k], prep[k], 1e-13, 1e-16, k)
    wide = B.reference(case, np.longdouble) if key[0] == "drift" else None
    worst = compare_outputs(case, got, ref, B.case_id(key), wide)
    if got["alpha_e"] is not None:
        assert_close(got["alpha_e"], ref["diag"]["alpha_e"], 1e-12, 0.0, "alpha_e")
    print("oracle against the restatement, worst |difference| / bound: %.4f" % worst)


@pytest.mark.parametrize("kind", ["plastic", "ad_spread"])
@pytest.mark.parametrize("rows", [(1, 2, 4), (2, 3, 5)], ids=["1-2-4", "2-3-5"])
def test_oracle_row_ranges_agree_with_the_restatement(kind, rows):
    """130 x 5 with the row ranges (k0, j0, j1) of nsdg_mevp_iterate: the oracle's stress on [k0, j1) and its velocity on the node rows
    of [j0, j1) are the restatement's there, and the restatement's row range equals its whole-array result on those rows bit for bit"""
    k0, j0, j1 = rows
    key = B.shape_case(kind, 130, 5)
    case, full = B.built(key)
    ref = B.reference(case, k0=k0, j0=j0, j1=j1)
    g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == 5 else 0)
    assert (g0, g1) == {(1, 2, 4): (4, 8), (2, 3, 5): (6, 11)}[rows]
    for a, b in zip(ref["S"], full["S"]):
        assert np.array_equal(a[:, k0:j1], b[:, k0:j1])
    assert np.array_equal(ref["u"][g0:g1], full["u"][g0:g1]) and np.array_equal(ref["v"][g0:g1], full["v"][g0:g1])
    inp = case["c"]
    outside = np.ones(5, dtype=bool)
    outside[k0:j1] = False
    for a, b in zip(ref["S"], inp["S"]):
        assert np.array_equal(a[:, outside], b[:, outside])
    got = oracle_iterate(case, k0, j0, j1)
    cut = lambda r: dict(S=[x[:, k0:j1] for x in r["S"]], u=r["u"][g0:g1], v=r["v"][g0:g1])
    compare_outputs(case, cut(got), cut(ref), "%s rows %s" % (kind, rows))
