"""Writes tests/golden/ref_column_v1.npz: inputs, parameters and outputs of the reference's own column physics
(oracle/_ref/libref_column.so, built by `make -C oracle ref` where the reference sources are present), recorded so that
tests/test_oracle_column.py (the oracle, bit for bit) and tests/test_gpu_parity.py (the HIP kernel) can be held to them on
every machine.

    python tools/gen_ref_column_golden.py            # regenerate from oracle/_ref
    python tools/gen_ref_column_golden.py --check    # recompute and compare with the committed file, exit 1 on any difference

Module sets (SETS): the defaults; UNESCO freezing with CCSM albedo at non-default albedos; SMU2 albedo without flooding; and a
set in which every one of the 12 ColumnParams values differs from its default.  Each set is recorded in a fresh child process:
HiblerConcentration::freeze latches 1/h0 in a function-local static on its first call (physics/src/modules/HiblerConcentration.cpp:36),
so a second set in the same process would keep the first set's h0.

Groups per set (all recorded from a fresh element, newice = 0 in):
    random      a seeded synthetic.column_fields draw of 256 elements, dt = 600 s
    edge        a grid over the branch points (edge_cases()), dt = 600 s; under the defaults also dt = 1 s and 86 400 s
    chain       10 chained steps of 32 elements with forcing that changes per step, state and newice after every step
The fixture's "meta" entry (JSON) lists the sets with their parameters (C99 hex floats) and the groups, each with the prefix of
its inputs, and the h0 note.  The random and chain inputs do not depend on the set and are stored once ("random/in/...",
"chain/in/..."); the edge grid is the set's own ("<set>/<group>/in/...").  Outputs are "<set>/<group>/out/...".  The sizes keep
the file small: random float64 values hardly compress.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import oracle_lib as O  # noqa: E402
from nextsimdg_amd import synthetic  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "ref_column_v1.npz")
SETS = {
    "default": dict(),
    "unesco_ccsm": dict(freezing="unesco", albedo="ccsm", ccsm_ice_albedo=0.63, ccsm_snow_albedo=0.88),
    "smu2_noflood": dict(albedo="smu2", flooding=0),
    "all_params": dict(drag_ocean_q=1.7e-3, drag_ocean_t=0.9e-3, drag_ice_t=1.1e-3, ocean_albedo=0.1, i0=0.2, min_conc=1e-3,
                       min_thick=0.05, ks=0.25, h0=0.4, phi_m=0.7, ccsm_ice_albedo=0.5, ccsm_snow_albedo=0.78, albedo="ccsm"),
}
NRANDOM, NCHAIN, CHAIN_STEPS = 256, 32, 10
H0_NOTE = ("HiblerConcentration::freeze keeps 1/h0 in a function-local static set on its first call "
           "(physics/src/modules/HiblerConcentration.cpp:36); every set was recorded in its own process, so each set's h0 is its own")


def edge_cases(params):
    """State x forcing grid around the branch points of the column step, for one parameter set (min_conc / min_thick are the
    set's own; the freezing point is the set's own law at sss = 32)."""
    tf = O.lib().oracle_freezing_point(params.freezing_kind, 32.0)
    mc, mt = params.min_conc, params.min_thick
    concs = [0.0, mc / 2, mc, np.nextafter(mc, 1.0), 0.5, 1.0]
    thicks = [0.0, mt / 2, mt, np.nextafter(mt, 1.0), 0.3, 2.0]  # true thickness
    snows = [0.0, 1.0]  # true snow depth; 1 m on 0.3 m of ice floods
    tices = [0.0, -1e-3, -30.0]
    # forcing: at the freezing point in the cold; below it in a 1 m mixed layer with snowfall on open water; warm air
    # and sun over a mixed layer above freezing (surface and bottom melt)
    forcings = [dict(sst=tf, tair=-20.0, qsw=0.0, qlw=180.0, mld=30.0, snowfall=0.0),
                dict(sst=tf - 0.05, tair=-30.0, qsw=0.0, qlw=160.0, mld=1.0, snowfall=5e-5),
                dict(sst=tf + 0.5, tair=4.0, qsw=300.0, qlw=320.0, mld=10.0, snowfall=0.0)]
    rows = []
    for c, h, hs, t, f in itertools.product(concs, thicks, snows, tices, forcings):
        rows.append(dict(hice=h * c if c > 0 else h, cice=c, hsnow=hs * c, tice0=t, sss=32.0, tdew=f["tair"] - 2.0,
                         slp=1.0e5, wind=8.0, **f))
    # NaN in: both sides must carry it the same way
    rows.append(dict(rows[-1], hice=np.nan))
    rows.append(dict(rows[-1], hice=0.3, tice0=np.nan))
    state = {k: np.array([r[k] for r in rows]) for k in O.STATE}
    forcing = {k: np.array([r[k] for r in rows]) for k in O.FORCING}
    return state, forcing


def chain_inputs():
    """32 elements of the random draw; forcing drawn afresh every step, with the mixed layer set to the lower of the two
    freezing points (linear, UNESCO) in a third of the (step, element) pairs, so that under every set new ice forms in some
    steps and not in the next (the carried m_newice)."""
    state, _, _ = synthetic.column_fields(NCHAIN)
    planes = [synthetic.column_fields(NCHAIN, seed=1000 + s)[1] for s in range(CHAIN_STEPS)]
    forcing = {k: np.stack([p[k] for p in planes]) for k in O.FORCING}
    e = np.arange(NCHAIN)
    for s in range(CHAIN_STEPS):
        cold = (s + e) % 3 == 0
        tf = np.array([min(O.lib().oracle_freezing_point(0, x), O.lib().oracle_freezing_point(1, x)) for x in forcing["sss"][s]])
        forcing["sst"][s, cold] = tf[cold]
        forcing["tair"][s, cold] = -25.0
        forcing["tdew"][s, cold] = -27.0
    return state, forcing


def groups(name):
    g = [("random", 600.0), ("edge", 600.0)]
    if name == "default":
        g += [("edge_dt1", 1.0), ("edge_dt86400", 86400.0)]
    return g + [("chain", 600.0)]


def inputs_key(name, group):
    """prefix of a group's inputs: random draw and chain are shared by every set"""
    return group + "/" if group in ("random", "chain") else "%s/%s/" % (name, group)


def inputs(name, group):
    if group == "random":
        state, forcing, _ = synthetic.column_fields(NRANDOM)
        return state, forcing, 1
    if group.startswith("edge"):
        return edge_cases(O.column_params(**SETS[name])) + (1,)
    return chain_inputs() + (CHAIN_STEPS,)


def record_set(name):
    """Runs in a child process: configure the reference once with this set, record every group."""
    R = O.ref_column()
    params = O.column_params(**SETS[name])
    assert R.ref_column_configure(O.ref_column_ini(params).encode()) == 0, name
    out = {}
    for group, dt in groups(name):
        state, forcing, nsteps = inputs(name, group)
        n = state["hice"].size
        key, ikey = "%s/%s/" % (name, group), inputs_key(name, group)
        for k in O.STATE:
            out[ikey + "in/" + k] = state[k].copy()
        for k in O.FORCING:
            out[ikey + "in/" + k] = np.ascontiguousarray(forcing[k])
        st = {k: state[k].copy() for k in O.STATE}
        newice, diag = np.zeros(n), np.zeros((len(O.DIAG), n))
        rec = np.zeros((nsteps, 5, n)) if nsteps > 1 else None
        rc = R.ref_column_run(n, nsteps, dt, n if nsteps > 1 else 0, *[O.dp(st[k]) for k in O.STATE],
                              *[O.dp(out[ikey + "in/" + k]) for k in O.FORCING], O.dp(newice), O.dp(diag),
                              O.dp(rec) if rec is not None else None)
        assert rc == 0, (name, group, rc)
        for k in O.STATE:
            out[key + "out/" + k] = st[k]
        out[key + "out/newice"] = newice
        out[key + "out/diag"] = diag
        if rec is not None:
            out[key + "out/record"] = rec
    return out


def compute():
    arrays, meta = {}, {"title": "outputs of the reference's own column physics (oracle/ref_column_driver.cpp), float64",
                        "h0_latch": H0_NOTE, "diag": O.DIAG, "state": O.STATE, "forcing": O.FORCING,
                        "record_planes": O.STATE + ["newice"], "sets": {}, "groups": []}
    for name in SETS:
        p = O.column_params(**SETS[name])
        meta["sets"][name] = {f: (getattr(p, f).hex() if isinstance(getattr(p, f), float) else getattr(p, f))
                              for f, _ in O.ColumnParams._fields_ if f != "reserved"}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "set.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", name, path])
            with np.load(path) as z:
                for k in z.files:
                    assert k not in arrays or same(arrays[k], z[k]), k  # shared inputs: the same in every child
                    arrays[k] = z[k]
        for group, dt in groups(name):
            meta["groups"].append({"set": name, "group": group, "dt": dt, "inputs": inputs_key(name, group),
                                   "nsteps": CHAIN_STEPS if group == "chain" else 1})
    arrays["meta"] = np.array(json.dumps(meta, indent=1))
    return arrays


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.dtype.kind != "f" or np.array_equal(a.view(np.int64), b.view(np.int64))) \
        and (a.dtype.kind == "f" or np.array_equal(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("SET", "OUT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if O.ref_column() is None:
        raise SystemExit("oracle/_ref/libref_column.so is not built (make -C oracle ref, with the reference sources present)")
    if args.child:
        np.savez(args.child[1], **record_set(args.child[0]))
        return
    d = compute()
    if args.check:
        with np.load(PATH) as z:
            ok = sorted(z.files) == sorted(d) and all(same(z[k], d[k]) for k in d)
        print("ref_column_v1.npz %s" % ("matches" if ok else "DIFFERS"))
        sys.exit(0 if ok else 1)
    np.savez_compressed(PATH, **d)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
