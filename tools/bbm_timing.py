"""Measurements of the brittle Bingham-Maxwell sub-cycle (csrc/bbm.hip) on the device; the record is profiles/r09_bbm.md.

  python tools/bbm_timing.py time [--n 2048] [--rounds 5] [--iters 40]
      ms per sub-iteration of nsdg_bbm_iterate beside nsdg_mevp_iterate (variant 1, the single-iteration marching kernel) on the same box,
      in ALTERNATING timed windows, and the share of the nsdg_copy_f64 peak that the kernel's stated traffic (1016 B per element and
      sub-iteration, csrc/bbm.hip) amounts to.
  python tools/bbm_timing.py courant [--n 64] [--steps 200] [--dt 120]
      the elastic-wave rule's Courant number: for each of 1, 0.7, 0.5, 0.35, 0.25 the box test (1 km cells, full undamaged cover, cyclone
      wind) runs `steps` model steps with nsub = nsdg_bbm_substep_count(courant) sub-iterations each; a run completes if every field stays
      finite and the largest speed stays below 1 m/s.

Both need a GPU: there is no fallback.  One JSON line per result."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nextsimdg_amd import abi, build, rowblock, synthetic  # noqa: E402

BBM_BYTES = 1016  # per element and sub-iteration (csrc/bbm.hip)
MEVP_BYTES = 776  # csrc/mevp_fused.hip
COURANTS = (1.0, 0.7, 0.5, 0.35, 0.25)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def time_kernels(n, rounds, iters):
    ctx = abi.Context(torch.device("cuda:0"))
    ctx.set_mevp_variant(1)
    bt = synthetic.BoxTest(n, n, L=1000.0 * n)
    alpha = bt.stable_alpha(120.0)  # the mEVP windows stay finite; the BBM pass ignores alpha and beta
    ctx.set_mevp_params(ctx.mevp_default_params(alpha=alpha, beta=alpha))
    H, A = bt.dg_fields()
    H[0] += 0.7
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    ctx.set_grid(n, n, bt.hx, bt.hy)
    dH, dA, D, Db = dev(H), dev(A), z(6, n, n), z(6, n, n)
    ua, va = (dev((512e3 / bt.L) * w) for w in bt.wind(0.0))
    uo, vo = (dev(w) for w in bt.ocean())
    nodal = (2 * n + 1, 2 * n + 1)
    u, v, ub, vb, zero = (z(*nodal) for _ in range(5))
    s, sb = [ctx.private_zeros(8, n, n, "cuda") for _ in range(3)], [ctx.private_zeros(8, n, n, "cuda") for _ in range(3)]
    gauss = [ctx.private_zeros(9, n, n, "cuda") for _ in range(3)]
    pg = ctx.private_zeros(9, n, n, "cuda")
    packed_b, packed_m = z(8 * u.numel()), z(8 * u.numel())
    ctx.bbm_prepare(dH, dA, *gauss)
    ctx.ice_strength(dH, dA, pg)
    # the two packings differ only in the time step: both passes read the context's pack_dt, so each window repacks first (untimed)
    pack_b = lambda: ctx.mevp_prepare(0.25, dH, dA, (ua, va), (uo, vo), (zero, zero), packed_b)
    pack_m = lambda: ctx.mevp_prepare(120.0, dH, dA, (ua, va), (uo, vo), (zero, zero), packed_m)
    bbm = [ctx.bind_bbm_iterate(0, 0, n, s, sb, D, Db, (u, v), (ub, vb), packed_b, gauss),
           ctx.bind_bbm_iterate(0, 0, n, sb, s, Db, D, (ub, vb), (u, v), packed_b, gauss)]
    mevp = [ctx.bind_mevp_iterate(0, 0, n, s, sb, (u, v), (ub, vb), packed_m, pg), ctx.bind_mevp_iterate(0, 0, n, sb, s, (ub, vb), (u, v), packed_m, pg)]
    pair = lambda calls: (lambda: (calls[0](), calls[1]()))
    big = z(1 << 27), z(1 << 27)  # 1 GiB each
    copy = lambda: ctx.copy_f64(big[0], big[1])
    pack_b(), window(pair(bbm), 4), pack_m(), window(pair(mevp), 4), window(copy, 4)  # warm-up of every timed shape
    t_b, t_m, t_c = [], [], []
    for _ in range(rounds):
        for f in (s + sb + [u, v, ub, vb, D, Db]):
            f.zero_()
        pack_b()
        t_b.append(window(pair(bbm), iters // 2) / 2)
        for f in (s + sb + [u, v, ub, vb]):
            f.zero_()
        pack_m()
        t_m.append(window(pair(mevp), iters // 2) / 2)
        t_c.append(window(copy, 10))
    assert all(bool(torch.isfinite(x).all()) for x in (u, v, D))
    peak = 2 * 8 * (1 << 27) / (min(t_c) * 1e-3) / 1e9
    out = dict(mode="time", n=n, rounds=rounds, iters=iters, bbm_ms=[round(x, 4) for x in t_b], mevp_v1_ms=[round(x, 4) for x in t_m],
               copy_peak_GBs=round(peak, 1))
    for name, t, nbytes in (("bbm", min(t_b), BBM_BYTES), ("mevp_v1", min(t_m), MEVP_BYTES)):
        gbs = nbytes * n * n / (t * 1e-3) / 1e9
        out[name + "_GBs"], out[name + "_share_of_copy_peak"] = round(gbs, 1), round(gbs / peak, 3)
    print(json.dumps(out), flush=True)
    ctx.close()


def courant_scan(n, steps, dt):
    ctx = abi.Context(torch.device("cuda:0"))
    bt = synthetic.BoxTest(n, n, L=1000.0 * n)
    H, A = bt.dg_fields()
    uo, vo = bt.ocean()
    scale = 512e3 / bt.L  # the cyclone of the 512 km box test on this box: winds of the same 15 m/s scale
    p = abi.bbm_default_params()
    mp = ctx.mevp_default_params()
    for courant in COURANTS:
        nsub = abi.bbm_substep_count(p, mp.rho_ice, min(bt.hx, bt.hy), dt, courant)
        core = rowblock.DynamicsCore(ctx, rowblock.RowBlock(n, n), bt.hx, bt.hy, dt, nsub, torch.device("cuda"), rheology="bbm")
        ua, va = bt.wind(0.0)
        core.load_global(H, A, np.ascontiguousarray(uo), np.ascontiguousarray(vo), np.ascontiguousarray(scale * ua), np.ascontiguousarray(scale * va),
                         D=np.zeros_like(H))
        done, vmax, ok = 0, 0.0, True
        while ok and done < steps:
            for _ in range(min(10, steps - done)):
                ua, va = bt.wind(done * dt)
                core.ua.copy_(torch.from_numpy(np.ascontiguousarray(scale * ua)))
                core.va.copy_(torch.from_numpy(np.ascontiguousarray(scale * va)))
                core.step()
                done += 1
            finite = all(bool(torch.isfinite(f).all()) for f in (core.H, core.A, core.D, core.u, core.v, *core.s))
            vmax = float(torch.sqrt(core.u * core.u + core.v * core.v).max()) if finite else float("nan")
            ok = finite and vmax < 1.0
        print(json.dumps(dict(mode="courant", n=n, dt=dt, courant=courant, nsub=nsub, steps_done=done, steps=steps, completed=bool(ok and done == steps),
                              max_speed=vmax, max_damage=float(core.D[0].max()) if ok else None)), flush=True)
        core.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    t = sub.add_parser("time")
    t.add_argument("--n", type=int, default=2048)
    t.add_argument("--rounds", type=int, default=5)
    t.add_argument("--iters", type=int, default=40)
    c = sub.add_parser("courant")
    c.add_argument("--n", type=int, default=64)
    c.add_argument("--steps", type=int, default=200)
    c.add_argument("--dt", type=float, default=120.0)
    a = ap.parse_args()
    build.build_lib(verbose=False)
    if not torch.cuda.is_available():
        sys.exit("bbm_timing.py needs a GPU: nothing is measured without one")
    if a.mode == "time":
        time_kernels(a.n, a.rounds, a.iters)
    else:
        courant_scan(a.n, a.steps, a.dt)


if __name__ == "__main__":
    main()
