"""Row-block decomposition of the structured mesh over the ranks of one node and the per-step driver
of the dynamics core (mEVP sub-cycle + DG2 transport of H and A).

One process per GPU; rank r owns the contiguous element rows [r*ny/R, (r+1)*ny/R) of the x-major
index e = iy*nx + ix (the reference's restart order i*nx + j, core/src/DevGridIO.cpp:107-109) and
keeps one ghost element row on each interior side.  The only communication is nearest-neighbour
send/recv of ghost rows through torch.distributed (backend "nccl" = RCCL over xGMI on the GPU box,
"gloo" in the CPU tests) -- there is no collective on the data path:

  per mEVP sub-iteration : velocity node rows   up: 2 rows x (u,v) x (2nx+1)     down: 1 row x (u,v)
   (single-iteration       (the stress of the ghost row below is NOT exchanged: it is updated
    kernel)                 redundantly by the rank itself, bit-identically to its owner)
  per GROUP of k passes  : kernels with v = 2, 3 or 4 sub-iterations per pass and ghost depth (d, d-1), d = v k:
   (v k sub-iterations)    d stress rows + 2d node rows travel up, d-1 stress rows + 2d-1 node rows down.
                           Between two exchanges a rank runs k passes on a row range that shrinks by v rows
                           on each side per pass -- the ghost rows are advanced redundantly, bit-identically
                           to their owners -- so the number of messages per step drops by v k
                           (latency-avoiding halo)
  per RK stage           : the ghost element rows of each advected field in both directions (ghost depth
                           >= 3: once per step, the first two stages advance ghost rows redundantly)

Ownership of CG2 nodes is bottom-left: rank r owns node rows [2*r0, 2*r1); the global top node row is a
Dirichlet boundary.  Everything that travels to one neighbour in one exchange (row blocks of several
arrays) is packed into one buffer and sent with one P2P op (HaloExchanger).

The numerical kernels are reached through an `ops` object with the method names of
nextsimdg_amd.abi.Context (the C-ABI binding).  Nothing here computes on the host.
"""
import os

import torch
import torch.distributed as dist

# NSDG_PHASE_* of include/nsdg.h: the ids of step()'s phase marks (names: abi.PHASES)
PHASE_FORCING, PHASE_COLUMN, PHASE_PREPARE, PHASE_SUBCYCLE, PHASE_TRANSPORT, PHASE_REDUCTION, PHASE_END = 0, 1, 2, 3, 4, 5, -1


def split_rows(ny, world, rank):
    return (rank * ny) // world, ((rank + 1) * ny) // world


class RowBlock:
    """index bookkeeping of one rank's local array.  `depth_below` / `depth_above` are the numbers of ghost
    element rows kept on the interior sides: (1, 1) for one mEVP sub-iteration per pass, (v k, v k - 1) for the
    kernels with v = 2 or 3 sub-iterations per pass and k passes between two ghost-row exchanges.  Such a
    kernel reads the stress of v element rows below and v - 1 above the rows it updates and the velocity up to
    the bottom node row of the v-th element row above (owned by that row), so complete rows shrink by v per
    pass on both sides; k = 1 gives the (2, 1) / (3, 2) of an exchange after every pass."""

    def __init__(self, nx, ny, rank=0, world=1, depth_below=1, depth_above=1):
        if ny < world * max(depth_below, depth_above, 1) * 2:
            raise ValueError("too few element rows per rank for the ghost depth")
        self.nx, self.ny_glob, self.rank, self.world = nx, ny, rank, world
        self.r0, self.r1 = split_rows(ny, world, rank)
        self.gb = depth_below if rank > 0 else 0  # ghost element rows below
        self.gt = depth_above if rank < world - 1 else 0  # ghost element rows above
        self.depth_below, self.depth_above = depth_below, depth_above
        self.lo, self.hi = self.r0 - self.gb, self.r1 + self.gt  # global rows held locally
        self.ny = self.hi - self.lo  # local element rows
        self.j0, self.j1 = self.gb, self.ny - self.gt  # owned local rows
        self.k0 = max(self.j0 - 1, 0)  # single-iteration kernel: stress is updated from one ghost row below
        self.below = rank - 1 if rank > 0 else None
        self.above = rank + 1 if rank < world - 1 else None

    def elem_slice(self):
        return slice(self.lo, self.hi)

    def node_slice(self):
        return slice(2 * self.lo, 2 * self.hi + 1)


class HaloPlan:
    """what one ghost-row exchange moves: lists of tensor views (row blocks) per direction"""

    def __init__(self):
        self.up_send, self.down_send, self.from_above, self.from_below = [], [], [], []
        self.buffers = None  # transport-private (packed send / receive buffers)
        self.ops = self.flat_up = self.flat_down = None  # transport-private (P2P ops and flattened views, built once)


class HaloExchanger:
    """nearest-neighbour ghost-row exchange.  Planning (which row blocks travel) is separate from transport:
    subclasses that move the data differently (the in-process exchanger of tests/test_gpu_multiblock.py, the
    no-op exchanger of tools/rank_share_timing.py) override _start / _finish only.

    Transport: everything that travels to one neighbour is packed into ONE buffer (torch.cat) and sent with ONE
    P2P op, so a batch has at most 2 sends + 2 receives whatever the number of fields -- the host cost of
    torch.distributed P2P ops (about 13 us each on the GPU box; 20 ops per batch made the 8-block sub-cycle
    host-bound) matters more than the extra device copy of a few MB."""

    def __init__(self, blk, group=None, loopback=False):
        self.blk, self.group = blk, group
        self._cache = {}
        # loopback (rehearsal on one GPU, tools/rank_share_timing.py --rccl-loopback): both neighbours are this
        # rank itself, so a send upwards must meet the receive from below -- receives are posted in that order
        self.loopback = loopback

    # ------------------------------------------------------------------ planning
    def _plan(self, key, build):
        plan = self._cache.get(key)
        if plan is None:
            plan = self._cache[key] = HaloPlan()
            if self.blk.world > 1:
                build(plan)
        return plan

    def _add_nodal(self, plan, fields, rows_down):
        """CG2 nodal arrays [2ny+1, 2nx+1]: 2*depth_below node rows travel upwards, `rows_down` rows (1 for the
        single-iteration kernel, 2*depth_above + 1 for the multi-iteration kernels) downwards"""
        b = self.blk
        up = 2 * b.depth_below
        for f in fields:
            if b.above is not None:
                plan.up_send.append(f[2 * b.j1 - up:2 * b.j1])
                plan.from_above.append(f[2 * b.j1:2 * b.j1 + rows_down])
            if b.below is not None:
                plan.down_send.append(f[2 * b.j0:2 * b.j0 + rows_down])
                plan.from_below.append(f[2 * b.j0 - up:2 * b.j0])

    def _add_rows(self, plan, fields, rows_of):
        """element-row arrays: depth_below rows travel upwards, depth_above rows downwards"""
        b = self.blk
        for f in fields:
            if b.above is not None:
                plan.up_send.append(rows_of(f, b.j1 - b.depth_below, b.j1))
                if b.gt:
                    plan.from_above.append(rows_of(f, b.j1, b.j1 + b.gt))
            if b.below is not None:
                if b.depth_above:
                    plan.down_send.append(rows_of(f, b.j0, b.j0 + b.depth_above))
                plan.from_below.append(rows_of(f, b.j0 - b.gb, b.j0))

    # ------------------------------------------------------------------ transport
    def _start(self, plan):
        b = self.blk
        if b.world == 1 or not (plan.up_send or plan.down_send or plan.from_above or plan.from_below):
            return None
        if plan.buffers is None:
            size = lambda views: sum(v.numel() for v in views)
            like = (plan.up_send or plan.down_send or plan.from_above or plan.from_below)[0]
            new = lambda n: torch.empty(n, dtype=like.dtype, device=like.device) if n else None
            plan.buffers = tuple(new(size(v)) for v in (plan.up_send, plan.down_send, plan.from_above, plan.from_below))
            # the P2P ops and the flattened source views are built once per plan
            s_up, s_down, r_above, r_below = plan.buffers
            ops = []
            if s_up is not None:
                ops.append(dist.P2POp(dist.isend, s_up, b.above, self.group))
            if s_down is not None:
                ops.append(dist.P2POp(dist.isend, s_down, b.below, self.group))
            recv_above = dist.P2POp(dist.irecv, r_above, b.above, self.group) if r_above is not None else None
            recv_below = dist.P2POp(dist.irecv, r_below, b.below, self.group) if r_below is not None else None
            ops += [r for r in ((recv_below, recv_above) if self.loopback else (recv_above, recv_below)) if r is not None]
            plan.ops = ops
            plan.flat_up = [v.reshape(-1) for v in plan.up_send] if all(v.is_contiguous() for v in plan.up_send) else None
            plan.flat_down = [v.reshape(-1) for v in plan.down_send] if all(v.is_contiguous() for v in plan.down_send) else None
        s_up, s_down = plan.buffers[0], plan.buffers[1]
        if s_up is not None:
            torch.cat(plan.flat_up if plan.flat_up is not None else [v.reshape(-1) for v in plan.up_send], out=s_up)
        if s_down is not None:
            torch.cat(plan.flat_down if plan.flat_down is not None else [v.reshape(-1) for v in plan.down_send], out=s_down)
        return dist.batch_isend_irecv(plan.ops), plan

    def _finish(self, handle):
        if handle is None:
            return
        works, plan = handle
        for w in works:
            w.wait()
        for views, buf in ((plan.from_above, plan.buffers[2]), (plan.from_below, plan.buffers[3])):
            if not views:
                continue
            chunks = buf.split([v.numel() for v in views])
            if all(v.is_contiguous() for v in views):  # one multi-tensor launch
                torch._foreach_copy_([v.view(-1) for v in views], list(chunks))
            else:
                for v, c in zip(views, chunks):
                    v.copy_(c.view(v.shape))

    # ------------------------------------------------------------------ the exchanges of the driver
    def nodal_start(self, fields, rows_down=1):
        """post the exchange of the ghost node rows of `fields`"""
        key = ("n", rows_down) + tuple(f.data_ptr() for f in fields)
        return self._start(self._plan(key, lambda p: self._add_nodal(p, fields, rows_down)))

    def finish(self, handle):
        self._finish(handle)

    def nodal(self, fields, rows_down=1):
        self.finish(self.nodal_start(fields, rows_down))

    def rows_exchange_start(self, fields, rows_of, nodal_fields=(), rows_down=1):
        """post ONE batch with the ghost rows of the private arrays `fields` (rows taken with ops.private_rows():
        for the tiled device layout a row range is one contiguous block) and, optionally, the ghost node rows of
        `nodal_fields`"""
        key = ("r", rows_down) + tuple(f.data_ptr() for f in fields) + tuple(f.data_ptr() for f in nodal_fields)

        def build(p):
            self._add_rows(p, fields, rows_of)
            self._add_nodal(p, nodal_fields, rows_down)

        return self._start(self._plan(key, build)), ()

    def rows_exchange_finish(self, handle, unused=()):
        self._finish(handle)

    def element(self, fields):
        """refresh the ghost element rows of DG arrays [nc, ny, nx] (after a transport stage)"""
        key = ("e",) + tuple(f.data_ptr() for f in fields)
        plan = self._plan(key, lambda p: self._add_rows(p, fields, lambda f, a, c: f[:, a:c, :]))
        self._finish(self._start(plan))


class NativeHaloExchanger(HaloExchanger):
    """the planning of HaloExchanger with the transport behind the C ABI (csrc/halo.hip): pack kernel, RCCL
    send/recv group on the context's communication stream, unpack kernel -- three C calls and no torch op per
    exchange.  `local_group`: in-process transport between thread-ranks instead of RCCL (one-GPU tests)."""

    def __init__(self, ctx, blk, device=None, group=None, loopback=False, local_group=None):
        super().__init__(blk, group, loopback)
        self.ctx = ctx
        if loopback:
            # rehearsal of an interior block on one GPU: a communicator of ONE rank, both neighbours are that rank
            # (what goes up arrives from below); the values wrap around, the calls and sizes are the real ones
            if local_group is not None:
                ctx.comm_init_local(local_group, 0, 1)
            else:
                ctx.comm_init_rccl(0, 1)
            self.peer_below = 0 if blk.below is not None else None
            self.peer_above = 0 if blk.above is not None else None
        else:
            if local_group is not None:
                ctx.comm_init_local(local_group, blk.rank, blk.world)
            else:
                ctx.comm_init_rccl(blk.rank, blk.world, group)
            self.peer_below, self.peer_above = blk.below, blk.above

    def _plan(self, key, build):
        plan = self._cache.get(key)
        if plan is None:
            plan = self._cache[key] = HaloPlan()
            if self.blk.world > 1:
                build(plan)
                if plan.up_send or plan.down_send or plan.from_above or plan.from_below:
                    plan.native = self.ctx.halo_plan(self.peer_below, self.peer_above, plan.up_send, plan.down_send,
                                                     plan.from_above, plan.from_below)
        return plan

    def _start(self, plan):
        native = getattr(plan, "native", None)
        if native is None:
            return None
        native.start()
        return native

    def _finish(self, handle):
        if handle is not None:
            handle.finish()


class DynamicsCore:
    """State and time step of the dynamics core on one rank's row block.

    step() = one model time step: nodal means of H and A, ice strength at the Gauss points, wind
    stress, `nsub` mEVP sub-iterations (velocity halo after each), advection-velocity preparation and
    one SSP-RK3 DG2 transport step of H and A (element halo after each stage)."""

    ORDER = 2
    # closure of the transported fields (include/nsdg.h "INPUT DOMAIN AND CLOSURE"): mean thickness H >= 0; concentration
    # 0 <= A <= 1 at the quadrature points with the cell mean capped at 1 (ridging) -- (lo, hi, cap_mean) per field
    BOUNDS = ((0.0, float("inf"), False), (0.0, 1.0, True))
    # the advected DG2 fields (attribute names), in the order of the step calls' field lists and of BOUNDS; CoupledCore with
    # advect_column_state adds the snow S and the weighted surface temperature Q
    TRANSPORTED = ("H", "A")

    LAND_OPS = ("set_land_mask", "land_clear", "land_clear_nodes")
    BBM_OPS = ("bbm_prepare", "bbm_iterate")
    DRIFTER_OPS = ("drifters_advance",)
    DAMAGE_BOUNDS = (0.0, 1.0, False)  # the damage D of the brittle rheology: in [0, 1], no cap of the cell mean
    # history output (include/nsdg.h "history output"; the names: abi.HISTORY_FIELDS): the fields of the column
    # state exist in a CoupledCore only
    HISTORY_COLUMN_FIELDS = ("hsnow", "tice")
    HAS_COLUMN_STATE = False
    series = None  # series=: off unless the constructor says otherwise

    def __init__(self, ops, blk, hx, hy, dt, nsub, device, exchanger=None, overlap=True, native=False, use_graph=False, closure=True,
                 phase_timing=False, land=None, rheology="mevp", bbm=None, history=None, series=None, series_capacity=1024, extent_conc=0.15,
                 drifters=None, drifter_min_conc=0.15):
        self.ops, self.blk, self.hx, self.hy, self.dt, self.nsub = ops, blk, hx, hy, dt, nsub
        # history: names of abi.HISTORY_FIELDS sampled once per model step (step(), or advance() with all its sub-steps) into one accumulator
        # on the device, read as time means by history_read().  None: nothing is asked of `ops` and nothing is allocated.  An entry may be
        # "name:stat" with a statistic of abi.HISTORY_STATS ("name" alone is the mean): ice-weighted means and the extremes of the window
        self.history = self._check_history(history, rheology, ops)
        # series: names of abi.SERIES_QUANTITIES; every model step leaves their row totals in the next of series_capacity slots of a device
        # buffer, read by series_read() and made domain totals by merge_series().  extent_conc: the concentration the ice extent counts from
        self.series = self._check_series(series, series_capacity, extent_conc, ops)
        self.series_capacity, self.extent_conc = int(series_capacity), float(extent_conc)
        # drifters: [n, 2] positions (x, y) in metres of the GLOBAL domain [0, nx hx] x [0, ny_global hy], or [n, 3] with the status (0 active,
        # 1 left the domain, 2 lost its ice, 3 on land) as a third column: Lagrangian points moved once per step() by the velocity the sub-cycle
        # left (include/nsdg.h "drifters").  Every rank keeps the whole list.  drifter_min_conc: the cell-mean
        # concentration below which a drifter has lost its ice.  None: nothing is asked of `ops` and nothing is allocated
        drift0 = self._check_drifters(drifters, drifter_min_conc, ops, exchanger)
        self.drifter_min_conc = float(drifter_min_conc)
        # rheology: "mevp", or "bbm" -- the brittle Bingham-Maxwell sub-cycle (include/nsdg.h "brittle rheology"):
        # nsub explicit sub-iterations of dt / nsub, a damage field D updated in the sub-cycle and advected with H and A.  bbm: an
        # abi.BbmParams set on the ops object (None: whatever the ops object holds, the library's defaults on a new context)
        if rheology not in ("mevp", "bbm"):
            raise ValueError("rheology must be 'mevp' or 'bbm', got %r" % (rheology,))
        self.rheology = rheology
        if rheology == "bbm":
            if native:
                raise ValueError("rheology='bbm' is not built in the native row-block plan (nsdg_rb_mevp_*): use native=False")
            if blk.world > 1 and (blk.depth_below, blk.depth_above) != (1, 1):
                raise ValueError("rheology='bbm' runs one sub-iteration per pass: a row block needs the ghost depth (1, 1), got (%d, %d)"
                                 % (blk.depth_below, blk.depth_above))
            missing = [m for m in self.BBM_OPS if not callable(getattr(ops, m, None))]
            if missing:
                raise ValueError("rheology='bbm' needs an ops object with the BBM calls of the C ABI (abi.Context); %s has no %s"
                                 % (type(ops).__name__, ", ".join(missing)))
            if len(self.TRANSPORTED) + 1 > 4:  # NSDG_RB_MAX_FIELDS
                raise ValueError("rheology='bbm' with advect_column_state=True would advect %d fields (%s and D); a transport step carries at most 4"
                                 % (len(self.TRANSPORTED) + 1, ", ".join(self.TRANSPORTED)))
            self.TRANSPORTED = self.TRANSPORTED + ("D",)
            self.BOUNDS = self.BOUNDS + (self.DAMAGE_BOUNDS,)
            if bbm is not None:
                ops.set_bbm_params(bbm)
        elif bbm is not None:
            raise ValueError("bbm= parameters need rheology='bbm'")
        # land: bool array [ny_global, nx] of the WHOLE domain (True = land; include/nsdg.h "land mask"): the nodes of
        # land elements hold u = v = 0 like the array edge.  This rank keeps its rows, ghost rows included -- the mask is static, nothing
        # is exchanged -- and sets them on the ops object whenever it sets the grid
        self.land, self._land_on_ops = None, False
        if land is not None:
            import numpy as np

            missing = [m for m in self.LAND_OPS if not callable(getattr(ops, m, None))]
            if missing:
                raise ValueError("land= needs an ops object with the land-mask calls of the C ABI (abi.Context); %s has no %s"
                                 % (type(ops).__name__, ", ".join(missing)))
            land = np.asarray(land)
            if land.shape != (blk.ny_glob, blk.nx):
                raise ValueError("land must be a [ny_global, nx] = [%d, %d] array, got shape %s" % (blk.ny_glob, blk.nx, land.shape))
            self.land = torch.from_numpy(np.ascontiguousarray(land[blk.elem_slice()] != 0).astype(np.uint8)).to(device)
        # phase_timing: step() brackets its parts with the library's phase marks (include/nsdg.h "per-phase device timing": one event per
        # mark on the ops' stream, read by phase_times()); off, nothing is asked of `ops` beyond the kernels
        self._phase_timing = bool(phase_timing)
        self._in_advance, self._phase_open = False, PHASE_END
        if self._phase_timing:
            missing = [m for m in ("phase_timing", "phase_mark", "phase_times") if not callable(getattr(ops, m, None))]
            if missing:
                raise ValueError("phase_timing=True needs an ops object with the phase calls of the C ABI (abi.Context); %s has no %s"
                                 % (type(ops).__name__, ", ".join(missing)))
            ops.phase_timing(True)
        self.overlap = overlap
        # closure: cap + scaling limiter at the end of every transport step (the ice-free-node rule is a parameter of the
        # sub-cycle, on by default).  False: the bare scheme of rounds 1-4 (frozen fixtures of that scheme)
        self.closure = closure
        # the native driver's plan carries the bounds itself (nsdg_rb_transport_desc.own_bounds); the Python sequence of step calls reads
        # them from the context: stated here, put back by close() (they apply to EVERY later step call on the context: include/nsdg.h)
        self._bounds_before = getattr(ops, "transport_bounds", ())
        ops.set_transport_bounds(self.BOUNDS if closure else ())
        nf = len(self.TRANSPORTED)
        # native: the sub-cycle and the transport of a step are ONE C call each (csrc/rowblock.hip runs the same
        # sequence of passes and exchanges as subcycle() / transport() below); needs the C-ABI ops and, with
        # neighbours, a NativeHaloExchanger (it owns the communicator).  use_graph: replay the launches between
        # two exchanges as one hipGraph.
        self.native, self.use_graph = native, use_graph
        self._calls = {}
        # v sub-iterations per kernel pass (v = 4: variant 4, v = 3: variant 3, v = 2: variant 2) need a (v k, v k - 1) ghost depth
        # for k passes between two exchanges; a single domain has no ghosts at all.  All variants produce
        # bit-identical results, so a variant-3 context on a (2k, 2k-1) block simply uses the two-iteration kernel.
        variant = getattr(ops, "mevp_variant", None)
        self.per_pass = 1
        for v in (4, 3, 2):
            deep = blk.depth_below >= v and blk.depth_below % v == 0 and blk.depth_above == blk.depth_below - 1
            if variant is not None and variant >= v and (blk.world == 1 or deep):
                self.per_pass = v
                break
        if rheology == "bbm":  # multi-iteration passes of the brittle sub-cycle are not built
            self.per_pass = 1
        self.two_per_pass = self.per_pass >= 2  # the ghost zones hold stress rows as well as velocity rows
        self.group_passes = blk.depth_below // self.per_pass if (self.per_pass >= 2 and blk.world > 1) else 1  # passes between two exchanges
        self.halo = exchanger if exchanger is not None else HaloExchanger(blk)
        nx, ny = blk.nx, blk.ny
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)
        nodal = (2 * ny + 1, 2 * nx + 1)
        for name in self.TRANSPORTED:
            setattr(self, name, z(6, ny, nx))
        # stress and ice strength are private to the sub-cycle: the ops object chooses their layout
        self.s = [ops.private_zeros(8, ny, nx, device) for _ in range(3)]
        self.sb = [ops.private_zeros(8, ny, nx, device) for _ in range(3)]
        self.pg = ops.private_zeros(9, ny, nx, device)
        self.u, self.v, self.ub, self.vb = z(*nodal), z(*nodal), z(*nodal), z(*nodal)
        self.ua, self.va = z(*nodal), z(*nodal)
        self.uo, self.vo = z(*nodal), z(*nodal)
        self.packed = z(nodal[0] * nodal[1] * 8)  # per-step momentum coefficients, 8 per node
        self.adv = (z(6, ny, nx), z(6, ny, nx), z(3, ny, nx + 1), z(3, ny + 1, nx))
        self.t1 = [z(6, ny, nx) for _ in range(nf)]
        self.t2 = [z(6, ny, nx) for _ in range(nf)]
        if rheology == "bbm":
            # the damage ping-pong of the sub-cycle, the three per-step Gauss arrays (layout of pg) and the zeros the packing takes as u0, v0
            self.Db = z(6, ny, nx)
            self.hg, self.eg, self.pm = (ops.private_zeros(9, ny, nx, device) for _ in range(3))
            self._zero_nodal = z(*nodal)
        if self.history is not None:
            self._hist_acc = z(len(self.history), blk.j1 - blk.j0, nx)  # the owned rows only: a sample is element-local
            self._hist_count = 0
            if any(st == "ice_mean" for _, st in self._hist_pairs or ()):
                self._hist_wacc = z(blk.j1 - blk.j0, nx)  # the summed weights of the window, one plane for every ice-weighted mean
        if self.series is not None:
            self._series_buf = z(self.series_capacity, len(self.series), blk.j1 - blk.j0)
            self._series_count = 0
        self._drift = self._drift_b = None
        if drift0 is not None:  # the whole list on every rank, and the partner an out-of-place step writes
            self._drift = torch.from_numpy(drift0).to(device)
            self._drift_b = torch.empty_like(self._drift)
        if native:
            self._init_native()

    def _check_drifters(self, drifters, min_conc, ops, exchanger):
        """drifters= as a float64 [3, n] array (x, y, status), or None; ValueError for a list this core cannot carry"""
        if drifters is None:
            return None
        import math

        import numpy as np

        b = self.blk
        missing = [m for m in self.DRIFTER_OPS if not callable(getattr(ops, m, None))]
        if missing:
            raise ValueError("drifters= needs an ops object with the drifter call of the C ABI (abi.Context); %s has no %s"
                             % (type(ops).__name__, ", ".join(missing)))
        if not math.isfinite(min_conc):
            raise ValueError("drifter_min_conc must be finite, got %r" % (min_conc,))
        xy = np.array(drifters, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[1] not in (2, 3):
            raise ValueError("drifters must be an [n, 2] array of positions or an [n, 3] array with the status, got shape %s" % (xy.shape,))
        if not np.all(np.isfinite(xy)):
            raise ValueError("drifter %d has a non-finite value" % int(np.argwhere(~np.isfinite(xy))[0][0]))
        Lx, Ly = b.nx * self.hx, b.ny_glob * self.hy
        outside = ~((xy[:, 0] >= 0) & (xy[:, 0] <= Lx) & (xy[:, 1] >= 0) & (xy[:, 1] <= Ly))
        if outside.any():
            k = int(np.argwhere(outside)[0][0])
            raise ValueError("drifter %d at (%r, %r) m is outside the domain [0, %r] x [0, %r] m" % (k, float(xy[k, 0]), float(xy[k, 1]), Lx, Ly))
        d = np.zeros((3, xy.shape[0]))
        d[:xy.shape[1]] = xy.T
        bad = ~np.isin(d[2], (0.0, 1.0, 2.0, 3.0))
        if bad.any():
            k = int(np.argwhere(bad)[0][0])
            raise ValueError("drifter %d has the status %r; known: 0 active, 1 left the domain, 2 lost its ice, 3 on land" % (k, float(d[2, k])))
        if b.world > 1 and not isinstance(exchanger, NativeHaloExchanger) and not (dist.is_available() and dist.is_initialized()):
            raise ValueError("drifters= on %d row blocks merges the ranks' lists after every step: it needs a NativeHaloExchanger "
                             "(comm_max_f64_array) or an initialised torch.distributed process group (all_reduce); %s has neither"
                             % (b.world, "HaloExchanger" if exchanger is None else type(exchanger).__name__))
        return d

    def _drifters_step(self):
        """the drifters of the owned rows move by one Heun step of self.dt with the velocity the sub-cycle left and the concentration the
        transport left, then the ranks' lists are merged: a rank writes -inf for what it does not own, so the elementwise maximum is the
        whole list.  Out of place: the two arrays swap.  No phase of its own; inside the span, before its end mark"""
        if self._drift is None or self._drift.shape[1] == 0:
            return
        b = self.blk
        if b.world > 1 and not self.two_per_pass:
            # a predictor may sit in the ghost row above, whose upper node rows a single-iteration sub-cycle never receives (it needs
            # the lowest only): one exchange of the velocity with the ghost rows complete
            self.halo.nodal((self.u, self.v), rows_down=2 * b.depth_above + 1)
        self.ops.drifters_advance(b.j0, b.j1, self.dt, self.drifter_min_conc, self.u, self.v, self.A, self._drift, self._drift_b)
        self._drift, self._drift_b = self._drift_b, self._drift
        if b.world > 1:
            if isinstance(self.halo, NativeHaloExchanger):
                self.halo.ctx.comm_max_f64_array(self._drift)
            else:
                dist.all_reduce(self._drift, op=dist.ReduceOp.MAX, group=self.halo.group)

    def drifters_read(self):
        """{"x", "y": float64 [n] in metres of the global domain, "status": int64 [n]} -- the whole list, identical on every rank (one
        download; waits for the last step)"""
        if self._drift is None:
            raise ValueError("drifters_read() needs a core constructed with drifters=")
        import numpy as np

        d = self._drift.detach().cpu().numpy()
        return {"x": d[0].copy(), "y": d[1].copy(), "status": d[2].astype(np.int64)}

    def _check_history(self, history, rheology, ops):
        """the entries of history= as a tuple, or None; ValueError for a list this core cannot sample.  Sets self._hist_pairs: None for a
        list of bare names -- sampled by ops.history_accumulate, as ever --, else the (field, stat) of every entry"""
        self._hist_pairs = None
        if history is None:
            return None
        from nextsimdg_amd import abi

        if isinstance(history, str):
            history = (history,)
        history = tuple(history)
        if not history:
            raise ValueError("history= needs at least one field (None turns it off)")
        pairs = [tuple(e.split(":", 1)) if ":" in e else (e, "mean") for e in history]
        names = [n for n, _ in pairs]
        unknown = [n for n in names if n not in abi.HISTORY_FIELDS]
        if unknown:
            raise ValueError("unknown history field %s (known: %s)" % (", ".join(repr(n) for n in unknown), " ".join(abi.HISTORY_FIELDS)))
        unknown = [e for e, (_, st) in zip(history, pairs) if st not in abi.HISTORY_STATS]
        if unknown:
            raise ValueError("unknown history statistic in %s (known: %s)" % (", ".join(repr(e) for e in unknown), " ".join(abi.HISTORY_STATS)))
        twice = sorted({e for e, p in zip(history, pairs) if pairs.count(p) > 1})
        if twice:
            raise ValueError("history field %s is listed twice" % ", ".join(repr(n) for n in twice))
        if "damage" in names and rheology != "bbm":
            raise ValueError("the history field 'damage' needs rheology='bbm': the mEVP sub-cycle has no damage")
        column = [n for n in names if n in self.HISTORY_COLUMN_FIELDS]
        if column and not self.HAS_COLUMN_STATE:
            raise ValueError("the history field %s is column state: it needs a CoupledCore" % ", ".join(repr(n) for n in column))
        weighted = [e for e, (_, st) in zip(history, pairs) if st == "ice_mean"]
        if weighted and "A" not in self.TRANSPORTED:
            raise ValueError("the history entry %s weights by the concentration: this core has no A" % ", ".join(repr(e) for e in weighted))
        call = "history_accumulate_stats" if any(":" in e for e in history) else "history_accumulate"
        if not callable(getattr(ops, call, None)):
            raise ValueError("history= needs an ops object with the history call of the C ABI (abi.Context); %s has no %s"
                             % (type(ops).__name__, call))
        if call == "history_accumulate_stats":
            self._hist_pairs = pairs
        return history

    def _check_series(self, series, capacity, extent_conc, ops):
        """the quantities of series= as a tuple, or None; ValueError for a list this core cannot total"""
        if series is None:
            return None
        import math

        from nextsimdg_amd import abi

        if isinstance(series, str):
            series = (series,)
        series = tuple(series)
        if not series:
            raise ValueError("series= needs at least one quantity (None turns it off)")
        unknown = [n for n in series if n not in abi.SERIES_QUANTITIES]
        if unknown:
            raise ValueError("unknown series quantity %s (known: %s)" % (", ".join(repr(n) for n in unknown), " ".join(abi.SERIES_QUANTITIES)))
        twice = sorted({n for n in series if series.count(n) > 1})
        if twice:
            raise ValueError("series quantity %s is listed twice" % ", ".join(repr(n) for n in twice))
        if "drift" in series and "area" not in series:
            raise ValueError("the series quantity 'drift' is the ice-weighted mean speed: it needs 'area', the sum of the weights, in the list")
        if "snow_volume" in series and not self.HAS_COLUMN_STATE:
            raise ValueError("the series quantity 'snow_volume' is column state: it needs a CoupledCore")
        if int(capacity) < 1:
            raise ValueError("series_capacity must be at least 1, got %r" % (capacity,))
        if not math.isfinite(extent_conc):
            raise ValueError("extent_conc must be finite, got %r" % (extent_conc,))
        if not callable(getattr(ops, "history_row_totals", None)):
            raise ValueError("series= needs an ops object with the row totals of the C ABI (abi.Context); %s has no history_row_totals"
                             % type(ops).__name__)
        return series

    def _history_sources(self):
        """the current ping-pong side of everything a sample reads"""
        src = {"H": self.H, "A": self.A, "u": self.u, "v": self.v, "s11": self.s[0], "s12": self.s[1], "s22": self.s[2]}
        if self.rheology == "bbm":
            src["D"] = self.D
        return src

    def _history_sample(self):
        """one sample of the owned rows at the end of a model step: one launch, after the step's last phase mark and outside every
        captured graph; the first sample of a window stores, the others add"""
        if self.series is not None:
            self._series_sample()
        if self.history is None:
            return
        b = self.blk
        if self._hist_pairs is None:
            self.ops.history_accumulate(b.j0, b.j1, self.history, self._history_sources(), self._hist_count == 0, b.j0, self._hist_acc)
        else:
            self.ops.history_accumulate_stats(b.j0, b.j1, self._hist_pairs, self._history_sources(), self._hist_count == 0, b.j0, self._hist_acc,
                                              getattr(self, "_hist_wacc", None))
        self._hist_count += 1

    def _series_room(self):
        """a model step begins: ValueError if its row totals would find no free slot.  The host counts the slots; nothing is synchronised"""
        if self.series is not None and not self._in_advance and self._series_count >= self.series_capacity:
            raise ValueError("the series buffer is full (series_capacity = %d samples): call series_read() before the next step"
                             % self.series_capacity)

    def _series_sample(self):
        """the row totals of the owned rows at the end of a model step: one launch into the next free slot"""
        b = self.blk
        self.ops.history_row_totals(b.j0, b.j1, self.series, self._history_sources(), self.extent_conc, b.j0, self._series_buf[self._series_count])
        self._series_count += 1

    def history_read(self, reset=True):
        """{"rows": (r0, r1), "count": n, name: float64 [rows, nx] = the mean of the n samples since the last reset} for the rows this rank
        owns (one download; waits for the last sample).  reset: the next sample opens a new window.  merge_history() joins the ranks"""
        if self.history is None:
            raise ValueError("history_read() needs a core constructed with history=")
        if self._hist_count == 0:
            raise ValueError("history_read(): no sample since the last reset")
        b, n = self.blk, self._hist_count
        acc = self._hist_acc.detach().cpu().numpy()
        out = {"rows": (b.r0, b.r1), "count": n}
        if self._hist_pairs is None:
            for k, name in enumerate(self.history):
                out[name] = acc[k] / n
        else:
            import numpy as np

            wacc = self._hist_wacc.detach().cpu().numpy() if hasattr(self, "_hist_wacc") else None
            for k, (entry, (_, stat)) in enumerate(zip(self.history, self._hist_pairs)):
                if stat == "mean":
                    out[entry] = acc[k] / n
                elif stat == "ice_mean":  # NaN where the window saw no ice
                    iced = wacc > 0
                    out[entry] = np.where(iced, acc[k] / np.where(iced, wacc, 1.0), np.nan)
                else:
                    out[entry] = acc[k].copy()
        if reset:
            self._hist_count = 0
        return out

    def series_read(self, reset=True):
        """{"rows": (r0, r1), "count": n, name: float64 [n, rows] = the row totals of the n steps since the last reset} for the rows this
        rank owns, as the device left them (one download; waits for the last step).  reset: the next step writes slot 0 again.
        merge_series() makes the totals of the whole domain"""
        if self.series is None:
            raise ValueError("series_read() needs a core constructed with series=")
        b, n = self.blk, self._series_count
        buf = self._series_buf[:n].detach().cpu().numpy()
        out = {"rows": (b.r0, b.r1), "count": n}
        for k, name in enumerate(self.series):
            out[name] = buf[:, k].copy()
        if reset:
            self._series_count = 0
        return out

    @staticmethod
    def merge_series(parts, hx, hy):
        """the ranks' series_read()s (any order) -> {"count": n, name: float64 [n]}: area and extent in m^2, volume and snow_volume in
        m^3, drift = sum(w speed) / sum(w) in m/s (NaN where there is no ice), speed_max, hice_max.  The rows of a sample are added one
        after the other in global row order, whatever the decomposition, so one block and N blocks give the same bits"""
        import numpy as np

        parts = sorted(parts, key=lambda p: p["rows"][0])
        if any(p["count"] != parts[0]["count"] for p in parts):
            raise ValueError("the ranks hold different numbers of samples: %s" % [p["count"] for p in parts])
        if any(a["rows"][1] != c["rows"][0] for a, c in zip(parts, parts[1:])):
            raise ValueError("the ranks' rows do not join: %s" % [p["rows"] for p in parts])
        n = parts[0]["count"]
        out = {"rows": (parts[0]["rows"][0], parts[-1]["rows"][1]), "count": n}
        raw = {}
        for k in parts[0]:
            if k in ("rows", "count"):
                continue
            rows = np.concatenate([p[k] for p in parts], axis=1)
            if k in ("speed_max", "hice_max"):  # np.maximum keeps a NaN, as the rows do
                raw[k] = np.maximum.accumulate(rows, axis=1)[:, -1] if n else np.zeros(0)
            else:  # sequential in row order: np.sum would add pairwise
                raw[k] = np.add.accumulate(rows, axis=1)[:, -1] if n else np.zeros(0)
        cell = hx * hy
        for k, v in raw.items():
            if k == "drift":
                if "area" not in raw:
                    raise ValueError("'drift' needs 'area' in the series")
                iced = raw["area"] > 0
                out[k] = np.where(iced, v / np.where(iced, raw["area"], 1.0), np.nan)
            elif k in ("area", "extent", "volume", "snow_volume"):
                out[k] = v * cell
            else:
                out[k] = v
        return out

    @staticmethod
    def merge_history(parts):
        """the ranks' history_read()s (any order) -> the record of the whole domain"""
        import numpy as np

        parts = sorted(parts, key=lambda p: p["rows"][0])
        if any(p["count"] != parts[0]["count"] for p in parts):
            raise ValueError("the ranks hold different numbers of samples: %s" % [p["count"] for p in parts])
        if any(a["rows"][1] != c["rows"][0] for a, c in zip(parts, parts[1:])):
            raise ValueError("the ranks' rows do not join: %s" % [p["rows"] for p in parts])
        out = {"rows": (parts[0]["rows"][0], parts[-1]["rows"][1]), "count": parts[0]["count"]}
        for k in parts[0]:
            if k not in ("rows", "count"):
                out[k] = np.concatenate([p[k] for p in parts], axis=0)
        return out

    def _init_native(self):
        b = self.blk
        if b.world > 1 and not isinstance(self.halo, NativeHaloExchanger):
            raise ValueError("the native driver exchanges ghost rows through the C ABI: pass a NativeHaloExchanger")
        peers = (self.halo.peer_below, self.halo.peer_above) if b.world > 1 else (None, None)
        self._sbuf, self._uvbuf, self._par = (self.s, self.sb), ((self.u, self.v), (self.ub, self.vb)), 0
        self._run_mevp, per_pass, group = self.ops.rb_mevp(b, peers, self.nsub, self.overlap, self.use_graph, self._sbuf, self._uvbuf,
                                                           self.packed, self.pg)
        assert (per_pass, group) == (self.per_pass, self.group_passes), "native plan and driver disagree on the pass structure"
        self._fbuf, self._tpar = (self._fields(), tuple(self.t1)), 0
        self._run_transport = self.ops.rb_transport(b, peers, self._fbuf[0], self._fbuf[1], self.t2, self.adv, bounds=self.BOUNDS if self.closure else ())

    def _fields(self):
        """the current buffers of the advected fields, in the order of TRANSPORTED"""
        return tuple(getattr(self, name) for name in self.TRANSPORTED)

    def _set_fields(self, fields):
        for name, f in zip(self.TRANSPORTED, fields):
            setattr(self, name, f)

    def close(self):
        """releases the native driver plans (device buffers and events of their ghost exchanges); call it before the
        context is closed"""
        for name in ("_run_mevp", "_run_transport"):
            run = getattr(self, name, None)
            if run is not None and hasattr(run, "close"):
                run.close()
            setattr(self, name, None)
        if self._bounds_before is not None:  # the context is as this core found it
            self.ops.set_transport_bounds(self._bounds_before)
            self._bounds_before = None
        if self._land_on_ops:  # set with the grid (_set_grid)
            self.ops.set_land_mask(None)
        self.land, self._land_on_ops = None, False

    def load_global(self, H, A, uo, vo, ua, va, u=None, v=None, D=None):
        """fill the local arrays (ghost rows included) from global numpy arrays; D: the damage of rheology="bbm" (None: left as it is)"""
        es, ns = self.blk.elem_slice(), self.blk.node_slice()
        put = lambda dst, src: dst.copy_(torch.from_numpy(src).to(dst.device))
        import numpy as np

        put(self.H, np.ascontiguousarray(H[:, es]))
        put(self.A, np.ascontiguousarray(A[:, es]))
        for dst, src in ((self.uo, uo), (self.vo, vo), (self.ua, ua), (self.va, va)):
            put(dst, np.ascontiguousarray(src[ns]))
        if u is not None:
            put(self.u, np.ascontiguousarray(u[ns]))
            put(self.v, np.ascontiguousarray(v[ns]))
        if D is not None:
            if self.rheology != "bbm":
                raise ValueError("a damage field needs rheology='bbm'")
            put(self.D, np.ascontiguousarray(D[:, es]))
        self._clear_land()

    def _clear_land(self):
        """no ice on land, no motion at land nodes: whatever a caller loaded there is cleared (a store: a NaN goes too)"""
        if self.land is None:
            return
        self._set_grid()
        for f in self._fields():
            self.ops.land_clear(f)
        self.ops.land_clear_nodes(self.u, self.v)

    def _set_grid(self):
        self.ops.set_grid(self.blk.nx, self.blk.ny, self.hx, self.hy)
        if self.land is not None:
            self.ops.set_land_mask(self.land)
            self._land_on_ops = True
        place = getattr(self.ops, "set_block", None)
        if place is not None:  # where the local array sits in the global domain (device-side forcing providers)
            place(self.blk.lo, self.blk.ny_glob)

    def device_wind(self, domain_size, t):
        """cyclone wind of the box test at model time t, evaluated on the device for this rank's rows"""
        self._set_grid()
        self.ops.boxtest_forcing(domain_size, t, wind=(self.ua, self.va))

    def _mark(self, phase):
        if self._phase_timing and phase != self._phase_open:  # (a phase that already runs goes on: CoupledCore.transport wraps this class's)
            self.ops.phase_mark(phase)
            self._phase_open = phase

    def phase_times(self, reset=False):
        """{phase name: (device ms, closed intervals), "total": (ms, spans)} of the steps so far; waits for the last mark.  A span is one
        step() -- or one advance(), with all its sub-steps -- timed from its first mark to its end by its own pair of events"""
        from nextsimdg_amd import abi

        if not self._phase_timing:
            raise ValueError("phase_times() needs a core constructed with phase_timing=True")
        phases, total = self.ops.phase_times(reset)
        out = {(abi.PHASES[k] if k < len(abi.PHASES) else "phase %d" % k): v for k, v in phases.items()}
        out["total"] = total
        return out

    def momentum(self):
        self._mark(PHASE_PREPARE)
        self.prepare()
        self._mark(PHASE_SUBCYCLE)
        self.subcycle()

    def prepare(self):
        """once per model step: ice strength at the Gauss points, nodal means of H and A, wind stress and the packed
        momentum coefficients (one launch); the velocity at the start of the step is read from the current iterate
        (it is only needed inside the packing)"""
        ops, b = self.ops, self.blk
        if self.rheology == "bbm":
            # the Gauss arrays of the brittle sub-cycle, and the mEVP packing for the sub-step dt / nsub with u0 = v0 = 0
            ops.bbm_prepare(self.H, self.A, self.hg, self.eg, self.pm, 0, b.ny)
            ops.mevp_prepare(self.dt / self.nsub, self.H, self.A, (self.ua, self.va), (self.uo, self.vo), (self._zero_nodal, self._zero_nodal),
                             self.packed)
            return
        ops.ice_strength(self.H, self.A, self.pg, 0, b.ny)
        ops.mevp_prepare(self.dt, self.H, self.A, (self.ua, self.va), (self.uo, self.vo), (self.u, self.v), self.packed)

    def passes_per_step(self):
        """kernel launches of the dominant kernel per sub-cycle on an unsplit block: (launches with per_pass
        sub-iterations, two-iteration remainders, single sub-iterations)"""
        n, v = self.nsub, self.per_pass
        if v == 1:
            return 0, 0, n
        full, rest = n // v, n % v  # the remainder runs through the kernels with fewer sub-iterations per pass: 3 -> one
        if rest == 3:  # three-iteration pass (counted with the "twos": a minority launch), 2 -> one two-iteration pass, 1 -> a single
            return full, 1, 0
        return full, rest // 2, rest % 2

    def subcycle(self):
        """the nsub mEVP sub-iterations of one model step (ghost rows exchanged as the ghost depth requires)"""
        ops, b = self.ops, self.blk
        if self.native:
            par = self._par = self._run_mevp(self._par)
            self.s, self.sb = self._sbuf[par], self._sbuf[1 - par]
            (self.u, self.v), (self.ub, self.vb) = self._uvbuf[par], self._uvbuf[1 - par]
            return
        it = 0
        if self.per_pass >= 2:
            # v sub-iterations per pass (the intermediate stress / velocity stay on chip).  With several ranks the
            # passes run in groups of k = group_passes: pass i of a group of m covers the owned rows plus
            # v(m-i) ghost rows on each side (what the remaining passes of the group will read), and only
            # after the last pass the ghost rows of the new stress and velocity are exchanged.  What is left
            # of nsub after the v-passes is done by a two-iteration pass and / or single sub-iterations.
            k = self.group_passes
            split_ok = self.overlap and b.world > 1 and (b.j1 - b.j0) >= b.depth_below + b.depth_above + 5
            for v in range(self.per_pass, 1, -1):
                while self.nsub - it >= v:
                    m = min(k, (self.nsub - it) // v)
                    for i in range(1, m + 1):
                        last = i == m
                        calls = self._pass_calls(v, split_ok and last, m - i)
                        for c in calls[:-1]:
                            c()
                        pending = self._ghost_exchange_start() if (split_ok and last) else None
                        calls[-1]()
                        if last:
                            if pending is None:
                                pending = self._ghost_exchange_start()
                            self._ghost_exchange_finish(pending)
                        self._swap()
                        it += v
        split = self.overlap and b.world > 1 and (b.j1 - b.j0) >= 4 and not self.two_per_pass
        for _ in range(self.nsub - it):
            uvn = (self.ub, self.vb)
            calls = self._iterate_calls(split)
            if not split:
                calls[0]()
                if self.two_per_pass:  # keep the deeper ghost zones (stress as well as velocity) of the multi-iteration passes consistent
                    self._ghost_exchange_finish(self._ghost_exchange_start())
                else:
                    self.halo.nodal(uvn)
            else:
                # boundary rows first, so that their node rows travel while the interior is computed:
                # the exchange is posted after the boundary launches and before the interior launch, the
                # communication stream therefore waits only for the former
                for c in calls[:-1]:
                    c()
                reqs = self.halo.nodal_start(uvn)
                calls[-1]()
                self.halo.finish(reqs)
            self._swap()
        if self.rheology == "bbm" and b.world > 1 and self.nsub > 0:
            # inside the sub-cycle the damage of the ghost row below is recomputed and the ghost row above is never read: one exchange
            # hands the transport its ghost rows
            self.halo.element([self.D])

    def _swap(self):
        """a pass has written the other half of the ping-pong: the velocity, the stress and, for the brittle rheology, the damage"""
        self.u, self.ub = self.ub, self.u
        self.v, self.vb = self.vb, self.v
        self.s, self.sb = self.sb, self.s
        if self.rheology == "bbm":
            self.D, self.Db = self.Db, self.D

    def _bind(self, name):
        """a call of ops.<name> with its arguments bound once: the binding fast path of the C ABI, or a closure"""
        ops = self.ops
        bind = getattr(ops, "bind_" + name, None)
        if bind is None:  # ops without a binding fast path (the CPU test stand-in)
            bind = lambda *a: (lambda: getattr(ops, name)(*a))
        return bind

    def _ghost_exchange_start(self):
        """ghost zones of the multi-iteration passes, depth (d, d-1) with d = v k: velocity node rows (2d up, 2d-1
        down) and stress rows (d up, d-1 down) in one batch"""
        if self.blk.world == 1:
            return None
        return self.halo.rows_exchange_start(self.sb, self.ops.private_rows, nodal_fields=(self.ub, self.vb),
                                             rows_down=2 * self.blk.depth_above + 1)

    def _ghost_exchange_finish(self, pending):
        if pending is not None:
            self.halo.rows_exchange_finish(*pending)

    def _pass_calls(self, v, split, ext=0):
        """launches of one pass of v (2, 3 or 4) sub-iterations for the current ping-pong parity (bound once, cached).
        ext > 0: a pass inside a group, one launch over the owned rows extended by v*ext ghost rows on each
        side.  ext == 0 and split: the rows whose results travel to the neighbours first, the interior last"""
        key = (self.u.data_ptr(), self.s[0].data_ptr(), split, v, ext)
        calls = self._calls.get(key)
        if calls is not None:
            return calls
        b = self.blk
        uv, uvn = (self.u, self.v), (self.ub, self.vb)
        bind = self._bind("mevp_iterate%d" % v)
        rng = []
        lo, hi = max(b.j0 - v * ext, 0), min(b.j1 + v * ext, b.ny)
        if split and ext == 0:
            if b.above is not None:  # top owned element rows: depth_below stress rows + 2*depth_below node rows go up
                rng.append((b.j1 - b.depth_below, b.j1))
                hi = b.j1 - b.depth_below
            if b.below is not None:  # bottom owned element rows: depth_above stress rows + 2*depth_above+1 node rows go down
                rng.append((b.j0, b.j0 + b.depth_above + 1))
                lo = b.j0 + b.depth_above + 1
        rng.append((lo, hi))
        calls = [bind(j0, j1, self.s, self.sb, uv, uvn, self.packed, self.pg) for (j0, j1) in rng]
        self._calls[key] = calls
        return calls

    def _iterate_calls(self, split):
        """the launches of one sub-iteration for the current ping-pong parity, bound once and cached"""
        bbm = self.rheology == "bbm"
        key = (self.u.data_ptr(), self.s[0].data_ptr(), split) + ((self.D.data_ptr(), self.Db.data_ptr()) if bbm else ())
        calls = self._calls.get(key)
        if calls is not None:
            return calls
        b = self.blk
        uv, uvn = (self.u, self.v), (self.ub, self.vb)
        bind = self._bind("bbm_iterate" if bbm else "mevp_iterate")
        rng = []
        if not split:
            rng.append((b.k0, b.j0, b.j1))  # k0 = j0 - 1: the ghost row just below is updated redundantly
        else:
            lo, hi = b.j0, b.j1
            if b.above is not None:  # top owned element row -> the two node rows sent upwards
                rng.append((b.j1 - 2, b.j1 - 1, b.j1))
                hi = b.j1 - 1
            if b.below is not None:  # bottom owned element row (+ redundant ghost-row stress) -> node row sent downwards
                rng.append((b.j0 - 1, b.j0, b.j0 + 1))
                lo = b.j0 + 1
            rng.append((lo - 1 if lo > 0 else 0, lo, hi))  # interior, launched after the exchange is posted
        if bbm:
            calls = [bind(k0, j0, j1, self.s, self.sb, self.D, self.Db, uv, uvn, self.packed, (self.hg, self.eg, self.pm)) for (k0, j0, j1) in rng]
        else:
            calls = [bind(k0, j0, j1, self.s, self.sb, uv, uvn, self.packed, self.pg) for (k0, j0, j1) in rng]
        self._calls[key] = calls
        return calls

    def transport(self):
        ops, b = self.ops, self.blk
        self._mark(PHASE_TRANSPORT)
        ops.prepare_advection(self.ORDER, self.u, self.v, *self.adv)
        if self.native:
            par = self._tpar = self._run_transport(self.dt, self._tpar)
            self._set_fields(self._fbuf[par])
            self.t1[:] = self._fbuf[1 - par]
            return
        f = list(self._fields())
        # Shu-Osher SSP-RK3: out = a*phi0 + b*(phis + dt L(phis)).  A stage reads one element row on each side
        # of the rows it updates: with at least 3 ghost rows per interior side the first two stages also
        # advance 2 / 1 ghost rows redundantly (bit-identically to their owners) and the ghost rows are
        # exchanged once per step instead of after every stage.
        deep = b.world > 1 and min(b.depth_below, b.depth_above) >= 3
        ext = (lambda e: (max(b.j0 - e, 0), min(b.j1 + e, b.ny))) if deep else (lambda e: (b.j0, b.j1))
        ops.transport_stage(self.ORDER, *ext(2), self.dt, 0.0, 1.0, f, f, self.t1, self.adv)
        if not deep:
            self.halo.element(self.t1)
        ops.transport_stage(self.ORDER, *ext(1), self.dt, 0.75, 0.25, f, self.t1, self.t2, self.adv)
        if not deep:
            self.halo.element(self.t2)
        ops.transport_stage(self.ORDER, b.j0, b.j1, self.dt, 1.0 / 3.0, 2.0 / 3.0, f, self.t2, self.t1, self.adv)
        if self.closure:  # the step entry points of the library do this themselves; a step composed of stages calls it
            ops.transport_limit(self.ORDER, b.j0, b.j1, self.t1)
        self.halo.element(self.t1)
        # the new state is t1 (ghost rows refreshed); swap buffers instead of copying
        new = list(self.t1)
        self.t1[:] = f
        self._set_fields(new)

    def step(self):
        self._series_room()
        self._set_grid()
        self.momentum()
        self.transport()
        self._drifters_step()
        if not self._in_advance:
            self._mark(PHASE_END)
            self._history_sample()

    # ---- sub-stepping (include/nsdg.h "sub-stepping"): a model step of model_dt run as n steps of model_dt / n
    def substep_count(self, model_dt, courant=None, max_substeps=16, params=None):
        """(n, amax, c): the number of sub-steps the state asks for (nsdg_substep_count) from the largest concentration of the owned rows
        (ops.concentration_max), the same on every rank: the maximum over the ranks goes through nsdg_comm_max_f64 on a
        NativeHaloExchanger's communicator and through torch.distributed (MAX on a CPU scalar) otherwise.  params: the MevpParams whose
        pstar, compaction and rho_ice give the wave speed (default: nsdg_mevp_default_params)"""
        from nextsimdg_amd import abi

        b = self.blk
        self._set_grid()
        amax = self.ops.concentration_max(self.H, self.A, b.j0, b.j1)
        if isinstance(self.halo, NativeHaloExchanger):
            amax = self.halo.ctx.comm_max_f64(amax)
        elif b.world > 1:
            t = torch.tensor([amax], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.halo.group)
            amax = float(t.item())
        if params is None:
            params = abi.MevpParams()
            abi.load_library().nsdg_mevp_default_params(abi.C.byref(params))
        n, c = abi.substep_count(params, amax, min(self.hx, self.hy), model_dt, abi.SUBSTEP_COURANT if courant is None else courant,
                                 max_substeps)
        return n, amax, c

    def advance(self, model_dt, substeps=1, courant=None, max_substeps=16, params=None):
        """one model step of model_dt as n calls of step() with self.dt = model_dt / n (restored afterwards); substeps: an int >= 1, or
        "auto" (n from the state at the start of the step, substep_count).  Returns n; substeps = 1 is step() at model_dt, bit for bit"""
        self._series_room()
        if substeps == "auto":
            self._mark(PHASE_REDUCTION)
            n = self.substep_count(model_dt, courant, max_substeps, params)[0]
        elif isinstance(substeps, int) and not isinstance(substeps, bool) and substeps >= 1:
            n = substeps
        else:
            raise ValueError("substeps must be an integer >= 1 or 'auto', got %r" % (substeps,))
        dt = self.dt
        self.dt = model_dt / n
        self._in_advance = True  # the span of the phase table is the model step: one end mark after the last sub-step
        try:
            for _ in range(n):
                self.step()
        finally:
            self.dt = dt
            self._in_advance = False
            self._mark(PHASE_END)
        self._history_sample()  # one sample per model step, after its last sub-step
        return n

    def owned(self, f):
        """owned element rows of a DG array / owned node rows of a nodal array (for gathering)"""
        b = self.blk
        if any(f is x for x in self.s + self.sb + [self.pg] + ([self.hg, self.eg, self.pm] if self.rheology == "bbm" else [])):
            return self.ops.private_rows(f, b.j0, b.j1)
        if f.dim() == 3:
            return f[:, b.j0:b.j1]
        top = 2 * b.j1 + (1 if b.above is None else 0)
        return f[2 * b.j0:top]


    # ---- checkpoint / resume (round 6).  The state a run carries from one step to the next: the DG2 fields H and A, the velocity and the
    # stress -- what the C++ host writes into its restart file (host/include/RectGrid.hpp: hice, cice, hice_dg, cice_dg, u, v, s11, s12,
    # s22), which the reference's restart files are the model for (core/src/DevGridIO.cpp:169-201: every prognostic field it has).
    def state_dict(self):
        """numpy arrays of the rows this rank OWNS (H, A: [6, rows, nx]; u, v: owned node rows; s11, s12, s22: [8, rows, nx] coefficient
        planes) and the position of the rows in the global domain: concatenating the ranks' dictionaries along the row axis gives the
        global state, load_state_dict takes either"""
        b = self.blk
        nx = b.nx
        out = {"rows": (b.r0, b.r1), "ny_global": b.ny_glob, "nx": nx}
        for name, f in (("H", self.H), ("A", self.A), ("u", self.u), ("v", self.v)):
            out[name] = self.owned(f).detach().cpu().numpy().copy()
        for name, f in zip(("s11", "s12", "s22"), self.s):
            out[name] = self.ops.private_to_planes(f, nx)[:, b.j0:b.j1].detach().cpu().numpy().copy()
        if self.rheology == "bbm":
            out["D"] = self.owned(self.D).detach().cpu().numpy().copy()
        if self._drift is not None:  # the whole list, not row-sliced: every rank holds the same
            out["drifters"] = self._drift.detach().cpu().numpy().copy()
        return out

    def load_state_dict(self, state):
        """resume from a GLOBAL state (rows (0, ny_global): e.g. the ranks' state_dict()s concatenated): fills the local arrays, ghost rows
        included, and the current ping-pong buffers; forcing (load_global) and column fields are loaded as for a fresh run"""
        import numpy as np

        b = self.blk
        if tuple(state["rows"]) != (0, b.ny_glob) or state["nx"] != b.nx:
            raise ValueError("load_state_dict needs the state of the whole domain (rows (0, %d)), got rows %s" % (b.ny_glob, (state["rows"],)))
        es, ns = b.elem_slice(), b.node_slice()
        put = lambda dst, src: dst.copy_(torch.from_numpy(np.ascontiguousarray(src)).to(dst.device))
        put(self.H, state["H"][:, es])
        put(self.A, state["A"][:, es])
        put(self.u, state["u"][ns])
        put(self.v, state["v"][ns])
        for f, name in zip(self.s, ("s11", "s12", "s22")):
            f.copy_(self.ops.planes_to_private(torch.from_numpy(np.ascontiguousarray(state[name][:, es])).to(f.device)))
        if self.rheology == "bbm":
            if "D" not in state:
                raise ValueError("a core with rheology='bbm' needs the damage D in the state")
            put(self.D, state["D"][:, es])
        if self._drift is not None:
            if "drifters" not in state or tuple(state["drifters"].shape) != tuple(self._drift.shape):
                raise ValueError("a core with drifters= needs the [3, %d] array 'drifters' in the state" % self._drift.shape[1])
            put(self._drift, state["drifters"])
        self._clear_land()

    @staticmethod
    def merge_states(states):
        """the ranks' state_dict()s (any order) -> the state of the whole domain"""
        import numpy as np

        states = sorted(states, key=lambda s: s["rows"][0])
        out = {"rows": (states[0]["rows"][0], states[-1]["rows"][1]), "ny_global": states[0]["ny_global"], "nx": states[0]["nx"]}
        for k in ("H", "A", "S", "D", "s11", "s12", "s22"):
            if k in states[0]:  # S: the snow of a CoupledCore with advect_column_state; D: the damage of rheology="bbm"
                out[k] = np.concatenate([s[k] for s in states], axis=1)
        for k in ("u", "v"):
            out[k] = np.concatenate([s[k] for s in states], axis=0)
        if "drifters" in states[0]:  # every rank holds the whole list
            assert all(np.array_equal(s["drifters"], states[0]["drifters"]) for s in states), "the ranks' drifter lists differ"
            out["drifters"] = states[0]["drifters"].copy()
        return out


class ForcingSeries:
    """Forcing records on one lattice at model times (include/nsdg.h "forcing from a file"; the C++ host reads the same records from a
    file, host/include/ForcingFile.hpp).  times: strictly increasing model times [s] (the clock of CoupledCore.time); fields: name ->
    float64 array [nt, nyr, nxr] on a cell-centred lattice over the square domain.  Names: the column planes tair tdew slp qsw qlw mld
    snowfall, and the pairs wind_u / wind_v and ocean_u / ocean_v (each pair complete or absent).  A time outside [times[0], times[-1]]
    is an error: there is no extrapolation."""

    COLUMN = ("tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall")
    WIND = ("wind_u", "wind_v")
    OCEAN = ("ocean_u", "ocean_v")

    def __init__(self, times, fields):
        import numpy as np

        t = np.array(times, dtype=np.float64)
        if t.ndim != 1 or t.size < 1:
            raise ValueError("times must be a 1-d array of at least one record time")
        if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
            raise ValueError("times must be finite and strictly increasing")
        if not fields:
            raise ValueError("a forcing series needs at least one field")
        known = self.COLUMN + self.WIND + self.OCEAN
        out = {}
        for name, a in fields.items():
            if name not in known:
                raise ValueError("unknown forcing field %r (known: %s)" % (name, " ".join(known)))
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.ndim != 3 or a.shape[0] != t.size or min(a.shape) < 1:
                raise ValueError("forcing field %r has shape %s, expected (%d, nyr, nxr)" % (name, a.shape, t.size))
            if not np.all(np.isfinite(a)):
                k = int(np.argwhere(~np.isfinite(a))[0][0])
                raise ValueError("forcing field %r has a non-finite value in record %d" % (name, k))
            out[name] = a
        shapes = {a.shape for a in out.values()}
        if len(shapes) != 1:
            raise ValueError("all forcing fields must be on one lattice, got shapes %s" % sorted(shapes))
        for pair in (self.WIND, self.OCEAN):
            if (pair[0] in out) != (pair[1] in out):
                raise ValueError("forcing fields %s and %s come as a pair" % pair)
        self.times, self.fields = t, out
        _, self.nyr, self.nxr = shapes.pop()

    def bracket(self, t):
        """(k0, k1, w): the records around model time t and the weight of k1 -- k0 is the last record with times[k0] <= t, k1 = k0 + 1,
        w = (t - times[k0]) / (times[k1] - times[k0]); at the last record itself k1 = k0 and w = 0"""
        import numpy as np

        t0, t1 = float(self.times[0]), float(self.times[-1])
        if not (t0 <= t <= t1):
            raise ValueError("model time %r s is outside the forcing records [%r, %r] s" % (t, t0, t1))
        k0 = int(np.searchsorted(self.times, t, side="right")) - 1
        if k0 == self.times.size - 1:
            return k0, k0, 0.0
        return k0, k0 + 1, (t - float(self.times[k0])) / (float(self.times[k0 + 1]) - float(self.times[k0]))


class CoupledCore(DynamicsCore):
    """BASELINE config 5: dynamics + column thermodynamics.  Each model step first advances the column
    physics of every owned element (the reference's DevStep::iterate, core/src/DevStep.cpp:14-23) and then
    the dynamics.  The coupling is zero-copy: the cell means of the DG fields ARE the column model's
    prognostic variables -- plane 0 of H is `hice`, plane 0 of A is `cice` -- so the column kernel reads
    and writes those planes in place; higher DG coefficients are left as they are (a thermodynamic
    source changes the mean, not the sub-cell shape).  The column step needs no exchange (elements are
    independent); it runs on the ghost rows too, redundantly, so that they stay consistent without a
    message.

    advect_column_state = True ("column state transport", include/nsdg.h): the snow and the surface temperature move with the ice.  The
    snow is a DG2 field S whose plane 0 IS the column's hsnow (col["hsnow"] is a view of it); tice0 travels as Q = H tice0, formed before
    the transport (nsdg_tracer_weight) and divided back after it (nsdg_tracer_recover, with min_conc / min_thick of the ice-free-node
    rule).  The transport then carries H, A, S and Q."""

    COLUMN_STATE = ("hsnow", "tice0")
    # closure of the column state transport's extra fields: snow volume S >= 0, the product Q = H T unbounded (include/nsdg.h)
    COLUMN_STATE_BOUNDS = ((0.0, float("inf"), False), (-float("inf"), float("inf"), False))
    COLUMN_FORCING = ("sst", "sss", "tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall", "wind")
    HAS_COLUMN_STATE = True

    def __init__(self, ops, blk, hx, hy, dt, nsub, device, forcing=None, advect_column_state=False, min_conc=1e-12, min_thick=0.01, **kw):
        """forcing: None = the forcing planes are whatever load_column() put there (constant in time);
        "dummy" / "winter" = regenerated on the device at every step's model time (nsdg_column_forcing) and the
        column wind speed is |u_a| of the dynamics' wind (nsdg_column_wind) -- the replacement of the reference's
        DummyExternalData (core/src/include/DummyExternalData.hpp:22-34) and of its never-set windSpeed;
        a ForcingSeries = records of a file sampled on the device at every step's model time (ops.forcing_sample): the column planes,
        and the wind (ua, va) and the ocean current (uo, vo) where the series holds them; the column wind speed as above.
        advect_column_state: the snow and the surface temperature ride on the ice (class docstring); min_conc / min_thick: the ice test of
        nsdg_tracer_recover (the defaults of the ice-free-node rule, nsdg_mevp_default_params; 0 and 0 with closure = False, as the C++ host)"""
        self.advect_column_state = bool(advect_column_state)
        if self.advect_column_state:  # before the base class allocates the advected fields and builds the transport plan
            self.TRANSPORTED = DynamicsCore.TRANSPORTED + ("S", "Q")
            self.BOUNDS = DynamicsCore.BOUNDS + self.COLUMN_STATE_BOUNDS
        super().__init__(ops, blk, hx, hy, dt, nsub, device, **kw)
        closure = kw.get("closure", True)
        self.min_conc, self.min_thick = (min_conc, min_thick) if closure else (0.0, 0.0)
        z = lambda: torch.zeros(blk.ny, blk.nx, dtype=torch.float64, device=device)
        self.col = {k: z() for k in self.COLUMN_STATE + self.COLUMN_FORCING}
        if self.advect_column_state:
            self.col["hsnow"] = self.S[0]
        self.newice = z()
        self.forcing, self.time = forcing, 0.0
        if isinstance(forcing, ForcingSeries):
            missing = [k for k in ForcingSeries.COLUMN if k not in forcing.fields]
            if missing:
                raise ValueError("the column step needs the forcing series to hold %s" % ", ".join(missing))
            # one launch per lattice and step: the column planes at the element centres, the wind and ocean pairs at the nodes
            self._series_groups = [("elements", ForcingSeries.COLUMN, [self.col[k] for k in ForcingSeries.COLUMN])]
            nodal = [(names, outs) for names, outs in ((ForcingSeries.WIND, (self.ua, self.va)), (ForcingSeries.OCEAN, (self.uo, self.vo)))
                     if names[0] in forcing.fields]
            if nodal:
                self._series_groups.append(("nodes", sum((n for n, _ in nodal), ()), [o for _, outs in nodal for o in outs]))
            self._records, self._device = {}, device
        elif forcing not in (None, "dummy", "winter"):
            raise ValueError("forcing must be None, 'dummy', 'winter' or a ForcingSeries, got %r" % (forcing,))

    def _history_sources(self):
        """and the column state: the snow plane the column step actually uses (plane 0 of S under advect_column_state) and tice0"""
        src = super()._history_sources()
        src["hsnow"], src["tice"] = self.col["hsnow"], self.col["tice0"]
        return src

    def load_column(self, fields):
        """fields: dict name -> global [ny, nx] numpy array for hsnow, tice0 and the 10 forcing fields"""
        import numpy as np

        es = self.blk.elem_slice()
        for k, dst in self.col.items():
            dst.copy_(torch.from_numpy(np.ascontiguousarray(fields[k][es])).to(dst.device))

    def transport(self):
        if not self.advect_column_state:
            return super().transport()
        b = self.blk
        self._mark(PHASE_TRANSPORT)
        # every local row, ghost rows included: both calls are element-local, the ghost rows stay equal to their owners
        self.ops.tracer_weight(self.ORDER, 0, b.ny, self.H, self.col["tice0"], self.Q)
        super().transport()
        self.ops.tracer_recover(self.ORDER, 0, b.ny, self.H, self.A, self.Q, self.min_conc, self.min_thick, self.col["tice0"])
        self.col["hsnow"] = self.S[0]  # the ping-pong buffer that holds the new snow

    def state_dict(self):
        """DynamicsCore.state_dict and, with advect_column_state, the snow S as [6, rows, nx] (plane 0 = hsnow)"""
        out = super().state_dict()
        if self.advect_column_state:
            out["S"] = self.owned(self.S).detach().cpu().numpy().copy()
        return out

    def load_state_dict(self, state):
        """DynamicsCore.load_state_dict and, with advect_column_state, the snow S (required: plane 0 is the column's hsnow)"""
        import numpy as np

        if self.advect_column_state and "S" not in state:
            raise ValueError("a CoupledCore with advect_column_state needs the snow S in the state")
        super().load_state_dict(state)
        if self.advect_column_state:
            self.S.copy_(torch.from_numpy(np.ascontiguousarray(state["S"][:, self.blk.elem_slice()])).to(self.S.device))
            self._clear_land()

    def thermodynamics(self):
        self._mark(PHASE_COLUMN)
        state = {"hice": self.H[0], "cice": self.A[0], "hsnow": self.col["hsnow"], "tice0": self.col["tice0"]}
        forcing = {k: self.col[k] for k in self.COLUMN_FORCING}
        self.ops.column_step(self.dt, state, forcing, self.newice)
        if self.land is not None:
            # the column step computes on land elements too (it is pinned to the reference case by case); its result there is discarded:
            # the cell means of H, A (and S), the snow and the new ice (still the COLUMN phase of the phase table)
            for f in (self.H[0], self.A[0], self.col["hsnow"], self.newice):
                self.ops.land_clear(f)

    def _record(self, k):
        """record k of the forcing series on the device: {name: [nyr, nxr] tensor}"""
        if k not in self._records:
            self._records[k] = {name: torch.from_numpy(a[k]).to(self._device) for name, a in self.forcing.fields.items()}
        return self._records[k]

    def external_forcing(self):
        self._mark(PHASE_FORCING)
        if isinstance(self.forcing, ForcingSeries):
            # the two records around the model time stay resident; a record is uploaded when the model time crosses into it
            k0, k1, w = self.forcing.bracket(self.time)
            for k in [k for k in self._records if k not in (k0, k1)]:
                del self._records[k]
            r0, r1 = self._record(k0), self._record(k1)
            for where, names, outs in self._series_groups:
                self.ops.forcing_sample(where, [r0[n] for n in names], [r1[n] for n in names], w, outs)
            self.ops.column_wind(self.ua, self.va, self.col["wind"])
        elif self.forcing is not None:
            self.ops.column_forcing(self.forcing, self.time, self.col)
            self.ops.column_wind(self.ua, self.va, self.col["wind"])

    def step(self):
        self._series_room()
        self._set_grid()
        self.external_forcing()
        self.thermodynamics()
        self.momentum()
        self.transport()
        self._drifters_step()
        self.time += self.dt
        if not self._in_advance:
            self._mark(PHASE_END)
            self._history_sample()
