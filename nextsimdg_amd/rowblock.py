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

A model step is ONE frame, DynamicsCore.step(); a subclass adds its phases in _phases().  History means, series and drifters are objects of
nextsimdg_amd/outputs.py that the frame calls once each; the reductions over the ranks belong to the exchanger, which owns the group.
"""
import numpy as np
import torch
import torch.distributed as dist

from nextsimdg_amd import abi, outputs

# NSDG_PHASE_* of include/nsdg.h: the ids of step()'s phase marks (names: abi.PHASES)
PHASE_FORCING, PHASE_COLUMN, PHASE_PREPARE, PHASE_SUBCYCLE, PHASE_TRANSPORT, PHASE_REDUCTION, PHASE_END = 0, 1, 2, 3, 4, 5, -1


def split_rows(ny, world, rank):
    return (rank * ny) // world, ((rank + 1) * ny) // world


def _put(dst, array):
    """a numpy array (any view) into a device tensor of its shape"""
    dst.copy_(torch.from_numpy(np.ascontiguousarray(array)).to(dst.device))


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
        self.native = None  # transport-private (NativeHaloExchanger: the plan behind the C ABI)


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
                self._prepare(plan)
        return plan

    def _prepare(self, plan):
        """a new plan knows what travels: a transport that builds something per plan does it here"""

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

        return self._start(self._plan(key, build))

    def element(self, fields):
        """refresh the ghost element rows of DG arrays [nc, ny, nx] (after a transport stage)"""
        key = ("e",) + tuple(f.data_ptr() for f in fields)
        plan = self._plan(key, lambda p: self._add_rows(p, fields, lambda f, a, c: f[:, a:c, :]))
        self.finish(self._start(plan))

    # ------------------------------------------------------------------ reductions over the ranks of the group
    def can_reduce(self):
        return dist.is_available() and dist.is_initialized()

    def max_scalar(self, value):
        """the maximum of a host float over the ranks (one block: the value itself, nothing is called)"""
        if self.blk.world == 1:
            return value
        t = torch.tensor([value], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return float(t.item())

    def max_array(self, tensor):
        """the elementwise maximum over the ranks, in place"""
        dist.all_reduce(tensor, op=dist.ReduceOp.MAX, group=self.group)


class NativeHaloExchanger(HaloExchanger):
    """the planning of HaloExchanger with the transport behind the C ABI (csrc/halo.hip): pack kernel, RCCL
    send/recv group on the context's communication stream, unpack kernel -- three C calls and no torch op per
    exchange.  `local_group`: in-process transport between thread-ranks instead of RCCL (one-GPU tests)."""

    def __init__(self, ctx, blk, device=None, group=None, loopback=False, local_group=None):
        super().__init__(blk, group, loopback)
        self.ctx = ctx
        # loopback: rehearsal of an interior block on one GPU: a communicator of ONE rank, both neighbours are that rank
        # (what goes up arrives from below); the values wrap around, the calls and sizes are the real ones
        rank, world = (0, 1) if loopback else (blk.rank, blk.world)
        if local_group is not None:
            ctx.comm_init_local(local_group, rank, world)
        else:
            ctx.comm_init_rccl(rank, world, group)  # (one rank: the group is not asked)
        self.peer_below, self.peer_above = (None if p is None else 0 if loopback else p for p in (blk.below, blk.above))

    def _prepare(self, plan):
        if plan.up_send or plan.down_send or plan.from_above or plan.from_below:
            plan.native = self.ctx.halo_plan(self.peer_below, self.peer_above, plan.up_send, plan.down_send, plan.from_above, plan.from_below)

    def _start(self, plan):
        if plan.native is not None:
            plan.native.start()
        return plan.native

    def _finish(self, handle):
        if handle is not None:
            handle.finish()

    def can_reduce(self):
        return True

    def max_scalar(self, value):
        return self.ctx.comm_max_f64(value)  # (also on one block: the communicator decides)

    def max_array(self, tensor):
        self.ctx.comm_max_f64_array(tensor)


class DynamicsCore:
    """State and time step of the dynamics core on one rank's row block.

    step() = one model time step: nodal means of H and A, ice strength at the Gauss points, wind
    stress, `nsub` mEVP sub-iterations (velocity halo after each), advection-velocity preparation and
    one SSP-RK3 DG2 transport step of H and A (element halo after each stage).

    tracers=("age", "origin"): named intensive planes that ride on the ice (include/nsdg.h "ice tracers") as
    Q = H T in a transport group of their own after the run of H and A; "age" grows by dt where there is ice, every other name is
    passive; tracers_read() / load_tracers() and the key "tracers" of state_dict() hold them.  None or (): no tracers, the same calls as
    ever.

    tilt="ssh" (include/nsdg_tilt.h): the sea-surface tilt is -m g grad(eta) of a sea-surface height, the nodal
    buffer self.ssh [m] -- filled by set_ssh() from a global array, by device_ssh() with the box test's, or by a ForcingSeries that holds
    "ssh" (CoupledCore) -- and (uo, vo) is the drag velocity alone.  prepare() sets the field on the ops object before the coefficient
    packing and clears it after it.  gravity: g [m s^-2], None = abi.GRAVITY.  tilt="geostrophic", the default: the tilt of the geostrophic
    current, -m f_c k x u_o, the same calls as ever.  The height is forcing: the state dict does not hold it.

    budget=("wind", "water", ...), budget_power=True (include/nsdg_budget.h): right after the sub-cycle of every
    step and sub-step -- H, A and the packed coefficients are still the sub-cycle's -- one launch on the owned rows writes the nodal forces
    of the named terms of the momentum balance (abi.BUDGET_TERMS) and, with budget_power, the power of all eight terms and the kinetic
    energy per element row.  budget_read() returns the last step's; merge_budget() joins the ranks.  The launch belongs to the sub-cycle
    phase of the phase table.  None / False: nothing is allocated, nothing is launched, the same calls as ever.  The state dict does not
    hold the forces: they are a diagnostic of the step that was run."""

    ORDER = 2
    # closure of the transported fields (include/nsdg.h "INPUT DOMAIN AND CLOSURE"): mean thickness H >= 0; concentration
    # 0 <= A <= 1 at the quadrature points with the cell mean capped at 1 (ridging) -- (lo, hi, cap_mean) per field
    BOUNDS = ((0.0, float("inf"), False), (0.0, 1.0, True))
    # the advected DG2 fields (attribute names), in the order of the step calls' field lists and of BOUNDS.  A subclass may state its own;
    # the constructor appends what _more_transported() returns (CoupledCore with advect_column_state: the snow S and the weighted surface
    # temperature Q) and the damage D of rheology="bbm", and leaves the complete lists on the instance
    TRANSPORTED = ("H", "A")

    LAND_OPS = ("set_land_mask", "land_clear", "land_clear_nodes")
    BASAL_OPS = ("set_basal_depth", "set_basal_params", "basal_critical")
    BBM_OPS = ("bbm_prepare", "bbm_iterate")
    BBM_NATIVE_OPS = ("rb_bbm", "rb_transport")
    DAMAGE_BOUNDS = (0.0, 1.0, False)  # the damage D of the brittle rheology: in [0, 1], no cap of the cell mean
    # tracers= (include/nsdg.h "ice tracers"): the calls it needs, the name that ages, and the names a tracer may not take -- the keys of
    # state_dict() and of the column state
    TRACER_OPS = ("tracers_weight", "tracers_recover", "tracers_dilute")
    TILT_OPS = ("set_tilt", "tilt_nodal", "boxtest_ssh")
    BUDGET_OPS = ("momentum_budget",)
    AGE_TRACER = "age"
    STATE_KEYS = ("rows", "ny_global", "nx", "H", "A", "S", "Q", "D", "u", "v", "s11", "s12", "s22", "drifters", "tracers", "hsnow", "tice0")
    HISTORY_COLUMN_FIELDS = outputs.History.COLUMN_FIELDS
    HAS_COLUMN_STATE = False
    merge_history, merge_series = staticmethod(outputs.merge_history), staticmethod(outputs.merge_series)
    merge_stations = staticmethod(outputs.merge_stations)

    def __init__(self, ops, blk, hx, hy, dt, nsub, device, exchanger=None, overlap=True, native=False, use_graph=False, closure=True,
                 phase_timing=False, land=None, rheology="mevp", bbm=None, history=None, series=None, series_capacity=1024, extent_conc=0.15,
                 drifters=None, drifter_min_conc=0.15, drifter_fields=None, stations=None, station_fields=None, station_capacity=256,
                 tracers=None, min_conc=1e-12, min_thick=0.01, bathymetry=None, basal=None, snow_load=False, rho_snow=None,
                 tilt="geostrophic", gravity=None, budget=None, budget_power=False):
        if snow_load or rho_snow is not None:  # (CoupledCore takes the two itself and does not pass them on)
            raise ValueError("snow_load= needs the column state of a CoupledCore: a DynamicsCore carries no snow")
        self.ops, self.blk, self.hx, self.hy, self.dt, self.nsub, self.overlap = ops, blk, hx, hy, dt, nsub, overlap
        # closure: cap + scaling limiter at the end of every transport step (the ice-free-node rule is a parameter of the
        # sub-cycle, on by default).  False: the bare scheme of rounds 1-4 (frozen fixtures of that scheme)
        self.closure = closure
        # native: the sub-cycle and the transport of a step are ONE C call each (csrc/rowblock.hip runs the same
        # sequence of passes and exchanges as subcycle() / transport() below); needs the C-ABI ops and, with
        # neighbours, a NativeHaloExchanger (it owns the communicator).  use_graph: replay the launches between
        # two exchanges as one hipGraph.
        self.native, self.use_graph = native, use_graph
        self.halo = exchanger if exchanger is not None else HaloExchanger(blk)
        # Everything that can refuse comes first: a constructor that raises has changed nothing on `ops`
        self._check_rheology(rheology, bbm)
        self._check_tilt(tilt, gravity)
        self._check_budget(budget, budget_power)
        self.TRANSPORTED, self.BOUNDS = self._transported()
        # tracers: names of intensive quantities that ride on the ice (include/nsdg.h "ice tracers"), "age" the one
        # that ages; min_conc / min_thick: the ice test of their recovery (the ice-free-node rule's defaults; 0 and 0 with closure = False)
        self.tracers = self._check_tracers(tracers)
        self.min_conc, self.min_thick = (float(min_conc), float(min_thick)) if closure else (0.0, 0.0)
        # land: bool array [ny_global, nx] of the WHOLE domain (True = land; include/nsdg.h "land mask"): the nodes of
        # land elements hold u = v = 0 like the array edge.  This rank keeps its rows, ghost rows included -- the mask is static, nothing
        # is exchanged -- and sets them on the ops object whenever it sets the grid
        self.land, self._land_on_ops, self._land_global = None, False, None
        if land is not None:
            outputs.require_ops(ops, self.LAND_OPS, "land=", "land-mask calls")
            land = np.asarray(land)
            if land.shape != (blk.ny_glob, blk.nx):
                raise ValueError("land must be a [ny_global, nx] = [%d, %d] array, got shape %s" % (blk.ny_glob, blk.nx, land.shape))
            self.land = torch.from_numpy(np.ascontiguousarray(land[blk.elem_slice()] != 0).astype(np.uint8)).to(device)
            if self.tilt == "ssh":
                self._land_global = land != 0  # set_ssh() asks where the height must be finite
        # bathymetry: float64 [ny_global, nx] water depth in metres of the WHOLE domain (include/nsdg_basal.h): ice
        # whose keels reach the seabed feels a basal stress and can stay fast over a shoal.  Like the mask: this rank keeps its rows, ghost
        # rows included, nothing is exchanged, and they go to the ops object with the grid.  basal: an abi.BasalParams (None: whatever
        # the ops object holds, the published defaults on a new context)
        self.depth, self._basal_params, self._depth_on_ops = None, basal, False
        if bathymetry is not None:
            outputs.require_ops(ops, self.BASAL_OPS, "bathymetry=", "landfast-ice calls")
            depth = np.asarray(bathymetry, dtype=np.float64)
            if depth.shape != (blk.ny_glob, blk.nx):
                raise ValueError("bathymetry must be a [ny_global, nx] = [%d, %d] array, got shape %s" % (blk.ny_glob, blk.nx, depth.shape))
            ocean = np.ones(depth.shape, dtype=bool) if land is None else np.asarray(land) == 0
            bad = ocean & ~(np.isfinite(depth) & (depth >= 0.0))
            if bad.any():
                iy, ix = (int(k) for k in np.argwhere(bad)[0])
                raise ValueError("bathymetry must be finite and >= 0 at ocean elements: %r at (row %d, column %d)" % (float(depth[iy, ix]), iy, ix))
            depth = np.where(ocean, depth, 0.0)  # land elements are stored as 0
            self.depth = torch.from_numpy(np.ascontiguousarray(depth[blk.elem_slice()])).to(device)
        elif basal is not None:
            raise ValueError("basal= parameters need bathymetry=")
        # phase_timing: step() brackets its parts with the library's phase marks (include/nsdg.h "per-phase device timing": one event per
        # mark on the ops' stream, read by phase_times()); off, nothing is asked of `ops` beyond the kernels
        self._phase_timing, self._phase_open = bool(phase_timing), PHASE_END
        if self._phase_timing:
            outputs.require_ops(ops, ("phase_timing", "phase_mark", "phase_times"), "phase_timing=True", "phase calls")
        # v sub-iterations per kernel pass (v = 4: variant 4, v = 3: variant 3, v = 2: variant 2) need a (v k, v k - 1) ghost depth
        # for k passes between two exchanges; a single domain has no ghosts at all.  All variants produce
        # bit-identical results, so a variant-3 context on a (2k, 2k-1) block simply uses the two-iteration kernel.
        # per_pass >= 2: the ghost zones hold stress rows as well as velocity rows
        variant = getattr(ops, "mevp_variant", None)
        self.per_pass = 1
        for v in (4, 3, 2):
            deep = blk.depth_below >= v and blk.depth_below % v == 0 and blk.depth_above == blk.depth_below - 1
            if variant is not None and variant >= v and (blk.world == 1 or deep) and rheology != "bbm":  # (no multi-iteration brittle passes)
                self.per_pass = v
                break
        self.group_passes = blk.depth_below // self.per_pass if (self.per_pass >= 2 and blk.world > 1) else 1  # passes between two exchanges
        # the outputs (nextsimdg_amd/outputs.py), each an object or None; history and series: the names, as given
        self._history = None if history is None else outputs.History(history, ops, blk, device, rheology, self.TRANSPORTED, self.HAS_COLUMN_STATE)
        self._series = None if series is None else outputs.Series(series, series_capacity, extent_conc, ops, blk, device, self.HAS_COLUMN_STATE)
        # a single-iteration sub-cycle leaves ghost node rows stale: the drifters complete them, unless the native plan does
        # drifter_fields= / station_fields=: the fields at a point (include/nsdg.h "point samples"), the history's names and refusals
        if drifter_fields is not None:
            if drifters is None:
                raise ValueError("drifter_fields= samples along the drifters' tracks: it needs drifters=")
            drifter_fields = outputs.point_fields(drifter_fields, "drifter_field", rheology, self.HAS_COLUMN_STATE)
        if (stations is None) != (station_fields is None):
            raise ValueError("stations= and station_fields= go together: the points and the fields sampled at them")
        if stations is not None:
            station_fields = outputs.point_fields(station_fields, "station_field", rheology, self.HAS_COLUMN_STATE)
        self._drifters = None if drifters is None else outputs.Drifters(drifters, drifter_min_conc, ops, blk, hx, hy, self.halo, device,
                                                                         complete_ghosts=self.per_pass == 1 and not self._plan_completes_nodes(),
                                                                         fields=drifter_fields, order=self.ORDER)
        self._stations = None if stations is None else outputs.Stations(stations, station_fields, station_capacity, ops, blk, hx, hy, device,
                                                                         order=self.ORDER)
        self.drifter_fields, self.station_fields = drifter_fields, station_fields
        self.history = self._history.entries if self._history is not None else None
        self.series = self._series.names if self._series is not None else None
        self.series_capacity, self.extent_conc, self.drifter_min_conc = int(series_capacity), float(extent_conc), float(drifter_min_conc)
        # from here on `ops` is changed; close() puts it back
        if bbm is not None:
            ops.set_bbm_params(bbm)
        if self._phase_timing:
            ops.phase_timing(True)
        # the native driver's plan carries the bounds itself (nsdg_rb_transport_desc.own_bounds); the Python sequence of step calls reads
        # them from the context: stated here, put back by close() (they apply to EVERY later step call on the context: include/nsdg.h)
        self._bounds_before = getattr(ops, "transport_bounds", ())
        ops.set_transport_bounds(self.BOUNDS if closure else ())
        self._calls = {}
        nx, ny, nf = blk.nx, blk.ny, len(self.TRANSPORTED)
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
        if self.tilt == "ssh":
            self.ssh = z(*nodal)  # the sea-surface height [m] at the nodes, ghost rows included: forcing, like uo and vo
        self.packed = z(nodal[0] * nodal[1] * 8)  # per-step momentum coefficients, 8 per node
        if self.budget is not None:
            # the planes of the terms asked for, on the local lattice (the launch writes the owned node rows), and the row totals
            self._budget_planes = {t + "_" + c: z(*nodal) for t in self.budget for c in "xy"}
            self._budget_power = z(abi.BUDGET_QUANTITIES, ny) if self.budget_power else None
        self.adv = (z(6, ny, nx), z(6, ny, nx), z(3, ny, nx + 1), z(3, ny + 1, nx))
        self.t1 = [z(6, ny, nx) for _ in range(nf)]
        self.t2 = [z(6, ny, nx) for _ in range(nf)]
        if rheology == "bbm":
            # the damage ping-pong of the sub-cycle, the three per-step Gauss arrays (layout of pg) and the zeros the packing takes as u0, v0
            self.Db = z(6, ny, nx)
            self.hg, self.eg, self.pm = (ops.private_zeros(9, ny, nx, device) for _ in range(3))
            self._zero_nodal = z(*nodal)
        if self.tracers:
            # the second transport group: one plane T per tracer, its product Q = H T and the stage buffers of the Qs' own transport run
            nt = len(self.tracers)
            self._tracer_kinds = tuple(abi.TRACER_AGE if name == self.AGE_TRACER else abi.TRACER_PASSIVE for name in self.tracers)
            self._tr = [z(ny, nx) for _ in range(nt)]
            self._tq, self._tq1, self._tq2 = ([z(6, ny, nx) for _ in range(nt)] for _ in range(3))
        if native:
            self._init_native()

    def _check_rheology(self, rheology, bbm):
        """rheology: "mevp", or "bbm" -- the brittle Bingham-Maxwell sub-cycle (include/nsdg.h "brittle rheology"):
        nsub explicit sub-iterations of dt / nsub, a damage field D updated in the sub-cycle and advected with H and A.  bbm: an
        abi.BbmParams set on the ops object (None: whatever the ops object holds, the library's defaults on a new context)"""
        blk = self.blk
        if rheology not in ("mevp", "bbm"):
            raise ValueError("rheology must be 'mevp' or 'bbm', got %r" % (rheology,))
        self.rheology = rheology
        if rheology == "bbm":
            if self.use_graph:
                raise ValueError("use_graph=True needs rheology='mevp': the brittle sub-cycle exchanges after every sub-iteration and replays no graph")
            if self.native:
                outputs.require_ops(self.ops, self.BBM_NATIVE_OPS, "rheology='bbm' with native=True", "native row-block calls")
            if blk.world > 1 and (blk.depth_below, blk.depth_above) != (1, 1):
                raise ValueError("rheology='bbm' runs one sub-iteration per pass: a row block needs the ghost depth (1, 1), got (%d, %d)"
                                 % (blk.depth_below, blk.depth_above))
            outputs.require_ops(self.ops, self.BBM_OPS, "rheology='bbm'", "BBM calls")
        elif bbm is not None:
            raise ValueError("bbm= parameters need rheology='bbm'")

    def _check_tilt(self, tilt, gravity):
        """tilt= and gravity=, refused before anything is asked of `ops` but the presence of the calls"""
        if tilt not in ("geostrophic", "ssh"):
            raise ValueError("tilt must be 'geostrophic' or 'ssh', got %r" % (tilt,))
        if gravity is not None and tilt != "ssh":
            raise ValueError("gravity= needs tilt='ssh'")
        self.tilt = tilt
        self.gravity = abi.GRAVITY if gravity is None else float(gravity)
        if tilt == "ssh":
            outputs.require_ops(self.ops, self.TILT_OPS, "tilt='ssh'", "sea-surface tilt calls")
            if not (np.isfinite(self.gravity) and self.gravity > 0.0):
                raise ValueError("gravity must be finite and > 0, got %r" % (self.gravity,))

    def _check_budget(self, budget, budget_power):
        """budget= as a tuple of term names (None: off; () with budget_power: the totals alone), refused before anything is asked of `ops`
        but the presence of the call"""
        self.budget, self.budget_power = None, bool(budget_power)
        if budget is None and not budget_power:
            return
        names = () if budget is None else ((budget,) if isinstance(budget, str) else tuple(budget))
        unknown = [n for n in names if n not in abi.BUDGET_TERMS]
        if unknown:
            raise ValueError("unknown budget term %s (known: %s)" % (", ".join(repr(n) for n in unknown), " ".join(abi.BUDGET_TERMS)))
        dup = sorted({n for n in names if names.count(n) > 1})
        if dup:
            raise ValueError("budget= names %s more than once" % ", ".join(dup))
        if not names and not budget_power:
            raise ValueError("budget= needs at least one term (None turns it off)")
        if self.rheology == "bbm":
            raise ValueError("budget= needs rheology='mevp': the brittle sub-cycle packs per sub-step with u0 = 0, and this balance -- the "
                             "implicit step of the mEVP sub-cycle -- does not describe it")
        outputs.require_ops(self.ops, self.BUDGET_OPS, "budget=", "momentum budget call")
        self.budget = names

    def _budget_launch(self):
        """nsdg_momentum_budget on the owned rows, at the state the sub-cycle has just left"""
        b = self.blk
        if self.tilt == "ssh":  # on the ops object for this launch alone, as for the packing
            self.ops.set_tilt(self.ssh, self.gravity)
        self.ops.momentum_budget(b.j0, b.j1, self.H, self.A, (self.ua, self.va), self.s, (self.u, self.v), self.packed, self._budget_planes,
                                 self._budget_power, 0)
        if self.tilt == "ssh":
            self.ops.set_tilt(None)

    def budget_read(self):
        """{"rows": (r0, r1), "<term>_x", "<term>_y": the owned node rows [N m^-2], "power": {term: [rows] W}, "ke": [rows] J} of the last
        step (its last sub-step); "power" and "ke" with budget_power only"""
        if self.budget is None:
            raise ValueError("budget_read() needs a core constructed with budget= or budget_power=True")
        b = self.blk
        out = {"rows": (b.r0, b.r1)}
        for k, t in self._budget_planes.items():
            out[k] = self.owned(t).detach().cpu().numpy().copy()
        if self._budget_power is not None:
            p = self._budget_power[:, b.j0:b.j1].detach().cpu().numpy()
            out["power"] = {t: p[i].copy() for i, t in enumerate(abi.BUDGET_TERMS)}
            out["ke"] = p[abi.BUDGET_KE].copy()
        return out

    @staticmethod
    def merge_budget(parts):
        """the ranks' budget_read()s (any order) -> the budget of the whole domain: the planes and the row totals joined in row order, and
        "power_total" {term: W}, "ke_total" J: the rows added one after the other in global row order, whatever the decomposition, so one
        block and N blocks give the same bits"""
        parts = sorted(parts, key=lambda p: p["rows"][0])
        for a, b in zip(parts, parts[1:]):
            if a["rows"][1] != b["rows"][0]:
                raise ValueError("merge_budget: the parts' rows %s and %s do not join" % (a["rows"], b["rows"]))
        out = {"rows": (parts[0]["rows"][0], parts[-1]["rows"][1])}
        for k in parts[0]:
            if k not in ("rows", "power", "ke"):
                out[k] = np.concatenate([p[k] for p in parts], axis=0)
        if "power" in parts[0]:
            out["power"] = {t: np.concatenate([p["power"][t] for p in parts]) for t in parts[0]["power"]}
            out["ke"] = np.concatenate([p["ke"] for p in parts])
            total = lambda rows: float(np.add.accumulate(rows)[-1])  # sequential in row order: np.sum would add pairwise
            out["power_total"] = {t: total(rows) for t, rows in out["power"].items()}
            out["ke_total"] = total(out["ke"])
        return out

    def _need_tilt(self, what):
        if self.tilt != "ssh":
            raise ValueError("%s needs a core constructed with tilt='ssh'" % what)

    def set_ssh(self, eta):
        """the sea-surface height [m] from a global [2 ny_global + 1, 2 nx + 1] array of the WHOLE domain's nodes: this rank keeps its
        rows, ghost rows included.  It must be finite at every node of every ocean element; strictly inside land it may be anything"""
        self._need_tilt("set_ssh()")
        b = self.blk
        eta = np.asarray(eta, dtype=np.float64)
        if eta.shape != (2 * b.ny_glob + 1, 2 * b.nx + 1):
            raise ValueError("ssh must be a [2 ny_global + 1, 2 nx + 1] = [%d, %d] array, got shape %s" % (2 * b.ny_glob + 1, 2 * b.nx + 1, eta.shape))
        needed = np.zeros(eta.shape, dtype=bool)  # the nodes of ocean elements
        ocean = np.ones((b.ny_glob, b.nx), dtype=bool) if self._land_global is None else ~self._land_global
        for dy in range(3):
            for dx in range(3):
                needed[dy:dy + 2 * b.ny_glob:2, dx:dx + 2 * b.nx:2] |= ocean
        bad = needed & ~np.isfinite(eta)
        if bad.any():
            gy, gx = (int(k) for k in np.argwhere(bad)[0])
            raise ValueError("ssh must be finite at the nodes of ocean elements: %r at node (row %d, column %d)" % (float(eta[gy, gx]), gy, gx))
        _put(self.ssh, eta[b.node_slice()])

    def device_ssh(self, domain_size, fc):
        """the sea-surface height whose geostrophic current is the box test's gyre (Coriolis parameter fc), evaluated on the device for
        this rank's rows"""
        self._need_tilt("device_ssh()")
        self._set_grid()
        self.ops.boxtest_ssh(domain_size, fc, self.gravity, self.ssh)

    def tilt_read(self):
        """(sx, sy): the gradient of the sea-surface height at the node rows this rank owns, what the next coefficient packing uses
        (nsdg_tilt_nodal)"""
        self._need_tilt("tilt_read()")
        self._set_grid()
        sx, sy = torch.zeros_like(self.ssh), torch.zeros_like(self.ssh)
        self.ops.set_tilt(self.ssh, self.gravity)
        self.ops.tilt_nodal(sx, sy)
        self.ops.set_tilt(None)
        return self.owned(sx), self.owned(sy)

    def _check_tracers(self, tracers):
        """tracers= as a tuple of names (None and () alike: none), refused before anything is asked of `ops` but the presence of the calls"""
        names = () if tracers is None else ((tracers,) if isinstance(tracers, str) else tuple(tracers))
        if not names:
            return ()
        if len(names) > abi.TRACERS_MAX:
            raise ValueError("tracers= names %d tracers (%s); the tracer group carries at most %d"
                             % (len(names), ", ".join(map(str, names)), abi.TRACERS_MAX))
        for name in names:
            if not isinstance(name, str) or not name.isidentifier():
                raise ValueError("tracer name %r is not an identifier" % (name,))
            if name in self.STATE_KEYS:
                raise ValueError("tracer name %r collides with a key of the state (%s)" % (name, " ".join(self.STATE_KEYS)))
        dup = sorted({n for n in names if names.count(n) > 1})
        if dup:
            raise ValueError("tracers= names %s more than once" % ", ".join(dup))
        outputs.require_ops(self.ops, self.TRACER_OPS, "tracers=", "ice tracer calls")
        return names

    def _more_transported(self):
        """(names, bounds) of the fields a subclass advects besides the class's TRANSPORTED"""
        return (), ()

    def _transported(self):
        """(names, bounds) of every advected field, stated once: the class's own, the subclass's additions, the damage of the brittle
        rheology -- and the one rule on their number"""
        more, more_bounds = self._more_transported()
        names, bounds = tuple(self.TRANSPORTED) + tuple(more), tuple(self.BOUNDS) + tuple(more_bounds)
        if self.rheology == "bbm":
            if len(names) + 1 > 4:  # NSDG_RB_MAX_FIELDS
                raise ValueError("rheology='bbm' with advect_column_state=True would advect %d fields (%s and D); a transport step carries at most 4"
                                 % (len(names) + 1, ", ".join(names)))
            names, bounds = names + ("D",), bounds + (self.DAMAGE_BOUNDS,)
        return names, bounds

    def _history_sources(self):
        """the current ping-pong side of everything a sample reads"""
        src = {"H": self.H, "A": self.A, "u": self.u, "v": self.v, "s11": self.s[0], "s12": self.s[1], "s22": self.s[2]}
        if self.rheology == "bbm":
            src["D"] = self.D
        return src

    def history_read(self, reset=True):
        """outputs.History.read: the means (and statistics) of the window since the last reset, for the rows this rank owns"""
        if self._history is None:
            raise ValueError("history_read() needs a core constructed with history=")
        return self._history.read(reset)

    def series_read(self, reset=True):
        """outputs.Series.read: the row totals of the steps since the last reset, for the rows this rank owns"""
        if self._series is None:
            raise ValueError("series_read() needs a core constructed with series=")
        return self._series.read(reset)

    def drifters_read(self):
        """outputs.Drifters.read: positions and statuses of the whole list"""
        if self._drifters is None:
            raise ValueError("drifters_read() needs a core constructed with drifters=")
        return self._drifters.read()

    def stations_read(self, reset=True):
        """outputs.Stations.read: the fields at the stations for the steps since the last reset, this rank's part (-inf where it does not
        own the point); merge_stations() joins the ranks"""
        if self._stations is None:
            raise ValueError("stations_read() needs a core constructed with stations=")
        return self._stations.read(reset)

    def _plan_completes_nodes(self):
        """the native brittle plan ends its call with the exchange of every ghost node row (nsdg_rb_bbm_desc.complete_nodes): the one place
        that says who completes them, asked by the drifters' constructor and by _init_native"""
        return self.native and self.rheology == "bbm"

    def _init_native(self):
        b = self.blk
        if b.world > 1 and not isinstance(self.halo, NativeHaloExchanger):
            raise ValueError("the native driver exchanges ghost rows through the C ABI: pass a NativeHaloExchanger")
        peers = (self.halo.peer_below, self.halo.peer_above) if b.world > 1 else (None, None)
        self._sbuf, self._uvbuf, self._par = (self.s, self.sb), ((self.u, self.v), (self.ub, self.vb)), 0
        self._fbuf, self._tpar = (self._fields(), tuple(self.t1)), 0
        if self.rheology == "bbm":
            # the brittle plan (nsdg_rb_bbm_*): the damage ends in the transport's current buffer of D, whatever nsub; Db is its partner
            # inside the call.  With drifters the plan completes the ghost node rows of the final velocity itself.  (_run_mevp: the
            # sub-cycle plan of either rheology, under the name the exchange statistics are read by)
            k = self.TRANSPORTED.index("D")
            plan = self._run_mevp = self.ops.rb_bbm(b, peers, self.nsub, self.overlap, self._sbuf, self._uvbuf, self.packed,
                                                    (self.hg, self.eg, self.pm), (self._fbuf[0][k], self._fbuf[1][k]), self.Db,
                                                    complete_nodes=self._plan_completes_nodes() and self._drifters is not None)
            self._run_subcycle = lambda par: plan(par, self._tpar)  # the transport's parity of the moment: where D is
        else:
            self._run_mevp, per_pass, group = self.ops.rb_mevp(b, peers, self.nsub, self.overlap, self.use_graph, self._sbuf, self._uvbuf,
                                                               self.packed, self.pg)
            assert (per_pass, group) == (self.per_pass, self.group_passes), "native plan and driver disagree on the pass structure"
            self._run_subcycle = self._run_mevp
        self._run_transport = self.ops.rb_transport(b, peers, self._fbuf[0], self._fbuf[1], self.t2, self.adv, bounds=self.BOUNDS if self.closure else ())
        if self.tracers:
            # the tracer group: a second plan without bounds (every Q is unbounded), with its own ping-pong parity
            self._qbuf, self._qpar = (tuple(self._tq), tuple(self._tq1)), 0
            self._run_tracers = self.ops.rb_transport(b, peers, self._qbuf[0], self._qbuf[1], self._tq2, self.adv, bounds=())

    def _fields(self):
        """the current buffers of the advected fields, in the order of TRANSPORTED"""
        return tuple(getattr(self, name) for name in self.TRANSPORTED)

    def _set_fields(self, fields):
        for name, f in zip(self.TRANSPORTED, fields):
            setattr(self, name, f)

    def close(self):
        """releases the native driver plans (device buffers and events of their ghost exchanges); call it before the
        context is closed"""
        for name in ("_run_mevp", "_run_transport", "_run_tracers"):
            run = getattr(self, name, None)
            if run is not None and hasattr(run, "close"):
                run.close()
            setattr(self, name, None)
        self._run_subcycle = None
        if self._bounds_before is not None:  # the context is as this core found it
            self.ops.set_transport_bounds(self._bounds_before)
            self._bounds_before = None
        if self._land_on_ops:  # set with the grid (_set_grid)
            self.ops.set_land_mask(None)
        self.land, self._land_on_ops = None, False
        if self._depth_on_ops:
            self.ops.set_basal_depth(None)
        self.depth, self._depth_on_ops = None, False

    def basal_read(self):
        """the critical stress T_b [N m^-2] of the grounding scheme at the node rows this rank owns, from the current H and A: what the
        next coefficient packing stores (nsdg_basal_critical)"""
        if self.depth is None:
            raise ValueError("basal_read() needs a core constructed with bathymetry=")
        self._set_grid()
        nodal = (2 * self.blk.ny + 1, 2 * self.blk.nx + 1)
        cgh, cga, tb = (torch.zeros(*nodal, dtype=torch.float64, device=self.H.device) for _ in range(3))
        self.ops.dg_to_cg(self.H, cgh)
        self.ops.dg_to_cg(self.A, cga)
        self.ops.basal_critical(cgh, cga, tb)
        return self.owned(tb)

    def load_global(self, H, A, uo, vo, ua, va, u=None, v=None, D=None):
        """fill the local arrays (ghost rows included) from global numpy arrays; D: the damage of rheology="bbm" (None: left as it is)"""
        es, ns = self.blk.elem_slice(), self.blk.node_slice()
        _put(self.H, H[:, es])
        _put(self.A, A[:, es])
        for dst, src in ((self.uo, uo), (self.vo, vo), (self.ua, ua), (self.va, va)):
            _put(dst, src[ns])
        if u is not None:
            _put(self.u, u[ns])
            _put(self.v, v[ns])
        if D is not None:
            if self.rheology != "bbm":
                raise ValueError("a damage field needs rheology='bbm'")
            _put(self.D, D[:, es])
        self._clear_land()

    def _clear_land(self):
        """no ice on land, no motion at land nodes: whatever a caller loaded there is cleared (a store: a NaN goes too)"""
        if self.land is None:
            return
        self._set_grid()
        for f in self._fields():
            self.ops.land_clear(f)
        self.ops.land_clear_nodes(self.u, self.v)
        if self.tracers:
            for t in self._tr:
                self.ops.land_clear(t)

    def _set_grid(self):
        self.ops.set_grid(self.blk.nx, self.blk.ny, self.hx, self.hy)
        if self.land is not None:
            self.ops.set_land_mask(self.land)
            self._land_on_ops = True
        if self.depth is not None:
            if self._basal_params is not None:
                self.ops.set_basal_params(self._basal_params)
            self.ops.set_basal_depth(self.depth)
            self._depth_on_ops = True
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
        if self.budget is not None:  # in the sub-cycle's phase: H, A and the packing are still the sub-cycle's
            self._budget_launch()

    def prepare(self):
        """once per model step: ice strength at the Gauss points, nodal means of H and A, wind stress and the packed
        momentum coefficients (one launch); the velocity at the start of the step is read from the current iterate
        (it is only needed inside the packing)"""
        if self.tilt == "ssh":
            # on the ops object for the packing alone: another core on the same context packs with its own tilt
            self.ops.set_tilt(self.ssh, self.gravity)
            self._pack()
            self.ops.set_tilt(None)
        else:
            self._pack()

    def _pack(self):
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
        """the nsub sub-iterations of one model step, mEVP or brittle (ghost rows exchanged as the ghost depth requires)"""
        ops, b = self.ops, self.blk
        if self.native:
            # (the brittle plan leaves D where the transport plan reads it: self.D stays the current buffer)
            par = self._par = self._run_subcycle(self._par)
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
        deep = self.per_pass >= 2
        split = self.overlap and b.world > 1 and (b.j1 - b.j0) >= 4 and not deep
        for _ in range(self.nsub - it):
            uvn = (self.ub, self.vb)
            calls = self._iterate_calls(split)
            if not split:
                calls[0]()
                if deep:  # keep the deeper ghost zones (stress as well as velocity) of the multi-iteration passes consistent
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
            self.halo.finish(pending)

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
        calls = self._calls[key] = [bind(j0, j1, self.s, self.sb, uv, uvn, self.packed, self.pg) for (j0, j1) in rng]
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
        if self.tracers:
            # every local row, ghost rows included (as the recovery below): both calls are element-local, the ghost rows stay equal to their
            # owners.  The products are formed with the thickness the step starts from
            ops.tracers_weight(self.ORDER, 0, b.ny, self.H, self._tr, self._tq)
        ops.prepare_advection(self.ORDER, self.u, self.v, *self.adv)
        if self.native:
            par = self._tpar = self._run_transport(self.dt, self._tpar)
            self._set_fields(self._fbuf[par])
            self.t1[:] = self._fbuf[1 - par]
        else:
            f = list(self._fields())
            self._transport_stages(f, self.t1, self.t2, self.closure)
            # the new state is t1 (ghost rows refreshed); swap buffers instead of copying
            new = list(self.t1)
            self.t1[:] = f
            self._set_fields(new)
        if self.tracers:
            self._transport_tracers()

    def _transport_stages(self, f, t1, t2, limit):
        """one SSP-RK3 step of the fields f composed from the stage calls; the new state is left in t1, its ghost rows refreshed"""
        ops, b = self.ops, self.blk
        # Shu-Osher SSP-RK3: out = a*phi0 + b*(phis + dt L(phis)).  A stage reads one element row on each side
        # of the rows it updates: with at least 3 ghost rows per interior side the first two stages also
        # advance 2 / 1 ghost rows redundantly (bit-identically to their owners) and the ghost rows are
        # exchanged once per step instead of after every stage.
        deep = b.world > 1 and min(b.depth_below, b.depth_above) >= 3
        ext = (lambda e: (max(b.j0 - e, 0), min(b.j1 + e, b.ny))) if deep else (lambda e: (b.j0, b.j1))
        ops.transport_stage(self.ORDER, *ext(2), self.dt, 0.0, 1.0, f, f, t1, self.adv)
        if not deep:
            self.halo.element(t1)
        ops.transport_stage(self.ORDER, *ext(1), self.dt, 0.75, 0.25, f, t1, t2, self.adv)
        if not deep:
            self.halo.element(t2)
        ops.transport_stage(self.ORDER, b.j0, b.j1, self.dt, 1.0 / 3.0, 2.0 / 3.0, f, t2, t1, self.adv)
        if limit:  # the step entry points of the library do this themselves; a step composed of stages calls it
            ops.transport_limit(self.ORDER, b.j0, b.j1, t1)
        self.halo.element(t1)

    def _transport_tracers(self):
        """the second transport group: the products Q_k = H T_k in a run of their own -- the prepared velocity and
        the dt of the first, stage buffers of their own, no limiter (every Q is unbounded) -- and the division back, which ages "age" by dt"""
        ops, b = self.ops, self.blk
        if self.native:
            par = self._qpar = self._run_tracers(self.dt, self._qpar)
            self._tq, self._tq1 = list(self._qbuf[par]), list(self._qbuf[1 - par])
        else:
            self._transport_stages(self._tq, self._tq1, self._tq2, False)
            self._tq, self._tq1 = self._tq1, self._tq
        ops.tracers_recover(self.ORDER, 0, b.ny, self.H, self.A, self._tq, self._tracer_kinds, self.dt, self.min_conc, self.min_thick, self._tr)

    # ---- the tracers' values (include/nsdg.h "ice tracers"): one [ny, nx] plane each, zero where there is no ice
    def tracers_read(self):
        """{name: numpy [owned rows, nx]} of the tracers"""
        b = self.blk
        return {name: t[b.j0:b.j1].detach().cpu().numpy().copy() for name, t in zip(self.tracers, self._tr if self.tracers else ())}

    def load_tracers(self, fields):
        """fields: {name: global [ny_global, nx] array} for some or all of the tracers; fills the local rows, ghost rows included"""
        unknown = [k for k in fields if k not in self.tracers]
        if unknown:
            raise ValueError("load_tracers: %s: not among this core's tracers (%s)" % (", ".join(map(str, unknown)), ", ".join(self.tracers) or "none"))
        es = self.blk.elem_slice()
        for name, t in zip(self.tracers, self._tr if self.tracers else ()):
            if name in fields:
                a = np.asarray(fields[name], dtype=np.float64)
                if a.shape != (self.blk.ny_glob, self.blk.nx):
                    raise ValueError("tracer %r must be a [ny_global, nx] = [%d, %d] array, got shape %s" % (name, self.blk.ny_glob, self.blk.nx, a.shape))
                _put(t, a[es])
        self._clear_land()

    # ---- the frame of a model step: begin, one or several sub-steps of the phases, end
    def step(self):
        self._begin_step()
        self._substep()
        self._end_step()

    def _begin_step(self):
        for output in (self._series, self._stations):
            if output is not None:
                output.room()

    def _substep(self):
        """the grid, the phases and the drifters at self.dt: step() runs it once, advance() n times"""
        self._set_grid()
        self._phases()
        if self._drifters is not None:
            if self._drifters.fields is None:
                self._drifters.step(self.dt, self.u, self.v, self.A)
            else:  # the fields along the track are sampled at the new positions, from the state the phases left
                self._drifters.step(self.dt, self.u, self.v, self.A, self._history_sources())

    def _phases(self):
        """what a step computes, in order; a subclass puts its own phases around these"""
        self.momentum()
        self.transport()

    def _end_step(self):
        """the end mark of the span and one sample per model step, after its last sub-step: the row totals, the history, the stations"""
        self._mark(PHASE_END)
        for output in (self._series, self._history, self._stations):
            if output is not None:
                output.sample(self._history_sources())

    # ---- sub-stepping (include/nsdg.h "sub-stepping"): a model step of model_dt run as n steps of model_dt / n
    def substep_count(self, model_dt, courant=None, max_substeps=16, params=None):
        """(n, amax, c): the number of sub-steps the state asks for (nsdg_substep_count) from the largest concentration of the owned rows
        (ops.concentration_max), the same on every rank: the maximum over the ranks is the exchanger's (nsdg_comm_max_f64 on a
        NativeHaloExchanger's communicator, torch.distributed MAX on a CPU scalar otherwise).  params: the MevpParams whose
        pstar, compaction and rho_ice give the wave speed (default: nsdg_mevp_default_params)"""
        self._set_grid()
        amax = self.halo.max_scalar(self.ops.concentration_max(self.H, self.A, self.blk.j0, self.blk.j1))
        if params is None:
            params = abi.MevpParams()
            abi.load_library().nsdg_mevp_default_params(abi.C.byref(params))
        n, c = abi.substep_count(params, amax, min(self.hx, self.hy), model_dt, abi.SUBSTEP_COURANT if courant is None else courant,
                                 max_substeps)
        return n, amax, c

    def advance(self, model_dt, substeps=1, courant=None, max_substeps=16, params=None):
        """one model step of model_dt as n sub-steps with self.dt = model_dt / n (restored afterwards); substeps: an int >= 1, or
        "auto" (n from the state at the start of the step, substep_count).  Returns n; substeps = 1 is step() at model_dt, bit for bit"""
        if substeps != "auto" and not (isinstance(substeps, int) and not isinstance(substeps, bool) and substeps >= 1):
            raise ValueError("substeps must be an integer >= 1 or 'auto', got %r" % (substeps,))
        self._begin_step()
        if substeps == "auto":
            self._mark(PHASE_REDUCTION)
            substeps = self.substep_count(model_dt, courant, max_substeps, params)[0]
        dt = self.dt
        self.dt = model_dt / substeps
        try:
            for _ in range(substeps):
                self._substep()
        finally:
            self.dt = dt
            self._mark(PHASE_END)  # the span of the phase table is the model step, also one that failed
        self._end_step()
        return substeps

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
        for name in ("H", "A", "u", "v") + (("D",) if self.rheology == "bbm" else ()):
            out[name] = self.owned(getattr(self, name)).detach().cpu().numpy().copy()
        for name, f in zip(("s11", "s12", "s22"), self.s):
            out[name] = self.ops.private_to_planes(f, nx)[:, b.j0:b.j1].detach().cpu().numpy().copy()
        if self._drifters is not None:
            out["drifters"] = self._drifters.state()
        if self.tracers:
            out["tracers"] = self.tracers_read()
        return out

    def load_state_dict(self, state):
        """resume from a GLOBAL state (rows (0, ny_global): e.g. the ranks' state_dict()s concatenated): fills the local arrays, ghost rows
        included, and the current ping-pong buffers; forcing (load_global) and column fields are loaded as for a fresh run"""
        b = self.blk
        if tuple(state["rows"]) != (0, b.ny_glob) or state["nx"] != b.nx:
            raise ValueError("load_state_dict needs the state of the whole domain (rows (0, %d)), got rows %s" % (b.ny_glob, (state["rows"],)))
        es, ns = b.elem_slice(), b.node_slice()
        _put(self.H, state["H"][:, es])
        _put(self.A, state["A"][:, es])
        _put(self.u, state["u"][ns])
        _put(self.v, state["v"][ns])
        for f, name in zip(self.s, ("s11", "s12", "s22")):
            f.copy_(self.ops.planes_to_private(torch.from_numpy(np.ascontiguousarray(state[name][:, es])).to(f.device)))
        if self.rheology == "bbm":
            if "D" not in state:
                raise ValueError("a core with rheology='bbm' needs the damage D in the state")
            _put(self.D, state["D"][:, es])
        if self._drifters is not None:
            self._drifters.load_state(state)
        if self.tracers:  # a state without the key, or without one of the names, loads zeros
            held = state.get("tracers", {})
            for name, t in zip(self.tracers, self._tr):
                if name in held:
                    _put(t, held[name][es])
                else:
                    t.zero_()
        self._clear_land()

    @staticmethod
    def merge_states(states):
        """the ranks' state_dict()s (any order) -> the state of the whole domain"""
        states = sorted(states, key=lambda s: s["rows"][0])
        out = {"rows": (states[0]["rows"][0], states[-1]["rows"][1]), "ny_global": states[0]["ny_global"], "nx": states[0]["nx"]}
        for k in ("H", "A", "S", "D", "s11", "s12", "s22"):
            if k in states[0]:  # S: the snow of a CoupledCore with advect_column_state; D: the damage of rheology="bbm"
                out[k] = np.concatenate([s[k] for s in states], axis=1)
        for k in ("u", "v"):
            out[k] = np.concatenate([s[k] for s in states], axis=0)
        for k in ("sst", "sss"):
            if k in states[0]:  # the slab ocean of a CoupledCore with slab_ocean: [rows, nx] planes
                out[k] = np.concatenate([s[k] for s in states], axis=0)
        if "drifters" in states[0]:  # every rank holds the whole list
            assert all(np.array_equal(s["drifters"], states[0]["drifters"]) for s in states), "the ranks' drifter lists differ"
            out["drifters"] = states[0]["drifters"].copy()
        if "tracers" in states[0]:
            out["tracers"] = {name: np.concatenate([s["tracers"][name] for s in states], axis=0) for name in states[0]["tracers"]}
        return out


class ForcingSeries:
    """Forcing records on one lattice at model times (include/nsdg.h "forcing from a file"; the C++ host reads the same records from a
    file, host/include/ForcingFile.hpp).  times: strictly increasing model times [s] (the clock of CoupledCore.time); fields: name ->
    float64 array [nt, nyr, nxr] on a cell-centred lattice over the square domain.  Names: the column planes tair tdew slp qsw qlw mld
    snowfall, the pairs wind_u / wind_v and ocean_u / ocean_v (each pair complete or absent), and the sea-surface height ssh [m] of a core
    with tilt="ssh" (sampled at the nodes with the pairs).  A time outside [times[0], times[-1]]
    is an error: there is no extrapolation."""

    COLUMN = ("tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall")
    WIND = ("wind_u", "wind_v")
    OCEAN = ("ocean_u", "ocean_v")
    SLAB = ("sst", "sss")  # the relaxation targets of a slab ocean (CoupledCore(slab_ocean=True)), a pair
    SSH = ("ssh",)  # the sea-surface height of tilt="ssh" (include/nsdg_tilt.h), a nodal variable like the pairs

    def __init__(self, times, fields):
        t = np.array(times, dtype=np.float64)
        if t.ndim != 1 or t.size < 1:
            raise ValueError("times must be a 1-d array of at least one record time")
        if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
            raise ValueError("times must be finite and strictly increasing")
        if not fields:
            raise ValueError("a forcing series needs at least one field")
        known = self.COLUMN + self.WIND + self.OCEAN + self.SLAB + self.SSH
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
        for pair in (self.WIND, self.OCEAN, self.SLAB):
            if (pair[0] in out) != (pair[1] in out):
                raise ValueError("forcing fields %s and %s come as a pair" % pair)
        self.times, self.fields = t, out
        _, self.nyr, self.nxr = shapes.pop()

    def bracket(self, t):
        """(k0, k1, w): the records around model time t and the weight of k1 -- k0 is the last record with times[k0] <= t, k1 = k0 + 1,
        w = (t - times[k0]) / (times[k1] - times[k0]); at the last record itself k1 = k0 and w = 0"""
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
    rule).  The transport then carries H, A, S and Q.

    tracers= (DynamicsCore): the column step's growth dilutes them -- plane 0 of H is copied before the column step and
    nsdg_tracers_dilute runs after it (and its land clear): ice that grew carries the value 0.

    slab_ocean = True (include/nsdg_ocean.h): col["sst"] and col["sss"] are prognostic.  The column step is the
    fused nsdg_column_step_ocean, which advances them by the fluxes it computes, on every local row (element-local: the ghost rows stay
    equal to their owners without a message); land elements keep their sst, sss bits (`skip` = the land mask's local rows).  slab: an
    abi.SlabParams (None: the defaults, no relaxation).  With a relaxation time col["sst_ext"] / col["sss_ext"] hold the targets:
    load_column fills them from the keys sst_ext / sss_ext, or from sst / sss without them, and a ForcingSeries that holds the pair
    sst, sss samples it into them at every step.

    snow_load = True (include/nsdg_snow.h): the momentum equation feels the snow's weight.  prepare() hands the
    snow as it stands after this step's column step -- the DG field S under advect_column_state, else the plane col["hsnow"] -- to the
    ops object immediately before the coefficient packing, which takes the nodal mass from rho_i cgH + rho_snow max(cgS, 0) where the
    node is neither land nor ice-free.  Both rheologies pack through the same call.  The state dict is what it was: the snow is in it."""

    COLUMN_STATE = ("hsnow", "tice0")
    # closure of the column state transport's extra fields: snow volume S >= 0, the product Q = H T unbounded (include/nsdg.h)
    COLUMN_STATE_BOUNDS = ((0.0, float("inf"), False), (-float("inf"), float("inf"), False))
    COLUMN_FORCING = ("sst", "sss", "tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall", "wind")
    HAS_COLUMN_STATE = True
    SLAB_OPS = ("column_step_ocean", "slab_default_params", "set_slab_params")
    SNOW_OPS = ("set_snow_load", "snow_load_nodal")

    def __init__(self, ops, blk, hx, hy, dt, nsub, device, forcing=None, advect_column_state=False, min_conc=1e-12, min_thick=0.01,
                 slab_ocean=False, slab=None, snow_load=False, rho_snow=None, **kw):
        """forcing: None = the forcing planes are whatever load_column() put there (constant in time);
        "dummy" / "winter" = regenerated on the device at every step's model time (nsdg_column_forcing) and the
        column wind speed is |u_a| of the dynamics' wind (nsdg_column_wind) -- the replacement of the reference's
        DummyExternalData (core/src/include/DummyExternalData.hpp:22-34) and of its never-set windSpeed;
        a ForcingSeries = records of a file sampled on the device at every step's model time (ops.forcing_sample): the column planes,
        and the wind (ua, va) and the ocean current (uo, vo) where the series holds them; the column wind speed as above.
        advect_column_state: the snow and the surface temperature ride on the ice (class docstring); min_conc / min_thick: the ice test of
        nsdg_tracer_recover (the defaults of the ice-free-node rule, nsdg_mevp_default_params; 0 and 0 with closure = False, as the C++ host)"""
        self.advect_column_state = bool(advect_column_state)  # (read by _more_transported() while the base class constructs)
        if kw.get("tracers"):  # (refused before the base class changes anything on `ops`)
            outputs.require_ops(ops, ("copy_f64",), "tracers= in a coupled core", "copy call")
        self.snow_load = bool(snow_load)
        if rho_snow is not None and not self.snow_load:
            raise ValueError("rho_snow= needs snow_load=True")
        self.rho_snow = abi.SNOW_DENSITY if rho_snow is None else float(rho_snow)
        if self.snow_load:
            outputs.require_ops(ops, self.SNOW_OPS, "snow_load=True", "snow-load calls")
            if not (np.isfinite(self.rho_snow) and self.rho_snow >= 0.0):
                raise ValueError("rho_snow must be finite and >= 0, got %r" % (self.rho_snow,))
        self._snow_on_ops = False
        if isinstance(forcing, ForcingSeries):
            # the tilt and the series agree on who states it (refused before the base class changes anything on `ops`)
            ssh_tilt, has_ssh = kw.get("tilt", "geostrophic") == "ssh", "ssh" in forcing.fields
            if has_ssh and not ssh_tilt:
                raise ValueError("the forcing series holds ssh: it needs tilt='ssh'")
            if ssh_tilt and "ocean_u" in forcing.fields and not has_ssh:
                raise ValueError("tilt='ssh' with ocean_u / ocean_v from the forcing series needs the series to hold ssh as well: "
                                 "the current is then the drag velocity alone")
        self.slab_ocean = bool(slab_ocean)
        if slab is not None and not self.slab_ocean:
            raise ValueError("slab= needs slab_ocean=True")
        if self.slab_ocean:
            outputs.require_ops(ops, self.SLAB_OPS, "slab_ocean=True", "slab-ocean calls")
            if set(kw.get("tracers") or ()) & {"sst", "sss"}:
                raise ValueError("a tracer name collides with the slab ocean's sst / sss")
            for k in ("relax_t", "relax_s", "ice_salinity"):
                v = float(getattr(slab, k)) if slab is not None else 0.0
                if not (np.isfinite(v) and v >= 0.0):
                    raise ValueError("slab.%s must be finite and >= 0, got %r" % (k, v))
        super().__init__(ops, blk, hx, hy, dt, nsub, device, min_conc=min_conc, min_thick=min_thick, **kw)
        z = lambda: torch.zeros(blk.ny, blk.nx, dtype=torch.float64, device=device)
        if self.tracers:
            self._h_before = z()  # the mean thickness the column step starts from (nsdg_tracers_dilute)
        self.col = {k: z() for k in self.COLUMN_STATE + self.COLUMN_FORCING}
        if self.advect_column_state:
            self.col["hsnow"] = self.S[0]
        self.newice = z()
        self.forcing, self.time = forcing, 0.0
        self._slab_ext = None
        if self.slab_ocean:
            self._slab = slab if slab is not None else ops.slab_default_params()
            # the relaxation targets exist only under a relaxation time
            for k, on in (("sst", self._slab.relax_t > 0), ("sss", self._slab.relax_s > 0)):
                if on:
                    self.col[k + "_ext"] = z()
            self._slab_ext = {k: self.col.get(k + "_ext") for k in ("sst", "sss")}
        if isinstance(forcing, ForcingSeries):
            missing = [k for k in ForcingSeries.COLUMN if k not in forcing.fields]
            if missing:
                raise ValueError("the column step needs the forcing series to hold %s" % ", ".join(missing))
            # one launch per lattice and step: the column planes at the element centres, the wind and ocean pairs at the nodes
            self._series_groups = [("elements", ForcingSeries.COLUMN, [self.col[k] for k in ForcingSeries.COLUMN])]
            nodal = [(names, outs) for names, outs in ((ForcingSeries.WIND, (self.ua, self.va)), (ForcingSeries.OCEAN, (self.uo, self.vo)),
                                                        (ForcingSeries.SSH, (getattr(self, "ssh", None),)))
                     if names[0] in forcing.fields]
            if nodal:
                self._series_groups.append(("nodes", sum((n for n, _ in nodal), ()), [o for _, outs in nodal for o in outs]))
            if self.slab_ocean and "sst" in forcing.fields:
                # the slab's relaxation targets, a launch of their own (NSDG_FORCING_MAX_FIELDS planes per launch)
                ext = [(k, self.col[k + "_ext"]) for k in ForcingSeries.SLAB if k + "_ext" in self.col]
                if ext:
                    self._series_groups.append(("elements", tuple(k for k, _ in ext), [o for _, o in ext]))
            self._records, self._device = {}, device
        elif forcing not in (None, "dummy", "winter"):
            raise ValueError("forcing must be None, 'dummy', 'winter' or a ForcingSeries, got %r" % (forcing,))

    def _more_transported(self):
        return (("S", "Q"), self.COLUMN_STATE_BOUNDS) if self.advect_column_state else ((), ())

    def prepare(self):
        if self.snow_load:
            # the transport's ping-pong moves S (and the plane col["hsnow"] with it): the pointer is set before every packing
            snow = self.S[:(1, 3, 6)[self.ORDER]] if self.advect_column_state else self.col["hsnow"]
            self.ops.set_snow_load(snow, self.rho_snow)
            self._snow_on_ops = True
        super().prepare()

    def close(self):
        if self._snow_on_ops:
            self.ops.set_snow_load(None)
            self._snow_on_ops = False
        super().close()

    def _history_sources(self):
        """and the column state: the snow plane the column step actually uses (plane 0 of S under advect_column_state) and tice0"""
        src = super()._history_sources()
        src["hsnow"], src["tice"] = self.col["hsnow"], self.col["tice0"]
        return src

    def load_column(self, fields):
        """fields: dict name -> global [ny, nx] numpy array for hsnow, tice0 and the 10 forcing fields"""
        es = self.blk.elem_slice()
        for k, dst in self.col.items():
            if k.endswith("_ext") and k not in fields:  # a slab ocean's relaxation target: the initial sst / sss without a key of its own
                k = k[:-4]
            _put(dst, fields[k][es])

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
        if self.slab_ocean:
            out.update({k: v for k, v in self.ocean_read().items() if k != "rows"})
        return out

    def ocean_read(self):
        """the slab ocean's state on the owned rows: {"rows": (r0, r1), "sst": [rows, nx], "sss": [rows, nx]}"""
        if not self.slab_ocean:
            raise ValueError("ocean_read needs slab_ocean=True")
        b = self.blk
        out = {"rows": (b.r0, b.r1)}
        for k in ("sst", "sss"):
            out[k] = self.col[k][b.j0:b.j1].detach().cpu().numpy().copy()
        return out

    def load_state_dict(self, state):
        """DynamicsCore.load_state_dict and, with advect_column_state, the snow S (required: plane 0 is the column's hsnow)"""
        if self.advect_column_state and "S" not in state:
            raise ValueError("a CoupledCore with advect_column_state needs the snow S in the state")
        if self.slab_ocean and not ("sst" in state and "sss" in state):
            raise ValueError("a CoupledCore with slab_ocean needs sst and sss in the state")
        super().load_state_dict(state)
        if self.slab_ocean:
            for k in ("sst", "sss"):
                _put(self.col[k], state[k][self.blk.elem_slice()])
        if self.advect_column_state:
            _put(self.S, state["S"][:, self.blk.elem_slice()])
            self._clear_land()

    def thermodynamics(self):
        self._mark(PHASE_COLUMN)
        state = {"hice": self.H[0], "cice": self.A[0], "hsnow": self.col["hsnow"], "tice0": self.col["tice0"]}
        forcing = {k: self.col[k] for k in self.COLUMN_FORCING}
        if self.tracers:
            self.ops.copy_f64(self._h_before, self.H[0])
        if self.slab_ocean:
            self.ops.set_slab_params(self._slab)  # (host only: a context that several cores share holds this core's at its call)
            self.ops.column_step_ocean(self.dt, state, forcing, self.newice, self._slab_ext, self.land)
        else:
            self.ops.column_step(self.dt, state, forcing, self.newice)
        if self.land is not None:
            # the column step computes on land elements too (it is pinned to the reference case by case); its result there is discarded:
            # the cell means of H, A (and S), the snow and the new ice (still the COLUMN phase of the phase table)
            for f in (self.H[0], self.A[0], self.col["hsnow"], self.newice):
                self.ops.land_clear(f)
        if self.tracers:
            # ice that grew carries the value 0 (every local row: element-local, as the column step)
            self.ops.tracers_dilute(0, self.blk.ny, self._h_before, self.H[0], self._tr)

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

    def _phases(self):
        self.external_forcing()
        self.thermodynamics()
        super()._phases()
        self.time += self.dt
