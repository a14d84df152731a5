"""What a run of the row-block driver (nextsimdg_amd/rowblock.py) leaves behind besides its state: time means and window statistics of
fields (History), per-step row totals (Series), Lagrangian points (Drifters) with the fields sampled along their tracks, and the fields at
fixed points (Stations).  Each class checks its own constructor arguments, owns its
device buffers and has the one call the driver's step frame makes per model step, and read().  A core holds each as an object or None; with
None nothing is asked of `ops` and nothing is allocated.  The C++ host keeps the same concerns apart (HistoryOutput, Drifters, Stations)."""
import math

import numpy as np
import torch

from nextsimdg_amd import abi


def require_ops(ops, calls, what, kind):
    """ValueError unless `ops` has the optional `calls` of abi.Context that the feature `what` needs (kind: how the message names them)"""
    missing = [m for m in calls if not callable(getattr(ops, m, None))]
    if missing:
        raise ValueError("%s needs an ops object with the %s of the C ABI (abi.Context); %s has no %s" % (what, kind, type(ops).__name__, ", ".join(missing)))


def _names(arg, what, kind):
    """history= / series= as a tuple of at least one name"""
    names = (arg,) if isinstance(arg, str) else tuple(arg)
    if not names:
        raise ValueError("%s= needs at least one %s (None turns it off)" % (what, kind))
    return names


COLUMN_FIELDS = ("hsnow", "tice")  # the fields of the column state exist in a CoupledCore only


def check_known(names, what):
    """ValueError for a name that is no field of abi.HISTORY_FIELDS (what: how the message names the list's entries, e.g. "history field")"""
    unknown = [n for n in names if n not in abi.HISTORY_FIELDS]
    if unknown:
        raise ValueError("unknown %s %s (known: %s)" % (what, ", ".join(repr(n) for n in unknown), " ".join(abi.HISTORY_FIELDS)))


def check_carried(names, what, rheology, column_state):
    """ValueError for a field the core does not carry: the damage without the brittle rheology, column state without a column.  Stated
    once for the history, the drifters' fields and the stations"""
    if "damage" in names and rheology != "bbm":
        raise ValueError("the %s 'damage' needs rheology='bbm': the mEVP sub-cycle has no damage" % what)
    column = [n for n in names if n in COLUMN_FIELDS]
    if column and not column_state:
        raise ValueError("the %s %s is column state: it needs a CoupledCore" % (what, ", ".join(repr(n) for n in column)))


def point_fields(arg, what, rheology, column_state):
    """drifter_fields= / station_fields= as a tuple of names the core can sample at a point; ValueError otherwise"""
    names = _names(arg, what + "s", "field")
    label = what.replace("_", " ")
    check_known(names, label)
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise ValueError("%s %s is listed twice" % (label, ", ".join(repr(n) for n in twice)))
    check_carried(names, label, rheology, column_state)
    return names


def check_points(xy, what, Lx, Ly, columns):
    """positions as a float64 array [n, 2] (or a width of `columns`): finite and inside the domain [0, Lx] x [0, Ly]; ValueError otherwise"""
    xy = np.array(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] not in columns:
        raise ValueError({"drifter": "drifters must be an [n, 2] array of positions or an [n, 3] array with the status, got shape %s",
                          "station": "stations must be an [n, 2] array of positions, got shape %s"}[what] % (xy.shape,))
    if not np.all(np.isfinite(xy)):
        raise ValueError("%s %d has a non-finite value" % (what, int(np.argwhere(~np.isfinite(xy))[0][0])))
    outside = ~((xy[:, 0] >= 0) & (xy[:, 0] <= Lx) & (xy[:, 1] >= 0) & (xy[:, 1] <= Ly))
    if outside.any():
        k = int(np.argwhere(outside)[0][0])
        raise ValueError("%s %d at (%r, %r) m is outside the domain [0, %r] x [0, %r] m" % (what, k, float(xy[k, 0]), float(xy[k, 1]), Lx, Ly))
    return xy


class History:
    """history=: names of abi.HISTORY_FIELDS sampled once per model step (step(), or advance() with all its sub-steps) into one accumulator
    on the device, read as time means by read().  An entry may be "name:stat" with a statistic of abi.HISTORY_STATS ("name" alone is the
    mean): ice-weighted means and the extremes of the window (include/nsdg.h "history output")"""

    COLUMN_FIELDS = COLUMN_FIELDS

    def __init__(self, entries, ops, blk, device, rheology, transported, column_state):
        """ValueError for a list the core cannot sample"""
        self.entries = entries = _names(entries, "history", "field")
        self.pairs = pairs = [tuple(e.split(":", 1)) if ":" in e else (e, "mean") for e in entries]
        names = [n for n, _ in pairs]
        check_known(names, "history field")
        unknown = [e for e, (_, st) in zip(entries, pairs) if st not in abi.HISTORY_STATS]
        if unknown:
            raise ValueError("unknown history statistic in %s (known: %s)" % (", ".join(repr(e) for e in unknown), " ".join(abi.HISTORY_STATS)))
        twice = sorted({e for e, p in zip(entries, pairs) if pairs.count(p) > 1})
        if twice:
            raise ValueError("history field %s is listed twice" % ", ".join(repr(n) for n in twice))
        check_carried(names, "history field", rheology, column_state)
        weighted = [e for e, (_, st) in zip(entries, pairs) if st == "ice_mean"]
        if weighted and "A" not in transported:
            raise ValueError("the history entry %s weights by the concentration: this core has no A" % ", ".join(repr(e) for e in weighted))
        # a list of bare names is sampled by ops.history_accumulate, as ever: a test double without the statistics keeps working
        self.with_stats = any(":" in e for e in entries)
        require_ops(ops, ("history_accumulate_stats" if self.with_stats else "history_accumulate",), "history=", "history call")
        self.ops, self.blk = ops, blk
        self.acc = torch.zeros(len(entries), blk.j1 - blk.j0, blk.nx, dtype=torch.float64, device=device)  # the owned rows only: a sample is element-local
        # the summed weights of the window, one plane for every ice-weighted mean; None: no entry asks for one
        self.wacc = torch.zeros(blk.j1 - blk.j0, blk.nx, dtype=torch.float64, device=device) if weighted else None
        self.count = 0

    def sample(self, sources):
        """one sample of the owned rows at the end of a model step: one launch, after the step's last phase mark and outside every
        captured graph; the first sample of a window stores, the others add"""
        b = self.blk
        if self.with_stats:
            self.ops.history_accumulate_stats(b.j0, b.j1, self.pairs, sources, self.count == 0, b.j0, self.acc, self.wacc)
        else:
            self.ops.history_accumulate(b.j0, b.j1, self.entries, sources, self.count == 0, b.j0, self.acc)
        self.count += 1

    def read(self, reset=True):
        """{"rows": (r0, r1), "count": n, name: float64 [rows, nx] = the mean of the n samples since the last reset} for the rows this rank
        owns (one download; waits for the last sample).  reset: the next sample opens a new window.  merge_history() joins the ranks"""
        if self.count == 0:
            raise ValueError("history_read(): no sample since the last reset")
        b, n = self.blk, self.count
        acc = self.acc.detach().cpu().numpy()
        wacc = self.wacc.detach().cpu().numpy() if self.wacc is not None else None
        out = {"rows": (b.r0, b.r1), "count": n}
        for k, (entry, (_, stat)) in enumerate(zip(self.entries, self.pairs)):
            if stat == "mean":
                out[entry] = acc[k] / n
            elif stat == "ice_mean":  # NaN where the window saw no ice
                iced = wacc > 0
                out[entry] = np.where(iced, acc[k] / np.where(iced, wacc, 1.0), np.nan)
            else:
                out[entry] = acc[k].copy()
        if reset:
            self.count = 0
        return out


class Series:
    """series=: names of abi.SERIES_QUANTITIES; every model step leaves their row totals in the next of `capacity` slots of a device buffer,
    read by read() and made domain totals by merge_series().  extent_conc: the concentration the ice extent counts from"""

    def __init__(self, names, capacity, extent_conc, ops, blk, device, column_state):
        """ValueError for a list the core cannot total"""
        self.names = names = _names(names, "series", "quantity")
        unknown = [n for n in names if n not in abi.SERIES_QUANTITIES]
        if unknown:
            raise ValueError("unknown series quantity %s (known: %s)" % (", ".join(repr(n) for n in unknown), " ".join(abi.SERIES_QUANTITIES)))
        twice = sorted({n for n in names if names.count(n) > 1})
        if twice:
            raise ValueError("series quantity %s is listed twice" % ", ".join(repr(n) for n in twice))
        if "drift" in names and "area" not in names:
            raise ValueError("the series quantity 'drift' is the ice-weighted mean speed: it needs 'area', the sum of the weights, in the list")
        if "snow_volume" in names and not column_state:
            raise ValueError("the series quantity 'snow_volume' is column state: it needs a CoupledCore")
        if int(capacity) < 1:
            raise ValueError("series_capacity must be at least 1, got %r" % (capacity,))
        if not math.isfinite(extent_conc):
            raise ValueError("extent_conc must be finite, got %r" % (extent_conc,))
        require_ops(ops, ("history_row_totals",), "series=", "row totals")
        self.ops, self.blk, self.capacity, self.extent_conc = ops, blk, int(capacity), float(extent_conc)
        self.buf = torch.zeros(self.capacity, len(names), blk.j1 - blk.j0, dtype=torch.float64, device=device)
        self.count = 0

    def room(self):
        """a model step begins: ValueError if its row totals would find no free slot.  The host counts the slots; nothing is synchronised"""
        if self.count >= self.capacity:
            raise ValueError("the series buffer is full (series_capacity = %d samples): call series_read() before the next step" % self.capacity)

    def sample(self, sources):
        """the row totals of the owned rows at the end of a model step: one launch into the next free slot"""
        b = self.blk
        self.ops.history_row_totals(b.j0, b.j1, self.names, sources, self.extent_conc, b.j0, self.buf[self.count])
        self.count += 1

    def read(self, reset=True):
        """{"rows": (r0, r1), "count": n, name: float64 [n, rows] = the row totals of the n steps since the last reset} for the rows this
        rank owns, as the device left them (one download; waits for the last step).  reset: the next step writes slot 0 again.
        merge_series() makes the totals of the whole domain"""
        b, n = self.blk, self.count
        buf = self.buf[:n].detach().cpu().numpy()
        out = {"rows": (b.r0, b.r1), "count": n}
        for k, name in enumerate(self.names):
            out[name] = buf[:, k].copy()
        if reset:
            self.count = 0
        return out


class Drifters:
    """drifters=: [n, 2] positions (x, y) in metres of the GLOBAL domain [0, nx hx] x [0, ny_global hy], or [n, 3] with the status (0 active,
    1 left the domain, 2 lost its ice, 3 on land) as a third column: Lagrangian points moved once per step() by the velocity the sub-cycle
    left (include/nsdg.h "drifters").  Every rank keeps the whole list.  min_conc: the cell-mean concentration below
    which a drifter has lost its ice.  halo: the core's exchanger, which merges the ranks' lists; complete_ghosts: the sub-cycle leaves the
    velocity of the ghost rows incomplete (one sub-iteration per pass), so a step first exchanges it.  fields: drifter_fields=, names of
    abi.HISTORY_FIELDS sampled at the NEW position of every drifter after every step (include/nsdg.h "point samples", DESIGN.md section
    6.5), or None; order: the DG order of the core's fields"""

    def __init__(self, points, min_conc, ops, blk, hx, hy, halo, device, complete_ghosts, fields=None, order=2):
        """ValueError for a list the core cannot carry (the core has checked `fields` with point_fields())"""
        require_ops(ops, ("drifters_advance",), "drifters=", "drifter call")
        if fields is not None:
            require_ops(ops, ("points_sample",), "drifter_fields=", "point-sample call")
        if not math.isfinite(min_conc):
            raise ValueError("drifter_min_conc must be finite, got %r" % (min_conc,))
        xy = check_points(points, "drifter", blk.nx * hx, blk.ny_glob * hy, (2, 3))
        d = np.zeros((3, xy.shape[0]))  # (x, y, status) by rows
        d[:xy.shape[1]] = xy.T
        bad = ~np.isin(d[2], (0.0, 1.0, 2.0, 3.0))
        if bad.any():
            k = int(np.argwhere(bad)[0][0])
            raise ValueError("drifter %d has the status %r; known: 0 active, 1 left the domain, 2 lost its ice, 3 on land" % (k, float(d[2, k])))
        if blk.world > 1 and not halo.can_reduce():
            raise ValueError("drifters= on %d row blocks merges the ranks' lists after every step: it needs a NativeHaloExchanger "
                             "(comm_max_f64_array) or an initialised torch.distributed process group (all_reduce); %s has neither"
                             % (blk.world, type(halo).__name__))
        self.ops, self.blk, self.halo, self.min_conc, self.complete_ghosts = ops, blk, halo, float(min_conc), complete_ghosts
        self.now = torch.from_numpy(d).to(device)  # the whole list on every rank, and the partner an out-of-place step writes
        self.other = torch.empty_like(self.now)
        # the samples along the track, [nfields, n], the whole table on every rank; NaN until the first step has sampled
        self.fields, self.order = fields, order
        self.samples = None if fields is None else torch.full((len(fields), d.shape[1]), float("nan"), dtype=torch.float64, device=device)

    def step(self, dt, u, v, A, sources=None):
        """the drifters of the owned rows move by one Heun step of dt with the velocity the sub-cycle left and the concentration the
        transport left, then the ranks' lists are merged: a rank writes -inf for what it does not own, so the elementwise maximum is the
        whole list.  Out of place: the two arrays swap.  No phase of its own; inside the span, before its end mark.  With fields, the
        merged list is then sampled at its NEW positions from `sources` (name -> tensor, as the history's): every rank samples the points
        of its own rows and writes -inf for the others, and one more maximum over the ranks makes the whole table"""
        if self.now.shape[1] == 0:
            return
        b = self.blk
        if b.world > 1 and self.complete_ghosts:
            # a predictor may sit in the ghost row above, whose upper node rows a single-iteration sub-cycle never receives (it needs
            # the lowest only): one exchange of the velocity with the ghost rows complete
            self.halo.nodal((u, v), rows_down=2 * b.depth_above + 1)
        self.ops.drifters_advance(b.j0, b.j1, dt, self.min_conc, u, v, A, self.now, self.other)
        self.now, self.other = self.other, self.now
        if b.world > 1:
            self.halo.max_array(self.now)
        if self.fields is not None:
            self.ops.points_sample(b.j0, b.j1, self.order, self.now[0], self.now[1], self.fields, sources, self.samples)
            if b.world > 1:
                self.halo.max_array(self.samples)

    def read(self):
        """{"x", "y": float64 [n] in metres of the global domain, "status": int64 [n]} -- the whole list, identical on every rank (one
        download; waits for the last step)"""
        d = self.now.detach().cpu().numpy()
        out = {"x": d[0].copy(), "y": d[1].copy(), "status": d[2].astype(np.int64)}
        if self.fields is not None:  # "fields": {name: float64 [n]}, the samples at these positions (NaN before the first step)
            smp = self.samples.detach().cpu().numpy()
            out["fields"] = {name: smp[k].copy() for k, name in enumerate(self.fields)}
        return out

    def state(self):
        """the [3, n] array of state_dict(): the whole list, not row-sliced -- every rank holds the same"""
        return self.now.detach().cpu().numpy().copy()

    def load_state(self, state):
        if "drifters" not in state or tuple(state["drifters"].shape) != tuple(self.now.shape):
            raise ValueError("a core with drifters= needs the [3, %d] array 'drifters' in the state" % self.now.shape[1])
        self.now.copy_(torch.from_numpy(np.ascontiguousarray(state["drifters"])).to(self.now.device))
        if self.samples is not None:  # what was sampled belongs to other positions: NaN until the next step samples the loaded ones
            self.samples.fill_(float("nan"))


class Stations:
    """stations=: [n, 2] fixed positions (x, y) in metres of the global domain, validated like drifter positions; fields: station_fields=,
    names of abi.HISTORY_FIELDS.  Every model step leaves the fields AT those points (include/nsdg.h "point samples", DESIGN.md section
    6.5) in the next of `capacity` slots of a device buffer [capacity][nfields][n]: -inf where this rank does not own the point.  No
    collective: read() gives this rank's part, merge_stations() the whole table"""

    def __init__(self, points, fields, capacity, ops, blk, hx, hy, device, order=2):
        """ValueError for a list the core cannot sample (the core has checked `fields` with point_fields())"""
        require_ops(ops, ("points_sample",), "stations=", "point-sample call")
        xy = check_points(points, "station", blk.nx * hx, blk.ny_glob * hy, (2,))
        if int(capacity) < 1:
            raise ValueError("station_capacity must be at least 1, got %r" % (capacity,))
        self.ops, self.blk, self.fields, self.order, self.capacity = ops, blk, fields, order, int(capacity)
        self.xy = torch.from_numpy(np.ascontiguousarray(xy.T)).to(device)  # [2, n]: x and y by rows
        self.buf = torch.zeros(self.capacity, len(fields), xy.shape[0], dtype=torch.float64, device=device)
        self.count = 0

    def room(self):
        """a model step begins: ValueError if its samples would find no free slot.  The host counts the slots; nothing is synchronised"""
        if self.count >= self.capacity:
            raise ValueError("the station buffer is full (station_capacity = %d samples): call stations_read() before the next step" % self.capacity)

    def sample(self, sources):
        """the fields at the stations of the owned rows at the end of a model step: one launch into the next free slot, after the step's
        last phase mark and outside every captured graph"""
        b = self.blk
        if self.xy.shape[1]:
            self.ops.points_sample(b.j0, b.j1, self.order, self.xy[0], self.xy[1], self.fields, sources, self.buf[self.count])
        self.count += 1

    def read(self, reset=True):
        """{"count": n, "x", "y": float64 [points], name: float64 [n, points] = the samples of the n steps since the last reset}, -inf where
        this rank does not own the point (one download; waits for the last step).  reset: the next step writes slot 0 again"""
        n = self.count
        buf = self.buf[:n].detach().cpu().numpy()
        xy = self.xy.detach().cpu().numpy()
        out = {"count": n, "x": xy[0].copy(), "y": xy[1].copy()}
        for k, name in enumerate(self.fields):
            out[name] = buf[:, k].copy()
        if reset:
            self.count = 0
        return out


def merge_stations(parts):
    """the ranks' stations_read()s (any order) -> the record of the whole domain: exactly one rank owns a station and the others hold
    -inf, so the elementwise maximum is the whole table (np.maximum keeps a NaN sample)"""
    parts = list(parts)
    if any(p["count"] != parts[0]["count"] for p in parts):
        raise ValueError("the ranks hold different numbers of samples: %s" % [p["count"] for p in parts])
    if any(not (np.array_equal(p["x"], parts[0]["x"]) and np.array_equal(p["y"], parts[0]["y"])) for p in parts):
        raise ValueError("the ranks hold different stations")
    out = {"count": parts[0]["count"], "x": parts[0]["x"].copy(), "y": parts[0]["y"].copy()}
    for k in parts[0]:
        if k not in ("count", "x", "y"):
            out[k] = parts[0][k].copy()
            for p in parts[1:]:
                out[k] = np.maximum(out[k], p[k])
    return out


def _joined(parts):
    """the ranks' records in row order; ValueError unless they hold the same number of samples and their rows join"""
    parts = sorted(parts, key=lambda p: p["rows"][0])
    if any(p["count"] != parts[0]["count"] for p in parts):
        raise ValueError("the ranks hold different numbers of samples: %s" % [p["count"] for p in parts])
    if any(a["rows"][1] != c["rows"][0] for a, c in zip(parts, parts[1:])):
        raise ValueError("the ranks' rows do not join: %s" % [p["rows"] for p in parts])
    return parts, {"rows": (parts[0]["rows"][0], parts[-1]["rows"][1]), "count": parts[0]["count"]}


def merge_history(parts):
    """the ranks' history_read()s (any order) -> the record of the whole domain"""
    parts, out = _joined(parts)
    for k in parts[0]:
        if k not in ("rows", "count"):
            out[k] = np.concatenate([p[k] for p in parts], axis=0)
    return out


def merge_series(parts, hx, hy):
    """the ranks' series_read()s (any order) -> {"count": n, name: float64 [n]}: area and extent in m^2, volume and snow_volume in
    m^3, drift = sum(w speed) / sum(w) in m/s (NaN where there is no ice), speed_max, hice_max.  The rows of a sample are added one
    after the other in global row order, whatever the decomposition, so one block and N blocks give the same bits"""
    parts, out = _joined(parts)
    n = out["count"]
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
