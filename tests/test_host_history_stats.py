"""The C++ host's history statistics and time series (host/include/HistoryOutput.hpp; include/nsdg.h "history output") on the device: the
128 x 96 box of tests/test_host_history.py, 8 steps of 120 s with 24 sub-iterations.  The series file and the records are compared byte
for byte between 1 and 4 row blocks and across a restart; with every new key absent, the restart bytes are those of a run that knows
none of them."""
import os

import numpy as np
import pytest

import test_host_history as H
from test_host_history import host, runs  # noqa: F401  (the module's fixtures: every configuration runs once)

pytestmark = pytest.mark.gpu

STATS = "hice,hice:min,hice:max,speed:ice_mean,shear:ice_mean,cice:ice_mean,sigma_s:max,u"
SERIES = "area,extent,volume,drift,speed_max,hice_max"


def keys(buffer=3, fields=SERIES):
    """the series in the run's own directory; a buffer of three samples flushes twice in eight steps and once more at stop()"""
    return "series_file = totals.txt\nseries_fields = %s\nseries_buffer = %d\n" % (fields, buffer)


def series(final):
    """(header line, [data lines]) of the series file beside a run's restart file"""
    with open(os.path.join(os.path.dirname(final), "totals.txt"), "rb") as f:
        lines = f.read().decode().splitlines()
    return lines[0], lines[1:]


def values(lines):
    return np.array([[float(x) for x in line.split()] for line in lines])


def test_the_series_of_one_row_block_and_of_four_are_byte_identical(runs):
    one, _, final1 = runs("series1", H.output(480, STATS) + keys())
    four, _, final4 = runs("series4", H.output(480, STATS) + keys(), "row_blocks = 4\n")
    head, lines = series(final1)
    assert head == "# time " + SERIES.replace(",", " ") and len(lines) == 8
    assert (head, lines) == series(final4) and one == four
    v = values(lines)
    assert np.array_equal(v[:, 0], np.arange(120, 1080, 120)) and np.all(np.isfinite(v))
    cell, cells = (256e3 / H.NSLOW) * (256e3 / H.NFAST), H.NSLOW * H.NFAST
    area, extent, volume, drift, speed_max, hice_max = v[:, 1:].T
    assert np.all(area > 0) and np.all(area <= extent) and np.all(extent <= cells * cell * (1 + 1e-12))
    assert np.all(np.abs(extent / cell - np.round(extent / cell)) < 1e-6)  # whole cells
    assert np.all(np.abs(volume - volume[0]) <= 1e-12 * volume[0])  # a closed box
    assert np.all(drift > 0) and np.all(drift <= speed_max) and np.all(hice_max >= 0.3 * (1 - 1e-9))
    # one flush of everything at stop() writes the same lines as a flush every three steps
    _, _, final = runs("series_late", H.output(480, STATS) + keys(buffer=256))
    assert series(final) == (head, lines)


def test_the_stat_records_of_one_row_block_and_of_four_are_equal(runs):
    _, rec1, _ = runs("series1", H.output(480, STATS) + keys())
    _, rec4, _ = runs("series4", H.output(480, STATS) + keys(), "row_blocks = 4\n")
    assert sorted(rec1) == [480, 960] and rec1 == rec4
    h, f = H.record(rec1[960])
    assert h["fields"] == STATS and h["samples"] == "4"
    assert np.all(f["hice:min"] <= f["hice"]) and np.all(f["hice"] <= f["hice:max"]) and np.any(f["hice:min"] < f["hice:max"])
    assert np.all(np.isfinite(f["speed:ice_mean"])) and np.max(f["speed:ice_mean"]) > 1e-4 and np.all(f["cice:ice_mean"] <= 1.0)
    # the plain entries are the plain run's planes, bit for bit: a statistic beside them changes nothing
    plain = H.record(runs("one", H.output(480))[1][960])[1]
    assert np.array_equal(f["hice"], plain["hice"]) and np.array_equal(f["u"], plain["u"])
    assert np.all(f["sigma_s:max"] >= plain["sigma_s"])


def test_the_lines_of_a_restarted_run_are_those_of_the_whole_run(runs):
    _, _, whole = runs("series1", H.output(480, STATS) + keys())
    _, _, first = runs("series_first", H.output(480, STATS) + keys(), stop=480)
    _, _, second = runs("series_second", H.output(480, STATS) + keys(), start=480, stop=960, init_file=first)
    head, lines = series(whole)
    assert series(first) == (head, lines[:4]) and series(second) == (head, lines[4:])  # the file is truncated at start()


def test_without_the_new_keys_the_restart_bytes_are_unchanged(runs):
    off, none, final = runs("off")
    assert none == {} and not os.path.exists(os.path.join(os.path.dirname(final), "totals.txt"))
    assert runs("series1", H.output(480, STATS) + keys())[0] == off  # and with all of them on
    assert runs("series_only", keys())[0] == off


def test_the_snow_volume_of_a_coupled_run(runs):
    _, _, final = runs("series_thermo", keys(fields="snow_volume,volume,area"), H.THERMO)
    head, lines = series(final)
    v = values(lines)
    assert head == "# time snow_volume volume area" and len(lines) == 8 and np.all(v[:, 1] > 0) and np.all(v[:, 1] < v[:, 2])
