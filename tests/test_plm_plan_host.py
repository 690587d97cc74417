"""The plmDCA engine's launch planner (pydca_amd/csrc/plm_plan.h: plm_make_plan, host code that PlmEngine::configure runs)
against the decisions of the commit that introduced it, on the CPU.  tests/golden/plm_plans.npz was recorded by running that
commit's parent's configure() arithmetic -- pasted verbatim into a stand-alone program, its environment reads routed through a
table -- over the shapes and knob settings below; the file names that parent commit.  Every recorded column has to come out equal for
every row: the float32 gradient's bits depend on this geometry (it fixes the order in which the slabs of G are summed), and
so do the timings.  A pull request that changes the model on purpose records the file anew from its own planner and says so.

Five facts that the planner's comments quote are asserted by name as well, so that a regenerated fixture cannot drift from
them unnoticed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SHAPE = ["N", "L", "q", "elemBytes", "halo", "chunkArg", "warmArg", "carryMode", "stripWorld", "stripRank", "strips"]
KNOBS = ["scatterRem", "scatterSplit", "scatterCanon", "scatterWaves", "plmPairs", "scatterMerge", "foldMerge", "fuseFx"]
SCALARS = ["cS0", "cS1", "Lloc", "oLo", "oHi", "pairBegin", "pairEnd", "chunk", "warm", "numScanChunks", "numScatChunks", "P", "Cs", "pairs",
           "gUnits", "pairJT", "Wrows", "Grows", "Npad", "NT", "scatJW", "scatWaves", "scatSplit", "scatChunksPerSplit", "scatBlockChunks",
           "scatPerBlock", "scatRemCT", "scatRemSplit", "scatRemChunksPerSplit", "nFxPart", "nRegPart", "grecvTotal", "xsendTotal", "xrecvTotal"]
MAX_WORLD = 8
COLUMNS = (SCALARS + ["siteB%d" % r for r in range(MAX_WORLD + 1)] +
           ["%s%d" % (n, r) for n in ("grecvOff", "xsendOff", "xrecvOff") for r in range(MAX_WORLD)])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "plm_plans.npz"))


@pytest.fixture(scope="module")
def planned(golden, tmp_path_factory):
    """the planner's output for every row of the fixture: {column: int64 array}"""
    so = str(tmp_path_factory.mktemp("plan") / "libplm_plan_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-fast-math", "-ffp-contract=off", "-shared", "-fPIC", "-Wall",
                           "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "plm_plan_driver.cpp")])
    fn = C.CDLL(so).plm_plan_driver
    fn.restype = None
    shape = np.stack([golden["in_" + n] for n in SHAPE], axis=1).astype(np.int32)
    knobs = np.stack([golden["knob_" + n] for n in KNOBS], axis=1).astype(np.int32)
    ks = (C.c_int * 6)(*golden["kernel_shapes"].tolist())
    assert int(shape[:, SHAPE.index("stripWorld")].max()) <= MAX_WORLD
    out = np.zeros((len(shape), len(COLUMNS)), dtype=np.int64)
    buf = (C.c_longlong * len(COLUMNS))()
    for i in range(len(shape)):
        fn((C.c_int * len(SHAPE))(*shape[i].tolist()), (C.c_int * len(KNOBS))(*knobs[i].tolist()), ks, MAX_WORLD, buf)
        out[i] = buf[:]
    return {n: out[:, j] for j, n in enumerate(COLUMNS)}


def test_the_fixture_covers_the_grid(golden):
    n = len(golden["in_N"])
    assert n > 3000 and str(golden["parent_commit"])
    assert {int(v) for v in golden["in_elemBytes"]} == {4, 8} and {int(v) for v in golden["in_q"]} == {5, 21}
    assert {int(v) for v in golden["in_stripWorld"]} == {1, 4, 8} and {int(v) for v in golden["in_halo"]} == {0, 64}
    assert {int(v) for v in golden["in_carryMode"]} == {0, 1, 2} and 64 in golden["in_chunkArg"]
    for k, vals in (("scatterRem", {0, 1}), ("scatterSplit", {3}), ("scatterCanon", {1, 2}), ("scatterWaves", {8}), ("plmPairs", {0})):
        assert vals <= {int(v) for v in golden["knob_" + k]}, k


@pytest.mark.parametrize("column", COLUMNS)
def test_same_plan_as_recorded(golden, planned, column):
    want, got = golden["out_" + column], planned[column]
    bad = np.flatnonzero(want != got)
    rows = [({n: int(golden["in_" + n][i]) for n in SHAPE}, {n: int(golden["knob_" + n][i]) for n in KNOBS if golden["knob_" + n][i] != -1},
             int(want[i]), int(got[i])) for i in bad[:5]]
    assert bad.size == 0, "%d rows differ, (shape, knobs, recorded, planned): %r" % (bad.size, rows)


def _row(golden, N, L, q, elem_bytes):
    m = np.ones(len(golden["in_N"]), dtype=bool)
    for n, v in (("N", N), ("L", L), ("q", q), ("elemBytes", elem_bytes), ("halo", 0), ("chunkArg", 0), ("carryMode", 1), ("stripWorld", 1)):
        m &= golden["in_" + n] == v
    for n in KNOBS:
        m &= golden["knob_" + n] == -1
    (i,) = np.flatnonzero(m)
    return int(i)


CONFIG = {"C": (10000, 200, 21), "D": (50000, 500, 21), "E": (200000, 150, 5)}


def _facts(planned, i, elem_bytes):
    p = {n: int(planned[n][i]) for n in SCALARS}
    p["strips"] = -(-p["Cs"] // (512 // elem_bytes))
    return p


def test_config_c_float32_33_strips_one_left_over_in_a_6_way_split(golden, planned):
    p = _facts(planned, _row(golden, *CONFIG["C"], 4), 4)
    assert (p["strips"], p["scatSplit"], p["scatRemCT"], p["scatRemSplit"]) == (33, 1, 1, 6)


def test_config_c_float64_66_strips(golden, planned):
    assert _facts(planned, _row(golden, *CONFIG["C"], 8), 8)["strips"] == 66


def test_config_d_float32_83_strips_three_left_over_in_a_5_way_split(golden, planned):
    p = _facts(planned, _row(golden, *CONFIG["D"], 4), 4)
    assert (p["strips"], p["scatSplit"], p["scatRemCT"], p["scatRemSplit"]) == (83, 1, 3, 5)


def test_config_e_float32_6_strips_split_28_pair_tile_11(golden, planned):
    p = _facts(planned, _row(golden, *CONFIG["E"], 4), 4)
    assert (p["strips"], p["scatSplit"], p["scatRemCT"], p["pairs"], p["pairJT"]) == (6, 28, 0, 1, 11)


def test_config_e_float64_12_by_5_workgroups_13_blocks_slab_per_block(golden, planned):
    p = _facts(planned, _row(golden, *CONFIG["E"], 8), 8)
    site_groups = -(-p["gUnits"] // (16 * p["scatJW"]))
    assert (p["strips"], site_groups, p["scatSplit"], p["scatPerBlock"], p["scatBlockChunks"]) == (12, 5, 13, 1, 16384 // 128)
