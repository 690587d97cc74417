"""Host side of the greedy ascent (dca_plm_ascend, dca_mf_ascend, find_local_maxima and its sub-command):
exports and declarations, the Python argument checks (before any device work), the sub-command's options and files through a
stand-in, the launch plan of ascent_plan.h, and the float64 restatement of tests/ascent_reference.py against the longdouble path
on fresh tables on every model tests/test_ascent.py uses (the mf models here are the oracle's; the GPU file checks the device's
own again), with planted faults that must change the restated path."""
import os
import subprocess

import numpy as np
import pytest

import ascent_reference as R
from conftest import data_file
from pydca_amd import _lib, _potts, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.plmdca.plmdca import PlmDCAException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dca_plm_ascend", "dca_mf_ascend")
TOY_RNA = data_file("toy_rna.fa")


# ---------------------------------------------------------------- C ABI
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert "int " + name + "(dca_ctx* ctx, const uint8_t* X /* n x L */, int n, const int32_t* free_sites, int num_free, int max_steps," in header
    assert '"ascent_init"' in header and '"ascent"' in header and "DESIGN.md section 24" in header
    assert "DCA_ASCENT_PASS" in header and "DCA_ASCENT_LDS" in header
    assert "## 24." in open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "DCA_ASCENT_PASS" in readme and "DCA_ASCENT_LDS" in readme and "find_local_maxima" in readme
    assert hasattr(_lib.Context, "plm_ascend") and hasattr(_lib.Context, "mf_ascend")
    assert "ascent.hip" in open(os.path.join(ROOT, "pydca_amd", "csrc", "Makefile")).read()


def test_entries_refuse_without_a_context():
    lib = _lib.lib()
    X = np.zeros((2, 4), dtype=np.uint8)
    out = np.zeros((2, 4), dtype=np.uint8)
    steps = np.zeros(2, dtype=np.int32)
    conv = np.zeros(2, dtype=np.uint8)
    sites = np.array([1, 2], dtype=np.int32)
    for name in ENTRIES:
        assert getattr(lib, name)(None, X.ctypes.data, 2, sites.ctypes.data, 2, 3, 0.0, out.ctypes.data, steps.ctypes.data,
                                  conv.ctypes.data, None, None, None) == _lib.DCA_ERR_ARG


# ---------------------------------------------------------------- Python argument checks
class Boom(Exception):
    pass


class Quiet:
    def info(self, *a):
        pass

    error = info


class Model(_potts.PottsModel):
    """PottsModel over a recorded _potts_call: L = 6 RNA sites; the ascent moves nothing and the energy is the row's code sum"""
    _potts_exc = Boom
    _potts_table = 0
    _potts_logger = Quiet()

    def __init__(self, devices=None, final=None, converged=None):
        self.calls, self.devices, self.final, self.converged = [], devices, final, converged

    def _potts_dims(self):
        return _lib.DCA_BIOMOLECULE_RNA, 6, 5

    def _potts_devices(self):
        return self.devices

    def _potts_default_source(self):
        return ["ACGUAC", "UUUUUU"]

    def _potts_call(self, name, *args, **kw):
        self.calls.append((name, args, kw))
        X = np.asarray(args[0])
        if name == "energies":
            return X.sum(axis=1).astype(np.float64)
        n = X.shape[0]
        codes = X.copy() if self.final is None else np.asarray(self.final, dtype=np.uint8)
        conv = np.ones(n, bool) if self.converged is None else np.asarray(self.converged, dtype=bool)
        res = {"codes": codes, "steps": np.arange(n, dtype=np.int32) % 2, "converged": conv, "gains": np.zeros(n)}
        if kw.get("paths"):
            res["path"] = np.tile(np.array([[[2, 4]]], dtype=np.int32), (n, 1, 1))
            res["path_gains"] = np.full((n, 1), 0.5)
        return res


def test_argument_checks_come_before_the_device():
    m = Model()
    with pytest.raises(Boom, match="exactly one"):
        m.find_local_maxima(["ACGUAC"], free_sites=[1], fixed_sites=[2])
    with pytest.raises(Boom, match="twice"):
        m.find_local_maxima(["ACGUAC"], free_sites=[1, 3, 1])
    for bad in ([6], [-1, 2]):
        with pytest.raises(Boom, match="0 .. 5"):
            m.find_local_maxima(["ACGUAC"], free_sites=bad)
    with pytest.raises(Boom, match="integers"):
        m.find_local_maxima(["ACGUAC"], fixed_sites=[1.5])
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(Boom, match="max_steps"):
            m.find_local_maxima(["ACGUAC"], max_steps=bad)
    for bad in (-0.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(Boom, match="min_gain"):
            m.find_local_maxima(["ACGUAC"], min_gain=bad)
    assert m.calls == []                                        # every rejection came before the device call
    with pytest.raises(Boom, match="one GPU"):
        Model(devices=[0, 1]).find_local_maxima(["ACGUAC"])
    with pytest.raises(Boom, match="record 2"):
        m.find_local_maxima(["ACGUAC", "ACG"])
    assert m.calls == []


def test_defaults_sites_and_the_result():
    m = Model()
    res = m.find_local_maxima()                                 # the training alignment's rows, every site free, 4 F steps
    name, args, kw = m.calls[0]
    assert name == "ascend" and args[0].tolist() == [[0, 1, 2, 3, 0, 1], [3, 3, 3, 3, 3, 3]]
    assert args[1].dtype == np.int32 and args[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert kw == {"max_steps": 24, "min_gain": 0.0, "paths": False}
    assert [c[0] for c in m.calls] == ["ascend", "energies", "energies"]
    assert set(res) == {"sequences", "energies", "start_energies", "num_steps", "converged", "gains", "maxima", "basin",
                        "basin_sizes"}
    assert res["sequences"] == ["ACGUAC", "UUUUUU"] and res["energies"].tolist() == [7.0, 18.0]
    assert res["maxima"] == ["UUUUUU", "ACGUAC"] and res["basin"].tolist() == [1, 0] and res["basin_sizes"].tolist() == [1, 1]
    m.find_local_maxima(["ACGUAC"], free_sites=(4, 0, 2), max_steps=0, min_gain=1.5)
    assert m.calls[-3][1][1].tolist() == [0, 2, 4] and m.calls[-3][2] == {"max_steps": 0, "min_gain": 1.5, "paths": False}
    m.find_local_maxima(["ACGUAC"], fixed_sites=iter([5, 1]))
    assert m.calls[-3][1][1].tolist() == [0, 2, 3, 4] and m.calls[-3][2]["max_steps"] == 16
    m.find_local_maxima(["ACGUAC"], free_sites=[])
    assert m.calls[-3][1][1].size == 0 and m.calls[-3][2]["max_steps"] == 0
    res = m.find_local_maxima(["ACGUAC", "CCCCCC"], return_paths=True)
    assert m.calls[-3][2]["paths"] is True
    assert res["paths"] == [[], [(2, "-", 0.5)]]                # num_steps of the stand-in: 0 and 1


def test_basins_order_and_counts():
    final = np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 4], [1, 1, 1, 1, 1, 1], [4, 4, 4, 4, 4, 4], [0, 0, 0, 0, 4, 0],
                      [0, 0, 0, 0, 0, 4], [2, 2, 2, 2, 2, 2]], dtype=np.uint8)
    conv = [True, True, True, False, True, True, True]
    res = Model(final=final, converged=conv).find_local_maxima(["ACGUAC"] * 7)
    # energies (code sums): 6, 4, 6, 24, 4, 4, 12; the two maxima of energy 4 in lexicographic order of their codes
    assert res["maxima"] == ["GGGGGG", "CCCCCC", "AAAAA-", "AAAA-A"]
    assert res["basin"].tolist() == [1, 2, 1, -1, 3, 2, 0]
    assert res["basin_sizes"].tolist() == [1, 2, 2, 1]
    count = {}
    for k, seq in enumerate(res["sequences"]):
        if conv[k]:
            count[seq] = count.get(seq, 0) + 1
    assert [count[s] for s in res["maxima"]] == res["basin_sizes"].tolist()
    none = Model(final=final, converged=[False] * 7).find_local_maxima(["ACGUAC"] * 7)
    assert none["maxima"] == [] and none["basin"].tolist() == [-1] * 7 and none["basin_sizes"].size == 0


def test_context_binding_checks_the_shape():
    class Ctx(_lib.Context):
        def __init__(self):                                     # no device: only the host-side checks are reached
            self._l, self._h, self.L = _lib.lib(), None, 4
    with pytest.raises(ValueError, match="uint8"):
        Ctx().plm_ascend(np.zeros((2, 5), dtype=np.uint8), [0])
    with pytest.raises(ValueError, match="uint8"):
        Ctx().mf_ascend(np.zeros(4, dtype=np.uint8), [0])


# ---------------------------------------------------------------- command lines
@pytest.mark.parametrize("main,run", [(plmdca_main, "run_plm_dca"), (mfdca_main, "run_meanfield_dca")])
def test_find_local_maxima_arguments(monkeypatch, main, run):
    assert "find_local_maxima" in _potts.POTTS_SUBCOMMANDS
    seen = {}
    monkeypatch.setattr(main, "execute_from_command_line", lambda *a, **kw: seen.update(kw) or "done")
    assert getattr(main, run)(["find_local_maxima", "rna", "x.fa", "--query_file", "q.fa", "--free_sites", "10-30,45", "--max_steps", "7",
                               "--min_gain", "0.25"]) == "done"
    assert seen["the_command"] == "find_local_maxima" and seen["query_file"] == "q.fa"
    assert seen["ascent"] == {"free_sites": "10-30,45", "fixed_sites": None, "max_steps": 7, "min_gain": 0.25}
    getattr(main, run)(["find_local_maxima", "rna", "x.fa", "--fixed_sites", "1-3"])
    assert seen["query_file"] is None
    assert seen["ascent"] == {"free_sites": None, "fixed_sites": "1-3", "max_steps": None, "min_gain": 0.0}
    getattr(main, run)(["find_local_maxima", "rna", "x.fa"])
    assert seen["ascent"] == {"free_sites": None, "fixed_sites": None, "max_steps": None, "min_gain": 0.0}
    with pytest.raises(SystemExit):
        getattr(main, run)(["find_local_maxima", "rna", "x.fa", "--free_sites", "1", "--fixed_sites", "2"])
    with pytest.raises(SystemExit):                            # the other sub-commands do not take the new options
        getattr(main, run)(["compute_energies", "rna", "x.fa", "--max_steps", "2"])


class StandIn:
    """The calls run_subcommand makes for find_local_maxima, recorded"""
    sequences_len = 10

    def __init__(self):
        self.calls = []

    def find_local_maxima(self, sequences, **kw):
        self.calls.append((sequences, kw))
        return {"sequences": ["ACGU-ACGU-", "-----AAAAA", "ACGU-ACGU-"], "energies": np.array([2.5, 1.0 / 3.0, 2.5]),
                "start_energies": np.array([-1.25, 0.125, 2.5]), "num_steps": np.array([3, 40, 0], dtype=np.int32),
                "converged": np.array([True, False, True]), "gains": np.array([3.75, 0.2, 0.0]), "maxima": ["ACGU-ACGU-"],
                "basin": np.array([0, -1, 0]), "basin_sizes": np.array([2])}


def test_subcommand_files(tmp_path):
    inst = StandIn()
    out = str(tmp_path / "out")
    opts = {"free_sites": "8-9,2", "fixed_sites": None, "max_steps": 40, "min_gain": None}
    paths = _potts.run_subcommand(inst, "find_local_maxima", "MFDCA", TOY_RNA, out, ["# meta"], _lib.DCA_BIOMOLECULE_RNA, 1,
                                  PlmDCAException, query_file="q.fa", ascent=opts)
    assert [os.path.basename(p) for p in paths] == ["MFDCA_local_maxima_toy_rna.fa", "MFDCA_local_maxima_toy_rna.txt"]
    assert inst.calls[0] == ("q.fa", {"max_steps": 40, "min_gain": 0.0, "free_sites": [7, 8, 1]})
    assert open(paths[0]).read().splitlines() == [">maximum_of_1 energy=2.5", "ACGU-ACGU-", ">maximum_of_2 energy=%.17g" % (1.0 / 3.0),
                                                   "-----AAAAA", ">maximum_of_3 energy=2.5", "ACGU-ACGU-"]
    assert fasta_reader.get_alignment_from_fasta_file(paths[0]) == ["ACGU-ACGU-", "-----AAAAA", "ACGU-ACGU-"]
    lines = open(paths[1]).read().splitlines()
    assert "# meta" in lines and any("q.fa" in ln for ln in lines) and any(ln.endswith("local maxima among the converged sequences: 1")
                                                                            for ln in lines)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert rows == [["1", "-1.25", "2.5", "3", "1", "1"], ["2", "0.125", "%.17g" % (1.0 / 3.0), "40", "0", "0"],
                    ["3", "2.5", "2.5", "0", "1", "1"]]
    opts.update(free_sites=None, fixed_sites="1-8", min_gain=0.5, max_steps=None)
    _potts.run_subcommand(inst, "find_local_maxima", "PLMDCA", TOY_RNA, out, None, _lib.DCA_BIOMOLECULE_RNA, 0, PlmDCAException,
                          ascent=opts)
    assert inst.calls[1] == (None, {"max_steps": None, "min_gain": 0.5, "fixed_sites": list(range(8))})
    _potts.run_subcommand(inst, "find_local_maxima", "PLMDCA", TOY_RNA, out, None, _lib.DCA_BIOMOLECULE_RNA, 0, PlmDCAException,
                          ascent={})
    assert inst.calls[2] == (None, {"max_steps": None, "min_gain": 0.0})
    for bad in ({"free_sites": "1", "fixed_sites": "2"}, {"free_sites": "0"}, {"fixed_sites": "5-4"}):
        with pytest.raises(PlmDCAException):
            _potts.run_subcommand(inst, "find_local_maxima", "MFDCA", TOY_RNA, out, None, _lib.DCA_BIOMOLECULE_RNA, 1, PlmDCAException,
                                  ascent=dict({"free_sites": None, "fixed_sites": None}, **bad))


# ---------------------------------------------------------------- the launch plan
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("ascent_plan")), "ascent_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "ascent_plan_driver.cpp")])

    def run(groups):
        """groups: (q, elem, F, ldsCap, maxSteps, paths, n, envPass) -> one dict per group"""
        argv = [str(v) for g in groups for v in g]
        out = []
        for ln in subprocess.check_output([exe] + argv).decode().splitlines():
            tok = ln.split()
            out.append({k: int(v) for k, v in zip(tok[::2], tok[1::2])})
        return out
    return run


LDS = 160 * 1024


def side_bytes(F):
    return 4 * F + (F + 15) // 16 * 16


def largest_lds_F(q, total, cap):
    F = min(cap, total) // (8 * q)
    while F > 0 and 8 * q * F + side_bytes(F) > total:
        F -= 1
    return F


def test_plan_numbers(plan):
    base = plan([(2, 4, 1, -1, 0, 0, 1, 0)])[0]
    total, budget = base["ldsTotal"], base["budget"]
    assert total < LDS and budget == 1 << 30
    groups, want = [], []
    for q in range(2, 33):
        for elem in (4, 8):
            for cap in (-1, 0, 1000, 84000):
                lim = total if cap < 0 else min(cap, total)
                Fs = largest_lds_F(q, total, lim)
                for F in sorted({1, 25, 500, max(Fs, 1), Fs + 1, 3 * Fs + 7}):
                    groups.append((q, elem, F, cap, 4 * F, 0, 10000, 0))
                    want.append((q, elem, F, F <= Fs))
    got = plan(groups)
    for p, (q, elem, F, inLds) in zip(got, want):
        what = (q, elem, F)
        QM = 8 if q <= 8 else 24 if q <= 24 else 32
        assert (p["q"], p["elem"], p["F"], p["QM"]) == (q, elem, F, QM), what
        assert p["CJ"] >= 1 and p["chunkVals"] == p["CJ"] * q * q <= p["regVals"] == 256 * (16 if elem == 4 else 8), what
        assert p["ldsInit"] >= 2 * p["CJ"] * q * QM * elem and p["ldsInit"] <= 48 * 1024, what
        assert p["tableBytes"] == 8 * q * F and p["sideBytes"] == side_bytes(F), what
        assert p["inLds"] == int(inLds), what                    # the switch falls where the header says
        assert p["ldsAscent"] == (p["tableBytes"] if inLds else 0) + p["sideBytes"], what
        if inLds:
            assert p["ldsAscent"] <= total < LDS, what
        assert p["perChain"] == p["tableBytes"] and p["pass"] == min(10000, max(1, budget // p["perChain"])), what
        assert p["pass"] * p["perChain"] <= budget or p["pass"] == 1, what
    d = plan([(21, 4, 500, -1, 2000, 0, 10000, 0), (21, 4, 500, -1, 2000, 1, 10000, 0), (21, 4, 500, -1, 2000, 0, 10000, 64),
              (21, 4, 500, 0, 2000, 0, 10000, 0), (5, 8, 3, -1, 12, 0, 0, 0), (32, 8, 1 << 20, -1, 5, 1, 7, 0)])
    assert d[0]["tableBytes"] == 84000 and d[0]["inLds"] == 1 and d[0]["pass"] == 10000          # config D's shape sits in LDS
    assert d[1]["perChain"] == 84000 + 2000 * 16 and d[1]["pass"] == (1 << 30) // (84000 + 32000)  # path records join the scratch
    assert d[2]["pass"] == 64 and d[3]["inLds"] == 0 and d[3]["ldsAscent"] == side_bytes(500)
    assert d[4]["pass"] == 1 and d[5]["pass"] == 3 and d[5]["inLds"] == 0          # 256 MiB tables and their records: three at once


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module", params=R.MODELS, ids=R.model_id)
def model(request):
    return R.cpu_model(request.param)


def test_restatement_follows_the_fresh_path(model):
    h, Jp, X = model
    L = h.shape[0]
    for free in R.site_lists(L):
        margin, drift = R.check_margins(h, Jp, X, free, 4 * free.size)
        print("F %d of L %d: margin %.3g, drift %.3g" % (free.size, L, margin, drift))
    margin, drift = R.check_margins(h, Jp, X[:5], np.arange(L), 4 * L, min_gain=1e6)
    assert margin > 1e5


def test_restatement_outputs():
    h, Jp, X = R.cpu_model(("plm", 5, 23, 32))
    L = 23
    free = np.setdiff1d(np.arange(L), [3, 11])
    full = R.ascend(h, Jp, X[:9], free, 4 * free.size)
    assert full["converged"].all() and (full["steps"] > 0).all()
    assert np.array_equal(full["codes"][:, [3, 11]], X[:9, [3, 11]])
    k = int(np.argmax(full["steps"]))
    T = int(full["steps"][k])
    for cap, conv in ((T, True), (T - 1, False), (1, T == 1), (0, False)):
        cut = R.ascend(h, Jp, X[k], free, cap)
        assert cut["steps"][0] == cap and bool(cut["converged"][0]) == conv
        assert np.array_equal(cut["path"][0], full["path"][k, :cap]) and np.array_equal(cut["path_gains"][0], full["path_gains"][k, :cap])
    assert np.array_equal(R.ascend(h, Jp, X[k], free, 0)["codes"][0], X[k])
    again = R.ascend(h, Jp, full["codes"], free, 4 * free.size)              # a start that is a previous output
    assert not again["steps"].any() and again["converged"].all() and np.array_equal(again["codes"], full["codes"])
    for r in range(9):                                                        # gains: the sequential sum; path past steps -1 / 0
        t = int(full["steps"][r])
        acc = 0.0
        for g in full["path_gains"][r, :t]:
            acc += g
        assert acc == full["gains"][r] and (full["path"][r, t:] == -1).all() and not full["path_gains"][r, t:].any()
        s = X[r].copy()                                                       # the path rebuilds the output
        for i, a in full["path"][r, :t]:
            assert i in free and s[i] != a
            s[i] = a
        assert np.array_equal(s, full["codes"][r])
    none = R.ascend(h, Jp, X[:3], [], 0)
    assert np.array_equal(none["codes"], X[:3]) and none["converged"].all() and not none["steps"].any()


def tie_model(L, q):
    """states 1 and 2 carry the same parameters everywhere: exact ties between them"""
    h, Jp = R.plm_model(R.plm_x(q, L, 32), L, q)
    h, Jp = h.copy(), Jp.copy()
    h[:, 2] = h[:, 1]
    Jp[:, 2, :] = Jp[:, 1, :]
    Jp[:, :, 2] = Jp[:, :, 1]
    return h, Jp


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_change_the_path(fault):
    L, q = 23, 5
    h, Jp, X = R.cpu_model(("plm", q, L, 32))
    X = X[:12]
    free = np.arange(L)
    min_gain = 0.0
    if fault == "tie_reversed":
        h, Jp = tie_model(L, q)
    if fault == "clamped_moves":
        free = np.arange(0, L, 2)
    good = R.ascend(h, Jp, X, free, 4 * free.size, min_gain)
    if fault == "ge_min_gain":                  # a start that is already a maximum under min_gain = its own best gain
        assert good["steps"][0] > 0
        min_gain = float(good["path_gains"][0, 0])
        X = X[:1]
        good = R.ascend(h, Jp, X, free, 4 * free.size, min_gain)
        assert good["steps"][0] == 0 and good["converged"][0]
    bad = R.ascend(h, Jp, X, free, 4 * free.size, min_gain, fault=fault)
    assert not np.array_equal(good["path"], bad["path"]), fault
