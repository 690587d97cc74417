"""Host side of the log-partition-function estimate: the C ABI (argument struct, exports), dca_ais_estimate against a
restatement of its documented order, the schedule / base-field / option checks in Python, the compute_log_likelihood
sub-command's options and the file it writes (through a stand-in model).  No GPU needed."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts, mfdca_main, plmdca_main  # noqa: E402
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCAException  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException  # noqa: E402

TOY_RNA = os.path.join(ROOT, "tests", "golden", "data", "toy_rna.fa")
ENTRIES = ("dca_plm_ais", "dca_mf_ais", "dca_ais_estimate")


def estimate_ref(logw, log_z0):
    """dca_ais_estimate's order, restated: scalar double operations with the C library's exp / log (math)"""
    n = len(logw)
    m = max(float(v) for v in logw)
    s1 = 0.0
    for v in logw:
        s1 += math.exp(float(v) - m)
    s2 = 0.0
    for v in logw:
        s2 += math.exp(2.0 * (float(v) - m))
    log_z = ((log_z0 + m) + math.log(s1)) - math.log(float(n))
    return log_z, s1 * s1 / s2, math.sqrt(max(0.0, s2 / (s1 * s1) - 1.0 / n))


def test_entries_and_argument_struct():
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    assert "typedef struct dca_ais_args" in header and all(name + "(" in header for name in ENTRIES)
    A = _lib.AisArgs
    assert [getattr(A, f).offset for f in ("chains", "temperatures", "betas", "sweeps_per_temperature", "seed", "first_chain",
                                            "base_fields")] == [0, 4, 8, 16, 24, 32, 40]
    assert C.sizeof(A) == 48


def test_entries_refuse_without_a_context():
    lib = _lib.lib()
    w = np.zeros(4)
    z0 = C.c_double(0)
    args = _lib.AisArgs(4, 2, None, 1, 0, 0, None)
    assert lib.dca_plm_ais(None, C.byref(args), w.ctypes.data, C.byref(z0), None) == _lib.DCA_ERR_ARG
    assert lib.dca_mf_ais(None, C.byref(args), w.ctypes.data, C.byref(z0), None) == _lib.DCA_ERR_ARG


@pytest.mark.parametrize("case", ["one", "equal", "spread", "random"])
def test_estimate_matches_restatement(case):
    rng = np.random.default_rng(7)
    logw = {"one": np.array([-3.25]), "equal": np.full(37, 2.5), "spread": np.linspace(-700.0, 0.0, 513),
            "random": rng.normal(0, 3, 1000)}[case]
    log_z0 = -17.125 if case != "random" else 123.456
    got = _lib.ais_estimate(logw, log_z0)
    ref = estimate_ref(logw, log_z0)
    assert got == ref, (got, ref)
    if case == "one":
        assert got == (log_z0 + logw[0], 1.0, 0.0)
    if case == "equal":
        assert got[1] == len(logw) and got[2] == 0.0 and got[0] == log_z0 + 2.5 + math.log(1.0 * len(logw)) - math.log(len(logw))
    if case == "spread":
        assert math.isfinite(got[0]) and 1.0 <= got[1] < 2.0


def test_estimate_argument_errors():
    lib = _lib.lib()
    out = C.c_double(0)
    w = np.array([0.0, 1.0])
    assert lib.dca_ais_estimate(None, 2, 0.0, C.byref(out), None, None) == _lib.DCA_ERR_ARG
    assert lib.dca_ais_estimate(w.ctypes.data, 0, 0.0, C.byref(out), None, None) == _lib.DCA_ERR_ARG
    assert lib.dca_ais_estimate(w.ctypes.data, 2, float("nan"), C.byref(out), None, None) == _lib.DCA_ERR_ARG
    bad = np.array([0.0, float("inf")])
    assert lib.dca_ais_estimate(bad.ctypes.data, 2, 0.0, C.byref(out), None, None) == _lib.DCA_ERR_ARG
    assert lib.dca_ais_estimate(w.ctypes.data, 2, 0.0, None, None, None) == _lib.DCA_OK
    with pytest.raises(_lib.DcaBackendError):
        _lib.ais_estimate([], 0.0)


def test_schedule_checks():
    assert _lib.ais_schedule(3) is None
    assert np.array_equal(_lib.ais_schedule(2, [0.0, 0.25, 1.0]), [0.0, 0.25, 1.0])
    for K, b in ((0, None), (2, [0.0, 1.0]), (2, [0.1, 0.5, 1.0]), (2, [0.0, 0.5, 0.99]), (2, [0.0, 0.5, 0.5, 1.0]),
                 (2, [0.0, 0.6, 0.5]), (2, [0.0, float("nan"), 1.0]), (1, [0.0, float("inf")]), (2, [0.0, 0.0, 1.0])):
        with pytest.raises(ValueError):
            _lib.ais_schedule(K, b)


def test_base_field_checks():
    assert _lib.ais_base_fields(None, 3, 5) is None
    h = _lib.ais_base_fields(np.arange(15.0), 3, 5)
    assert h.shape == (3, 5) and h.dtype == np.float64
    for bad in (np.zeros((3, 4)), np.full((3, 5), np.nan), np.full((3, 5), -np.inf)):
        with pytest.raises(ValueError):
            _lib.ais_base_fields(bad, 3, 5)
    with pytest.raises(PlmDCAException):
        _potts.ais_base("uniform", None, None, 3, 5, None, PlmDCAException)
    with pytest.raises(MeanFieldDCAException):
        _potts.ais_base(np.zeros((2, 5)), None, None, 3, 5, None, MeanFieldDCAException)
    assert _potts.ais_base("fields", None, None, 3, 5, None, PlmDCAException) is None


def test_profile_fields():
    X = np.array([[0, 1], [0, 2], [1, 2]], dtype=np.uint8)
    w = np.array([1.0, 0.5, 0.5])
    h = _potts.profile_fields(X, w, 3, pseudocount=0.3)
    f = np.array([[1.5, 0.5, 0.0], [0.0, 1.0, 1.0]]) / 2.0
    assert np.allclose(h, np.log(0.7 * f + 0.1), rtol=1e-15, atol=0)
    h_default = _potts.profile_fields(X, w, 3)
    assert np.allclose(h_default, np.log(0.5 * f + 0.5 / 3), rtol=1e-15, atol=0)     # lambda = 1 / Meff = 1 / 2
    assert np.all(np.isfinite(_potts.ais_base("profile", X, w, 2, 3, None, PlmDCAException)))


@pytest.mark.parametrize("kw", [dict(num_chains=0), dict(num_chains=2.5), dict(num_chains=True), dict(num_temperatures=0),
                                dict(sweeps_per_temperature=-1), dict(seed=-1), dict(pseudocount=0.0), dict(pseudocount=1.5),
                                dict(num_chains=(1 << 24) + 1)])
def test_option_checks(kw):
    args = dict(num_chains=10, num_temperatures=5, sweeps_per_temperature=1, seed=0, pseudocount=None)
    args.update(kw)
    with pytest.raises(PlmDCAException):
        _potts.ais_options(exc_type=PlmDCAException, **args)


def test_class_methods_refuse_several_devices():
    inst = PlmDCA(TOY_RNA, "rna", devices=[0, 1])
    for call in (inst.compute_log_partition_function, inst.compute_log_likelihood, inst.compute_sequence_log_probabilities):
        with pytest.raises(PlmDCAException, match="one GPU"):
            call()


@pytest.mark.parametrize("main", ["plm", "mf"])
def test_subcommand_options(monkeypatch, main):
    mod, run = (plmdca_main, plmdca_main.run_plm_dca) if main == "plm" else (mfdca_main, mfdca_main.run_meanfield_dca)
    seen = {}
    monkeypatch.setattr(mod, "execute_from_command_line", lambda *a, **kw: seen.update(kw, args=a) or "done")
    run(["compute_log_likelihood", "rna", TOY_RNA, "--num_chains", "64", "--num_temperatures", "30", "--sweeps_per_temperature", "2",
         "--seed", "9", "--base", "fields", "--base_pseudocount", "0.25"])
    assert seen["the_command"] == "compute_log_likelihood"
    assert seen["ais"] == dict(num_chains=64, num_temperatures=30, sweeps_per_temperature=2, seed=9, base="fields",
                               base_pseudocount=0.25)
    run(["compute_log_likelihood", "rna", TOY_RNA])
    assert seen["ais"] == dict(num_chains=1000, num_temperatures=1000, sweeps_per_temperature=1, seed=0, base="profile",
                               base_pseudocount=None)
    with pytest.raises(SystemExit):
        run(["compute_log_likelihood", "rna", TOY_RNA, "--base", "uniform"])


class StandIn:
    """The three calls run_log_likelihood makes, recorded"""
    def __init__(self):
        self.calls = []

    def compute_log_partition_function(self, **kw):
        self.calls.append(("log_z", kw))
        return {"log_z": 10.0 / 3.0, "log_z_stderr": 0.125, "ess": 17.5, "log_z_base": -2.0, "log_weights": np.zeros(4)}

    def compute_log_likelihood(self, log_z=None):
        self.calls.append(("ll", log_z))
        return -1.0 / 7.0

    def compute_sequence_log_probabilities(self, sequences=None, log_z=None):
        self.calls.append(("logp", sequences, log_z))
        return np.array([-1.5, -2.0 / 3.0])


def test_subcommand_file(tmp_path):
    inst = StandIn()
    out = str(tmp_path / "out")
    opts = dict(num_chains=64, num_temperatures=30, sweeps_per_temperature=2, seed=9, base="fields", base_pseudocount=None)
    path = _potts.run_subcommand(inst, "compute_log_likelihood", "MFDCA", TOY_RNA, out, ["# meta"], _lib.DCA_BIOMOLECULE_RNA, 1,
                                 MeanFieldDCAException, ais=opts)
    assert os.path.basename(path) == "MFDCA_log_likelihood_toy_rna.txt"
    assert inst.calls == [("log_z", dict(num_chains=64, num_temperatures=30, sweeps_per_temperature=2, seed=9, base="fields",
                                         pseudocount=None)),
                          ("ll", 10.0 / 3.0), ("logp", None, 10.0 / 3.0)]
    lines = open(path).read().splitlines()
    assert "# meta" in lines
    head = "\n".join(ln for ln in lines if ln.startswith("#"))
    for text in ("%.17g" % (10.0 / 3.0), "0.125", "17.5", "-2", "K = 30", "64 chains", "2 sweeps", "seed 9", "base fields"):
        assert text in head, text
    rows = [ln for ln in lines if not ln.startswith("#")]
    assert rows == ["average_log_likelihood %.17g" % (-1.0 / 7.0), "-1.5", "%.17g" % (-2.0 / 3.0)]
    assert float(rows[2]) == -2.0 / 3.0
