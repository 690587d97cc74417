"""Host side of the principal-component entries (dca_pca_fit, dca_pca_project).  The small dense pieces of
the fit (pydca_amd/csrc/pca_host.h) are compiled behind tests/pca_host_driver.cpp with a plain host compiler and held against
numpy.linalg.eigh: the cyclic Jacobi solver, the order of the eigenpairs, the sign rule, the null rule and the drop threshold of
the orthonormalisation.  Then the declarations, the Python argument checks and the command-line flags.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, data_file
import pca_reference
from pydca_amd import _compare, _lib, _potts, ardca_main, mfdca_main, plmdca_main
from pydca_amd.ardca.ardca import ArDCA, ArDCAException
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException

TOY_RNA = data_file("toy_rna.fa")
_DP = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_DP)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pca") / "libpca_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-shared", "-fPIC", "-Wall",
                           "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "pca_host_driver.cpp")])
    lib = C.CDLL(so)
    lib.pca_driver_eigh.argtypes = [C.c_int, _DP, _DP, _DP]
    lib.pca_driver_fix_sign.argtypes = [C.c_long, _DP]
    lib.pca_driver_fix_sign.restype = C.c_long
    lib.pca_driver_is_null.argtypes = [C.c_double, C.c_double, C.c_double]
    lib.pca_driver_orth_transform.argtypes = [C.c_int, _DP, _DP]
    return lib


def jacobi(host, H):
    n = H.shape[0]
    H = np.ascontiguousarray(H, dtype=np.float64)
    U, lam = np.zeros((n, n)), np.zeros(n)
    sweeps = host.pca_driver_eigh(n, _p(H), _p(U), _p(lam))
    return lam, U, sweeps


def symmetric_cases():
    rng = np.random.default_rng(20)
    cases = []
    for b in (1, 2, 9, 72):
        A = rng.standard_normal((b, b))
        cases.append(("random b=%d" % b, 0.5 * (A + A.T)))
    Q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    cases.append(("repeated eigenvalue", (Q * np.array([3.0, 3.0, 3.0, 1.0, 1.0, 0.5, 0.25, -2.0, -2.0])) @ Q.T))
    B = rng.standard_normal((9, 4))
    cases.append(("singular", B @ B.T))
    cases.append(("zero", np.zeros((5, 5))))
    return cases


@pytest.mark.parametrize("what, H", symmetric_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_jacobi_against_lapack(host, what, H):
    b = H.shape[0]
    assert b <= host.pca_driver_max_block()
    lam, U, sweeps = jacobi(host, H)
    ref = np.linalg.eigvalsh(0.5 * (H + H.T))[::-1]
    bound = 64 * b * 2.0 ** -53 * np.linalg.norm(H)
    err, orth = np.abs(lam - ref).max(), np.abs(U.T @ U - np.eye(b)).max()
    back = np.abs((U * lam) @ U.T - 0.5 * (H + H.T)).max()
    print(what, "sweeps", sweeps, "eigenvalue error", err, "bound", bound, "|U^T U - I|", orth, "|U L U^T - H|", back)
    assert np.all(np.diff(lam) <= 0)                              # descending
    assert err <= bound
    assert orth <= 64 * b * 2.0 ** -53
    assert back <= bound + 64 * b * 2.0 ** -53 * np.abs(ref).max()
    lam2, U2, _ = jacobi(host, H)
    assert np.array_equal(lam, lam2) and np.array_equal(U, U2)    # a fixed sweep order: the same bits again


def test_sort_is_stable_on_equal_values(host):
    lam, U, _ = jacobi(host, np.diag([1.0, 2.0, 1.0, 2.0]))
    assert lam.tolist() == [2.0, 2.0, 1.0, 1.0]
    assert np.array_equal(U, np.eye(4)[:, [1, 3, 0, 2]])          # equal values keep the order of their columns


def test_sign_rule(host):
    for v, at, flipped in (([0.5, -2.0, 1.0], 1, True), ([0.5, 2.0, -1.0], 1, False), ([-3.0, 3.0, 1.0], 0, True),
                           ([3.0, -3.0, 1.0], 0, False), ([0.0, 0.0], 0, False), ([-1.0], 0, True)):
        a = np.array(v)
        got = host.pca_driver_fix_sign(a.size, _p(a))
        assert got == at and np.array_equal(a, -np.array(v) if flipped else np.array(v))
        assert np.array_equal(pca_reference.sign_rule(v), a)      # the reference states the same rule


def test_null_rule(host):
    assert host.pca_driver_is_null(1e-11, 1.0, 1e-10) == 1 and host.pca_driver_is_null(1e-10, 1.0, 1e-10) == 1
    assert host.pca_driver_is_null(1.1e-10, 1.0, 1e-10) == 0 and host.pca_driver_is_null(1.0, 1.0, 1e-10) == 0
    assert host.pca_driver_is_null(0.0, 0.0, 1e-10) == 1 and host.pca_driver_is_null(-1e-18, 1.0, 1e-10) == 1
    assert host.pca_driver_is_null(float("nan"), 1.0, 1e-10) == 1


@pytest.mark.parametrize("b", [4, 12, 72])
def test_orthonormalisation_drops_dependent_directions(host, b):
    rng = np.random.default_rng(b)
    rows = 3 * b
    Z = rng.standard_normal((rows, b)) * np.logspace(0, -3, b)[None, :]           # columns of very different lengths
    Z[:, b - 3:] = Z[:, :b - 3] @ rng.standard_normal((b - 3, 3))                 # rank b - 3
    G = np.ascontiguousarray(Z.T @ Z)
    T = np.zeros((b, b))
    kept = host.pca_driver_orth_transform(b, _p(G), _p(T))
    assert kept == b - 3
    assert np.array_equal(T[:, b - 3:], np.zeros((b, 3)))                          # the dropped directions: zero columns
    V = Z @ T
    err = np.abs(V[:, :kept].T @ V[:, :kept] - np.eye(kept)).max()
    print("b", b, "kept", kept, "|V^T V - I| after one pass", err)
    assert err <= 1e-6                                                             # one pass; the fit applies two
    G2 = np.ascontiguousarray(V.T @ V)
    T2 = np.zeros((b, b))
    assert host.pca_driver_orth_transform(b, _p(G2), _p(T2)) == kept               # zero columns stay dropped
    V2 = V @ T2
    nz = np.abs(V2).sum(axis=0) > 0
    assert nz.sum() == kept
    assert np.abs(V2[:, nz].T @ V2[:, nz] - np.eye(kept)).max() <= 64 * b * 2.0 ** -53
    # a full-rank block keeps everything, an all-zero block nothing
    F = rng.standard_normal((rows, b))
    Gf = np.ascontiguousarray(F.T @ F)
    assert host.pca_driver_orth_transform(b, _p(Gf), _p(T)) == b
    Gz = np.zeros((b, b))
    assert host.pca_driver_orth_transform(b, _p(Gz), _p(T)) == 0 and not T.any()


# ---------------------------------------------------------------- the C ABI as far as the host reaches
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = " ".join(open(os.path.join(ROOT, "include", "dca_hip.h")).read().split())
    for name in ("dca_pca_fit", "dca_pca_project"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "#define DCA_PCA_SLAB %d" % _lib.PCA_SLAB in header
    for tag in ('"pca_project"', '"pca_back"', '"pca_small"'):
        assert tag in header
    lam, v = np.zeros(1), np.zeros(8)
    conv = C.c_int(0)
    assert lib.dca_pca_fit(None, 1, 1e-10, 10, 0, lam.ctypes.data, v.ctypes.data, lam.ctypes.data, None, None, None,
                           C.byref(conv)) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()
    assert lib.dca_pca_project(None, None, 0, 1, v.ctypes.data, lam.ctypes.data, v.ctypes.data) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()


def test_argument_rules():
    assert _lib.pca_arguments(2, 1e-10, 1000, 0, 10, 5) == (2, 1e-10, 1000, 0)
    assert _lib.pca_arguments(np.int64(50), 1, 1, 2 ** 64 - 1, 10, 5) == (50, 1.0, 1, 2 ** 64 - 1)
    assert _lib.pca_arguments(64, 1e-3, 5, 7, 40, 21)[0] == 64
    for bad in (dict(num_components=0), dict(num_components=65, L=40, q=21), dict(num_components=6, L=1, q=5),
                dict(num_components=2.0), dict(num_components=True), dict(tolerance=0.0), dict(tolerance=-1e-3),
                dict(tolerance=float("nan")), dict(tolerance="1e-3"), dict(max_iterations=0), dict(max_iterations=1.5),
                dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5)):
        kw = dict(num_components=2, tolerance=1e-10, max_iterations=1000, seed=0, L=10, q=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib.pca_arguments(**kw)


@pytest.mark.parametrize("cls, exc", [(PlmDCA, PlmDCAException), (ArDCA, ArDCAException)])     # MeanFieldDCA opens its device when made
def test_class_argument_checks(cls, exc):
    inst = cls(TOY_RNA, "rna")
    for method in (inst.compute_principal_components, lambda **kw: inst.project_sequences(None, **kw)):
        for bad in (0, -1, 65, 51):                              # L q = 50 for the toy RNA alignment
            with pytest.raises(exc, match="num_components must be between 1 and"):
                method(num_components=bad)
        for bad in (2.0, "2", None, True):
            with pytest.raises(exc, match="num_components must be an integer"):
                method(num_components=bad)
        for bad in (0.0, -1.0, float("inf")):
            with pytest.raises(exc, match="tolerance must be a finite number > 0"):
                method(tolerance=bad)
        with pytest.raises(exc, match="max_iterations must be >= 1"):
            method(max_iterations=0)
        with pytest.raises(exc, match="seed must be in"):
            method(seed=-1)
    with pytest.raises(exc, match="pca must be >= 0"):
        inst.compare_with_alignment(["ACGUACGUAC"], pca=-1)
    with pytest.raises(exc, match="pca must be an integer"):
        inst.compare_with_alignment(["ACGUACGUAC"], pca=2.0)


def test_methods_and_options_on_every_class_and_command_line(monkeypatch, capsys):
    for cls in (PlmDCA, MeanFieldDCA, ArDCA):
        assert issubclass(cls, _compare.SequenceComparison)
        for name in ("compute_principal_components", "project_sequences", "compare_with_alignment"):
            assert getattr(cls, name) is getattr(_compare.SequenceComparison, name)
    assert "compute_pca" in _potts.POTTS_SUBCOMMANDS and "compute_pca" in ardca_main.ARDCA_SUBCOMMANDS
    for mod, run in ((plmdca_main, plmdca_main.run_plm_dca), (mfdca_main, mfdca_main.run_meanfield_dca), (ardca_main, ardca_main.run_ardca)):
        with pytest.raises(SystemExit):
            run(["compute_pca", "--help"])
        text = capsys.readouterr().out
        for flag in ("--num_components", "--query_file", "--seed"):
            assert flag in text
        seen = {}
        monkeypatch.setattr(mod, "execute_from_command_line", lambda *a, **kw: seen.update(kw, args=a) or "done")
        run(["compute_pca", "rna", TOY_RNA, "--num_components", "5", "--query_file", "s.fa", "--seed", "3"])
        assert seen["the_command"] == "compute_pca" and seen["query_file"] == "s.fa"
        opts = seen["pca"] if isinstance(seen.get("pca"), dict) else seen
        assert opts["num_components"] == 5 and opts["seed"] == 3
        run(["compare_sequences", "rna", TOY_RNA, "--query_file", "s.fa", "--pca", "4"])
        assert (seen["pca"]["pca"] if isinstance(seen["pca"], dict) else seen["pca"]) == 4
        run(["compare_sequences", "rna", TOY_RNA, "--query_file", "s.fa"])
        assert not (seen["pca"]["pca"] if isinstance(seen["pca"], dict) else seen["pca"])


class StandIn:
    sequences_len = 4

    def __init__(self):
        self.kw = None

    def compare_with_alignment(self, sequences, **kw):
        self.kw = kw
        out = {"pearson_cij": 0.5, "num_sequences": 2}
        if kw.get("pca"):
            out.update(pca_eigenvalues=np.array([0.5, 0.25]), pca_set_mean=np.array([0.125, -0.5]), pca_set_variance=np.array([1.0, 2.0]))
        return out

    def compute_distances_to_alignment(self, sequences, return_index=False, return_histogram=False):
        return np.array([1, 4], dtype=np.int32), np.array([7, 0], dtype=np.int32), np.array([0, 1, 0, 0, 1], dtype=np.uint64)

    def compute_alignment_self_distances(self, return_index=False, return_histogram=False):
        return np.array([2], dtype=np.int32), np.array([0, 0, 6, 0, 0], dtype=np.uint64)


def test_compare_sequences_passes_pca_only_when_asked(tmp_path):
    inst = StandIn()
    plain = _compare.run_compare(inst, "PLMDCA", TOY_RNA, str(tmp_path / "a"), ["# meta"], "q.fa", PlmDCAException)
    assert inst.kw == {}                                              # the call of today, so the file of today
    with_pca = _compare.run_compare(inst, "PLMDCA", TOY_RNA, str(tmp_path / "b"), ["# meta"], "q.fa", PlmDCAException, pca=2)
    assert inst.kw == {"pca": 2}
    a, b = open(plain).read().splitlines(), open(with_pca).read().splitlines()
    assert sorted(set(b) - set(a)) == ["#\tpca_eigenvalues_1: 0.5", "#\tpca_eigenvalues_2: 0.25", "#\tpca_set_mean_1: 0.125",
                                       "#\tpca_set_mean_2: -0.5", "#\tpca_set_variance_1: 1", "#\tpca_set_variance_2: 2"]
    assert [ln for ln in b if ln in a] == a


# ---------------------------------------------------------------- the reference itself
def test_reference_definitions():
    rng = np.random.default_rng(3)
    X = pca_reference.planted_alignment(5, 6, 40, 2, 1)
    assert X.shape == (40, 6) and X.dtype == np.uint8 and X.max() < 5
    w = rng.uniform(0.1, 1.0, 40)
    lam, V, Cm, f = pca_reference.eigh(X, w, 5)
    fi = f.reshape(6, 5)
    assert np.allclose(fi.sum(axis=1), 1.0, atol=1e-14)
    assert abs(np.trace(Cm) - (1.0 - (fi ** 2).sum(axis=1)).sum()) <= 1e-13     # total_variance is the trace
    # a diagonal block is diag(f_i) - f_i f_i^T, an off-diagonal block f_ij - f_i f_j^T
    assert np.allclose(Cm[:5, :5], np.diag(fi[0]) - np.outer(fi[0], fi[0]), atol=1e-14)
    H = pca_reference.one_hot(X, 5)
    f01 = (H[:, :5] * w[:, None]).T @ H[:, 5:10] / w.sum()
    assert np.allclose(Cm[:5, 5:10], f01 - np.outer(fi[0], fi[1]), atol=1e-14)
    assert np.all(np.diff(lam) <= 1e-15) and np.allclose(V @ V.T, np.eye(30), atol=1e-13)
    # projections: weighted mean 0, weighted covariance diag(lambda)
    c = V[:3] @ f
    P = pca_reference.project(X, V[:3].reshape(3, 6, 5), c)
    assert np.allclose((w[:, None] * P).sum(axis=0) / w.sum(), 0.0, atol=1e-14)
    assert np.allclose((P * w[:, None]).T @ P / w.sum(), np.diag(lam[:3]), atol=1e-13)
    assert np.array_equal(pca_reference.gaps([5.0, 3.0, 2.5, 0.0]), np.array([2.0, 0.5, 0.5, 2.5]))
