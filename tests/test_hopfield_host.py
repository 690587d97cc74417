"""Host side of the Hopfield-Potts entries (dca_mf_hopfield_fit, dca_hopfield_project, dca_dense_apply): the
identities of the numpy reference, the selection rule on hand-made spectra, the plan header (pydca_amd/csrc/hopfield_plan.h)
against its driver, the conditions the inputs of the GPU cases must satisfy, and the declarations, argument rules and
command-line flags.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, data_file
import hopfield_cases as hc
import hopfield_reference as href
from pydca_amd import _compare, _lib, _potts, hopfield_main
from pydca_amd.hopfield_dca.hopfield_dca import HopfieldPottsDCA
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA

TOY_RNA = data_file("toy_rna.fa")


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("shape", ["n8", "n32", "n60"])
def test_reference_identities(shape):
    ref = hc.reference(shape, "random")
    C_, lam, U, G, L, q, n = (ref[k] for k in ("C", "lam", "U", "G", "L", "q", "n"))
    qm = q - 1
    D = href.block_diag(href.blocks(C_, L, qm))
    assert abs(np.trace(G) - n) <= 64 * n * hc.U and abs(lam.mean() - 1.0) <= 64 * n * hc.U     # trace Gamma = n: the mean is 1
    assert lam.min() > 0 and np.all(np.diff(lam) <= 0)
    for i in range(L):                                             # identity diagonal blocks
        assert np.abs(G[i * qm:(i + 1) * qm, i * qm:(i + 1) * qm] - np.eye(qm)).max() <= 64 * qm * hc.U
    assert np.abs(U.T @ D @ U - np.eye(n)).max() <= 1e-12          # u^T D u = 1
    assert np.abs(C_ @ U - (D @ U) * lam).max() <= 1e-12           # C u = lambda D u
    for m in range(n):                                             # the sign rule
        assert U[np.argmax(np.abs(U[:, m])), m] > 0
    # the whole spectrum gives D^-1 - C^-1: off the diagonal blocks the mfDCA couplings
    J = href.couplings(lam, U, list(range(n)))
    full = np.linalg.inv(D) - np.linalg.inv(C_)
    scale = np.abs(np.linalg.inv(C_)).max()
    assert np.abs(J - full).max() <= 1e-11 * scale
    mask = href.off_diagonal_mask(L, qm)
    assert np.abs(J - (-np.linalg.inv(C_)))[mask].max() <= 1e-11 * scale
    # patterns: J = sum s xi xi^T
    idx = href.selected(n, 2, 3)
    xi, s = href.patterns(lam, U, idx)
    assert np.abs((xi.T * s) @ xi - href.couplings(lam, U, idx)).max() <= 1e-13 * scale
    assert s.tolist() == [1 if lam[m] > 1 else -1 for m in idx]
    # the two formulations agree to rounding, and not exactly
    eps = href.epsilon(C_, L, qm)
    assert 0 < eps["eigenvalues"] <= 1e-12 and eps["couplings"] <= 1e-10 * scale


def test_selection_rule_on_hand_made_spectra():
    g = href.gain
    assert g(1.0) == 0.0 and g(2.0) > 0 and g(0.5) > 0
    # gains 2.0: 0.153, 3.0: 0.451, 0.5: 0.0966, 0.25: 0.318, 0.1: 0.701
    lam = [3.0, 2.0, 1.2, 0.9, 0.5, 0.25, 0.1]
    assert [href.select_likelihood(lam, p) for p in range(1, 8)] == [(0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (4, 3)]     # the last one left is 0.9 from either end: a tie
    # only attractive, only repulsive
    assert href.select_likelihood([5.0, 4.0, 3.0, 0.99], 3) == (3, 0)
    assert href.select_likelihood([1.01, 0.3, 0.2, 0.1], 3) == (0, 3)
    # an exact tie goes to the attractive side: two eigenvalues 1 (gain 0 on either side) ...
    assert href.select_likelihood([3.0, 1.0, 1.0, 0.5], 3) == (2, 1)
    # ... and an eigenvalue below 1 whose gain is bit for bit that of 2.0, where a bisection finds one
    lo, hi = 0.1, 0.9
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g(mid) > g(2.0) else (lo, mid)
    tie = next((x for x in (lo, hi, np.nextafter(lo, 0), np.nextafter(hi, 1)) if g(x) == g(2.0)), None)
    if tie is not None:
        assert href.select_likelihood([2.0, 1.5, 0.95, tie], 1) == (1, 0)
    below = np.nextafter(lo, 0)
    while g(below) <= g(2.0):
        below = np.nextafter(below, 0)
    assert href.select_likelihood([2.0, 1.5, 0.95, below], 1) == (0, 1)          # one step more gain: the repulsive side
    assert href.selected(7, 2, 3) == [0, 1, 6, 5, 4]


# ---------------------------------------------------------------- the plan header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("hopfield_plan")), "hopfield_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-fno-fast-math", "-ffp-contract=off", "-I", os.path.join(ROOT, "pydca_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "hopfield_plan_driver.cpp")])

    def run(*args):
        return subprocess.check_output([exe] + [repr(float(a)) if isinstance(a, float) else str(a) for a in args]).decode().splitlines()
    return run


def test_plan_header_against_its_driver(driver):
    groups = [(n, b, k) for n in (1, 8, 63, 64, 65, 132, 260, 1024, 1025, 1100, 10000) for b, k in ((1, 1), (9, 1), (16, 8), (17, 9), (72, 64))]
    lines = driver("plan", *[v for g in groups for v in g])
    assert len(lines) == len(groups)
    for (n, b, k), ln in zip(groups, lines):
        tok = ln.split()
        d = {key: int(v) for key, v in zip(tok[::2], tok[1::2])}
        assert (d["maxPerEnd"], d["maxBlock"], d["rows"], d["slab"], d["waves"], d["asmTile"]) == (64, 72, 64, 1024, 4, 64)
        assert d["maxPerEnd"] == _lib.HOPFIELD_MAX_PER_END and d["maxBlock"] == d["maxPerEnd"] + 8
        slabs = -(-n // 1024)
        assert (d["n"], d["b"], d["colTiles"], d["rowGroups"], d["slabs"]) == (n, b, -(-b // 16), -(-n // 64), slabs)
        assert d["partDoubles"] == (slabs * n * b if slabs > 1 else 0)
        assert d["block"] == min(n, k + 8)
        assert 1 <= d["colTiles"] <= 5                              # the kernel's instantiations
    assert driver("plan", 5, 3, 0)[0].split()[15] == "0"            # no pattern of an end: no block


def test_gain_and_selection_of_the_header_against_the_reference(driver):
    lam = [0.05, 0.3, 0.5, 0.999, 1.0, 1.001, 2.0, 17.5]
    got = np.array([float(v) for v in driver("gain", *lam)])
    ref = href.gain(lam)
    assert np.abs(got - ref).max() <= 4 * hc.U * np.abs(ref).max() and got[4] == 0.0
    rng = np.random.default_rng(9)
    for trial in range(40):
        n = int(rng.integers(4, 40))
        spec = np.sort(np.exp(rng.normal(0, 0.8, n)))[::-1]
        if trial % 5 == 0:
            spec[n // 2] = spec[n // 2 - 1] = 1.0                   # a tie at gain 0
        p = int(rng.integers(1, n + 1))
        k = min(p, n)
        rc, a, r = (int(v) for v in driver("select", p, k, k, *[float(v) for v in spec[:k]], *[float(v) for v in spec[::-1][:k]])[0].split())
        assert rc == 0 and (a, r) == href.select_likelihood(spec, p), (trial, spec, p)
    # an end that runs out before p patterns are taken is reported, not guessed
    assert driver("select", 5, 2, 5, 9.0, 8.0, 0.9, 0.91, 0.92, 0.93, 0.94)[0].split()[0] == "-1"


# ---------------------------------------------------------------- the inputs of the GPU cases
@pytest.mark.parametrize("shape, weights", hc.CASES)
def test_inputs_of_the_gpu_cases_satisfy_their_conditions(shape, weights):
    ref = hc.reference(shape, weights)
    lam, n = ref["lam"], ref["n"]
    a, r = hc.split(shape, weights)
    assert a <= 64 and r <= 64 and 1 <= a + r <= n
    idx = href.selected(n, a, r)
    # the vector check: at least one selected pattern stands clear of the rest of the spectrum, at both ends where both are asked
    compared = hc.compared_patterns(ref, idx)
    print(shape, weights, "n", n, "split", (a, r), "compared", len(compared), "of", len(idx), "lambda", lam[0], lam[-1], "eps", ref["eps"])
    assert compared and any(k < a for k in compared) == (a > 0)
    # n = 132 and 260: the smallest eigenvalues lie closer together than 1 % of the range whatever the seed or the number of
    # sequences (they cluster under the pseudocount); there the repulsive patterns are held by the eigenvalue, residual,
    # orthonormality and coupling checks only
    if shape not in ("n132", "n260"):
        assert any(k >= a for k in compared) == (r > 0)
    # the selection check: the last gain taken and the first one left differ by more than twice what the eigenvalue bound moves them
    if hc.SELECTION[shape][0] == "likelihood":
        g = href.gain(lam)
        taken = np.zeros(n, dtype=bool)
        taken[idx] = True
        last, first_left = g[taken].min(), g[~taken].max()
        move = max(0.5 * abs(1.0 - 1.0 / lam[m]) * (hc.residual_bound(ref, lam[m]) + ref["eps"]) for m in (int(np.argmin(np.where(taken, g, np.inf))), int(np.argmax(np.where(taken, -np.inf, g)))))
        assert last - first_left > 2.0 * move
        assert a > 0 and r > 0                                      # both ends take part
    # the couplings bound is finite: the selected and the unselected eigenvalues are apart
    if a + r < n:
        sel = np.zeros(n, dtype=bool)
        sel[idx] = True
        assert np.abs(lam[sel][:, None] - lam[~sel][None, :]).min() > 1e-3


@pytest.mark.parametrize("shape, a", hc.IDENTITY)
def test_identity_cases_take_the_whole_spectrum(shape, a):
    n = hc.reference(shape, "seqid")["n"]
    assert 0 <= a <= 64 and 0 <= n - a <= 64


# ---------------------------------------------------------------- the C ABI and the Python surface as far as the host reaches
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = " ".join(open(os.path.join(ROOT, "include", "dca_hip.h")).read().split())
    for name in ("dca_mf_hopfield_fit", "dca_mf_model_kind", "dca_mf_hopfield_couplings", "dca_hopfield_project", "dca_dense_apply"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and "int %s(" % name in header
    for tag in ('"hopfield_whiten"', '"hopfield_apply"', '"hopfield_assemble"'):
        assert tag in header
    assert "#define DCA_HOPFIELD_LIKELIHOOD %d" % _lib.HOPFIELD_LIKELIHOOD in header
    assert "#define DCA_MF_MODEL_HOPFIELD %d" % _lib.MF_MODEL_HOPFIELD in header
    assert C.sizeof(_lib.HopfieldArgs) == 40 and C.sizeof(_lib.HopfieldInfo) == 24
    x = np.zeros(8)
    assert lib.dca_mf_hopfield_fit(None, 0.5, None, None, None, None, None, None, None) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()
    assert lib.dca_dense_apply(None, x.ctypes.data, 1, 1, x.ctypes.data, 1, x.ctypes.data) == _lib.DCA_ERR_ARG
    assert lib.dca_hopfield_project(None, None, 0, 1, x.ctypes.data, x.ctypes.data) == _lib.DCA_ERR_ARG


def test_argument_rules():
    ok = dict(num_patterns=None, num_attractive=None, num_repulsive=None, tolerance=1e-10, max_iterations=1000, seed=0, L=10, q=5)
    assert _lib.hopfield_arguments(**dict(ok, num_patterns=6)) == (_lib.HOPFIELD_LIKELIHOOD, 6, 0, 0, 1e-10, 1000, 0)
    assert _lib.hopfield_arguments(**dict(ok, num_attractive=3)) == (_lib.HOPFIELD_EXPLICIT, 0, 3, 0, 1e-10, 1000, 0)
    assert _lib.hopfield_arguments(**dict(ok, num_attractive=np.int64(30), num_repulsive=10))[2:4] == (30, 10)
    assert _lib.hopfield_arguments(**dict(ok, num_patterns=128, L=40, q=21))[1] == 128
    for bad in (dict(), dict(num_patterns=0), dict(num_patterns=41), dict(num_patterns=129, L=40, q=21), dict(num_patterns=2, num_attractive=1),
                dict(num_patterns=2.0), dict(num_patterns=True), dict(num_attractive=65, L=40, q=21), dict(num_repulsive=-1),
                dict(num_attractive=0, num_repulsive=0), dict(num_attractive=30, num_repulsive=11), dict(num_patterns=2, tolerance=0.0),
                dict(num_patterns=2, tolerance=float("nan")), dict(num_patterns=2, tolerance="1e-3"), dict(num_patterns=2, max_iterations=0),
                dict(num_patterns=2, seed=-1), dict(num_patterns=2, seed=2 ** 64)):
        with pytest.raises(ValueError):
            _lib.hopfield_arguments(**dict(ok, **bad))


def test_class_and_command_line_surface(monkeypatch, capsys):
    assert issubclass(HopfieldPottsDCA, MeanFieldDCA) and issubclass(HopfieldPottsDCA, _potts.PottsModel)
    assert issubclass(HopfieldPottsDCA, _compare.SequenceComparison)
    for name in ("compute_patterns", "project_on_patterns", "compute_sorted_FN", "compute_sorted_FN_APC", "compute_sorted_DI",
                 "compute_sorted_DI_APC", "compute_fields", "compute_params", "get_couplings", "compute_sequence_energies",
                 "sample_sequences", "find_local_maxima", "compute_log_partition_function", "compare_with_alignment"):
        assert callable(getattr(HopfieldPottsDCA, name))
    for name in ("_device_scores", "get_couplings", "_with_couplings"):       # the three places where MeanFieldDCA fits its model
        assert getattr(HopfieldPottsDCA, name) is not getattr(MeanFieldDCA, name)
    assert not hasattr(MeanFieldDCA, "compute_patterns")
    assert hopfield_main.SUBCOMMANDS == ("compute_fn", "compute_patterns", "project_sequences")
    for name in hopfield_main.SUBCOMMANDS + _potts.POTTS_SUBCOMMANDS:
        with pytest.raises(SystemExit):
            hopfield_main.run_hopfield_dca([name, "--help"])
        text = capsys.readouterr().out
        for flag in ("--num_patterns", "--num_attractive", "--num_repulsive", "--tolerance", "--max_iterations", "--pseudocount"):
            assert flag in text
    seen = {}
    monkeypatch.setattr(hopfield_main, "execute_from_command_line", lambda **kw: seen.update(kw) or "done")
    hopfield_main.run_hopfield_dca(["compute_fn", "rna", TOY_RNA, "--num_patterns", "7", "--apc", "--pseudocount", "0.3"])
    assert (seen["the_command"], seen["num_patterns"], seen["apc"], seen["pseudocount"]) == ("compute_fn", 7, True, 0.3)
    hopfield_main.run_hopfield_dca(["project_sequences", "rna", TOY_RNA, "--num_attractive", "2", "--num_repulsive", "3", "--query_file", "q.fa"])
    assert (seen["the_command"], seen["num_attractive"], seen["num_repulsive"], seen["query_file"]) == ("project_sequences", 2, 3, "q.fa")
    hopfield_main.run_hopfield_dca(["sample_sequences", "rna", TOY_RNA, "--num_patterns", "4", "--num_sequences", "5", "--seed", "3", "--fit_seed", "9"])
    assert seen["sampling"]["num_sequences"] == 5 and seen["sampling"]["seed"] == 3 and seen["fit_seed"] == 9
