"""Host side of sparse bmDCA: the decimation score against the exact symmetrised Kullback-Leibler divergence of an enumerated
model, its properties, the zero-sum gauge and the selection of tests/decimation_reference.py, the C ABI's new entries and
PlmDCA.decimate_boltzmann's argument checks.  No GPU needed."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import decimation_reference as ref  # noqa: E402
from pydca_amd import _lib, _potts, plmdca_main  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException  # noqa: E402

TOY_RNA = os.path.join(ROOT, "tests", "golden", "data", "toy_rna.fa")
ENTRIES = ("dca_plm_zero_sum_gauge", "dca_plm_bm_set_mask", "dca_plm_bm_get_mask", "dca_plm_bm_decimate")
LD = np.longdouble


def enumerated(L, q, seed):
    rng = np.random.default_rng(seed)
    iu, ju = ref.pairs_of(L)
    x = np.concatenate([rng.normal(0, 0.5, L * q), rng.normal(0, 0.7, iu.size * q * q)])
    S = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.int64)
    return x, S, iu, ju


def distribution(x, S, L, q):
    v = np.asarray(x, dtype=LD)
    h, J = v[:L * q].reshape(L, q), v[L * q:].reshape(-1, q, q)
    iu, ju = ref.pairs_of(L)
    E = h[np.arange(L)[None, :], S].sum(axis=1) + J[np.arange(iu.size)[None, :], S[:, iu], S[:, ju]].sum(axis=1)
    w = np.exp(E - E.max())
    return w / w.sum()


def test_score_is_the_symmetrised_kl_of_an_enumerated_model():
    L, q = 3, 3
    x, S, iu, ju = enumerated(L, q, 5)
    P = distribution(x, S, L, q)
    worst = 0.0
    for pr, a, b in itertools.product(range(iu.size), range(q), range(q)):
        off = L * q + (pr * q + a) * q + b
        hit = (S[:, iu[pr]] == a) & (S[:, ju[pr]] == b)
        p = P[hit].sum()
        x0 = x.copy()
        x0[off] = 0.0
        P0 = distribution(x0, S, L, q)
        kl = (P * (np.log(P) - np.log(P0))).sum() + (P0 * (np.log(P0) - np.log(P))).sum()
        D = ref.score(LD(x[off]), p, LD)
        worst = max(worst, float(abs(D - kl) / kl))
    assert worst <= 1e-15, worst


def test_score_properties():
    rng = np.random.default_rng(1)
    J = np.concatenate([rng.normal(0, 2.0, 4000), [800.0, -800.0, 800.0, -800.0, 1e-300, -1e-300, 0.0, -0.0, 3.0, -3.0]])
    p = np.concatenate([rng.random(4000), [0.5, 0.5, 1e-12, 1.0 - 1e-12, 0.3, 0.3, 0.4, 0.4, 0.0, 1.0]])
    for dt in (np.float64, LD):
        D = ref.score(J, p, dt)
        assert np.all(np.isfinite(D)) and np.all(D >= 0) and not np.any(np.signbit(D))
        assert np.all(D[-4:] == 0)                                   # J == 0, p == 0, p == 1
        assert np.all(D[:4000][J[:4000] != 0] > 0)
    # large |J|: D -> |J| p (1 - p) / (the surviving side)
    assert ref.score(800.0, 0.5) == 800.0 * 0.25 / 0.5 and ref.score(-800.0, 0.5) == 800.0 * 0.25 / 0.5
    # D / (J^2 p (1 - p)) -> 1 as J -> 0
    for Jv in (1e-4, -1e-4, 1e-7, -1e-7):
        pv = np.array([0.01, 0.3, 0.9])
        ratio = ref.score(Jv, pv) / (Jv * Jv * pv * (1 - pv))
        assert np.all(np.abs(ratio - 1.0) <= 2.0 * abs(Jv)), (Jv, ratio)
    # the float64 order against longdouble: a few roundings and the condition of the denominator
    D64, Dld = ref.score(J[:4000], p[:4000]), ref.score(J[:4000], p[:4000], LD)
    cond = 1.0 / np.minimum(p[:4000], 1.0 - p[:4000])
    assert np.all(np.abs(D64 - Dld) <= 8 * 2.0 ** -53 * cond * Dld)


def test_zero_sum_gauge_restatement():
    L, q = 3, 3
    x, S, iu, ju = enumerated(L, q, 9)
    y = ref.zero_sum_gauge(x, L, q)
    E0, mag = ref.energies(x, S, L, q)
    E1, _ = ref.energies(y, S, L, q)
    shift = E1 - E0
    assert np.max(np.abs(shift - shift[0])) <= 64 * 2.0 ** -53 * mag.max()
    J = y[L * q:].reshape(-1, q, q)
    scale = np.abs(x[L * q:]).max()
    assert np.abs(J.sum(axis=1)).max() <= 16 * 2.0 ** -53 * scale and np.abs(J.sum(axis=2)).max() <= 16 * 2.0 ** -53 * scale
    assert np.abs(y[:L * q].reshape(L, q).sum(axis=1)).max() <= 64 * 2.0 ** -53 * (np.abs(x).max() * L)
    y32 = ref.zero_sum_gauge(x.astype(np.float32), L, q)
    assert y32.dtype == np.float32
    assert np.array_equal(y32, ref.zero_sum_gauge(x.astype(np.float32).astype(np.float64), L, q).astype(np.float32))
    z = ref.zero_sum_gauge(y, L, q)                                  # a second pass moves nothing beyond rounding
    assert np.max(np.abs(z - y)) <= 64 * 2.0 ** -53 * np.abs(x).max() * L


def test_selection_reference_against_lexsort():
    rng = np.random.default_rng(3)
    n = 5000
    D = rng.random(n) * 1e-3
    D[rng.random(n) < 0.3] = 0.0                                     # the tie group at +0
    D[rng.integers(0, n, 200)] = D[7]                                # planted ties above zero
    D[rng.random(n) < 0.1] = -1.0                                    # removed elements
    act = np.flatnonzero(D >= 0)
    order = act[np.lexsort((act, D[act].view(np.uint64)))]
    zeros = int((D == 0).sum())
    for k in (0, 1, zeros // 2, zeros, zeros + 1, int(np.searchsorted(np.sort(D[act]), D[7])) + 50, act.size):
        got = ref.select(D, k)
        assert np.array_equal(got, np.sort(order[:k])), k
        info = ref.selection_info(D, k)
        assert info["active_before"] == act.size and info["active_after"] == act.size - k
        if k:
            assert info["threshold"] == D[order[k - 1]] == D[got].max()
            assert abs(info["removed_sum"] - D[got].sum()) <= 1e-12 * max(D[got].sum(), 1e-300)


def test_entries_and_struct():
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    assert "dca_bm_decimation;" in header and all(name + "(" in header for name in ENTRIES)
    A = _lib.BmDecimation
    assert [getattr(A, f).offset for f in ("active_before", "removed", "active_after", "threshold", "removed_sum")] == [0, 8, 16, 24, 32]
    assert C.sizeof(A) == 40
    assert C.sizeof(_lib.BmArgs) == 72                                # dca_bm_args is ABI: no field was added


def test_entries_refuse_without_a_context():
    lib = _lib.lib()
    buf = np.zeros(8, dtype=np.uint8)
    assert lib.dca_plm_zero_sum_gauge(None) == _lib.DCA_ERR_ARG
    assert lib.dca_plm_bm_set_mask(None, buf.ctypes.data) == _lib.DCA_ERR_ARG
    assert lib.dca_plm_bm_get_mask(None, buf.ctypes.data) == _lib.DCA_ERR_ARG
    assert lib.dca_plm_bm_decimate(None, 0, None, None) == _lib.DCA_ERR_ARG


@pytest.mark.parametrize("kw", [dict(target_density=-0.01), dict(target_density=1.01), dict(target_density=float("nan")),
                                dict(drop_fraction=0.0), dict(drop_fraction=1.5), dict(drop_fraction=-0.1), dict(gauge="lattice"),
                                dict(gauge=None), dict(iterations_per_check=0), dict(max_iterations_per_round=0),
                                dict(warmup_iterations=2.5), dict(num_chains=0), dict(learning_rate=-1.0), dict(init="random"),
                                dict(pearson_target=float("nan"))])
def test_decimate_boltzmann_argument_checks(kw):
    inst = PlmDCA(TOY_RNA, "rna")
    with pytest.raises(PlmDCAException):
        inst.decimate_boltzmann(**kw)


def test_decimate_boltzmann_refuses_several_devices():
    with pytest.raises(PlmDCAException, match="one GPU"):
        PlmDCA(TOY_RNA, "rna", devices=[0, 1]).decimate_boltzmann()


def test_subcommand_options(monkeypatch):
    seen = {}
    monkeypatch.setattr(plmdca_main, "execute_from_command_line", lambda *a, **kw: seen.update(kw, args=a) or "done")
    plmdca_main.run_plm_dca(["decimate_boltzmann", "rna", TOY_RNA, "--target_density", "0.3", "--drop_fraction", "0.2", "--gauge", "keep",
                             "--num_chains", "64", "--bm_lambda_J", "0.02", "--num_samples", "4"])
    want = dict(target_density=0.3, drop_fraction=0.2, pearson_target=0.95, iterations_per_check=10, max_iterations_per_round=500,
                warmup_iterations=500, gauge="keep", num_chains=64, sweeps_per_iteration=10, equilibration_sweeps=100,
                learning_rate=0.05, bm_lambda_h=1e-4, bm_lambda_J=0.02, pseudocount=None, seed=0, init="plm", num_samples=4,
                num_sweeps=1000)
    assert seen["the_command"] == "decimate_boltzmann" and seen["decimation"] == want
    assert set(_potts.DECIMATION_OPTIONS) == set(want)
    with pytest.raises(SystemExit):
        plmdca_main.run_plm_dca(["decimate_boltzmann", "rna", TOY_RNA, "--gauge", "ising"])


class StandIn:
    def __init__(self):
        self.calls = []

    def decimate_boltzmann(self, **kw):
        self.calls.append(kw)
        mask = np.array([[[True, False], [False, True]]])
        return {"history": np.zeros((3, 3)), "rounds": np.array([[2.0, 4.0, 2.0, 0.5, 0.125, 1.0 / 3.0]]), "mask": mask, "density": 0.5,
                "fields_and_couplings": np.array([0, 0, 0, 0, 1, 0, 0, 2], dtype=np.float32)}


def test_subcommand_files(tmp_path):
    inst = StandIn()
    opts = dict(target_density=0.5, drop_fraction=0.5, gauge="keep", bm_lambda_h=0.1, bm_lambda_J=0.2, pseudocount=None, seed=5,
                num_samples=None, num_sweeps=4)
    files = _potts.run_decimation(inst, "PLMDCA", TOY_RNA, str(tmp_path / "out"), ["# meta"], _lib.DCA_BIOMOLECULE_RNA, opts)
    assert [os.path.basename(f) for f in files] == ["PLMDCA_decimation_toy_rna.txt", "PLMDCA_decimation_params_toy_rna.npy",
                                                    "PLMDCA_decimation_mask_toy_rna.npy"]
    assert inst.calls == [dict(target_density=0.5, drop_fraction=0.5, gauge="keep", lambda_h=0.1, lambda_J=0.2, pseudocount=None, seed=5)]
    lines = open(files[0]).read().splitlines()
    assert "# meta" in lines
    rows = [ln for ln in lines if not ln.startswith("#")]
    assert rows == ["2 4 2 0.5 0.125 %.17g" % (1.0 / 3.0)]
    assert np.load(files[2]).dtype == np.bool_ and np.load(files[1]).dtype == np.float32
