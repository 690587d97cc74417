"""Host side of replica-exchange Gibbs sampling (dca_plm_sample_tempered, dca_mf_sample_tempered): the
exported entries, the argument checks of sample_sequences_tempered, temperature_ladder, the sample_tempered sub-command, and
the numpy restatement the GPU tests compare with (tempered_reference.py), held here to the plain sampler's restatement and to
exact enumeration.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts, mfdca_main, plmdca_main  # noqa: E402
from pydca_amd.fasta_reader import fasta_reader  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCAException  # noqa: E402
from tempered_reference import energies_np, exact_distribution, tempered_ref  # noqa: E402
from test_potts_sampling import _g_test, gibbs_ref, random_start  # noqa: E402

ENTRIES = ("dca_plm_sample_tempered", "dca_mf_sample_tempered")
TOY_RNA = os.path.join(ROOT, "tests", "data", "toy_rna.fa")


def random_model(L, q, seed, sigma=0.5):
    rng = np.random.default_rng(seed)
    return rng.normal(0, sigma, (L, q)), rng.normal(0, sigma, (L * (L - 1) // 2, q, q))


# ---------------------------------------------------------------- the restatement
def test_without_exchange_every_walker_is_the_plain_restatement():
    L, q, M = 7, 5, 9
    h, Jp = random_model(L, q, 1)
    betas = np.array([0.0, 0.6, 1.7])
    R = betas.size
    res = tempered_ref(h, Jp, betas, M, 4, 0, 21, first_ladder=3, first_sweep=2)
    assert res["rounds"] == 0 and res["trace"].shape == (0, M, R) and not res["attempts"].any()
    assert res["levels"].tolist() == list(range(R)) * M
    for r in range(R):
        chains = (3 + np.arange(M)) * R + r
        want, _m = gibbs_ref(h, Jp, betas[r], 21, chains, 2, 4, random_start(21, chains, L, q))
        assert np.array_equal(res["codes"][r::R], want)


def test_restatement_rounds_pairs_and_bookkeeping():
    L, q, M = 6, 4, 30
    h, Jp = random_model(L, q, 2)
    betas = np.array([0.0, 0.4, 0.9, 1.5, 2.2])
    R = betas.size
    res = tempered_ref(h, Jp, betas, M, 12, 3, 5, first_ladder=7, first_sweep=2)
    assert res["rounds"] == (2 + 12) // 3 - 2 // 3 == 4                    # rounds 0 .. 3 of the global count, after sweeps 2, 5, 8, 11
    assert res["attempts"].tolist() == [2 * M, 2 * M, 2 * M, 2 * M]       # even rounds pair (0,1), (2,3); odd rounds (1,2), (3,4)
    assert (res["accepts"] <= res["attempts"]).all() and res["accepts"].sum() > 0
    lv = res["levels"].reshape(M, R)
    assert (np.sort(lv, axis=1) == np.arange(R)).all()
    # the last trace row is E of the walkers before round 3, which follows sweep 11: the final energies of a run that ends there
    assert res["trace"].shape == (4, M, R)
    short = tempered_ref(h, Jp, betas, M, 10, 3, 5, first_ladder=7, first_sweep=2)
    assert np.array_equal(short["trace"], res["trace"]) and np.array_equal(short["accepts"], res["accepts"])
    E = energies_np(h, Jp, short["codes"]).reshape(M, R)
    assert np.array_equal(np.sort(res["trace"][-1], axis=1), np.sort(E, axis=1))
    # split by ladders and continuation at a first_sweep that is no multiple of I
    a = tempered_ref(h, Jp, betas, 11, 12, 3, 5, first_ladder=7, first_sweep=2)
    b = tempered_ref(h, Jp, betas, M - 11, 12, 3, 5, first_ladder=18, first_sweep=2)
    assert np.array_equal(np.vstack([a["codes"], b["codes"]]), res["codes"])
    assert np.array_equal(np.concatenate([a["levels"], b["levels"]]), res["levels"])
    assert np.array_equal(a["accepts"] + b["accepts"], res["accepts"])
    assert np.array_equal(np.concatenate([a["trace"], b["trace"]], axis=1), res["trace"])
    head = tempered_ref(h, Jp, betas, M, 5, 3, 5, first_ladder=7, first_sweep=2)
    tail = tempered_ref(h, Jp, betas, M, 7, 3, 5, first_ladder=7, first_sweep=7, initial=head["codes"], initial_levels=head["levels"])
    assert np.array_equal(tail["codes"], res["codes"]) and np.array_equal(tail["levels"], res["levels"])
    assert np.array_equal(head["accepts"] + tail["accepts"], res["accepts"])
    assert np.array_equal(np.concatenate([head["trace"], tail["trace"]]), res["trace"])


def test_restatement_samples_the_exact_distribution_at_every_level():
    """L = 4, q = 5, betas (0, 0.5, 1, 2), 20 000 ladders, 30 sweeps, an exchange round after every sweep: per level the final
    states pass test_distribution_of_final_states' criteria against exact enumeration (G-test p > 1e-6, the mean energy within
    5 sigma)."""
    L, q, M = 4, 5, 20000
    h, Jp = random_model(L, q, 77)
    betas = np.array([0.0, 0.5, 1.0, 2.0])
    R = betas.size
    res = tempered_ref(h, Jp, betas, M, 30, 1, 2024)
    assert res["rounds"] == 30
    acc = res["accepts"] / res["attempts"]
    assert (acc > 0.05).all() and (acc < 1.0).all(), acc
    at = np.argsort(res["levels"].reshape(M, R), axis=1)
    codes = res["codes"].reshape(M, R, L)
    for k, beta in enumerate(betas):
        out = codes[np.arange(M), at[:, k]]
        _states, E, P = exact_distribution(h, Jp, beta)
        idx = np.ravel_multi_index(out.T.astype(np.int64), (q,) * L)
        p = _g_test(np.bincount(idx, minlength=q ** L).astype(np.float64), M * P)
        assert p > 1e-6, (beta, p)
        mean, var = float(np.dot(P, E)), float(np.dot(P, (E - np.dot(P, E)) ** 2))
        assert abs(E[idx].mean() - mean) <= 5.0 * math.sqrt(var / M), beta


# ---------------------------------------------------------------- C ABI
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert "int " + name + "(dca_ctx* ctx, const dca_pt_args* args, uint8_t* out /* M*R x L */, int32_t* levels_out /* M*R */," in header
    assert "typedef struct dca_pt_args {" in header and "} dca_pt_args;" in header
    for field in ("int ladders, levels;", "const double* betas;", "int sweeps, swap_interval;", "uint64_t seed, first_ladder, first_sweep;",
                  "const uint8_t* initial;", "const int32_t* initial_levels;"):
        assert field in header
    assert '"pt_energy"' in header and '"pt_swap"' in header and "DESIGN.md section 25" in header
    assert "## 25." in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert hasattr(_lib.Context, "plm_sample_tempered") and hasattr(_lib.Context, "mf_sample_tempered")
    assert [f for f, _t in _lib.PtArgs._fields_] == ["ladders", "levels", "betas", "sweeps", "swap_interval", "seed", "first_ladder",
                                                     "first_sweep", "initial", "initial_levels"]
    internal = open(os.path.join(ROOT, "pydca_amd", "csrc", "dca_internal.h")).read()
    assert "5 the exchange decision" in internal
    assert "tempered.hip" in open(os.path.join(ROOT, "pydca_amd", "csrc", "Makefile")).read()


def test_entries_refuse_without_a_context():
    lib = _lib.lib()
    betas = np.array([0.5, 1.0])
    args = _lib.PtArgs(1, 2, betas.ctypes.data, 1, 1, 0, 0, 0, None, None)
    out = np.zeros((2, 4), dtype=np.uint8)
    levels = np.zeros(2, dtype=np.int32)
    import ctypes
    for name in ENTRIES:
        assert getattr(lib, name)(None, ctypes.byref(args), out.ctypes.data, levels.ctypes.data, None, None, None, None, None) == _lib.DCA_ERR_ARG


def test_context_binding_checks_the_shapes():
    class Ctx(_lib.Context):
        def __init__(self):                                     # no device: only the host-side checks are reached
            self._l, self._h, self.L = _lib.lib(), None, 4
    with pytest.raises(ValueError, match="uint8"):
        Ctx().plm_sample_tempered(2, [0.5, 1.0], 1, initial=np.zeros((2, 4), dtype=np.uint8))          # needs 4 rows
    with pytest.raises(ValueError, match="initial_levels"):
        Ctx().mf_sample_tempered(2, [0.5, 1.0], 1, initial_levels=[0, 1])


# ---------------------------------------------------------------- Python argument checks
class Boom(Exception):
    pass


class Quiet:
    def info(self, *a):
        pass

    error = info


class Model(_potts.PottsModel):
    """PottsModel over a recorded _potts_call: L = 6 RNA sites.  The recorded sample_tempered puts walker r of ladder m at level
    (r + m) mod R, gives its row the codes (r + m) mod R ... and the energy 100 m + r; every trace entry is 10 round + level."""
    _potts_exc = Boom
    _potts_table = 0
    _potts_logger = Quiet()

    def __init__(self, devices=None):
        self.calls, self.devices = [], devices

    def _potts_dims(self):
        return _lib.DCA_BIOMOLECULE_RNA, 6, 5

    def _potts_devices(self):
        return self.devices

    def _potts_call(self, name, *args, **kw):
        self.calls.append((name, args, kw))
        M, betas, sweeps = args
        R, I = len(betas), kw["swap_interval"]
        rounds = sweeps // I if I else 0
        m, r = np.divmod(np.arange(M * R), R) if R else (np.zeros(0, int), np.zeros(0, int))
        levels = (r + m) % R
        codes = np.repeat((levels % 5).astype(np.uint8)[:, None], 6, axis=1)
        trace = 10.0 * np.arange(rounds)[:, None, None] + np.arange(R)[None, None, :] + np.zeros((rounds, M, R))
        return {"codes": codes, "levels": levels.astype(np.int32), "energies": 100.0 * m + r,
                "attempts": np.full(max(R - 1, 0), 8, dtype=np.uint64) * np.uint64(rounds > 0),
                "accepts": np.arange(max(R - 1, 0), dtype=np.uint64) * np.uint64(rounds > 0), "rounds": rounds, "trace": trace}


def test_argument_checks_come_before_the_device():
    m = Model()
    for bad in ([], [0.0, 1.0], [-1.0], [float("nan")], "abc", None, [1.0, "x"]):
        with pytest.raises(Boom, match="temperature"):
            m.sample_sequences_tempered(2, bad)
    for kw in ({"num_sweeps": -1}, {"swap_interval": -1}, {"seed": -3}, {"burn_in_sweeps": -1}, {"num_sweeps": 2.5}, {"swap_interval": True}):
        with pytest.raises(Boom, match="integer"):
            m.sample_sequences_tempered(2, [1.0, 2.0], **kw)
    with pytest.raises(Boom, match="integer"):
        m.sample_sequences_tempered(-1, [1.0])
    with pytest.raises(Boom, match="2\\^24"):
        m.sample_sequences_tempered(1 << 23, [1.0, 2.0, 3.0])
    with pytest.raises(Boom, match="records"):
        m.sample_sequences_tempered(3, [1.0, 2.0], initial=["ACGUAC", "ACGUAC"])
    with pytest.raises(Boom, match="record 1"):
        m.sample_sequences_tempered(1, [1.0, 2.0], initial="ACGU")
    assert m.calls == []
    with pytest.raises(Boom, match="one GPU"):
        Model(devices=[0, 1]).sample_sequences_tempered(2, [1.0])


def test_result_follows_the_callers_temperature_order():
    m = Model()
    T = [1.0, float("inf"), 0.5, 2.0, 1.0]                                # betas ascending: 0, 0.5, 1, 2 -> levels 2, 0, 3, 1, 2
    res = m.sample_sequences_tempered(3, T, num_sweeps=8, swap_interval=2, seed=9, initial="ACGUAC", burn_in_sweeps=4)
    name, args, kw = m.calls[-1]
    assert name == "sample_tempered" and args[0] == 3 and args[1].tolist() == [0.0, 0.5, 1.0, 2.0] and args[2] == 8
    assert kw["swap_interval"] == 2 and kw["seed"] == 9 and kw["trace"] is True
    assert kw["initial"].shape == (12, 6) and (kw["initial"] == np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8)).all()
    assert sorted(res) == sorted(["temperatures", "sequences", "energies", "swap_acceptance", "swap_attempts", "mean_energy",
                                  "heat_capacity", "num_rounds"])
    assert res["temperatures"].tolist() == T and res["num_rounds"] == 4
    want_level = [2, 0, 3, 1, 2]
    letters = "ACGU-"
    for t, lv in enumerate(want_level):
        assert res["sequences"][t] == [letters[lv] * 6] * 3              # the recorded walker at level lv carries the code lv
        # ... and it is walker (lv - m) mod R of ladder m, whose recorded energy is 100 m + r
        assert res["energies"][t].tolist() == [100.0 * mm + (lv - mm) % 4 for mm in range(3)]
    assert res["energies"].shape == (5, 3)
    assert res["swap_attempts"].tolist() == [8, 8, 8] and res["swap_acceptance"].tolist() == [0.0, 0.125, 0.25]
    # rounds end sweeps 1, 3, 5, 7: past burn_in_sweeps = 4 are rounds 2 and 3 -> values 20 + lv and 30 + lv
    assert res["mean_energy"].tolist() == [25.0 + lv for lv in want_level]
    betas = np.array([0.0, 0.5, 1.0, 2.0])
    assert np.allclose(res["heat_capacity"], (betas ** 2 * 25.0)[want_level], rtol=1e-15)
    codes = m.sample_sequences_tempered(3, T, num_sweeps=8, return_codes=True)["sequences"]
    assert len(codes) == 5 and codes[0].dtype == np.uint8 and codes[0].shape == (3, 6) and (codes[2] == 3).all()
    assert m.calls[-1][2]["initial"] is None and m.calls[-1][2]["swap_interval"] == 1
    # no exchange, or nothing past burn-in: NaN
    res = m.sample_sequences_tempered(2, [1.0, 2.0], num_sweeps=6, swap_interval=0)
    assert res["num_rounds"] == 0 and np.isnan(res["swap_acceptance"]).all() and np.isnan(res["mean_energy"]).all()
    assert np.isnan(res["heat_capacity"]).all()
    res = m.sample_sequences_tempered(2, [1.0, 2.0], num_sweeps=6, burn_in_sweeps=6)
    assert res["num_rounds"] == 6 and np.isnan(res["mean_energy"]).all()
    res = m.sample_sequences_tempered(2, [1.0, 2.0], num_sweeps=6)                  # burn-in 3: rounds 3, 4, 5
    assert res["mean_energy"].tolist() == [41.0, 40.0]
    assert m.sample_sequences_tempered(0, [1.0, 2.0], num_sweeps=2)["energies"].shape == (2, 0)
    assert m.sample_sequences_tempered(2, [3.0], num_sweeps=2)["swap_acceptance"].shape == (0,)


def test_temperature_ladder():
    t = _potts.temperature_ladder(0.5, 2.0, 5)
    assert t.dtype == np.float64 and t[0] == 0.5 and t[-1] == 2.0 and np.allclose(t[1:] / t[:-1], 2.0 ** 0.5, rtol=1e-14)
    assert _potts.temperature_ladder(0.3, 0.3, 1).tolist() == [0.3] and _potts.temperature_ladder(1, 4, 2).tolist() == [1.0, 4.0]
    for bad in ((0.0, 1.0, 3), (-1.0, 1.0, 3), (2.0, 1.0, 3), (1.0, float("inf"), 3), (1.0, 2.0, 0), (1.0, 2.0, 2.5), (1.0, 1.0, 2),
                (float("nan"), 1.0, 2)):
        with pytest.raises(ValueError):
            _potts.temperature_ladder(*bad)


# ---------------------------------------------------------------- command lines
@pytest.mark.parametrize("main,run", [(plmdca_main, "run_plm_dca"), (mfdca_main, "run_meanfield_dca")])
def test_sample_tempered_arguments(monkeypatch, main, run):
    assert "sample_tempered" in _potts.POTTS_SUBCOMMANDS
    seen = {}
    monkeypatch.setattr(main, "execute_from_command_line", lambda *a, **kw: seen.update(kw) or "done")
    assert getattr(main, run)(["sample_tempered", "rna", "x.fa", "--num_sequences", "7", "--temperatures", "0.5,0.7,1,1.5",
                               "--num_sweeps", "30", "--swap_interval", "2", "--seed", "11", "--initial_file", "s.fa"]) == "done"
    assert seen["the_command"] == "sample_tempered"
    assert seen["tempered"] == {"num_sequences": 7, "temperatures": "0.5,0.7,1,1.5", "num_sweeps": 30, "swap_interval": 2, "seed": 11,
                                "initial_file": "s.fa"}
    getattr(main, run)(["sample_tempered", "rna", "x.fa", "--num_sequences", "2", "--temperatures", "1"])
    assert seen["tempered"] == {"num_sequences": 2, "temperatures": "1", "num_sweeps": 1000, "swap_interval": 1, "seed": 0,
                                "initial_file": None}
    for argv in (["--num_sequences", "2"], ["--temperatures", "1,2"]):
        with pytest.raises(SystemExit):
            getattr(main, run)(["sample_tempered", "rna", "x.fa"] + argv)
    with pytest.raises(SystemExit):                            # the plain sampler's sub-command does not take the new options
        getattr(main, run)(["sample_sequences", "rna", "x.fa", "--num_sequences", "2", "--temperatures", "1,2"])


class StandIn:
    """The call run_subcommand makes for sample_tempered, recorded"""
    sequences_len = 10

    def __init__(self):
        self.calls = []

    def sample_sequences_tempered(self, n, temperatures, **kw):
        self.calls.append((n, list(temperatures), kw))
        T = len(temperatures)
        codes = [np.array([[0, 1, 2, 3, 4, 0, 1, 2, 3, 4], [t % 5] * 10], dtype=np.uint8) for t in range(T)]
        return {"temperatures": np.array(temperatures, dtype=np.float64), "sequences": codes,
                "energies": np.array([[-1.25 - t, 1.0 / 3.0] for t in range(T)]), "swap_acceptance": np.array([0.25, np.nan]),
                "swap_attempts": np.array([40, 0], dtype=np.uint64), "mean_energy": np.arange(T) + 0.5,
                "heat_capacity": np.arange(T) * 2.0, "num_rounds": 12}


def test_subcommand_files(tmp_path):
    inst = StandIn()
    out = str(tmp_path / "out")
    opts = {"num_sequences": 2, "temperatures": "1,inf,0.5", "num_sweeps": 12, "swap_interval": None, "seed": None, "initial_file": "s.fa"}
    fa, txt = _potts.run_subcommand(inst, "sample_tempered", "MFDCA", TOY_RNA, out, ["# meta"], _lib.DCA_BIOMOLECULE_RNA, 1,
                                    PlmDCAException, tempered=opts)
    assert os.path.basename(fa) == "MFDCA_tempered_samples_toy_rna.fa" and os.path.basename(txt) == "MFDCA_tempered_sampling_toy_rna.txt"
    assert inst.calls == [(2, [1.0, float("inf"), 0.5], {"num_sweeps": 12, "swap_interval": 1, "seed": 0, "initial": "s.fa",
                                                         "return_codes": True})]
    assert open(fa).read().splitlines() == [
        ">sample_1 temperature=1 energy=-1.25", "ACGU-ACGU-", ">sample_2 temperature=1 energy=%.17g" % (1.0 / 3.0), "AAAAAAAAAA",
        ">sample_1 temperature=inf energy=-2.25", "ACGU-ACGU-", ">sample_2 temperature=inf energy=%.17g" % (1.0 / 3.0), "CCCCCCCCCC",
        ">sample_1 temperature=0.5 energy=-3.25", "ACGU-ACGU-", ">sample_2 temperature=0.5 energy=%.17g" % (1.0 / 3.0), "GGGGGGGGGG"]
    assert len(fasta_reader.get_alignment_from_fasta_file(fa)) == 6
    lines = open(txt).read().splitlines()
    assert "# meta" in lines and any("Exchange rounds: 12" in ln for ln in lines)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    # the ladder in ascending beta is inf, 1, 0.5: T = 1 exchanges with the colder 0.5 (nothing attempted), inf with 1, 0.5 is the coldest
    assert rows == [["1", "0.5", "0", "nan"], ["inf", "1.5", "2", "0.25"], ["0.5", "2.5", "4", "nan"]]
    for bad in ({"num_sequences": None}, {"temperatures": None}, {"temperatures": "1,,2"}, {"temperatures": "a"}):
        with pytest.raises(PlmDCAException):
            _potts.run_subcommand(inst, "sample_tempered", "MFDCA", TOY_RNA, out, None, _lib.DCA_BIOMOLECULE_RNA, 1, PlmDCAException,
                                  tempered=dict(opts, **bad))
