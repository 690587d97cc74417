"""Host side of the redundancy filter and the identity clusters (dca_identity_filter, dca_identity_clusters,
pydca_amd/redundancy.py and its sub-commands): exports and declarations, refusals that need no device,
the numpy reference of tests/redundancy_reference.py against a hand-computed example and against independent restatements, the
threshold rules, the launch plan of redundancy_plan.h, the split's host logic, the sub-commands through a stand-in -- and the
FIXTURE CONDITIONS: what every case of tests/test_redundancy.py must offer so that it cannot pass vacuously, asserted here on
the CPU reference alone.

The conditions are asserted for the family fixture at its own threshold T on every grid shape with n >= 63 and L >= 31.  The
remaining grid points cannot meet them by construction and are kept as edge cases of the kernels, not as evidence: n <= 2 (no
cluster of three), L = 1 (similarity is equality, hence transitive: no chain) and the thresholds 1, L and L + 1 (everything /
only duplicates / nothing is similar)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import redundancy_reference as R
from pydca_amd import _lib, main, redundancy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dca_identity_filter", "dca_identity_clusters")


# ---------------------------------------------------------------- C ABI
def test_entries_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert "int " + name + "(dca_ctx* ctx, const uint8_t* X" in header
    assert "typedef struct { int32_t kept, blocks, block_rows; int64_t tile_pairs; } dca_filter_info;" in header
    assert "typedef struct { int32_t clusters, largest, rounds, stored_bits" in header
    assert C.sizeof(_lib.FilterInfo) == 24 and C.sizeof(_lib.ClusterInfo) == 16
    assert '"identity_filter", "identity_clusters"' in header
    srcs = open(os.path.join(ROOT, "pydca_amd", "csrc", "Makefile")).read()
    assert " redundancy.hip " in srcs


def test_entries_refuse_a_null_context():
    lib = _lib.lib()
    X = np.zeros((2, 4), dtype=np.uint8)
    keep = np.zeros(2, dtype=np.uint8)
    label = np.zeros(2, dtype=np.int32)
    assert lib.dca_identity_filter(None, X.ctypes.data, 2, 3, None, keep.ctypes.data, None, None) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()
    assert lib.dca_identity_clusters(None, X.ctypes.data, 2, 3, label.ctypes.data, None, None) == _lib.DCA_ERR_ARG
    assert b"null context" in lib.dca_last_error()


def test_python_argument_checks_need_no_device():
    X = np.zeros((4, 10), dtype=np.uint8)
    for bad in (dict(min_identical_sites=0), dict(min_identical_sites=12), dict(min_identical_sites=2.0), dict(identity="0.9"),
                dict(identity=float("nan")), dict(identity=0.0), dict(identity=-1.0)):
        with pytest.raises(ValueError):
            redundancy.identity_threshold(10, **bad)
    with pytest.raises(ValueError):
        redundancy.identity_threshold(0, 0.9)
    for bad in ("most_gaps", np.array([0, 1, 2]), np.array([0, 1, 2, 2]), np.array([0.0, 1.0, 2.0, 3.0]), np.array([0, 1, 2, 4])):
        with pytest.raises(ValueError):
            redundancy.priority_order(X, 5, bad)
    assert redundancy.priority_order(X, 5, "file") is None
    G = np.array([[4, 4, 0], [0, 0, 0], [4, 0, 0], [0, 1, 2]], dtype=np.uint8)
    assert redundancy.priority_order(G, 5, "fewest_gaps").tolist() == [1, 3, 2, 0]
    assert np.array_equal(redundancy.priority_order(G, 5, "fewest_gaps"), R.gap_order(G, 5))
    assert redundancy.priority_order(G, 5, [3, 1, 0, 2]).dtype == np.int32
    for bad in (-0.1, 0.6):
        with pytest.raises(ValueError):
            redundancy.split_by_labels(np.zeros(4, dtype=np.int32), bad, 0)


# ---------------------------------------------------------------- the reference
HAND = np.array([[0, 1, 2, 3, 4, 0],
                 [0, 1, 2, 3, 0, 0],
                 [0, 1, 2, 0, 0, 1],
                 [4, 4, 4, 4, 4, 4],
                 [0, 1, 0, 0, 0, 1]], dtype=np.uint8)


def test_hand_computed_example():
    ident = R.identity_matrix(HAND)
    assert ident.tolist() == [[6, 5, 3, 1, 2],
                              [5, 6, 4, 0, 3],
                              [3, 4, 6, 0, 5],
                              [1, 0, 0, 6, 0],
                              [2, 3, 5, 0, 6]]
    # T = 4: the similar pairs are (0,1), (1,2), (2,4): a chain 0 - 1 - 2 - 4, row 3 alone
    keep, rep = R.greedy_filter(ident, 4)
    assert keep.tolist() == [1, 0, 1, 1, 0] and rep.tolist() == [0, 0, 2, 3, 2]
    keep, rep = R.greedy_filter(ident, 4, [4, 3, 2, 1, 0])
    assert keep.tolist() == [0, 1, 0, 1, 1] and rep.tolist() == [1, 1, 4, 3, 4]
    assert R.components(ident, 4).tolist() == [0, 0, 0, 3, 0]
    assert R.degrees(ident, 4).tolist() == [2, 3, 3, 1, 2]
    # T = L + 1: nothing is similar, not even a row to itself
    keep, rep = R.greedy_filter(ident, 7)
    assert keep.all() and rep.tolist() == [0, 1, 2, 3, 4] and R.degrees(ident, 7).tolist() == [0] * 5
    assert R.components(ident, 7).tolist() == [0, 1, 2, 3, 4]
    # T = 1: rows 1 and 2 share no site with row 3, row 0 shares one: everything hangs together through row 0
    assert R.components(ident, 1).tolist() == [0] * 5
    keep, rep = R.greedy_filter(ident, 1)
    assert keep.tolist() == [1, 0, 0, 0, 0] and rep.tolist() == [0] * 5


@pytest.mark.parametrize("q,L,n", ((5, 33, 129), (21, 65, 200), (5, 1, 65), (21, 31, 63)))
def test_reference_against_independent_restatements(q, L, n):
    X, T = R.families(n, L, q, 77)
    ident = R.identity_matrix(X)
    assert np.array_equal(ident, ident.T) and (np.diag(ident) == L).all()
    k = np.random.default_rng(1).integers(0, n, size=(40, 2))
    assert all(ident[a, b] == int((X[a] == X[b]).sum()) for a, b in k)
    perm = np.random.default_rng(2).permutation(n)
    for t in sorted({1, T, L, L + 1}):
        for order in (None, perm, R.gap_order(X, q)):
            a, b = R.greedy_filter(ident, t, order), R.greedy_filter_rescan(ident, t, order)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(R.components(ident, t), R.components_closure(ident, t))


def test_path_fixture_is_one_component_of_full_diameter():
    for shuffled in (False, True):
        X = R.path(300, 100, 21, 90, 11, shuffled)              # the builder asserts the tridiagonal similarity itself
        ident = R.identity_matrix(X)
        assert (R.components(ident, 90) == 0).all()
        deg = R.degrees(ident, 90)
        assert sorted(np.bincount(deg).nonzero()[0].tolist()) == [2, 3] and (deg == 2).sum() == 2


# ---------------------------------------------------------------- the threshold rules
@pytest.mark.parametrize("L,identity,loose,strict", (
    (500, 0.9, 450, 451), (500, 1.0, 500, 501), (500, 0.8, 400, 401),
    (7, 0.9, 7, 7), (7, 3 / 7, 3, 4), (7, 1.0, 7, 8), (7, 0.5, 4, 4),
    (33, 0.8, 27, 27), (33, 1 / 3, 11, 12), (33, 0.7, 24, 24), (33, 1.0, 33, 34), (33, 1.5, 34, 34),
    (10, 0.1 * 3, 4, 4), (10, 0.3, 3, 4)))
def test_threshold_rules(L, identity, loose, strict):
    assert redundancy.identity_threshold(L, identity) == loose == R.threshold(L, identity)
    assert redundancy.identity_threshold(L, identity, strict=True) == strict == R.threshold(L, identity, True)
    # the definition once more in plain Python floats (IEEE double division)
    assert loose == next((k for k in range(L + 1) if k / L >= identity), L + 1)
    assert strict == next((k for k in range(L + 1) if k / L > identity), L + 1)
    assert redundancy.identity_threshold(L, identity, min_identical_sites=L + 1) == L + 1


# ---------------------------------------------------------------- the launch plan
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("redundancy_plan")), "redundancy_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "redundancy_plan_driver.cpp")])

    def run(groups):
        """groups: (n, q, envBlock, bitsCap) -> one dict per group"""
        out = []
        for ln in subprocess.check_output([exe] + [str(v) for g in groups for v in g]).decode().splitlines():
            tok = ln.split()
            out.append({k: int(v) for k, v in zip(tok[::2], tok[1::2])})
        return out
    return run


def test_launch_plan(plan):
    cases = [(1, 5, -1, -1), (63, 5, 64, -1), (64, 21, 64, -1), (65, 21, 64, -1), (200, 21, 64, -1), (700, 21, -1, -1), (700, 5, 192, -1),
             (700, 21, 100, -1), (50000, 21, -1, -1), (50000, 21, 100000, -1), (200000, 21, -1, -1), (700, 21, -1, 0), (300000, 21, -1, -1)]
    for (n, q, env, cap), p in zip(cases, plan(cases)):
        assert p["blockDefault"] == 2048 and p["blockMax"] == 8192 and p["capDefault"] == 8 << 30
        want = env if env > 0 else 2048
        want = min((min(want, 8192) + 63) // 64 * 64, (n + 63) // 64 * 64)
        assert p["B"] == want and p["B"] % 64 == 0 and p["blocks"] == -(-n // want) and p["W"] == want // 32
        tiles = 0
        for p0 in range(0, n, want):
            tq = -(-min(want, n - p0) // 64)
            tiles += tq * tq + tq * -(-p0 // 64)
        assert p["tilePairs"] == tiles
        assert p["ldsResolve"] == 4 * want <= 32768 and p["filterBits"] == want * want // 8
        # two staging buffers of 64 rows of 4 groups x padded planes + 2 dwords: 13 312 / 9 216 bytes of the 160 KiB
        assert p["ldsTile"] == (13312 if q > 8 else 9216)
        t = -(-n // 64)
        assert p["tiles"] == t and p["clusterW"] == 2 * t and p["allocDwords"] == 64 * t * 2 * t and p["units"] == 4 * t * t
        assert p["bitsBytes"] == n * -(-n // 32) * 4
        assert p["stored"] == int(p["bitsBytes"] <= ((8 << 30) if cap < 0 else cap))
        assert p["walkBlocks"] == (-(-t // 32)) ** 2 * 1024 < 2e9
    by_n = {c[0]: p for c, p in zip(cases, plan(cases)) if c[3] < 0 and c[2] < 0}
    assert by_n[50000]["bitsBytes"] == 312600000 and by_n[50000]["stored"] == 1            # config D: 0.31 GB
    assert by_n[200000]["bitsBytes"] == 5000000000 and by_n[200000]["stored"] == 1          # N = 200 000: 5 GB
    assert by_n[300000]["stored"] == 0                                                      # 11 GB: recomputed per round


# ---------------------------------------------------------------- the split's host logic
def test_split_on_given_labels():
    # clusters: {0..11} (12 rows: more than half of 20), {12, 13, 14}, {15, 16}, {17}, {18}, {19}
    labels = np.array([0] * 12 + [12] * 3 + [15] * 2 + [17, 18, 19], dtype=np.int32)
    for seed in range(8):
        for frac in (0.0, 0.05, 0.1, 0.25, 0.4):
            train, test = redundancy.split_by_labels(labels, frac, seed)
            assert np.array_equal(np.sort(np.concatenate([train, test])), np.arange(20))
            assert not set(labels[train]) & set(labels[test])                  # whole clusters only
            assert 0 not in test                                               # the cluster beyond half of n is skipped
            assert test.size >= frac * 20 and test.size <= 10
            assert np.array_equal(train, np.sort(train)) and np.array_equal(test, np.sort(test))
            again = redundancy.split_by_labels(labels, frac, seed)
            assert np.array_equal(again[0], train) and np.array_equal(again[1], test)
    # the order is that of the seeded permutation of the ascending labels; the loop stops at the first moment the side is full
    roots = np.array([0, 12, 15, 17, 18, 19])
    sizes = {0: 12, 12: 3, 15: 2, 17: 1, 18: 1, 19: 1}
    seq = roots[np.random.default_rng(3).permutation(6)]
    held, want = [], []
    for r in seq:
        if len(held) >= 0.25 * 20:
            break
        if len(held) + sizes[int(r)] > 10:
            continue
        held += np.nonzero(labels == r)[0].tolist()
        want.append(int(r))
    _train, test = redundancy.split_by_labels(labels, 0.25, 3)
    assert sorted(held) == test.tolist() and want
    assert redundancy.split_by_labels(labels, 0.0, 0)[1].size == 0
    summary = redundancy.cluster_summary(labels, rounds=2)
    assert summary["num_clusters"] == 6 and summary["sizes"] == sizes and summary["rounds"] == 2


# ---------------------------------------------------------------- the sub-commands through a stand-in
class StandIn:
    calls = []

    def __init__(self, msa_file, biomolecule, device=0):
        self.records = [("seq%d/1-4" % k, s) for k, s in enumerate(("ACDE", "ACDF", "AC-E", "WWWW"))]
        StandIn.calls.append(("init", msa_file, biomolecule, device))

    headers = property(lambda self: [h for h, _s in self.records])

    def filter(self, **kw):
        StandIn.calls.append(("filter", kw))
        return np.array([0, 3]), np.array([0, 0, 0, 3], dtype=np.int32)

    def clusters(self, **kw):
        StandIn.calls.append(("clusters", kw))
        return dict(labels=np.array([0, 0, 0, 3], dtype=np.int32), num_clusters=2, sizes={0: 3, 3: 1}, rounds=2,
                    degrees=np.array([3, 2, 2, 1], dtype=np.int32))

    def split(self, **kw):
        StandIn.calls.append(("split", kw))
        return np.array([0, 1, 2]), np.array([3])

    def write_fasta(self, path, indices):
        redundancy.write_fasta(path, self.records, indices)


def test_sub_commands_through_a_stand_in(monkeypatch, tmp_path):
    monkeypatch.setattr(redundancy, "AlignmentRedundancy", StandIn)
    monkeypatch.chdir(tmp_path)
    StandIn.calls = []
    out = main.run_pydca(["filter_by_identity", "protein", "some/dir/fam.fa", "--identity", "0.95", "--priority", "fewest_gaps", "--strict"])
    assert out == [os.path.join("Filtered_fam", "Filtered_fam.fa"), os.path.join("Filtered_fam", "Filtered_fam_representatives.txt")]
    assert StandIn.calls == [("init", "some/dir/fam.fa", "protein", 0),
                             ("filter", dict(identity=0.95, priority="fewest_gaps", strict=True, return_representatives=True))]
    assert open(out[0]).read() == ">seq0/1-4\nACDE\n>seq3/1-4\nWWWW\n"
    assert [ln.split("\t") for ln in open(out[1]).read().splitlines()[1:]] == [
        ["0", "seq0/1-4", "0"], ["1", "seq1/1-4", "0"], ["2", "seq2/1-4", "0"], ["3", "seq3/1-4", "3"]]
    StandIn.calls = []
    out = main.run_pydca(["cluster_sequences", "rna", "fam.fa", "--output_dir", str(tmp_path / "here"), "--device", "2"])
    assert out == [str(tmp_path / "here" / "Clusters_fam.txt")]
    assert StandIn.calls == [("init", "fam.fa", "rna", 2), ("clusters", dict(identity=0.8, strict=False, return_degrees=True))]
    rows = [ln.split("\t") for ln in open(out[0]).read().splitlines() if not ln.startswith("#")]
    assert rows == [["0", "seq0/1-4", "0", "3", "3"], ["1", "seq1/1-4", "0", "3", "2"], ["2", "seq2/1-4", "0", "3", "2"],
                    ["3", "seq3/1-4", "3", "1", "1"]]
    StandIn.calls = []
    out = main.run_pydca(["split_by_clusters", "protein", "fam.fa", "--identity", "0.7", "--test_fraction", "0.25", "--seed", "5"])
    assert out == [os.path.join("Split_fam", "Train_fam.fa"), os.path.join("Split_fam", "Test_fam.fa")]
    assert StandIn.calls[1] == ("split", dict(identity=0.7, test_fraction=0.25, seed=5, strict=False))
    assert open(out[1]).read() == ">seq3/1-4\nWWWW\n" and open(out[0]).read().count(">") == 3
    # defaults of the three parsers
    StandIn.calls = []
    main.run_pydca(["filter_by_identity", "protein", "fam.fa"])
    main.run_pydca(["split_by_clusters", "protein", "fam.fa"])
    assert StandIn.calls[1] == ("filter", dict(identity=0.9, priority="file", strict=False, return_representatives=True))
    assert StandIn.calls[3] == ("split", dict(identity=0.8, test_fraction=0.1, seed=0, strict=False))
    with pytest.raises(SystemExit):
        main.run_pydca(["filter_by_identity", "protein", "fam.fa", "--priority", "longest"])
    # the trimming sub-commands still parse as before
    with pytest.raises(SystemExit):
        main.run_pydca(["trim_by_gap_size"])


# ---------------------------------------------------------------- fixture conditions of the GPU cases
@pytest.mark.parametrize("L", (31, 32, 33, 64, 65, 100))
@pytest.mark.parametrize("q", (5, 21))
def test_fixture_conditions_of_the_gpu_grid(q, L):
    for n in (63, 64, 65, 129, 700, 128, 200):
        X, T = R.families(n, L, q, 1000 * n + 10 * L + q)            # the seeds of tests/test_redundancy.py::family_case
        assert T == R.fixture_T(L) and 1 < T < L
        c = R.fixture_conditions(X, T)
        assert 0.1 < c["kept_fraction"] < 0.9, (q, L, n, c)
        assert c["at_T"] and c["below_T"] and c["chain"] and c["late_representative"], (q, L, n, c)


@pytest.mark.parametrize("q,L", ((5, 33), (21, 65)))
def test_fixture_conditions_of_the_block_and_order_cases(q, L):
    n = 200
    X, T = R.families(n, L, q, 1000 * n + 10 * L + q)
    ident = R.identity_matrix(X)
    keep, rep = R.greedy_filter(ident, T)
    back = np.arange(n) // 64 - rep // 64                   # blocks of 64: the representative in the same block, one, two back
    assert {0, 1, 2} <= set(back[keep == 0].tolist())
    n = 700
    X, T = R.families(n, L, q, 1000 * n + 10 * L + q)
    ident = R.identity_matrix(X)
    perm = np.random.default_rng(3).permutation(n)
    for order in (perm, R.gap_order(X, q)):
        c = R.fixture_conditions(X, T, order)
        assert 0.1 < c["kept_fraction"] < 0.9 and c["late_representative"]
    assert not np.array_equal(R.greedy_filter(ident, T, perm)[0], R.greedy_filter(ident, T)[0])
    assert not np.array_equal(R.gap_order(X, q), np.arange(n))


def test_fixture_conditions_of_the_real_alignment():
    from conftest import data_file
    from pydca_amd.msa_trimmer.msa_trimmer import read_fasta_records
    recs = read_fasta_records(data_file("PF02826.faa"))
    X = _lib.encode_sequences([r.seq.upper() for r in recs], _lib.PROTEIN, len(recs[0].seq), 1)
    ident = R.identity_matrix(X)
    L = X.shape[1]
    for identity in (0.9, 0.8):
        T = R.threshold(L, identity)
        keep, _rep = R.greedy_filter(ident, T)
        lab = R.components(ident, T)
        assert 0 < (keep == 0).sum() and np.unique(lab).size < X.shape[0] and np.bincount(lab).max() >= 3
