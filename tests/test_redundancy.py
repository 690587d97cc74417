"""Redundancy filter and identity clusters on the GPU (dca_identity_filter, dca_identity_clusters, pydca_amd/redundancy.py and
the three sub-commands) against the numpy reference of tests/redundancy_reference.py.  Integer work:
every comparison is np.array_equal.  tests/test_redundancy_host.py asserts on the CPU that the fixtures used here hold similar
pairs at exactly T, non-similar pairs at T - 1, chains and late representatives, so that no case passes vacuously.

Rounds of the component search observed on the path fixtures (n = 300; see test_path_fixtures): recorded in DESIGN.md
section 29."""
import functools
import os

import numpy as np
import pytest

import redundancy_reference as R
from conftest import data_file
from pydca_amd import _lib, main, redundancy
from pydca_amd.msa_trimmer.msa_trimmer import read_fasta_records

pytestmark = pytest.mark.gpu

GRID_Q = (5, 21)
GRID_L = (1, 31, 32, 33, 64, 65, 100)
GRID_N = (1, 2, 63, 64, 65, 129, 700)

_contexts = {}


def context(q, L):
    """One context per (q, L): the entries take L and q from its alignment, the rows under test are passed as X"""
    if (q, L) not in _contexts:
        ctx = _lib.Context(0, _lib.DCA_F64)
        ctx.set_msa(R.isolated(3, L, q, 5), q)
        _contexts[(q, L)] = ctx
    return _contexts[(q, L)]


@pytest.fixture(scope="module", autouse=True)
def close_contexts():
    yield
    for ctx in _contexts.values():
        ctx.close()
    _contexts.clear()


@functools.lru_cache(maxsize=None)
def family_case(q, L, n):
    X, T = R.families(n, L, q, 1000 * n + 10 * L + q)
    ident = R.identity_matrix(X)
    ident.setflags(write=False)
    X.setflags(write=False)
    return X, T, ident


def check_filter(ctx, X, ident, T, order=None, what=""):
    keep, rep, info = ctx.identity_filter(T, X, order)
    k_ref, r_ref = R.greedy_filter(ident, T, order)
    assert np.array_equal(keep, k_ref), (what, "keep")
    assert np.array_equal(rep, r_ref), (what, "rep")
    assert info["kept"] == int(k_ref.sum()), (what, "kept")
    return keep, rep, info


def check_clusters(ctx, X, ident, T, what=""):
    label, degree, info = ctx.identity_clusters(T, X)
    l_ref = R.components(ident, T)
    assert np.array_equal(label, l_ref), (what, "label")
    assert np.array_equal(degree, R.degrees(ident, T)), (what, "degree")
    assert info["clusters"] == np.unique(l_ref).size and info["largest"] == np.bincount(l_ref).max(), (what, "count")
    assert info["rounds"] >= 1
    return label, degree, info


# ---------------------------------------------------------------- 1. the grid: plane counts, group edges, tile edges, thresholds
@pytest.mark.parametrize("n", GRID_N)
@pytest.mark.parametrize("L", GRID_L)
@pytest.mark.parametrize("q", GRID_Q)
def test_filter_and_clusters_on_the_grid(q, L, n):
    X, T, ident = family_case(q, L, n)
    ctx = context(q, L)
    for t in sorted({1, T, L, L + 1}):
        check_filter(ctx, X, ident, t, what=(q, L, n, t))
        check_clusters(ctx, X, ident, t, what=(q, L, n, t))


# ---------------------------------------------------------------- 2. block edges of the filter
@pytest.mark.parametrize("n", (63, 64, 65, 128, 129, 200))
@pytest.mark.parametrize("q,L", ((5, 33), (21, 65)))
def test_filter_block_edges(monkeypatch, q, L, n):
    monkeypatch.setenv("DCA_FILTER_BLOCK", "64")
    X, T, ident = family_case(q, L, n)
    _keep, rep, info = check_filter(context(q, L), X, ident, T, what=(q, L, n))
    assert info["block_rows"] == 64 and info["blocks"] == (n + 63) // 64
    if n == 200:            # the covering representative: in the same block, in the one before, two or more back
        back = np.arange(n) // 64 - rep // 64
        assert {0, 1, 2} <= set(back[rep != np.arange(n)].tolist())


@pytest.mark.parametrize("q,L", ((5, 33), (21, 100)))
def test_filter_does_not_depend_on_the_block(monkeypatch, q, L):
    X, T, ident = family_case(q, L, 700)
    ctx = context(q, L)
    monkeypatch.delenv("DCA_FILTER_BLOCK", raising=False)
    k0, r0, i0 = check_filter(ctx, X, ident, T)
    assert i0["block_rows"] == 704 and i0["blocks"] == 1          # the default block, capped by n rounded up to 64
    for block in (64, 192):
        monkeypatch.setenv("DCA_FILTER_BLOCK", str(block))
        k, r, i = ctx.identity_filter(T, X)
        assert i["block_rows"] == block and i["blocks"] == (700 + block - 1) // block
        assert np.array_equal(k, k0) and np.array_equal(r, r0), block


# ---------------------------------------------------------------- 3. priority orders
@pytest.mark.parametrize("q,L", ((5, 33), (21, 65)))
def test_filter_orders(monkeypatch, q, L):
    monkeypatch.setenv("DCA_FILTER_BLOCK", "128")
    n = 700
    X, T, ident = family_case(q, L, n)
    ctx = context(q, L)
    perm = np.random.default_rng(3).permutation(n).astype(np.int32)
    k_perm, r_perm, _ = check_filter(ctx, X, ident, T, perm, "permutation")
    gaps = R.gap_order(X, q)
    check_filter(ctx, X, ident, T, gaps, "fewest_gaps")
    k_none, r_none, _ = check_filter(ctx, X, ident, T, None)
    k_id, r_id, _ = ctx.identity_filter(T, X, np.arange(n, dtype=np.int32))
    assert np.array_equal(k_id, k_none) and np.array_equal(r_id, r_none)
    assert not np.array_equal(k_perm, k_none)                       # the order matters on this fixture
    # the module functions: the same through the public interface
    kept, rep = redundancy.filter(X, q, min_identical_sites=T, priority="fewest_gaps", return_representatives=True)
    k_ref, r_ref = R.greedy_filter(ident, T, gaps)
    assert np.array_equal(kept, np.nonzero(k_ref)[0]) and np.array_equal(rep, r_ref)
    kept = redundancy.filter(X, q, min_identical_sites=T, priority=perm)
    assert np.array_equal(kept, np.nonzero(k_perm)[0])
    with pytest.raises(_lib.DcaBackendError) as exc:                # not a permutation: refused by the library too
        ctx.identity_filter(T, X, np.zeros(n, dtype=np.int32))
    assert exc.value.code == _lib.DCA_ERR_ARG


# ---------------------------------------------------------------- 4. both cluster paths
@pytest.mark.parametrize("n", (65, 700))
@pytest.mark.parametrize("q,L", ((5, 33), (21, 100)))
def test_cluster_paths_agree(monkeypatch, q, L, n):
    X, T, ident = family_case(q, L, n)
    ctx = context(q, L)
    monkeypatch.delenv("DCA_CLUSTER_BITS_MAX", raising=False)
    l1, d1, i1 = check_clusters(ctx, X, ident, T, "stored")
    monkeypatch.setenv("DCA_CLUSTER_BITS_MAX", "0")
    l0, d0, i0 = check_clusters(ctx, X, ident, T, "recomputed")
    assert i1["stored_bits"] == 1 and i0["stored_bits"] == 0
    assert np.array_equal(l0, l1) and np.array_equal(d0, d1)


# ---------------------------------------------------------------- 5. path fixtures: one component of diameter n - 1
@pytest.mark.parametrize("bits_max", (None, "0"))
@pytest.mark.parametrize("shuffled", (False, True))
def test_path_fixtures(monkeypatch, shuffled, bits_max):
    if bits_max is None:
        monkeypatch.delenv("DCA_CLUSTER_BITS_MAX", raising=False)
    else:
        monkeypatch.setenv("DCA_CLUSTER_BITS_MAX", bits_max)
    q, L, n, T = 21, 100, 300, 90
    X = R.path(n, L, q, T, 11, shuffled)
    label, degree, info = context(q, L).identity_clusters(T, X)
    print("path fixture n=%d shuffled=%s stored_bits=%d: rounds %d" % (n, shuffled, info["stored_bits"], info["rounds"]))
    assert np.array_equal(label, np.zeros(n, dtype=np.int32))
    assert info["clusters"] == 1 and info["largest"] == n and info["rounds"] >= 1
    assert np.array_equal(degree, R.degrees(R.identity_matrix(X), T))
    assert sorted(np.bincount(degree).nonzero()[0].tolist()) == [2, 3]          # two ends, n - 2 inner rows


def test_duplicates_and_isolated_rows():
    q, L, n = 21, 65, 129
    ctx = context(q, L)
    X = R.duplicates(n, L, q, 4)
    ident = R.identity_matrix(X)
    keep, _rep, _ = check_filter(ctx, X, ident, L)                  # identity 1.0: exact duplicates go
    assert keep.sum() == 43
    _l, _d, info = check_clusters(ctx, X, ident, L)
    assert info["clusters"] == 43 and info["largest"] == 3
    X = R.isolated(n, L, q, 6)
    ident = R.identity_matrix(X)
    keep, rep, _ = check_filter(ctx, X, ident, R.fixture_T(L))
    assert keep.all() and np.array_equal(rep, np.arange(n))
    label, degree, _ = check_clusters(ctx, X, ident, R.fixture_T(L))
    assert np.array_equal(label, np.arange(n)) and (degree == 1).all()


# ---------------------------------------------------------------- 6. independent oracles already in the library
@pytest.mark.parametrize("q,L,n", ((5, 33, 700), (21, 100, 700)))
def test_degrees_are_the_weight_counts(q, L, n):
    X, _T, ident = family_case(q, L, n)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    for seqid in (0.8, 0.875):
        ctx.compute_weights(seqid, _lib.DCA_F64)
        T = redundancy.identity_threshold(L, seqid, strict=True)
        assert T == R.threshold(L, seqid, strict=True)
        _label, degree, _ = ctx.identity_clusters(T)               # X NULL: the context's alignment
        # weights_count_kernel counts the row itself (its diagonal tiles compare k with k), as degree_out does
        assert np.array_equal(degree.astype(np.uint32), ctx.weight_counts())
        assert np.array_equal(degree, R.degrees(ident, T))
    ctx.close()


@pytest.mark.parametrize("q,L,n", ((5, 33, 700), (21, 100, 700)))
def test_kept_rows_and_split_sides_are_far_apart(q, L, n):
    X, T, _ident = family_case(q, L, n)
    ctx = context(q, L)
    keep, _rep, _ = ctx.identity_filter(T, X)
    K = X[keep.astype(bool)]
    dist, _i, _h = ctx.hamming_nearest(None, K, True, return_index=False, return_histogram=False)
    assert (dist > L - T).all()
    train, test = redundancy.split(X, q, identity=T / L, test_fraction=0.2, seed=1)
    assert redundancy.identity_threshold(L, T / L) == T
    assert test.size >= 0.2 * n and np.array_equal(np.sort(np.concatenate([train, test])), np.arange(n))
    dist, _i, _h = ctx.hamming_nearest(X[test], X[train], False, return_index=False, return_histogram=False)
    assert (dist > L - T).all()


# ---------------------------------------------------------------- 7. no dependence on the rest of the context
def test_host_rows_and_the_context_alignment_agree_and_the_model_stays():
    q, L, n = 5, 33, 700
    X, T, ident = family_case(q, L, n)
    bare = _lib.Context(0, _lib.DCA_F64)
    bare.set_msa(X, q)
    full = _lib.Context(0, _lib.DCA_F64)
    full.set_msa(X, q)
    w = full.compute_weights(0.8, _lib.DCA_F64)
    scores = full.mf_run(0.5, True)
    order = R.gap_order(X, q)
    results = []
    for ctx, rows in ((bare, X), (bare, None), (full, X), (full, None), (context(q, L), X)):
        k, r, _ = ctx.identity_filter(T, rows, order)
        l, d, _ = ctx.identity_clusters(T, rows)
        results.append((k, r, l, d))
    k_ref, r_ref = R.greedy_filter(ident, T, order)
    for k, r, l, d in results:
        assert np.array_equal(k, k_ref) and np.array_equal(r, r_ref)
        assert np.array_equal(l, R.components(ident, T)) and np.array_equal(d, R.degrees(ident, T))
    assert np.array_equal(full.weights(), w)
    assert np.array_equal(full.mf_scores(True), scores)
    bare.close()
    full.close()


def test_refusals_on_the_device():
    q, L = 5, 33
    X, T, _ = family_case(q, L, 65)
    ctx = context(q, L)

    def code(call):
        with pytest.raises(_lib.DcaBackendError) as exc:
            call()
        return exc.value.code
    fresh = _lib.Context(0, _lib.DCA_F64)
    assert code(lambda: _lib.check(fresh._l.dca_identity_filter(fresh._h, _lib._ptr(X), 65, T, None, _lib._ptr(np.zeros(65, np.uint8)), None,
                                                                None))) == _lib.DCA_ERR_STATE
    assert code(lambda: _lib.check(fresh._l.dca_identity_clusters(fresh._h, _lib._ptr(X), 65, T, _lib._ptr(np.zeros(65, np.int32)), None,
                                                                  None))) == _lib.DCA_ERR_STATE
    fresh.close()
    for bad_T in (0, L + 2, -1):
        assert code(lambda: ctx.identity_filter(bad_T, X)) == _lib.DCA_ERR_ARG
        assert code(lambda: ctx.identity_clusters(bad_T, X)) == _lib.DCA_ERR_ARG
    bad = np.array(X)
    bad[64, 32] = q
    assert code(lambda: ctx.identity_filter(T, bad)) == _lib.DCA_ERR_ARG
    assert code(lambda: ctx.identity_clusters(T, bad)) == _lib.DCA_ERR_ARG
    assert code(lambda: _lib.check(ctx._l.dca_identity_filter(ctx._h, _lib._ptr(X), 0, T, None, _lib._ptr(np.zeros(65, np.uint8)), None, None))) \
        == _lib.DCA_ERR_ARG
    assert code(lambda: _lib.check(ctx._l.dca_identity_filter(ctx._h, _lib._ptr(X), 65, T, None, None, None, None))) == _lib.DCA_ERR_ARG
    assert code(lambda: _lib.check(ctx._l.dca_identity_clusters(ctx._h, _lib._ptr(X), 65, T, None, None, None))) == _lib.DCA_ERR_ARG
    keep, _r, _i = ctx.identity_filter(L + 1, X)                    # L + 1 is accepted: nothing is similar, not even a row to itself
    assert keep.all()
    _l, degree, info = ctx.identity_clusters(L + 1, X)
    assert (degree == 0).all() and info["clusters"] == 65


# ---------------------------------------------------------------- 8. end to end on a real alignment
@pytest.fixture(scope="module")
def pf02826():
    path = data_file("PF02826.faa")
    records = read_fasta_records(path)
    red = redundancy.AlignmentRedundancy(path, "protein")
    ident = R.identity_matrix(red.X)
    yield path, records, red, ident
    red.close()


def read_back(path):
    return [(r.id, r.seq) for r in read_fasta_records(path)]


def test_alignment_redundancy_class(pf02826):
    path, records, red, ident = pf02826
    L = red.sequences_len
    assert red.num_sequences == len(records) == 2030 and red.headers == [r.id for r in records]
    for identity, strict in ((0.9, False), (0.8, True), (1.0, False)):
        T = R.threshold(L, identity, strict)
        kept, rep = red.filter(identity=identity, strict=strict, return_representatives=True)
        k_ref, r_ref = R.greedy_filter(ident, T)
        assert np.array_equal(kept, np.nonzero(k_ref)[0]) and np.array_equal(rep, r_ref)
        res = red.clusters(identity=identity, strict=strict, return_degrees=True)
        l_ref = R.components(ident, T)
        assert np.array_equal(res["labels"], l_ref) and np.array_equal(res["degrees"], R.degrees(ident, T))
        assert res["num_clusters"] == np.unique(l_ref).size and sum(res["sizes"].values()) == 2030
    order = R.gap_order(red.X, 21)
    kept = red.filter(identity=0.9, priority="fewest_gaps")
    assert np.array_equal(kept, np.nonzero(R.greedy_filter(ident, R.threshold(L, 0.9), order)[0])[0])


def test_sub_commands_write_what_the_reference_gives(pf02826, tmp_path):
    path, records, red, ident = pf02826
    L = red.sequences_len
    all_records = [(r.id, r.seq) for r in records]
    # filter_by_identity
    out = main.run_pydca(["filter_by_identity", "protein", path, "--identity", "0.9", "--priority", "fewest_gaps",
                          "--output_dir", str(tmp_path / "f")])
    assert [os.path.basename(f) for f in out] == ["Filtered_PF02826.fa", "Filtered_PF02826_representatives.txt"]
    T = R.threshold(L, 0.9)
    k_ref, r_ref = R.greedy_filter(ident, T, R.gap_order(red.X, 21))
    assert read_back(out[0]) == [all_records[k] for k in np.nonzero(k_ref)[0]]           # original headers, original order
    rows = [ln.rstrip("\n").split("\t") for ln in open(out[1]) if not ln.startswith("#")]
    assert [int(r[0]) for r in rows] == list(range(2030)) and [r[1] for r in rows] == red.headers
    assert np.array_equal(np.array([int(r[2]) for r in rows]), r_ref)
    # cluster_sequences
    out = main.run_pydca(["cluster_sequences", "protein", path, "--identity", "0.8", "--strict", "--output_dir", str(tmp_path / "c")])
    assert [os.path.basename(f) for f in out] == ["Clusters_PF02826.txt"]
    T = R.threshold(L, 0.8, strict=True)
    l_ref = R.components(ident, T)
    rows = [ln.rstrip("\n").split("\t") for ln in open(out[0]) if not ln.startswith("#")]
    assert [r[1] for r in rows] == red.headers
    assert np.array_equal(np.array([int(r[2]) for r in rows]), l_ref)
    assert np.array_equal(np.array([int(r[3]) for r in rows]), np.bincount(l_ref)[l_ref])
    assert np.array_equal(np.array([int(r[4]) for r in rows]), R.degrees(ident, T))
    # split_by_clusters
    out = main.run_pydca(["split_by_clusters", "protein", path, "--identity", "0.8", "--test_fraction", "0.1", "--seed", "0",
                          "--output_dir", str(tmp_path / "s")])
    assert [os.path.basename(f) for f in out] == ["Train_PF02826.fa", "Test_PF02826.fa"]
    train, test = read_back(out[0]), read_back(out[1])
    tr_ref, te_ref = redundancy.split_by_labels(R.components(ident, R.threshold(L, 0.8)), 0.1, 0)
    assert train == [all_records[k] for k in tr_ref] and test == [all_records[k] for k in te_ref]
    assert len(test) >= 203 and not set(train) & set(test) and sorted(train + test) == sorted(all_records)
    # the guarantee: no test row is similar to any train row
    assert (ident[np.ix_(te_ref, tr_ref)] < R.threshold(L, 0.8)).all()
