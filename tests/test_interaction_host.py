"""Host checks of the inter-protein energies and the assignment solver: the float64 restatement of
tests/interaction_reference.py against the same sums in longdouble and against full Potts energies, the gauge's row-plus-column
structure, pydca_amd/csrc/interaction_plan.h through its driver (LDS budgets, and that the GPU test's case table reaches every
branch of the plan), and pydca_amd/csrc/assignment.h compiled alone against exhaustive search."""
import subprocess

import numpy as np
import pytest

import interaction_drivers as D
import interaction_reference as R

ALPHABETS = [2, 5, 21, 32]
LDS_PER_WORKGROUP = 160 * 1024 // 2                    # two workgroups per CU


def random_model(L, q, seed, sigma=0.7):
    rng = np.random.default_rng([seed, L, q])
    return rng.normal(0, sigma, (L, q)), rng.normal(0, sigma, (L * (L - 1) // 2, q, q))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return D.compile_plan_driver(tmp_path_factory.mktemp("interactionplan"))


@pytest.fixture(scope="module")
def solve(tmp_path_factory):
    return D.compile_assignment_driver(tmp_path_factory.mktemp("assignment"))


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("q", ALPHABETS)
@pytest.mark.parametrize("gauge", [0, 1])
def test_restatement_against_longdouble(q, gauge):
    """the double sums against the longdouble sums of the same (double) addends, within (LA + LB) 2^-53 sum |addends|"""
    LA, LB = 6, 7
    _h, Jp = random_model(LA + LB, q, 1)
    rng = np.random.default_rng(q)
    XA, XB = rng.integers(0, q, (40, LA)), rng.integers(0, q, (50, LB))
    Jt = R.cross_couplings(Jp, LA + LB, LA, gauge)
    E = R.cross_energies(R.cross_fields(Jt, XA), XB)
    El = R.cross_energies(R.cross_fields(Jt.astype(np.longdouble), XA), XB)
    bound = R.sum_bound(Jt, XA, XB)
    err = np.abs(E.astype(np.longdouble) - El).astype(np.float64)
    print("q %d gauge %d: largest error %.3g, bound there %.3g" % (q, gauge, err.max(), bound.ravel()[err.argmax()]))
    assert np.all(err <= bound)
    # grouped = the dense array's blocks
    oa, ob = np.array([0, 0, 13, 40]), np.array([0, 9, 9, 50])
    blocks = R.interaction_energies(Jp, LA + LB, LA, XA, XB, gauge, oa, ob)
    assert [b.shape for b in blocks] == [(0, 9), (13, 0), (27, 41)]
    assert blocks[2].tobytes() == np.ascontiguousarray(E[13:, 9:]).tobytes()


@pytest.mark.parametrize("q", [5, 21])
def test_four_energy_identity_in_longdouble(q):
    """gauge 0: E(a,b) - E(a,b') - E(a',b) + E(a',b') equals the same combination of full energies of the concatenated rows"""
    LA, LB = 5, 4
    L = LA + LB
    h, Jp = random_model(L, q, 2)
    rng = np.random.default_rng(q)
    XA, XB = rng.integers(0, q, (9, LA)), rng.integers(0, q, (8, LB))
    X = R.interaction_energies(Jp, L, LA, XA, XB, 0, dtype=np.longdouble)
    cat = np.concatenate([np.repeat(XA, 8, axis=0), np.tile(XB, (9, 1))], axis=1)
    F, sabs = R.full_energies(h, Jp, cat)
    F, sabs = F.reshape(9, 8), sabs.reshape(9, 8)

    def comb(M):
        return M[:-1, :-1] - M[:-1, 1:] - M[1:, :-1] + M[1:, 1:]
    eps = np.finfo(np.longdouble).eps
    T = L + L * (L - 1) // 2
    bound = T * eps * (sabs[:-1, :-1] + sabs[:-1, 1:] + sabs[1:, :-1] + sabs[1:, 1:])
    assert np.all(np.abs(comb(X) - comb(F)) <= bound)


@pytest.mark.parametrize("q", ALPHABETS)
def test_gauges_differ_by_row_and_column_terms(q):
    """E1(m, n) - E0(m, n) = f(m) + g(n): the double difference of the difference vanishes, and the best assignment of a square
    block is the same in both gauges"""
    LA, LB = 6, 7
    _h, Jp = random_model(LA + LB, q, 3)
    rng = np.random.default_rng(q)
    XA, XB = rng.integers(0, q, (6, LA)), rng.integers(0, q, (6, LB))
    E0 = R.interaction_energies(Jp, LA + LB, LA, XA, XB, 0, dtype=np.longdouble)
    E1 = R.interaction_energies(Jp, LA + LB, LA, XA, XB, 1, dtype=np.longdouble)
    diff = E1 - E0
    mixed = diff[:-1, :-1] - diff[:-1, 1:] - diff[1:, :-1] + diff[1:, 1:]
    scale = np.abs(R.addend_sums(R.cross_couplings(Jp, LA + LB, LA, 0), XA, XB)).max()
    assert np.abs(mixed).max() <= 64 * (LA * LB) * np.finfo(np.longdouble).eps * scale
    c0, t0, g0 = R.brute_assign_with_gaps(E0.astype(np.float64))
    c1, t1, g1 = R.brute_assign_with_gaps(E1.astype(np.float64))
    assert g0.min() > 1e-9 * scale                     # a condition on the inputs: the optimum is unique
    assert np.array_equal(c0, c1)
    assert np.allclose(g0, g1, rtol=0, atol=1e-9 * float(scale))


# ---------------------------------------------------------------- 2. the plan
@pytest.mark.parametrize("q", ALPHABETS)
def test_plan_budgets(plan, q):
    p = plan(q, 250)
    assert p["threads"] == 256 and p["qm"] >= q and p["qm"] % 2 == 0
    assert p["field_chunk"] >= 1 and p["field_chunk"] * q * q <= p["threads"] * p["field_regs"]
    assert p["field_lds"] == 2 * p["field_chunk"] * q * p["qm"] * 8 + p["field_chunk"] * (2 * q + 1) * 8
    assert p["field_lds"] <= LDS_PER_WORKGROUP
    assert p["item_pairs"] == p["threads"] * p["slots"] == p["dense_rows"] * p["window"]
    assert p["phi_lds"] + 1024 <= LDS_PER_WORKGROUP
    for rows, chunk in ((p["dense_rows"], p["chunk_dense"]), (p["sparse_rows"], p["chunk_sparse"])):
        assert 1 <= chunk <= 250 and rows * chunk * q * 8 <= p["phi_lds"]
    assert p["sparse_rows"] * p["single_tile_sparse"] * q * 8 <= p["phi_lds"] < p["sparse_rows"] * (p["single_tile_sparse"] + 1) * q * 8
    assert p["pass_budget"] == 1 << 30


def item_facts(plan, q, LB, groups):
    """what the items of one call look like: the set of branch names they reach"""
    cnt = R.row_counts(groups)
    p = plan(q, LB, cnt)
    seen = set()
    covered = np.zeros(len(cnt), dtype=np.int64)
    for a0, na, k0, chunk in p["items"]:
        assert 1 <= na <= p["sparse_rows"] and a0 + na <= len(cnt)
        pairs = sum(max(0, min(p["window"], cnt[a0 + r] - k0)) for r in range(na))
        assert 0 < pairs <= p["item_pairs"]
        assert na * chunk * q * 8 <= p["phi_lds"]
        for r in range(na):
            covered[a0 + r] += max(0, min(p["window"], cnt[a0 + r] - k0))
        if cnt[a0] > p["window"]:
            seen.add("dense")
            assert na <= p["dense_rows"]
            if k0 > 0:
                seen.add("dense_second_window")
            if cnt[a0] - k0 < p["window"]:
                seen.add("dense_partial_window")
        else:
            seen.add("sparse")
            assert k0 == 0
            if len(set(groups_of_rows(groups)[a0:a0 + na])) > 1:
                seen.add("sparse_several_groups")
            if na == p["sparse_rows"]:
                seen.add("sparse_row_limit")
            elif a0 + na < len(cnt) and 0 < cnt[a0 + na] <= p["window"] and pairs + cnt[a0 + na] > p["item_pairs"]:
                seen.add("sparse_pair_limit")
            if any(cnt[a0 + r] == 0 for r in range(na)):
                seen.add("sparse_empty_row")
        seen.add("one_chunk" if chunk >= LB else "several_chunks")
        if pairs > p["threads"]:
            seen.add("several_slots")
    assert covered.tolist() == cnt                      # every pair exactly once
    return seen


def groups_of_rows(groups):
    return [g for g, (a, _b) in enumerate(groups) for _ in range(a)]


@pytest.mark.parametrize("q", ALPHABETS)
def test_case_table_reaches_every_branch(plan, q):
    p = plan(q, 1)
    seen, field = set(), set()
    for LA, LB, groups in R.energy_cases(plan, q):
        seen |= item_facts(plan, q, LB, groups)
        steps = -(-LA // p["field_chunk"])
        field.add("one_staging_chunk" if steps == 1 else "several_staging_chunks")
        if LA % p["field_chunk"]:
            field.add("partial_staging_chunk")
        if steps > 1 and LA % p["field_chunk"] == 0:
            field.add("full_last_chunk")
        sizes = {a for a, _ in groups} | {b for _, b in groups}
        if (LA, LB) == (6, 7):
            assert {0, 1, 63, 64, 65, 257} <= sizes and {0, 1, 63, 64, 65, 257} <= {a for a, _ in groups} and \
                {0, 1, 63, 64, 65, 257} <= {b for _, b in groups}
    assert seen == {"dense", "dense_second_window", "dense_partial_window", "sparse", "sparse_several_groups", "sparse_row_limit",
                    "sparse_pair_limit", "sparse_empty_row", "one_chunk", "several_chunks", "several_slots"}, seen
    assert field == {"one_staging_chunk", "several_staging_chunks", "partial_staging_chunk", "full_last_chunk"}, field
    # the two plan-dependent shapes are what the issue asks for
    cases = R.energy_cases(plan, q)
    assert any(LB == p["single_tile_dense"] + 1 for _LA, LB, _g in cases) and any(LA == p["field_chunk"] + 1 for LA, _LB, _g in cases)
    # several blocks under DCA_CROSS_PASS, and the 1 GiB budget alone at the timing shape
    assert len(plan(q, 7, R.row_counts(R.MAIN_GROUPS), cross_pass=37)["blocks"]) > 1
    assert plan(q, 7, R.row_counts(R.MAIN_GROUPS))["blocks"] == [len(R.row_counts(R.MAIN_GROUPS))]


# ---------------------------------------------------------------- 3. the assignment solver
def all_shapes(limit=6):
    return [(nr, nc) for nr in range(1, limit + 1) for nc in range(1, limit + 1)]


def test_assignment_continuous_entries(solve):
    rng = np.random.default_rng(0)
    problems = [rng.normal(size=shape) for shape in all_shapes() for _ in range(3)]
    for E, (rc, total, cols, gaps) in zip(problems, solve(problems)):
        bc, bt, bg = R.brute_assign_with_gaps(E)
        assert rc == 0 and np.array_equal(cols, bc), E.shape           # the optimum is unique
        assert abs(total - bt) <= 1e-13 * np.abs(E).sum()
        fin = np.isfinite(bg)
        assert np.array_equal(np.isfinite(gaps), fin) and np.all(gaps >= 0)
        assert np.allclose(gaps[fin], bg[fin], rtol=0, atol=1e-13 * np.abs(E).sum())
        assert np.all(gaps[cols < 0] == 0)


def test_assignment_integer_entries_with_ties(solve):
    rng = np.random.default_rng(1)
    problems = [rng.integers(0, 4, size=shape).astype(np.float64) for shape in all_shapes() for _ in range(3)]
    for E, (rc, total, cols, gaps) in zip(problems, solve(problems)):
        nr, nc = E.shape
        assert rc == 0 and (cols >= 0).sum() == min(nr, nc)
        used = cols[cols >= 0]
        assert len(set(used.tolist())) == used.size and np.all(used < nc)
        assert total == sum(E[r, c] for r, c in enumerate(cols) if c >= 0)
        bt, _ = R.brute_assignment(E)
        assert total == bt
        for r, c in enumerate(cols):                                     # the gaps of the matching that came back
            if c < 0:
                assert gaps[r] == 0
                continue
            other, arg = R.brute_assignment(E, (r, int(c)))
            assert gaps[r] == (np.inf if arg is None else bt - other), (E, r, c)


def test_assignment_infinite_gaps_and_errors(solve):
    one = solve([np.array([[3.5]])])[0]
    assert one[0] == 0 and one[1] == 3.5 and one[2].tolist() == [0] and np.isinf(one[3][0])
    col = solve([np.array([[1.0], [2.0], [0.5]])])[0]                     # 3 x 1: the pair can move to another row
    assert col[2].tolist() == [-1, 0, -1] and col[3].tolist() == [0.0, 1.0, 0.0]
    row = solve([np.array([[1.0, 4.0, 2.0]])])[0]
    assert row[2].tolist() == [1] and row[3].tolist() == [2.0]
    for bad in (np.nan, np.inf, -np.inf):
        assert solve([np.array([[1.0, bad], [0.0, 1.0]])])[0][0] == -1
    res = solve([np.zeros((0, 0))] * 3 + [np.zeros((0, 0))] * 2, shapes=[(0, 3), (3, 0), (0, 0), (-1, 2), (2, -1)])
    assert [r[0] for r in res] == [0, 0, 0, -1, -1]
    assert res[1][2].tolist() == [-1, -1, -1] and res[1][1] == 0.0 and res[1][3].tolist() == [0.0, 0.0, 0.0]


def test_assignment_200_against_fresh_solves(solve):
    rng = np.random.default_rng(2)
    E = rng.normal(size=(200, 200))
    rc, total, cols, gaps = solve([E])[0]
    assert rc == 0 and sorted(cols.tolist()) == list(range(200))
    rows = list(range(0, 200, 20))
    forbidden = []
    for r in rows:
        F = E.copy()
        F[r, cols[r]] = -1e6                                              # never chosen: 200 entries of size ~1 cannot make up for it
        forbidden.append(F)
    for r, (rc2, t2, c2, _g) in zip(rows, solve(forbidden)):
        assert rc2 == 0 and c2[r] != cols[r]
        assert gaps[r] >= 0 and abs((total - t2) - gaps[r]) <= 1e-11
    rect = rng.normal(size=(60, 200))                                     # rectangular both ways
    for M in (rect, rect.T.copy()):
        rc, total, cols, gaps = solve([M])[0]
        r = int(np.flatnonzero(cols >= 0)[7])
        F = M.copy()
        F[r, cols[r]] = -1e6
        t2 = solve([F])[0][1]
        assert abs((total - t2) - gaps[r]) <= 1e-11


def test_assignment_driver_under_sanitizers(tmp_path):
    """assignment.h once more with -fsanitize=address,undefined, the binary run directly"""
    try:
        san = D.compile_assignment_driver(tmp_path, sanitize=True)
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/assignment_driver.cpp failed")
    rng = np.random.default_rng(3)
    problems = [rng.normal(size=shape) for shape in all_shapes(5)] + [rng.integers(0, 3, size=(4, 6)).astype(np.float64),
                                                                     rng.normal(size=(40, 70)), rng.normal(size=(70, 40))]
    for E, (rc, total, cols, gaps) in zip(problems, san(problems)):
        assert rc == 0 and (cols >= 0).sum() == min(E.shape)
    assert san([np.array([[np.nan]])])[0][0] == -1


def test_library_entry_matches_driver(solve):
    """dca_assign_partners needs no device: the library's entry returns the driver's answers"""
    from pydca_amd import _lib
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (4, 4), (3, 7), (7, 3), (0, 2)):
        E = rng.normal(size=shape)
        cols, total, gaps = _lib.assign_partners(E)
        rc, t, c, g = solve([E], shapes=[shape])[0]
        assert rc == 0 and total == t and np.array_equal(cols, c) and gaps.tobytes() == g.tobytes()
    with pytest.raises(_lib.DcaBackendError):
        _lib.assign_partners(np.array([[np.inf]]))
