"""The element audit of the SPD inverse (tests/spd_inverse_reference.py) on the CPU: the exactness of the Kronecker construction and
the tightness of the reference inverses, the two matrix identities behind the bound matrix, LAPACK's measured ratios and the
constant c, the float64 restatement of the kernels' order within the bound on every case up to n = 1500 at both shifts (positive
control), every planted fault at 100 bounds or more (negative controls: the bound is not slack), the case table against the
launch decisions of pydca_amd/csrc/cholinv_plan.h (through tests/cholinv_plan_driver.cpp), and the sweep's workspace condition.
tests/test_spd_inverse_audit.py runs the same audit on what the MI355X returns."""
import numpy as np
import pytest

import spd_inverse_reference as R

HOST_MAX_N = 1500


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("cholplan"))


@pytest.fixture(scope="module")
def table(plan):
    return R.derive_table(plan)


@pytest.fixture(scope="module")
def measured(plan, table):
    """per (case, shift) up to HOST_MAX_N: LAPACK's two ratios (once per matrix) and the restatement's, computed once"""
    out, lap = {}, {}
    for c in table[0]:
        if c.np > HOST_MAX_N:
            continue
        for shift in R.SHIFTS:
            ref = R.reference(c, shift)
            A = ref.A
            if (c.base, shift) not in lap:
                lap[(c.base, shift)] = {k: ref.ratio(v)[0] for k, v in R.lapack_routes(A)}
            X = R.restated_inverse(A, plan, c.env)
            out[(c.name, shift)] = dict(case=c, lapack=lap[(c.base, shift)], restated=ref.ratio(X), symmetric=bool(np.array_equal(X, X.T)))
    return out


def test_kronecker_products_are_exact_and_the_reference_is_tight(table):
    """Every Kronecker case of the table: the factors are symmetric multiples of 2^-12 short enough for exact products (every
    case), the float64 product equals the longdouble product (asserted in reference() up to n = 1600, and here at one large
    case by rows), and the reference's own error -- bounded by the exact residual of the factor inverses, propagated through the
    product -- stays below 2^-8 of u E (asserted where a reference is made; repeated here)."""
    worst = 0.0
    for c in table[0]:
        if not c.kron:
            continue
        for shift in R.SHIFTS:
            ref = R.reference(c, shift)
            f1, f2 = ref.f
            assert R.kron_is_exact(f1["A"], f2["A"]), c
            assert ref.ref_err < 2.0 ** -8
            worst = max(worst, ref.ref_err)
    print("\n[spd-audit] worst reference error over u E, Kronecker cases: %.2e (limit %.2e)" % (worst, 2.0 ** -8))
    big = [c for c in table[0] if c.kron and c.n >= 8000][0]
    f1, f2 = R.reference(big, 0.5).f
    for i1 in (0, f1["A"].shape[0] - 1):
        row = f1["A"][i1:i1 + 1]
        assert np.array_equal(np.kron(row.astype(R.LD), f2["A"].astype(R.LD)), np.kron(row, f2["A"]).astype(R.LD))


def test_unstructured_references_are_tight(table):
    worst = max(R.reference(c, s).ref_err for c in table[0] if not c.kron for s in R.SHIFTS)
    print("\n[spd-audit] worst reference error over u E, unstructured cases: %.2e (limit %.2e)" % (worst, 2.0 ** -8))
    assert worst < 2.0 ** -8


def test_the_two_identities_behind_the_bound_matrix():
    """|X (x) Y| = |X| (x) |Y| and (X (x) Y)(Z (x) W) = XZ (x) YW, exactly on integer matrices; and on a small case E1 (x) E2 is
    |A^-1| |A| |A^-1| of the product matrix computed densely, to the rounding of that dense product."""
    rng = np.random.default_rng(5)
    X, Z = (rng.integers(-9, 10, (5, 5)).astype(float) for _ in range(2))
    Y, W = (rng.integers(-9, 10, (7, 7)).astype(float) for _ in range(2))
    assert np.array_equal(np.abs(np.kron(X, Y)), np.kron(np.abs(X), np.abs(Y)))
    assert np.array_equal(np.kron(X, Y) @ np.kron(Z, W), np.kron(X @ Z, Y @ W))
    ref = R.reference(R.Case(15 * 12, (), (15, 12)), 0.5)
    f1, f2 = ref.f
    A, Xd = np.kron(f1["A"], f2["A"]), np.kron(f1["X"], f2["X"])
    E = R.bound_matrix(A, Xd)
    assert np.allclose(E, np.kron(f1["E"], f2["E"]), rtol=1e-12, atol=0)
    # ... and the product of the factor inverses is the inverse of the product (longdouble residual)
    assert float(np.abs(np.eye(180, dtype=R.LD) - A.astype(R.LD) @ Xd).max()) < 2.0 ** -50


def test_lapack_ratios_and_the_constant(measured):
    """c is LAPACK's worst err / (u E) over the whole table (R.LAPACK_MEASURED, both routes): the recorded table's own worst is
    c, neither guessed nor padded.  The cases up to n = 1500 are measured again here, on whatever BLAS, thread count and CPU
    this suite runs with.  Another blocking or kernel selection draws other roundings from the same distribution, and each
    figure is the maximum of 10^3 - 10^6 such draws, so it moves by tens of per cent and not by a factor: the worst measured
    here has to lie within a factor R.LAPACK_REMEASURED of c either way.  Beyond that either the reference or the bound matrix
    is no longer what the recorded table was measured against."""
    worst = 0.0
    for (name, shift), m in sorted(measured.items()):
        print("\n[spd-audit] %-46s shift %.2f  LAPACK getri %.3f  potrf route %.3f" % (name, shift, m["lapack"]["getri"], m["lapack"]["potrf"]), end="")
        worst = max(worst, *m["lapack"].values())
    recorded = max(max(v[0][1:] + v[1][1:]) for v in R.LAPACK_MEASURED.values())
    print("\n[spd-audit] worst here %.3f, worst of the recorded table %.3f, c = %.2f, device constant %.2f" % (worst, recorded, R.C_LAPACK, R.C_DEVICE))
    assert R.C_LAPACK / R.LAPACK_REMEASURED <= worst <= R.C_LAPACK * R.LAPACK_REMEASURED
    assert recorded <= R.C_LAPACK < recorded * 1.01
    assert R.C_DEVICE == 8 * R.C_LAPACK


def test_recorded_lapack_table_covers_the_case_table(table):
    assert {c.base for c in table[0]} <= set(R.LAPACK_MEASURED)


def test_restatement_is_within_the_bound(measured):
    """The algorithm as written (the launch list executed in float64) meets the device's bound on every case up to n = 1500 at
    both shifts, and returns a bit-symmetric matrix; undefined storage is never read (NaN poison, asserted inside restate)."""
    worst = 0.0
    for (name, shift), m in sorted(measured.items()):
        r, where = m["restated"]
        print("\n[spd-audit] %-46s shift %.2f  restatement %.3f of u E at %s (bound %.2f)" % (name, shift, r, where, R.C_DEVICE), end="")
        assert m["symmetric"], name
        assert r <= R.C_DEVICE, (name, shift, r, where)
        worst = max(worst, r)
    print("\n[spd-audit] worst restatement ratio %.3f" % worst)
    # the restatement is an inverse through a Cholesky factor like LAPACK's: it sits at LAPACK's level, not at the bound's
    assert worst <= 2 * R.C_LAPACK


FAULT_CASES = {
    # fault -> (padded size, knob set, ragged n, shifts at which it is judged)
    "syrk k-tile of 16 dropped": (448, 0, True, R.SHIFTS),
    "mask k < row on a diagonal tile": (448, 0, True, R.SHIFTS),
    "output tile not mirrored": (448, 0, True, R.SHIFTS),
    "padding diagonal 0": (448, 0, True, R.SHIFTS),
    "sweep tile stale": (1088, 1, True, R.SHIFTS),
    "Cin read from C": (1088, 1, True, R.SHIFTS),
    # an absolute 1e-10: at shift 0.01 the BOUND ITSELF is of that size (|A^-1| ~ 10^2, E ~ 10^4 .. 10^5), so the fault is judged where
    # an error of 1e-10 is an error: shift 0.5.  Its figure at shift 0.01 is printed.
    "one element off by 1e-10": (448, 0, True, (0.5,)),
    # ... and the same fault relative to the largest entry of the inverse (1.5e-10 at shift 0.5, 1.4e-9 at shift 0.01): an error
    # of one size in the old criterion's own measure, judged at both shifts
    "one element off by 1e-10 of the largest": (448, 0, True, R.SHIFTS),
}


def test_every_planted_fault_is_a_hundred_bounds_out(plan):
    """Each fault of R.FAULTS on one tile or step of the restatement: the worst error is at least 100 device bounds (or the
    factorisation stops, which the device reports as DCA_ERR_NOT_SPD).  Beside each: whether the criterion of the tests before
    this audit (Frobenius ratio below 1e-11 against the inverse) lets it pass."""
    assert set(FAULT_CASES) == set(R.FAULTS)
    passes_old, stops = [], []
    for kind in R.FAULTS:
        np_, k, ragged, shifts = FAULT_CASES[kind]
        c = R.make_case(np_, R.KNOB_SETS[k], ragged)
        for shift in R.SHIFTS:
            ref = R.reference(c, shift)
            f = R.Fault(kind)
            Y = R.restated_inverse(ref.A, plan, c.env, f)
            assert f.hit is not None, (kind, "was not applied")
            if Y is None:
                print("\n[spd-audit] fault %-34s %-12s shift %.2f (%s): the factorisation stops -> reported as not SPD" % (kind, c, shift, f.hit), end="")
                stops.append((kind, shift))
                continue
            r = ref.ratio(Y)[0] / R.C_DEVICE
            old = R.rel_err(Y, ref.inverse64())
            print("\n[spd-audit] fault %-34s %-12s shift %.2f (%s): %.3g bounds; old criterion %.2e -> %s" %
                  (kind, c, shift, f.hit, r, old, "PASSES" if old < 1e-11 else "fails"), end="")
            if shift in shifts:
                assert r >= R.FAULT_MARGIN, (kind, shift, r)
                if old < 1e-11:
                    passes_old.append((kind, shift))
    print()
    assert ("one element off by 1e-10", 0.5) in passes_old
    assert all(("one element off by 1e-10 of the largest", s) in passes_old for s in R.SHIFTS)
    # a fault that only ever stops the factorisation would never be measured against the bound: each has a figure at one shift
    # at least, but for the padding diagonal, which is a zero pivot at either shift
    assert {k for k in R.FAULTS if all((k, s) in stops for s in R.SHIFTS)} == {"padding diagonal 0"}


def test_case_table_reaches_every_form_the_header_can_return(plan, table):
    """The union of the driver's launch lists over the table names every product form of cholinv_plan.h (the driver lists them),
    both leaves, both forms of the sweep at both panel widths it takes by default, the side-stream fork, and the sweep's edge
    geometries.  Every case's first-reached feature is reached at that case: the table is derived, not chosen."""
    cases, first = table
    assert plan.forms == R.ALL_FORMS
    seen = set()
    for c in cases:
        seen |= R.features(plan(c.np, c.env))
    forms = {f[1] for f in seen if f[0] == "form"}
    assert forms == set(plan.forms), set(plan.forms) - forms
    assert {("leaf", 64), ("leaf", 128), ("recursion", "side fork"), ("recursion", "in line"), ("sweep", "factor", 256), ("sweep", "P", 256),
            ("sweep", "P", 512), ("sweep", "factor", 128), ("sweep", "P", 128), ("sweep", "ragged last panel"), ("sweep", "64-column last panel"),
            ("sweep", "last tile row of 64"), ("form", "dma128banded", "side"), ("form", "dma64", "side"), ("form", "small32", "side")} <= seen
    assert set(first) <= seen
    # under DEFAULT settings the 128 x 128 and 128 x 64 LDS-DMA forms are not reached by their dispatcher at any size up to 8192
    # (the sweep takes over at 2560 and its products are panels): only DCA_SWEEP=0 reaches them, at n = 8192 and n = 2944
    default = set()
    for np_ in range(64, R.SCAN_MAX + 1, 64):
        default |= {f[1] for f in R.features(plan(np_)) if f[0] == "form"}
    assert default == {"small32", "small32pair", "dma64", "dma128banded"}
    assert first[("form", "dma128", "chain")] == (8192, {"DCA_SWEEP": "0"}) and first[("form", "dma128x64", "chain")] == (2944, {"DCA_SWEEP": "0"})
    # thresholds and padding edges are members
    names = {c.name for c in cases}
    assert {"n1", "n63", "n64", "n65", "n127", "n129", "n2560_64x40", "n4544_64x71", "n7040_64x110", "n2496_64x39"} <= names
    for c in cases:
        assert c.kron is None or max(c.kron) <= 128


def test_pinned_table_is_the_derived_table(table):
    assert [(c.n, c.kron, c.env) for c in table[0]] == [(c.n, c.kron, c.env) for c in R.pinned_cases()]


def test_sweep_workspace_condition(plan):
    """Wherever the driver decides for the sweep, the workspace it lays out (4 n B + 7 B^2 doubles and 16 counters per panel) fits
    the 2 n^2 doubles the callers provide (the driver prints `nomem` otherwise), under every knob set; and the decision is the
    formula: with 256-column panels n = 768 is still the recursion and n = 832 is swept."""
    for env in R.KNOB_SETS + [{"DCA_SWEEP_MIN": "128", "DCA_SWEEP_PANEL": "512"}, {"DCA_SWEEP_MIN": "128", "DCA_SWEEP_PANEL": "1024"}]:
        minN, wide, narrow, wideMinN, _ = R.cfg_of(env)
        for np_ in range(64, R.SCAN_MAX + 1, 64):
            p = plan(np_, env)
            B = wide if np_ >= wideMinN else narrow
            assert bool(p["swept"]) == R.sweep_runs(np_, env), (np_, env)
            if p["swept"]:
                panels = [o for o in p["ops"] if o["op"] == "panel"]
                assert panels and sum(o["w"] for o in panels) == np_ and all(o["w"] % 64 == 0 for o in panels)
                assert 4 * np_ * B + 7 * B * B + 2 * len(panels) * 8 <= 2 * np_ * np_
    env = R.KNOB_SETS[2]
    assert not plan(768, env)["swept"] and plan(832, env)["swept"]


def test_sweep_defaults_are_the_header_s(plan):
    """cfg_of() repeats the defaults of SweepCfg because the driver takes all five as arguments; the driver prints
    sweep_cfg_defaults() of cholinv_plan.h, and the two agree.  A changed default in the header fails here before the case table
    and the workspace test follow a stale copy."""
    assert plan.defaults == R.cfg_of({})


def test_swept_cases_of_the_table(plan):
    """The cases on which the GPU test compares the sweep's bits under two tile hand-outs are the cases whose launch list is a
    sweep -- every one of them, 22: twelve default ones from n = 2556 to 7104 (both forms, both panel widths, both chain bounds)
    and ten forced ones; n = 384 at 128-column panels and n = 768 at 256-column panels stay in the recursion (the workspace)."""
    swept = [c for c in R.pinned_cases() if R.sweep_runs(c.np, c.env)]
    assert [c.name for c in swept] == [c.name for c in R.pinned_cases() if plan(c.np, c.env)["swept"]]
    assert len(swept) == 22 and sum(1 for c in swept if not c.env) == 12
    assert {(plan(c.np, c.env)["factorForm"], plan(c.np, c.env)["B"], plan(c.np, c.env)["small32Max"]) for c in swept if c.np >= 5952} == \
        {(0, 256, 400), (0, 256, 16), (0, 512, 16)}
