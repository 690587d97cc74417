"""The SPD inverse of the MI355X (pydca_amd/csrc/cholinv.hip through ctx.spd_inverse, and the mfDCA entry with scale -1) element by
element: |X - A^-1|_ij <= C_DEVICE u (|A^-1| |A| |A^-1|)_ij against a reference known to more than float64, on the case table that
tests/spd_inverse_reference.py derives from the launch decisions (every product form, both leaves, the side-stream fork, both
forms of the block sweep, its thresholds and edge geometries, up to n = 8192), at condition numbers of about 10^2 and 10^4 - 10^5.
Bits: a repeated call and the sweep under tiny workgroup caps return the same matrix.  A planted non-positive pivot comes back
as DCA_ERR_NOT_SPD with LAPACK's pivot.  tests/test_spd_inverse_audit_host.py holds the reference, the bound's constant, the
restatement and the planted faults on the CPU.  Every check prints the figure it asserts (pytest -s).

Run on an MI355X:  python -m pytest tests/test_spd_inverse_audit.py -q -m gpu -s"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mf_shape_cases as M
import spd_inverse_audit_child as child
import spd_inverse_reference as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = R.pinned_cases()
DEFAULT = [c for c in CASES if not c.env]
KNOBBED = [c for c in CASES if c.env]
CAPS = {"DCA_SWEEP_CAP": "8", "DCA_SWEEP_PRIO_CAP": "8"}

@pytest.fixture(scope="module")
def L_():
    from pydca_amd import _lib
    _lib.lib()
    return _lib


def run_child(args, env, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(HERE, "spd_inverse_audit_child.py")] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr[-2000:]
    return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]


def case_args(c):
    return [c.n, c.kron[0] if c.kron else 0, c.kron[1] if c.kron else 0]


def judge(r, repeat=True):
    print("\n[spd-audit] %-46s shift %.2f cond %.1e  worst %.3f u E at %s (bound %.2f)  %.1f s" %
          (r["case"], r["shift"], r["cond"], r["ratio"], tuple(r["where"]), R.C_DEVICE, r["seconds"]), end="")
    assert r["symmetric"], "the inverse is not bit-symmetric"
    assert r["ratio"] <= R.C_DEVICE, r
    if repeat:
        assert r["repeat"] is True, "a second call in the same process gave other bits"


@pytest.mark.parametrize("shift", R.SHIFTS)
@pytest.mark.parametrize("case", DEFAULT, ids=repr)
def test_every_element_under_default_settings(L_, case, shift):
    """The fused recursion below n = 2560 (from 2048 on with its top-level product on the side stream), the block sweep above (from X
    below 4500, through P above, 512-column panels from 7000, chain products on larger workgroups from 6000)."""
    judge(child.audit(L_, case, shift))


@pytest.mark.parametrize("case", KNOBBED, ids=repr)
def test_every_element_under_the_knobs(case):
    """The sweep forced onto small matrices in both forms and both panel widths (ragged last panel, 64-column last panel, last
    tile row of 64), and DCA_SWEEP=0: the recursion at the sizes where its dispatcher reaches the 128 x 64 and the 128 x 128
    LDS-DMA products (n = 2944, 8192), which no default setting reaches.  One child process per case, both shifts in it.  The
    largest case, n = 8192, takes about 4 s per shift, nearly all of it on the host (the Kronecker product, the padded copy, the
    longdouble comparison by rows): the repeated call stays in at every size."""
    out = run_child(["ratio"] + case_args(case), case.env)
    assert [r["shift"] for r in out] == list(R.SHIFTS)
    for r in out:
        r["case"] = case.name
        judge(r)


# every case of the table whose launch list is a sweep (R.sweep_runs, held to the launch decisions by the host test): the twelve
# default ones from n = 2556 to 7104 and the ten forced ones; n = 384 and n = 768 under the knobs stay in the recursion
SWEPT = [c for c in CASES if R.sweep_runs(c.np, c.env)]


@pytest.mark.parametrize("case", SWEPT, ids=repr)
def test_sweep_bits_do_not_depend_on_the_tile_hand_out(case):
    """DCA_SWEEP_CAP = DCA_SWEEP_PRIO_CAP = 8 changes which workgroup takes which tile (the lists wrap, the XCD chunks are stolen
    from); the values must not change: same bits as under the default caps, at both shifts, wherever the sweep runs."""
    a = run_child(["hash"] + case_args(case), case.env)
    b = run_child(["hash"] + case_args(case), dict(case.env, **CAPS))
    assert len(a) == len(b) == len(R.SHIFTS)
    for x, y in zip(a, b):
        print("\n[spd-audit] %-46s shift %.2f  default caps %s  caps 8 / 8 %s" % (case.name, x["shift"], x["sha"][:16], y["sha"][:16]), end="")
        assert x["sha"] == y["sha"]


def check_pivots(reports):
    for r in reports:
        print("\n[spd-audit] %-30s row %5d  potrf stops at %5d  device: %s" % (r["case"], r["row"], r["potrf"], r["message"]), end="")
        assert r["potrf"] == r["row"] + 1
        assert r["code"] == r["not_spd"] and "(pivot %d)" % r["potrf"] in r["message"], r


def test_pivot_report_of_the_recursion(L_):
    """A[r][r] = -1 at row 0, the last row of the first leaf, the first row of the second, 127 / 128 / 129 and the last real row
    of a matrix that is padded (n = 421: leaves of 128, 128, 64 and 128 rows, the 64-leaf at row 256): DCA_ERR_NOT_SPD with the
    pivot LAPACK's potrf names."""
    case = R.Case(421)
    check_pivots([child.pivot_report(L_, case, 0.5, r) for r in (0, 127, 128, 129, 256, 319, 320, 420)])


@pytest.mark.parametrize("k", [1, 3], ids=["from_X", "through_P"])
def test_pivot_report_of_the_sweep(k):
    """The same in both forms of the block sweep (n = 1085, 128-column panels): also the first row of a later panel (640) and
    the last real row (1084)."""
    case = R.Case(1085, R.KNOB_SETS[k], (35, 31))
    check_pivots(run_child(["pivot"] + case_args(case) + [0, 127, 128, 129, 640, 1084], case.env))


MF_CASES = [c for c in M.DYADIC if c.inverse and c.n <= 640]


@pytest.mark.parametrize("case", MF_CASES, ids=repr)
def test_mf_couplings_every_element(L_, case):
    """The mfDCA entry (scale -1, which ctx.spd_inverse never takes): mf_couplings() against the negated longdouble inverse of the
    matrix mf_corr_mat returns, padded with an identity block to a multiple of 64 as mf_engine.hip pads it, within the same
    bound.  The condition number of a real correlation matrix (pseudocount 0.5) is printed: it sits near the shift 0.5 family."""
    X, k = M.alignment(case.name)
    ctx = L_.Context(0, L_.DCA_F64)
    ctx.set_msa(X, case.q)
    ctx.set_weights(k / 8.0)
    C = ctx.mf_corr_mat(M.THETA)
    J = ctx.mf_couplings()
    ctx.close()
    n = case.n
    assert C.shape == (n, n) and np.array_equal(J, J.T)
    Xl, E = R.plain_inverse(R.pad(C))
    err = np.abs(J.astype(R.LD) + Xl[:n, :n]).astype(np.float64)
    ratio = float((err / (R.U * E[:n, :n])).max())
    w = np.linalg.eigvalsh(C)
    print("\n[spd-audit] mf %-20s n = %4d  cond %.2e  worst %.3f u E (bound %.2f)" % (case, n, w[-1] / w[0], ratio, R.C_DEVICE), end="")
    assert ratio <= R.C_DEVICE
