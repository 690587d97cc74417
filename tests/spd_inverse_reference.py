"""TEST INFRASTRUCTURE ONLY: the element audit of the SPD inverse (pydca_amd/csrc/cholinv.hip).

What is compared.  X = the device's inverse of an SPD matrix A, against A^-1 known to more than float64:
    |X - A^-1|_ij  <=  c u E_ij,    E = |A^-1| |A| |A^-1|,  u = 2^-53
the componentwise form of Higham's bound for an inverse obtained through a Cholesky factor (Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 14.3 with 10.1: the computed factor is the exact factor of A + dA, |dA| <= c1 u |R^T||R|, and for an
SPD matrix |R^T||R| and |A| differ by a modest factor; the inverse of the perturbed matrix moves by |A^-1||dA||A^-1|).  The
constant is MEASURED, not guessed: C_LAPACK is the worst err / (u E) of float64 LAPACK (getrf / getri through np.linalg.inv,
and potrf + trtri + X^T X) against this module's reference over the whole case table, and the device is allowed
C_DEVICE = 8 C_LAPACK -- the same class of algorithm with other blockings and k-chains of four on the matrix cores may differ
from LAPACK by rounding, not by a term.  The margin of 8 holds only as long as every planted fault (FAULTS) is at least 100
bounds out; tests/test_spd_inverse_audit_host.py asserts that.

Matrices.  Two families, each at two shifts (0.5: condition number about 10^2, 0.01: about 10^4 - 10^5), entries rounded to
multiples of 2^-12 and symmetrised:
  * Kronecker products A = A1 (x) A2 of two such matrices with m1, m2 <= 128.  The product is exact in float64 (asserted), dense,
    has no zeros, and A^-1 = A1^-1 (x) A2^-1, E = E1 (x) E2 (|X (x) Y| = |X| (x) |Y| and (X (x) Y)(Z (x) W) = XZ (x) YW, asserted on
    small factors), so reference and bound cost O(n^2) at every size, up to n = 8192.
  * random SPD matrices that are no Kronecker product, n <= 448: guards against a blind spot of the first family.
Reference inverses: longdouble Gauss-Jordan, then Newton steps X <- X + X (I - A X) whose residual is EXACT: A 2^12 is a matrix of
small integers and X is cut into 26-bit fixed-point pieces, so every float64 BLAS product A X_p is exact whatever its
summation order, and the pieces recombine exactly in longdouble.  The error that is left is bounded by |X| |I - A X| with that
exact residual (refined_inverse) and has to stay below 2^-8 of u E, asserted wherever a reference is made.

The float64 restatement (restate) performs the fused recursion and the block sweep in the kernels' order from the launch list
that tests/cholinv_plan_driver.cpp prints (pydca_amd/csrc/cholinv_plan.h: the same split, panel boundaries, masks, lower-only
outputs with mirroring, X = inv(chol) leaves followed by X^T X).  Storage that the kernels leave undefined is poisoned with NaN,
so the restatement also shows that nothing reads it.  It carries the planted faults.
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
FRAC_BITS = 12
SHIFTS = (0.5, 0.01)
INT_MAX = 2 ** 31 - 1

# measured once on the whole table (worst err / (u E) of float64 LAPACK; OpenBLAS through numpy 2 / scipy 1.15): case -> (condition number,
# getri, potrf route) at shift 0.5 and at shift 0.01
LAPACK_MEASURED = {
    "n1": ((1.00e0, 0.214, 0.916), (1.00e0, 0.619, 1.023)),
    "n63": ((1.14e1, 1.000, 1.759), (2.61e2, 0.157, 0.140)),
    "n64": ((1.17e1, 1.156, 1.876), (2.59e2, 0.149, 0.268)),
    "n65": ((1.07e1, 0.944, 1.656), (2.81e2, 0.142, 0.186)),
    "n127": ((1.12e1, 1.029, 1.527), (3.67e2, 0.110, 0.156)),
    "n128": ((1.08e1, 1.067, 1.958), (4.23e2, 0.146, 0.141)),
    "n129": ((1.15e1, 1.386, 1.930), (3.70e2, 0.130, 0.162)),
    "n192": ((1.17e1, 1.301, 2.484), (3.84e2, 0.102, 0.134)),
    "n256": ((1.20e1, 1.201, 2.738), (3.95e2, 0.119, 0.137)),
    "n421": ((1.18e1, 1.539, 1.808), (4.28e2, 0.121, 0.121)),
    "n1280_64x20": ((1.20e2, 0.851, 1.301), (1.25e4, 0.090, 0.094)),
    "n1344_64x21": ((1.02e2, 1.145, 1.896), (1.08e4, 0.091, 0.108)),
    "n1408_64x22": ((1.29e2, 0.887, 1.088), (3.35e4, 0.073, 0.092)),
    "n2432_64x38": ((1.02e2, 1.118, 1.476), (2.66e4, 0.063, 0.078)),
    "n2496_64x39": ((1.23e2, 0.802, 1.752), (5.83e4, 0.047, 0.050)),
    "n2556_71x36": ((1.06e2, 1.021, 1.687), (4.10e4, 0.047, 0.050)),
    "n2560_64x40": ((1.21e2, 1.176, 1.304), (8.14e4, 0.046, 0.063)),
    "n2624_64x41": ((1.33e2, 1.085, 1.313), (5.32e4, 0.054, 0.063)),
    "n4480_64x70": ((1.39e2, 0.831, 1.653), (7.34e4, 0.033, 0.042)),
    "n4544_64x71": ((1.18e2, 0.928, 1.647), (6.52e4, 0.030, 0.035)),
    "n4608_64x72": ((1.33e2, 1.124, 1.126), (8.32e4, 0.032, 0.036)),
    "n5952_64x93": ((1.36e2, 0.931, 1.440), (8.27e4, 0.027, 0.032)),
    "n6016_64x94": ((1.26e2, 0.912, 1.292), (8.82e4, 0.028, 0.030)),
    "n6080_64x95": ((1.32e2, 0.758, 1.224), (8.42e4, 0.032, 0.027)),
    "n6976_64x109": ((1.30e2, 0.840, 1.074), (9.01e4, 0.027, 0.030)),
    "n7040_64x110": ((1.37e2, 0.878, 1.194), (8.84e4, 0.025, 0.030)),
    "n7104_64x111": ((1.24e2, 0.955, 1.448), (9.16e4, 0.027, 0.027)),
    "n2880_64x45": ((1.23e2, 1.081, 1.363), (3.35e4, 0.041, 0.075)),
    "n2944_64x46": ((1.27e2, 0.987, 1.209), (3.65e4, 0.046, 0.043)),
    "n3008_64x47": ((1.38e2, 0.851, 1.315), (3.63e4, 0.052, 0.058)),
    "n8128_64x127": ((1.33e2, 0.921, 1.619), (8.01e4, 0.025, 0.025)),
    "n8192_64x128": ((1.30e2, 0.974, 1.440), (7.93e4, 0.024, 0.028)),
    "n384": ((1.20e1, 1.758, 3.184), (4.06e2, 0.094, 0.086)),
    "n448": ((1.18e1, 0.996, 2.289), (4.05e2, 0.127, 0.146)),
    "n512_64x8": ((8.17e1, 0.968, 1.314), (5.87e3, 0.118, 0.128)),
    "n1085_35x31": ((1.28e2, 1.084, 1.754), (1.53e4, 0.075, 0.083)),
    "n768_64x12": ((9.54e1, 1.140, 2.407), (5.65e3, 0.211, 0.184)),
    "n832_64x13": ((1.04e2, 0.941, 1.504), (1.11e4, 0.110, 0.105)),
    "n896_64x14": ((8.03e1, 0.952, 1.462), (4.94e3, 0.114, 0.153)),
}
# c: the worst figure of that table (potrf route, n = 384, shift 0.5: 3.184; getri's worst is 1.758 at the same case), rounded up.
# tests/test_spd_inverse_audit_host.py measures every case up to n = 1500 again; its worst has to come out within a factor
# LAPACK_REMEASURED of c (another BLAS build rounds in another order: the figures move, c and the device's bound do not).
C_LAPACK = 3.19
LAPACK_REMEASURED = 2.0
C_DEVICE = 8.0 * C_LAPACK
FAULT_MARGIN = 100.0


# ----------------------------------------------------------------------------- matrices
def spd_matrix(n, shift, seed=None):
    """B B^T / n + shift diag(0.5 .. 1.5), the family of tests/test_gpu_parity.py, rounded to multiples of 2^-12 and symmetrised."""
    rng = np.random.default_rng(1000 * n + int(round(shift * 100)) if seed is None else seed)
    B = rng.standard_normal((n, n + 8))
    A = B @ B.T / n + shift * np.diag(rng.random(n) + 0.5)
    A = np.rint(np.tril(A) * 2.0 ** FRAC_BITS) / 2.0 ** FRAC_BITS
    return np.tril(A) + np.tril(A, -1).T


def gauss_jordan(A):
    """Plain Gauss-Jordan inverse in longdouble, no pivoting (A is SPD)."""
    n = A.shape[0]
    M = np.array(A, dtype=LD)
    X = np.eye(n, dtype=LD)
    for k in range(n):
        piv = M[k, k]
        if not piv > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % (k + 1))
        rk, xk = M[k] / piv, X[k] / piv
        col = M[:, k].copy()
        col[k] = 0
        M -= np.outer(col, rk)
        X -= np.outer(col, xk)
        M[k], X[k] = rk, xk
    return X


PIECE_BITS, PIECES = 26, 6


def exact_residual(A, X):
    """I - A X for a float64 A whose entries are multiples of 2^-12 (below 8 at n = 2048, 128 at n = 128) and a longdouble X, exact up to the returned absolute
    truncation (X is cut off 156 bits below its largest entry)."""
    n = A.shape[0]
    Ai = A * 2.0 ** FRAC_BITS
    amax = float(np.abs(Ai).max())
    assert np.array_equal(Ai, np.rint(Ai)) and amax * 2.0 ** PIECE_BITS * n <= 2.0 ** 53      # every sum of n products is an exact integer
    e = int(np.ceil(np.log2(float(np.abs(X).max())))) + 1
    Y = X * LD(2.0) ** -e                                  # |Y| < 1, exact scaling
    R = np.eye(n, dtype=LD)
    scale = LD(2.0) ** (e - FRAC_BITS)
    for _ in range(PIECES):
        Y = Y * LD(2.0 ** PIECE_BITS)
        T = np.rint(Y)
        Y = Y - T                                           # exact: the fraction that is left
        scale = scale * LD(2.0 ** -PIECE_BITS)
        R = R - (Ai @ T.astype(np.float64)).astype(LD) * scale      # integers below 2^52; R stays a short multiple of `scale`
    return R, float(n * amax * 2.0 ** (e - FRAC_BITS - PIECE_BITS * PIECES))


def refined_inverse(A, start=None):
    """(X, d): the inverse in longdouble and an elementwise bound on |X - A^-1|.  Gauss-Jordan, two Newton steps on the exact
    residual, then d = |X| (|I - A X| + truncation), which bounds |A^-1 (I - A X)| because |A^-1| <= |X| + d and the residual is
    of the order of 2^-64 (the factor 1.001 covers the second order and the rounding of this product itself)."""
    X = gauss_jordan(A) if start is None else np.array(start, dtype=LD)
    for _ in range(2):
        R, _ = exact_residual(A, X)
        Rf = R.astype(np.float64)
        hi = X.astype(np.float64)
        lo = (X - hi).astype(np.float64)
        X = X + ((hi @ Rf).astype(LD) + (lo @ Rf).astype(LD))        # the correction is ~2^-50 of X: float64 products do
    X = (X + X.T) / 2
    R, trunc = exact_residual(A, X)
    d = 1.001 * (np.abs(X).astype(np.float64) @ (np.abs(R).astype(np.float64) + trunc)) + 1e-300
    return X, d


def bound_matrix(A, X):
    """E = |X| |A| |X| in float64 (its own rounding, n 2^-53 relative, does not matter to a bound that is compared at 2^-8)."""
    aX = np.abs(X).astype(np.float64)
    return aX @ np.abs(A) @ aX


class Reference:
    """A, its inverse (longdouble) and E, either dense (n <= 448) or as Kronecker factors.  ratio(Y) = max |Y - A^-1| / (u E)."""

    def __init__(self, name, shift, factors):
        self.name, self.shift = name, shift
        self.f = []
        for A in factors:
            X, d = refined_inverse(A)
            self.f.append(dict(A=A, X=X, E=bound_matrix(A, X), d=d))
        self.n = int(np.prod([f["A"].shape[0] for f in self.f]))
        self.kron = len(self.f) == 2
        # the reference's own error over u E.  Kronecker: |X1 (x) X2 - T1 (x) T2| <= d1 (x) |X2| + |X1| (x) d2 + d1 (x) d2, and
        # |X| <= E elementwise ((|X| |A| |X|)_ij >= |X|_ij (|A| |X|)_jj >= |X|_ij |(A X)_jj|), so the worst ratio to E1 (x) E2
        # is at most r1 + r2 + r1 r2 with ri = max di / Ei
        r = [float((f["d"] / f["E"]).max()) / U for f in self.f]
        self.ref_err = r[0] if not self.kron else r[0] + r[1] + r[0] * r[1] * U
        assert self.ref_err < 2.0 ** -8, (name, shift, self.ref_err)

    @property
    def A(self):
        if not self.kron:
            return self.f[0]["A"]
        return np.kron(self.f[0]["A"], self.f[1]["A"])

    def cond(self):
        c = 1.0
        for f in self.f:
            w = np.linalg.eigvalsh(f["A"])
            c *= w[-1] / w[0]
        return float(c)

    def rows(self, i1):
        """(inverse, E) of the rows of block row i1: all rows for a dense reference"""
        if not self.kron:
            return self.f[0]["X"], self.f[0]["E"]
        f1, f2 = self.f
        return np.kron(f1["X"][i1:i1 + 1], f2["X"]), np.kron(f1["E"][i1:i1 + 1], f2["E"])

    def ratio_matrix_rows(self, Y, i1):
        X, E = self.rows(i1)
        m2 = X.shape[0]
        Yr = Y if not self.kron else Y[i1 * m2:(i1 + 1) * m2]
        return np.abs((Yr.astype(LD) - X)).astype(np.float64) / (U * E)

    def ratio(self, Y):
        """(worst |Y - A^-1|_ij / (u E_ij), its position)"""
        assert Y.shape == (self.n, self.n)
        worst, where = -1.0, None
        for i1 in range(self.f[0]["A"].shape[0] if self.kron else 1):
            r = self.ratio_matrix_rows(Y, i1)
            k = int(np.argmax(r))
            v = float(r.flat[k]) if np.isfinite(r.flat[k]) else np.inf
            if not np.all(np.isfinite(r)):
                v = np.inf
            if v > worst:
                m2 = r.shape[0]
                worst, where = v, ((i1 * m2 if self.kron else 0) + k // self.n, k % self.n)
        return worst, where

    def inverse64(self):
        """the reference rounded to float64 (for the old criterion and the planted faults)"""
        if not self.kron:
            return self.f[0]["X"].astype(np.float64)
        return np.concatenate([self.rows(i)[0].astype(np.float64) for i in range(self.f[0]["A"].shape[0])])


def factors_of(case, shift):
    """the case's matrix as its factors: one unstructured matrix, or the two factors of the Kronecker product"""
    if not case.kron:
        return [spd_matrix(case.n, shift)]
    m1, m2 = case.kron
    return [spd_matrix(m1, shift), spd_matrix(m2, shift, seed=77 * m2 + int(shift * 100) + 5)]


def matrix(case, shift):
    f = factors_of(case, shift)
    return f[0] if len(f) == 1 else np.kron(f[0], f[1])


_refs = {}


def reference(case, shift):
    """The shared, unchanged reference of one case at one shift."""
    key = (case.n, case.kron, shift)
    if key not in _refs:
        ref = Reference(case.name, shift, factors_of(case, shift))
        if case.kron and case.n <= 1600:
            # the construction is exact: the longdouble product has the float64 product's values
            f1, f2 = ref.f
            assert np.array_equal(np.kron(f1["A"].astype(LD), f2["A"].astype(LD)), np.kron(f1["A"], f2["A"]).astype(LD))
        _refs[key] = ref
    return _refs[key]


def kron_is_exact(A1, A2):
    """Every product of two entries fits float64: both are multiples of 2^-12 below 2^14 in magnitude (26 + 26 bits at most)."""
    ok = True
    for A in (A1, A2):
        Ai = A * 2.0 ** FRAC_BITS
        ok = ok and np.array_equal(Ai, np.rint(Ai)) and np.abs(Ai).max() < 2 ** 26 and np.array_equal(A, A.T)
    return bool(ok)


def rel_err(a, b):
    """today's criterion (tests/conftest.py)"""
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def lapack_routes(A):
    """float64 LAPACK inverses: getrf / getri, and potrf + trtri + X^T X (the device's route)"""
    from scipy.linalg import lapack
    yield "getri", np.linalg.inv(A)
    c, info = lapack.dpotrf(A, lower=1)
    assert info == 0
    x, info = lapack.dtrtri(c, lower=1)
    assert info == 0
    x = np.tril(x)
    yield "potrf", x.T @ x


def potrf_pivot(A):
    """the 1-based pivot at which LAPACK's Cholesky factorisation of the lower triangle stops, 0 if it does not"""
    from scipy.linalg import lapack
    return int(lapack.dpotrf(np.tril(A), lower=1)[1])


# ----------------------------------------------------------------------------- the plan driver
KNOB_SETS = [
    {},
    {"DCA_SWEEP_MIN": "256", "DCA_SWEEP_PANEL": "128"},
    {"DCA_SWEEP_MIN": "256", "DCA_SWEEP_PANEL": "256"},
    {"DCA_SWEEP_MIN": "256", "DCA_SWEEP_PANEL": "128", "DCA_SWEEP_FACTOR_MAX_N": "0"},
    {"DCA_SWEEP_MIN": "256", "DCA_SWEEP_PANEL": "256", "DCA_SWEEP_FACTOR_MAX_N": "0"},
    {"DCA_SWEEP": "0"},
]


def cfg_of(env):
    """sweep_cfg() of cholinv.hip under these variables: (minN, wide, narrow, wideMinN, factorMaxN).  The defaults repeat
    sweep_cfg_defaults() of cholinv_plan.h; the host test holds them to what the driver prints from the header."""
    minN, wide, narrow, wideMinN, factorMaxN = 2560, 512, 256, 7000, 4500
    if "DCA_SWEEP_FACTOR_MAX_N" in env:
        factorMaxN = int(env["DCA_SWEEP_FACTOR_MAX_N"])
    if "DCA_SWEEP_MIN" in env:
        minN = int(env["DCA_SWEEP_MIN"])
    if "DCA_SWEEP" in env and int(env["DCA_SWEEP"]) == 0:
        minN = INT_MAX
    if "DCA_SWEEP_PANEL" in env:
        wide = narrow = max(128, int(env["DCA_SWEEP_PANEL"]) // 128 * 128)
    return minN, wide, narrow, wideMinN, factorMaxN


def sweep_runs(np_, env=()):
    """whether an inverse of padded size np is swept under these variables (sweep_wanted of cholinv_plan.h: the size threshold, two
    panels at least, and the workspace 4 n B + 7 B^2 doubles and 8 counters per panel within the 2 n^2 doubles of the callers).
    The GPU tests choose their swept cases by it without the driver; the host test holds it to the driver at every size."""
    minN, wide, narrow, wideMinN, _ = cfg_of(dict(env))
    B = wide if np_ >= wideMinN else narrow
    return np_ >= minN and np_ >= 2 * B and 4 * np_ * B + 7 * B * B + (np_ // B + 2) * 8 + 8 <= 2 * np_ * np_


def knob_key(env):
    return tuple(sorted(env.items()))


def compile_plan_driver(directory):
    """tests/cholinv_plan_driver.cpp compiled with the host compiler -> plan(np, env) = dict(n, swept, B, factorForm, sideSet,
    small32Max, ops = [dict(op = leaf / gemm / panel / update, ...)] in issue order)"""
    exe = os.path.join(str(directory), "cholinv_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cholinv_plan_driver.cpp")])
    cache = {}

    def plan(np_, env=()):
        env = dict(env)
        key = (np_,) + cfg_of(env)
        if key not in cache:
            out = subprocess.check_output([exe] + [str(v) for v in key]).decode().splitlines()
            head = out[0].split()
            assert head[0] == "inverse" and int(head[1]) == np_
            p = dict(zip(["n", "swept", "B", "factorForm", "sideSet", "small32Max"], [int(t) for t in head[1:]]))
            ops = []
            for ln in out[1:]:
                t = ln.split()
                if t[0] == "leaf":
                    ops.append(dict(op="leaf", size=int(t[1]), buf=t[2], off=int(t[3]), pivotBase=int(t[4]), stream=t[5]))
                elif t[0] == "gemm":
                    ops.append(dict(op="gemm", tag=t[1], form=t[2], buf=t[3], off=int(t[4]), M=int(t[5]), N=int(t[6]), K=int(t[7]), maskA=int(t[8]),
                                    maskB=int(t[9]), lowerOnly=int(t[10]), walk=int(t[11]), stream=t[12], cin=int(t[13])))
                elif t[0] == "panel":
                    ops.append(dict(op="panel", p=int(t[1]), c=int(t[2]), w=int(t[3])))
                elif t[0] == "update":
                    ops.append(dict(op="update", kind=t[1], p=int(t[2]), tiles=int(t[3]), stream=t[4]))
                else:
                    raise AssertionError(ln)
            p["ops"] = ops
            cache[key] = p
        return cache[key]

    plan.forms = tuple(subprocess.check_output([exe, "forms"]).decode().split())
    plan.defaults = tuple(int(t) for t in subprocess.check_output([exe, "defaults"]).decode().split())
    return plan


ALL_FORMS = ("small32", "small32pair", "dma64", "dma128", "dma128x64", "dma128banded")


def features(p):
    """what one inverse exercises: kernel form x stream of every product, leaf kinds, the sweep's form and panel width"""
    f = set()
    for o in p["ops"]:
        if o["op"] == "gemm":
            f.add(("form", o["form"], o["stream"]))
        elif o["op"] == "leaf":
            f.add(("leaf", o["size"]))
    if p["swept"]:
        f.add(("sweep", "factor" if p["factorForm"] else "P", p["B"]))
        ws = [o["w"] for o in p["ops"] if o["op"] == "panel"]
        if ws[-1] != p["B"]:
            f.add(("sweep", "ragged last panel"))
        if ws[-1] == 64:
            f.add(("sweep", "64-column last panel"))
        if p["n"] % 128 == 64:
            f.add(("sweep", "last tile row of 64"))
    else:
        f.add(("recursion", "side fork" if any(o["op"] == "gemm" and o["stream"] == "side" for o in p["ops"]) else "in line"))
    return f


class Case:
    def __init__(self, n, env=(), kron=None, why=""):
        self.n, self.env, self.kron, self.why = n, dict(env), kron, why
        self.np = (n + 63) // 64 * 64
        assert kron is None or kron[0] * kron[1] == n
        self.name = "n%d%s%s" % (n, "" if not kron else "_%dx%d" % kron, "".join("_%s%s" % (k.replace("DCA_SWEEP", "S").replace("_", ""), v) for k, v in sorted(self.env.items())))

    @property
    def base(self):
        """the name without the knobs: the matrix (and the key of LAPACK_MEASURED)"""
        return "n%d%s" % (self.n, "" if not self.kron else "_%dx%d" % self.kron)

    def __repr__(self):
        return self.name


def kron_dims(np_, ragged=False):
    """n in (np - 64, np] as a product of two factors between 8 and 128: np itself as 64 x (np / 64), or -- ragged -- the largest n below it"""
    if not ragged and np_ // 64 >= 8:
        return (64, np_ // 64) if np_ // 64 <= 128 else None
    for n in range(np_ - 1, np_ - 64, -1):
        for m1 in range(128, 7, -1):
            if n % m1 == 0 and 8 <= n // m1 <= 128:
                return (m1, n // m1)
    return None


def make_case(np_, env=(), ragged=False, why=""):
    """the case of padded size np: unstructured below 448, a Kronecker product above"""
    if np_ <= 448:
        return Case(np_ - (27 if ragged else 0), env, None, why)
    k = kron_dims(np_, ragged)
    assert k, np_
    return Case(k[0] * k[1], env, k, why)


SCAN_MAX = 8192
PADDING_EDGES = (1, 63, 64, 65, 127, 129)
SWEEP_THRESHOLDS = (2560, 4500, 7000)


def derive_table(plan):
    """The case table from the driver (nothing chosen by eye): for every feature (features()) the smallest padded size that reaches
    it under default settings or, where one of the knob sets the tests already use reaches it sooner, under that set; that size
    and one 64-step to either side; the padding edges; the sweep's thresholds with a 64-step to either side."""
    first = {}
    for env in KNOB_SETS:
        for np_ in range(64, SCAN_MAX + 1, 64):
            for f in features(plan(np_, env)):
                if f not in first or np_ < first[f][0]:
                    first[f] = (np_, env)
    cases = {}

    def add(c):
        cases.setdefault(c.name, c)

    for n in PADDING_EDGES:
        add(Case(n, (), None, "padding edge"))
    add(make_case(448, (), True, "unstructured, ragged"))
    for f, (np_, env) in sorted(first.items(), key=lambda kv: (kv[1][0], str(kv[0]))):
        for d in (-64, 0, 64):
            if 64 <= np_ + d <= SCAN_MAX:
                add(make_case(np_ + d, env, False, "%s%s" % (f, "" if d == 0 else " %+d" % d)))
    for t in SWEEP_THRESHOLDS:
        for d in (-64, 0, 64):
            add(make_case((t + 63) // 64 * 64 + d, (), False, "threshold %d %+d" % (t, d)))
    add(make_case(2560, (), True, "default sweep, ragged n"))
    add(make_case(1088, KNOB_SETS[1], True, "forced sweep (from X), ragged n"))
    add(make_case(1088, KNOB_SETS[3], True, "forced sweep (through P), ragged n"))
    return sorted(cases.values(), key=lambda c: (knob_key(c.env), c.n)), first


# The derived table, pinned so that the GPU tests can be parametrised without the driver: (n, Kronecker factors, index into
# KNOB_SETS).  tests/test_spd_inverse_audit_host.py asserts that derive_table() gives exactly this.
PINNED_TABLE = (
    (1, None, 0), (63, None, 0), (64, None, 0), (65, None, 0), (127, None, 0), (128, None, 0), (129, None, 0),
    (192, None, 0), (256, None, 0), (421, None, 0), (1280, (64, 20), 0), (1344, (64, 21), 0), (1408, (64, 22), 0),
    (2432, (64, 38), 0), (2496, (64, 39), 0), (2556, (71, 36), 0), (2560, (64, 40), 0), (2624, (64, 41), 0),
    (4480, (64, 70), 0), (4544, (64, 71), 0), (4608, (64, 72), 0), (5952, (64, 93), 0), (6016, (64, 94), 0),
    (6080, (64, 95), 0), (6976, (64, 109), 0), (7040, (64, 110), 0), (7104, (64, 111), 0), (2880, (64, 45), 5),
    (2944, (64, 46), 5), (3008, (64, 47), 5), (8128, (64, 127), 5), (8192, (64, 128), 5), (384, None, 3), (448, None, 3),
    (512, (64, 8), 3), (1085, (35, 31), 3), (768, (64, 12), 4), (832, (64, 13), 4), (896, (64, 14), 4), (384, None, 1),
    (448, None, 1), (512, (64, 8), 1), (1085, (35, 31), 1), (768, (64, 12), 2), (832, (64, 13), 2), (896, (64, 14), 2),
)


def pinned_cases():
    return [Case(n, KNOB_SETS[k], kron) for n, kron, k in PINNED_TABLE]


def plain_inverse(A):
    """(X, E) for a matrix whose entries are general float64 numbers (the mfDCA correlation matrix): longdouble Gauss-Jordan and one
    Newton step X + X (I - A X) in longdouble.  No exact residual here: the error left is a few longdouble roundings of E's
    size, 2^-11 u E each."""
    X = gauss_jordan(A)
    Al = np.array(A, dtype=LD)
    X = X + X @ (np.eye(A.shape[0], dtype=LD) - Al @ X)
    X = (X + X.T) / 2
    return X, bound_matrix(np.asarray(A, dtype=np.float64), X)


# ----------------------------------------------------------------------------- the float64 restatement
class Fault:
    """One planted fault; `hit` is set where it was applied."""

    def __init__(self, kind):
        self.kind, self.hit = kind, None


FAULTS = ("syrk k-tile of 16 dropped", "sweep tile stale", "mask k < row on a diagonal tile", "output tile not mirrored",
          "padding diagonal 0", "Cin read from C", "one element off by 1e-10", "one element off by 1e-10 of the largest")


def pad(A, diag=1.0):
    """dca_spd_inverse's padding: the lower triangle mirrored, rows / columns up to a multiple of 64 as an identity block"""
    n = A.shape[0]
    np_ = (n + 63) // 64 * 64
    P = np.zeros((np_, np_))
    P[:n, :n] = np.tril(A) + np.tril(A, -1).T
    for r in range(n, np_):
        P[r, r] = diag
    return P


def _masked(X, mask):
    return np.tril(X) if mask == 1 else np.triu(X) if mask == 2 else X


def _nt(Aop, maskA, Bop, maskB):
    return _masked(Aop, maskA) @ _masked(Bop, maskB).T


def _store(C, V, lowerOnly, Cm=None, fault=None, tag=None):
    """C <- V (the lower triangle only where lowerOnly), mirrored into Cm (Cm[j][i] = C[i][j], off the diagonal where lowerOnly)"""
    if lowerOnly:
        il = np.tril_indices(V.shape[0])
        C[il] = V[il]
    else:
        C[...] = V
    if Cm is not None:
        Vt = V.T.copy()
        if fault is not None and fault.kind == "output tile not mirrored" and fault.hit is None and V.shape[0] >= 128:
            Vt[0:64, 64:128] = Cm[0:64, 64:128]                  # tile (1, 0) of the output: its mirror image is never written
            fault.hit = tag
        if lowerOnly:
            iu = np.triu_indices(V.shape[0], 1)
            Cm[iu] = Vt[iu]
        else:
            Cm[...] = Vt


def _run_recursion(ops, i, buf, tmp, fault, top):
    """executes leaf / L21 / SYRK / TT / X21 lines on `buf` until a line that is none of them; returns the next index"""
    while i < len(ops):
        o = ops[i]
        if o["op"] == "leaf":
            s, f = o["size"], o["off"]
            blk = buf[f:f + s, f:f + s]
            low = np.tril(blk)
            if np.isnan(low).any():
                raise AssertionError("a leaf reads undefined storage")
            try:
                L = np.linalg.cholesky(low + np.tril(low, -1).T)
            except np.linalg.LinAlgError:
                raise np.linalg.LinAlgError("not positive definite in the leaf at pivot base %d" % o["pivotBase"])
            from scipy.linalg import solve_triangular
            X = np.tril(solve_triangular(L, np.eye(s), lower=True))
            blk[...] = X + np.tril(X, -1).T
        elif o["op"] == "gemm" and o["tag"] in ("L21", "SYRK", "TT", "X21"):
            f, tag = o["off"], o["tag"]
            if tag == "L21":
                n2, n1 = o["M"], o["N"]
                tmp[("n", f)] = (n1, n2)
            n1, n2 = tmp[("n", f)]
            M11, M12 = buf[f:f + n1, f:f + n1], buf[f:f + n1, f + n1:f + n1 + n2]
            M21, M22 = buf[f + n1:f + n1 + n2, f:f + n1], buf[f + n1:f + n1 + n2, f + n1:f + n1 + n2]
            if tag == "L21":
                assert (o["M"], o["N"], o["K"]) == (n2, n1, n1)
                V = _nt(M21, o["maskA"], M11, o["maskB"])
                if fault is not None and fault.kind == "mask k < row on a diagonal tile" and fault.hit is None and top and n1 >= 128:
                    # output tile column 1 (64 columns): its rows of the triangular operand lose their diagonal element
                    Bm = np.tril(M11[64:128]).copy()
                    Bm[np.arange(64), 64 + np.arange(64)] = 0.0
                    V[0:64, 64:128] = M21[0:64] @ Bm.T
                    fault.hit = "L21 at offset %d" % f
                tmp[("L21", f)] = V
            elif tag == "SYRK":
                assert (o["M"], o["N"], o["K"], o["lowerOnly"]) == (n2, n2, n1, 1)
                L21 = tmp[("L21", f)]
                P = _nt(L21, o["maskA"], L21, o["maskB"])
                if fault is not None and fault.kind == "syrk k-tile of 16 dropped" and fault.hit is None and top and n2 >= 128 and n1 >= 64:
                    P[64:128, 0:64] -= L21[64:128, 16:32] @ L21[0:64, 16:32].T
                    fault.hit = "SYRK at offset %d" % f
                _store(M22, M22 - P, 1)
            elif tag == "TT":
                if o["form"] == "dma128banded":
                    # one line per band of tile rows: the bands together are the whole product
                    done = tmp.get(("TTrows", f), 0)
                    if done == 0:
                        tmp[("Tt", f)] = np.full((n1, n2), np.nan)
                    rows = slice(done, done + o["M"])
                    tmp[("Tt", f)][rows] = np.triu(M11)[rows] @ tmp[("L21", f)].T
                    tmp[("TTrows", f)] = done + o["M"]
                else:
                    assert (o["M"], o["N"], o["K"]) == (n1, n2, n1)
                    tmp[("Tt", f)] = _nt(M11, o["maskA"], tmp[("L21", f)], o["maskB"])
            else:
                assert (o["M"], o["N"], o["K"]) == (n2, n1, n2)
                Tt = tmp[("Tt", f)]
                assert not np.isnan(Tt).any()
                _store(M21, -_nt(M22, o["maskA"], Tt, o["maskB"]), 0, M12, fault if top else None, "X21 at offset %d" % f)
        else:
            break
        i += 1
    return i


def restate(A, plan_, fault=None):
    """The inverse of the PADDED matrix A (both halves) in float64 in the order of the launch list plan_; returns the padded
    result.  fault: a Fault applied at its first eligible place."""
    n = plan_["n"]
    assert A.shape == (n, n)
    ops = plan_["ops"]
    M = A.copy()
    if not plan_["swept"]:
        i = _run_recursion(ops, 0, M, {}, fault, True)
        o = ops[i]
        assert o["tag"] == "XTX" and i == len(ops) - 1 and (o["maskA"], o["maskB"], o["lowerOnly"]) == (2, 2, 1)
        out = np.full((n, n), np.nan)
        _store(out, _nt(M, 2, M, 2), 1, out)
        return out
    B = plan_["B"]
    M[np.triu_indices(n, 1)] = np.nan                      # the sweep keeps the lower triangle; the upper one is stale until the end
    panels = [o for o in ops if o["op"] == "panel"]
    S = [np.full((B, B), np.nan), np.full((B, B), np.nan)]
    Pb = [None, None]
    S[0][:panels[0]["w"], :panels[0]["w"]] = A[:panels[0]["w"], :panels[0]["w"]]

    def gather(c, w):
        Q = np.empty((n, w))
        Q[c:] = M[c:, c:c + w]
        Q[:c] = M[c:c + w, :c].T
        return Q

    Q = gather(0, panels[0]["w"])
    i = 0
    for p, po in enumerate(panels):
        assert ops[i] is po
        c, w = po["c"], po["w"]
        last = p + 1 == len(panels)
        c1, w1 = (n, 0) if last else (panels[p + 1]["c"], panels[p + 1]["w"])
        Sp = S[p & 1][:w, :w]
        i = _run_recursion(ops, i + 1, Sp, {}, None, False)
        Wn = None
        P = None
        while i < len(ops) and ops[i]["op"] == "gemm":
            o = ops[i]
            if o["tag"] == "P":
                P = np.full((w, w), np.nan)
                _store(P, _nt(Sp, o["maskA"], Sp, o["maskB"]), o["lowerOnly"], P)
            elif o["tag"] == "WN":
                MnJ = M[c1:c1 + w1, c:c + w]
                assert (o["M"], o["N"], o["K"]) == (w1, w, w)
                Wn = _nt(MnJ, o["maskA"], Sp if plan_["factorForm"] else P, o["maskB"])
            elif o["tag"] == "S":
                Sn = S[(p + 1) & 1]
                Cin = M[c1:c1 + w1, c1:c1 + w1]
                if not o["cin"]:
                    Sn[:w1, :w1] = Cin                    # copy_block: the whole block, stale upper half included
                    Cin = Sn[:w1, :w1]
                elif fault is not None and fault.kind == "Cin read from C" and fault.hit is None and p >= 1:
                    # one 64 x 64 output tile below the diagonal takes what the output buffer held there (the pivot block of two
                    # steps ago); the whole block read so would only stop the factorisation
                    Cin = Cin.copy()
                    Cin[64:128, 0:64] = np.nan_to_num(Sn[64:128, 0:64])
                    fault.hit = "S of step %d, tile (1, 0)" % p
                _store(Sn[:w1, :w1], Cin - _nt(Wn, 0, Wn if plan_["factorForm"] else MnJ, 0), o["lowerOnly"])
                Sn[:w1, :w1][np.triu_indices(w1, 1)] = np.nan
            elif o["tag"] == "W":
                assert (o["M"], o["N"], o["K"]) == (n, w, w) and not np.isnan(P).any()
                W = _nt(Q, 0, P, 0)
            else:
                raise AssertionError(o)
            i += 1
        # finalize: the swept panel in the lower triangle
        M[c + w:, c:c + w] = W[c + w:]
        M[c:c + w, :c] = W[:c].T
        blk = M[c:c + w, c:c + w]
        il = np.tril_indices(w)
        blk[il] = (-P)[il]
        # the rank-w update of every lower element outside the pivot rows and columns, but for the next pivot block (the chain's)
        while i < len(ops) and ops[i]["op"] == "update":
            i += 1
        idx = np.r_[0:c, c + w:n]
        if idx.size:
            Dl = np.tril(W[idx] @ Q[idx].T)
            if w1:
                a = np.searchsorted(idx, c1)
                Dl[a:a + w1, a:a + w1] = 0.0
            if fault is not None and fault.kind == "sweep tile stale" and fault.hit is None and p == 1:
                Dl[-192:-64, 0:128] = 0.0                    # one 128 x 128 tile keeps its previous value
                fault.hit = "update of step %d" % p
            sub = M[np.ix_(idx, idx)]
            il = np.tril_indices(idx.size)
            sub[il] = sub[il] - Dl[il]
            M[np.ix_(idx, idx)] = sub
        if not last:
            Q = gather(c1, w1)
    assert i == len(ops)
    low = np.tril(M)
    assert not np.isnan(low).any()
    out = -(low + np.tril(low, -1).T)
    return out


def restated_inverse(A, plan, env=(), fault=None):
    """restate() on dca_spd_inverse's padding of A, cut back to n x n.  A planted fault that makes the factorisation stop comes
    back as None (the device would report DCA_ERR_NOT_SPD)."""
    n = A.shape[0]
    P = pad(A, 0.0 if fault is not None and fault.kind == "padding diagonal 0" else 1.0)
    if fault is not None and fault.kind == "padding diagonal 0":
        fault.hit = "rows %d .. %d" % (n, P.shape[0] - 1)
    try:
        with np.errstate(all="ignore"):
            out = restate(P, plan(P.shape[0], env), fault)[:n, :n]
    except np.linalg.LinAlgError:
        return None
    if fault is not None and fault.kind == "one element off by 1e-10":
        out = out.copy()
        i, j = (2 * n) // 3, n // 3
        out[i, j] += 1e-10
        out[j, i] = out[i, j]
        fault.hit = "element (%d, %d)" % (i, j)
    if fault is not None and fault.kind == "one element off by 1e-10 of the largest":
        # the same fault in the measure of the old criterion, which is relative to the inverse's size: where the largest entry of
        # A^-1 is 14 (n = 421, shift 0.01) the element moves by 1.4e-9 and the Frobenius ratio stays near its value at shift 0.5
        out = out.copy()
        i, j = (2 * n) // 3, n // 3
        out[i, j] += 1e-10 * float(np.abs(out).max())
        out[j, i] = out[i, j]
        fault.hit = "element (%d, %d)" % (i, j)
    return out
