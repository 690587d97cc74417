"""TEST INFRASTRUCTURE ONLY: the device side of the SPD inverse audit (tests/test_spd_inverse_audit.py), importable and runnable.
sweep_cfg() of cholinv.hip is read once per process, so every case under DCA_SWEEP* knobs runs in a child process of its own:
    python spd_inverse_audit_child.py ratio n m1 m2      -> one JSON line per shift: worst err / (u E), position, symmetry, repeat, sha256
    python spd_inverse_audit_child.py hash n m1 m2       -> one JSON line per shift: sha256 of the inverse
    python spd_inverse_audit_child.py pivot n m1 m2 r..  -> one JSON line per planted row r: the error code and message
(m1 = m2 = 0: the unstructured family.)  The knobs come with the environment."""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spd_inverse_reference as R  # noqa: E402


def audit(L_, case, shift, repeat=True):
    """ctx.spd_inverse on the case's matrix in a context of its own -> dict(ratio, where, symmetric, repeat, sha, seconds)"""
    t0 = time.time()
    ref = R.reference(case, shift)
    A = ref.A
    ctx = L_.Context(0, L_.DCA_F64)
    inv = ctx.spd_inverse(A)
    same = bool(np.array_equal(inv, ctx.spd_inverse(A))) if repeat else None
    ctx.close()
    del A
    ratio, where = ref.ratio(inv)
    return dict(case=case.name, shift=shift, ratio=ratio, where=where, symmetric=bool(np.array_equal(inv, inv.T)), repeat=same,
                sha=hashlib.sha256(inv.tobytes()).hexdigest(), cond=ref.cond(), seconds=time.time() - t0)


def inverse_hash(L_, case, shift):
    ctx = L_.Context(0, L_.DCA_F64)
    inv = ctx.spd_inverse(R.matrix(case, shift))
    ctx.close()
    return dict(case=case.name, shift=shift, sha=hashlib.sha256(inv.tobytes()).hexdigest())


def pivot_report(L_, case, shift, row):
    """the matrix with A[row][row] = -1: (LAPACK's pivot, the device's error code, its message)"""
    A = R.matrix(case, shift)
    A[row, row] = -1.0
    ctx = L_.Context(0, L_.DCA_F64)
    code, msg = 0, ""
    try:
        ctx.spd_inverse(A)
    except L_.DcaBackendError as e:
        code, msg = e.code, str(e)
    ctx.close()
    return dict(case=case.name, row=row, potrf=R.potrf_pivot(A), code=code, message=msg, not_spd=L_.DCA_ERR_NOT_SPD)


def main(argv):
    from pydca_amd import _lib
    _lib.lib()
    mode, n, m1, m2 = argv[0], int(argv[1]), int(argv[2]), int(argv[3])
    case = R.Case(n, (), (m1, m2) if m1 else None)
    if mode == "pivot":
        for r in argv[4:]:
            print(json.dumps(pivot_report(_lib, case, 0.5, int(r))), flush=True)
        return
    for shift in R.SHIFTS:
        print(json.dumps(audit(_lib, case, shift) if mode == "ratio" else inverse_hash(_lib, case, shift)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
