"""The plmDCA evaluation and optimiser give the SAME BITS as the recorded commit at the shapes that reach each launch path of
the scatter stage (pydca_amd/csrc/plm_plan.h: plm_scatter_stage) and its neighbours.  tests/golden/plm_eval_pins.json holds,
per case, the sha256 of fx, of the gradient at plm_init_x, and of x after three L-BFGS iterations from there, recorded on an
MI355X with the library of the commit it names.  There is no tolerance: a mismatch is a launch that got other arguments, or a
summation order changed on purpose -- then run this module as a script on the GPU box to record the file anew
(python tests/test_plm_eval_pins.py <commit id> [output path]) and say so in the pull request.

Alignments come from a closed formula, X[n, i] = (7 n + 13 i + (n i mod 5)) mod q, weights from compute_weights(0.8), the
regularisation is smoke()'s."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PINS = os.path.join(ROOT, "tests", "golden", "plm_eval_pins.json")
LAMBDAS = {5: (1.8, 1.8), 21: (1.0, 5.0)}

# name: (precision bits, q, N, L, halo, environment, what the shape reaches)
CASES = {
    "f32_q21_300x7": (32, 21, 300, 7, 0, {}, "2 strips: (strip, split) pairs dealt to the XCDs"),
    "f32_q21_3000x60": (32, 21, 3000, 60, 0, {}, "10 strips, split 2 in blockIdx.y, two slabs folded"),
    "f32_q21_3000x60_rem": (32, 21, 3000, 60, 0, {"DCA_SCATTER_REM": "1"}, "left-over strips merged behind the main ones, column slab sum"),
    "f32_q5_16600x13": (32, 5, 16600, 13, 0, {}, "site pairs, tile 10, split 10, streaming slab sum"),
    "f32_q5_2000x151": (32, 5, 2000, 151, 0, {}, "site pairs, tile 11, odd L"),
    "f32_q21_3000x60_halo64": (32, 21, 3000, 60, 64, {}, "halo"),
    "f64_q21_1700x55": (64, 21, 1700, 55, 0, {}, "one workgroup, 8 waves"),
    "f64_q21_33000x40": (64, 21, 33000, 40, 0, {}, "slab per block, 3 blocks"),
    "f64_q5_2000x151": (64, 5, 2000, 151, 0, {}, "per-chunk column sums"),
}


def alignment(N, L, q):
    n = np.arange(N, dtype=np.int64)[:, None]
    i = np.arange(L, dtype=np.int64)[None, :]
    return ((7 * n + 13 * i + (n * i) % 5) % q).astype(np.uint8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def evaluate(name):
    """{"fx", "g", "x3"}: the hashes of one case, under its environment"""
    from pydca_amd import _lib
    bits, q, N, L, halo, env, _ = CASES[name]
    dtype = np.float32 if bits == 32 else np.float64
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = _lib.Context(0, _lib.DCA_F32 if bits == 32 else _lib.DCA_F64)
        ctx.set_msa(alignment(N, L, q), q)
        ctx.compute_weights(0.8)
        ctx.plm_configure(*LAMBDAS[q], halo=halo)
        ctx.plm_init_x()
        fx = ctx.plm_gradient()
        out = {"fx": sha(np.float64(fx)), "g": sha(ctx.plm_get_g(dtype))}
        ctx.plm_lbfgs_begin(100)
        ctx.plm_lbfgs_iterate(3)
        out["x3"] = sha(ctx.plm_get_x(dtype))
        ctx.close()
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_as_recorded(name):
    with open(PINS) as f:
        pins = json.load(f)
    assert pins["commit"] and sorted(pins["cases"]) == sorted(CASES)
    got = evaluate(name)
    print(name, got)
    assert got == pins["cases"][name], "%s (%s): not the bits of commit %s" % (name, CASES[name][6], pins["commit"])


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit("usage: python tests/test_plm_eval_pins.py <id of the commit whose library is loaded> [output path]")
    record = {"commit": sys.argv[1], "cases": {name: evaluate(name) for name in sorted(CASES)}}
    with open(sys.argv[2] if len(sys.argv) > 2 else PINS, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(record, indent=1, sort_keys=True))
