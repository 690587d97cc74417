#!/usr/bin/env python3
"""dca_plm_interaction_energies under the column-strip decomposition, which needs two ranks: two host THREADS on one GPU over the
stand-in tests/fake_rccl/libfake_rccl.so, in a process of its own (the library binds the first librccl it opens).  Every rank
expects DCA_ERR_STATE (the entry runs on one GPU only) before anything collective happens.  Prints one JSON line."""
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import golden  # noqa: E402
from pydca_amd import _lib  # noqa: E402

FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


def main():
    world = 2
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    x0 = np.zeros(L * q + L * (L - 1) // 2 * q * q, dtype=np.float32)
    uid = _lib.comm_unique_id(FAKE)
    out = [None] * world

    def run(rank):
        try:
            s = _lib.Context(0, _lib.DCA_F32)
            s.set_msa(X, q)
            s.set_weights(np.ones(X.shape[0]))
            s.comm_init(uid, world, rank, FAKE)
            s.plm_configure_strips(1.8, 1.8)
            s.plm_set_x(x0)
            try:
                s.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4)
                out[rank] = dict(code=_lib.DCA_OK, message="")
            except _lib.DcaBackendError as e:
                out[rank] = dict(code=e.code, message=str(e))
            s.close()
        except Exception as e:          # noqa: BLE001
            out[rank] = dict(code=None, message="%s: %s" % (type(e).__name__, e))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
