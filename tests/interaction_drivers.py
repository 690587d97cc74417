"""The host-side drivers of the interaction tests: tests/interaction_plan_driver.cpp (pydca_amd/csrc/interaction_plan.h) and
tests/assignment_driver.cpp (pydca_amd/csrc/assignment.h), compiled with the host compiler and run as child processes."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FLAGS = ["g++", "-std=c++17", "-O1", "-fno-fast-math", "-ffp-contract=off", "-Wall"]


def compile_plan_driver(directory):
    """tests/interaction_plan_driver.cpp compiled with the host compiler -> plan(q, LB, cnt=(), cross_pass=None) = dict"""
    exe = os.path.join(str(directory), "interaction_plan_driver")
    subprocess.check_call(HOST_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "interaction_plan_driver.cpp")])

    def plan(q, LB, cnt=(), cross_pass=None):
        env = dict(os.environ)
        env.pop("DCA_CROSS_PASS", None)
        if cross_pass is not None:
            env["DCA_CROSS_PASS"] = str(cross_pass)
        return json.loads(subprocess.check_output([exe, str(q), str(LB)] + [str(int(c)) for c in cnt], env=env))
    return plan


def compile_assignment_driver(directory, sanitize=False):
    """tests/assignment_driver.cpp (assignment.h alone) -> solve(list of 2-D arrays) = list of (rc, total, cols, gaps)"""
    exe = os.path.join(str(directory), "assignment_driver" + ("_san" if sanitize else ""))
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(HOST_FLAGS + extra + ["-o", exe, os.path.join(ROOT, "tests", "assignment_driver.cpp")])

    def solve(problems, shapes=None):
        text = []
        for k, E in enumerate(problems):
            E = np.asarray(E, dtype=np.float64)
            nr, nc = E.shape if shapes is None else shapes[k]
            text.append("%d %d\n%s\n" % (nr, nc, " ".join(float(v).hex() for v in E.ravel())))
        out = subprocess.run([exe], input="".join(text), capture_output=True, text=True, check=True).stdout.split("\n")
        res, k = [], 0
        for idx, E in enumerate(problems):
            nr = np.asarray(E).shape[0] if shapes is None else shapes[idx][0]
            rc, total = out[k].split()
            k += 1
            cols, gaps = [], []
            if int(rc) == 0:
                for _ in range(max(nr, 0)):
                    c, g = out[k].split()
                    k += 1
                    cols.append(int(c))
                    gaps.append(float.fromhex(g))
            res.append((int(rc), float.fromhex(total), np.array(cols, dtype=np.int64), np.array(gaps)))
        return res
    return solve
