"""Generate tests/golden/shortcut_paths.npz: the paths the CPU restatement's
search (oracle.OracleTerrain.plan) finds for the path-shortcutting tests'
cases (tests/shortcut_cases.py FOUND, plain and adaptive), states [n][8] and
actions [n-1][10] per case, plain data (np.savez, no pickle).

    python tools/make_shortcut_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import shortcut_cases as C  # noqa: E402


def main(out=C.GOLDEN):
    arrays = {}
    for case, batch, seed in C.FOUND:
        for adaptive in (False, True):
            S, A = C.plan_path(case, batch, seed, adaptive)
            k = C.path_key(case, batch, seed, adaptive)
            arrays[k + "_states"], arrays[k + "_actions"] = S, A
            print(k, S.shape[0], "states")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
