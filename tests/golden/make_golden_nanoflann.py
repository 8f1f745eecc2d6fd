"""Writes tests/golden/nanoflann_ref_golden.npz: what the reference's vendored nanoflann (include/nanoflann.hpp and
include/KDTreeVectorOfVectorsAdaptor.h, compiled into oracle/_ref by oracle/Makefile) returns for the inputs of
tests/test_oracle_cpu.py::test_knn_against_vendored_nanoflann and
tests/test_scancontext_cpu.py::test_ringkey_search_with_fewer_keys_than_candidates_and_ties, so that both tests run
where the reference tree is absent.  Needs oracle/_ref:  python tests/golden/make_golden_nanoflann.py

Stored: the 5-NN indices and squared distances of every query of the `small` configuration with a SHA-256 digest of
its map and queries (so a test can tell a changed input from a changed result), and (indices, squared distances,
found) of the three ring-key searches of the tie test.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from conftest import transform_points              # noqa: E402
from liorf_amd import synth                         # noqa: E402
from oracle import oracle as O                      # noqa: E402
from test_oracle_cpu import input_sha256            # noqa: E402
from test_scancontext_cpu import ringkey_tie_cases  # noqa: E402


def main():
    cfg = synth.make_config("small")
    m = cfg["map"]
    q = transform_points(O.getTransformation(cfg["pose_init"]), cfg["scan"])
    res = O.nanoflann_knn5(m, q)
    if res is None:
        raise SystemExit("oracle/_ref/libnanoflann_ref.so is not built: run build() where the reference tree is present")
    nidx, nd2 = res
    cases = ringkey_tie_cases()
    rk = [O.nanoflann_ringkey_knn(k, qq, 3) for k, qq in cases]
    out = os.path.join(HERE, "nanoflann_ref_golden.npz")
    np.savez_compressed(out, knn5_input_sha256=np.array(input_sha256(m, q)), knn5_idx=nidx, knn5_d2=nd2,
                        ringkey_idx=np.stack([r[0] for r in rk]), ringkey_d2=np.stack([r[1] for r in rk]),
                        ringkey_found=np.array([r[2] for r in rk], np.int32))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
