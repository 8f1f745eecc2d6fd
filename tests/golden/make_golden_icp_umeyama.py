"""Records tests/golden/icp_umeyama_bits.npz: the T words host_umeyama (liorf_amd/csrc/s2m_icp_close.hpp, built stand-alone by
the host compiler with -O2 -ffp-contract=off) gives for every case of tests/ref/icp_close_ref.py:umeyama_classes() whose
cross-covariance is not of exact rank 0 or 1, and for every case of tests/test_icp_grid_cpu.py:_umeyama_cases().

Recorded once, on the commit before U's completion for rank 0 and rank 1 was added to host_svd3, so that
tests/test_icp_close_cpu.py can hold every later header to those bits wherever the rank is 2 or 3. Run it again only to add
cases, and then on a header whose bits for the cases already recorded are unchanged (the script checks that).

    python tests/golden/make_golden_icp_umeyama.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "ref")):
    if p not in sys.path:
        sys.path.insert(0, p)

import icp_close_ref as R  # noqa: E402
from test_icp_grid_cpu import _umeyama_cases  # noqa: E402

OUT = os.path.join(HERE, "icp_umeyama_bits.npz")


def golden_cases():
    """(names, inputs (n, 15) fp32): the classes that are not exactly degenerate, then the cases of test_icp_grid_cpu"""
    names, rows = [], []
    for name, ms, mt, sg in R.umeyama_classes():
        if R.is_degenerate(name):
            continue
        names.append(name)
        rows.append(np.concatenate([ms, mt, sg.reshape(-1)]))
    for k, (ms, mt, sg) in enumerate(_umeyama_cases()):
        names.append(f"grid_cpu_{k}")
        rows.append(np.concatenate([ms, mt, sg.reshape(-1)]))
    return np.array(names), np.array(rows, np.float32)


def main():
    names, rows = golden_cases()
    with tempfile.TemporaryDirectory(prefix="icp_close_") as d:
        exe = R.build_close_exe(d)
        T = R.run_umeyama(exe, [(r[0:3], r[3:6], r[6:15]) for r in rows])
    if os.path.exists(OUT):
        old = np.load(OUT)
        keep = {(n, i.tobytes()): t for n, i, t in zip(old["names"], old["inputs"].view(np.uint32), old["T"])}
        for k, (n, i, t) in enumerate(zip(names, rows.view(np.uint32), T)):
            was = keep.get((n, i.tobytes()))
            if was is None:
                continue
            sg = rows[k, 6:15].reshape(3, 3)
            if min(np.any(sg != 0, 1).sum(), np.any(sg != 0, 0).sum()) <= 1:
                T[k] = was                                     # exact rank 0 or 1 (in _umeyama_cases): kept as recorded, not compared
            elif not np.array_equal(was, t):
                raise SystemExit(f"{n}: this header does not give the recorded bits; nothing written")
    np.savez_compressed(OUT, names=names, inputs=rows, T=T)
    print(f"wrote {OUT}: {len(names)} cases")


if __name__ == "__main__":
    main()
