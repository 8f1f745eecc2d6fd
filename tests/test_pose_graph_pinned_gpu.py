"""The pose graph bit for bit against the commit before its kernels were folded into one family:
tests/ref/pose_graph_pin.py's digests - optimise, fp64 estimates, marginals, every operator and the CG in the single and the
block form, the launched optimise - equal tests/golden/pose_graph_pinned.json, which that commit's build wrote on an MI355X.
The other pose-graph tests compare forms with each other; since the forms share their kernels, this is the anchor."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref"))
import pose_graph_pin as PIN  # noqa: E402
from liorf_amd import s2m  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_graph_pinned.json")))["digests"]


@pytest.fixture(scope="module")
def pair():
    a, b = s2m.MapOptimizationS2M(), s2m.MapOptimizationS2M()
    yield a, b
    a.close()
    b.close()


def test_the_golden_file_holds_every_graph():
    assert sorted(GOLDEN) == sorted(PIN.GRAPHS)


@pytest.mark.parametrize("name", list(PIN.GRAPHS))
def test_digests_equal_the_pinned_commit(pair, name):
    got = PIN.graph_digests(pair[0], pair[1], name)
    want = GOLDEN[name]
    differ = sorted(key for key in set(got) | set(want) if got.get(key) != want.get(key))
    print(name, len(got), "digests, differing:", differ)
    assert got == want, differ
