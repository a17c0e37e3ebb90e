import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
# MKL picks its code branch by CPU model, and the CPU oracle's first convolution (GEMM-based, 3 input channels) then sums its
# gradients in another order on every other CPU: round-off that tests/test_oracle.py's fixture comparisons resolve.  The fixtures
# were written on MKL's COMPATIBLE branch (tests/golden/make_golden.py), which gives the same bits on every x86 host.  MKL reads
# this on its first call, which no test has made yet.
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
