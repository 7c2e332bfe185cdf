import os
import sys

import pytest

# The fp32 oracle and the fp32 golden vectors are IEEE fp32 arithmetic.  A host default of ONEDNN_DEFAULT_FPMATH_MODE=BF16
# (or TF32 / ANY) lets torch's CPU convolutions round their fp32 operands to 16 bits; oneDNN reads the mode once, at its first
# primitive, so it is pinned here, before any test module runs a convolution (worker processes inherit it).
os.environ['ONEDNN_DEFAULT_FPMATH_MODE'] = 'STRICT'

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def pytest_configure(config):
  config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu on the GPU box)')


@pytest.fixture(scope='session')
def golden_dir():
  return os.path.join(ROOT, 'tests', 'golden')
