import os
import sys

# Before torch loads MKL: the golden vectors hold CPU results of MKL's COMPATIBLE branch (tools/make_golden.py), the one branch
# MKL runs alike on every x86 host -- its AVX2 / AVX-512 branches are Intel-only, so AMD and Intel hosts would differ in the last bit
os.environ['MKL_CBWR'] = 'COMPATIBLE'

import numpy as np  # noqa: E402
import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu on the GPU box)')


def pytest_collection_modifyitems(config, items):
    """`-m gpu` tests are skipped (not failed) when no GPU is visible, e.g. in the build container."""
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason='no GPU visible')
    for item in items:
        if 'gpu' in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope='session')
def golden():
    def load(name):
        return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    return load
