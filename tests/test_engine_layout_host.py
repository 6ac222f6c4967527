"""The engine's workspace carves, pinned on the CPU: the three size entries (orn_engine_ws_bytes, orn_engine_batch_ws_bytes,
orn_engine_eval_frames_ws_bytes) launch nothing, and tests/golden/engine_ws_bytes.json holds what they must return -- for the 720p
and 1080p generators in every block kind, head form, precision and loss kind, and for the small geometries of helpers.GEOS -- so
that an edit of layout() that moves or resizes a `take` shows without a GPU.  Totals only: what is carved inside them is the GPU
suite's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tool():
    from orn_amd import _build
    _build.build()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import make_golden_engine_ws
    finally:
        sys.path.pop(0)
    return make_golden_engine_ws


def test_workspace_sizes_match_the_fixture(tool):
    """What `tools/make_golden_engine_ws.py --check` checks: every size, and the error text of every refused descriptor."""
    diff = tool.check()
    assert not diff, '\n'.join(diff)


def test_the_fixture_covers_the_table(tool):
    import json
    import helpers
    with open(tool.PATH) as f:
        cases = json.load(f)['cases']
    assert len(cases) == 2 * 5 * 2 * 3 * 3 + len(helpers.GEOS)
    assert all(c['ws'] > 0 or c['error'] for c in cases.values())
    # a multi-resolution engine needs every stage above 160 for MS-SSIM: stage 0 of these generators is 45 x 80
    refused = {k: c for k, c in cases.items() if c['ws'] == 0}
    assert refused and all('/multi/' in k and k.endswith('Fusion10') for k in refused)
    assert all(c['error'].startswith('engine: stage 0 (45x80): the MS-SSIM losses need a side above 160') and c['batch'] == [0, 0]
               and c['eval'] == [0, 0] for c in refused.values())
    ok = cases['720p/ERB/single/p2/Fusion6']
    # (the frame table and stats of 1 and of 4 frames both fit one 256-byte unit: the batch sizes may be equal)
    assert 0 < ok['batch'][0] <= ok['batch'][1] and 0 < ok['eval'][0] < ok['eval'][1]
