"""tests/golden/engine_ws_bytes.json: the totals of the engine's workspace carves for a table of descriptors, so that a change of
csrc/orn_engine.hip's layout() (or of a size it asks another file for) shows on a machine without a GPU.  Per descriptor:
orn_engine_ws_bytes, orn_engine_batch_ws_bytes for 1 and 4 frames, orn_engine_eval_frames_ws_bytes for 1 and 8 frames; a refused
descriptor gives 0 and the library's error text.  The three size entries launch nothing.

    python tools/make_golden_engine_ws.py            # write the fixture from the library of this tree
    python tools/make_golden_engine_ws.py --check    # compare the library with the fixture (tests/test_engine_layout_host.py)
"""
import argparse
import json
import os
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(ROOT, 'tests', 'golden', 'engine_ws_bytes.json')

BRANCHES = ('ERB', 'NeRV_vanilla', 'ACB', 'RepVGG', 'ECB')
PRECISIONS = (0, 1, 2)
LOSSES = ('L2', 'Fusion6', 'Fusion10')
# the generator of tests/test_host_logic.py::_gen (720p) and its 1080p sibling
BIG = {'720p': [5, 2, 2, 2, 2], '1080p': [5, 3, 2, 2, 2]}


def _generator(fc, strides, lower_width, stem, branch, sin_res):
    """Shapes only (meta device): the descriptor needs no values."""
    import torch
    from orn_amd import model
    with torch.device('meta'):
        return model.Generator(embed_length=80, stem_dim_num=stem, fc_hw_dim=fc, expansion=1, num_blocks=1, norm='none', act='swish',
                               bias=True, reduction=2, conv_type='conv', stride_list=list(strides), sin_res=sin_res,
                               lower_width=lower_width, sigmoid=False, deploy=False, branch_type=branch)


def _sizes(gen, loss, precision):
    from orn_amd import _lib, engine
    L = _lib.lib()
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    d = engine.build_desc(gen, layout, total, loss, 0.5, 0.999, 1e-8, precision)
    rec = {'ws': int(L.orn_engine_ws_bytes(byref(d)))}
    if rec['ws'] == 0:
        rec['error'] = _lib.last_error()
    rec['batch'] = [int(L.orn_engine_batch_ws_bytes(byref(d), b)) for b in (1, 4)]
    rec['eval'] = [int(L.orn_engine_eval_frames_ws_bytes(byref(d), c)) for c in (1, 8)]
    return rec


def table():
    """{case name: sizes} of every descriptor of the table, from the library _lib.lib() loads."""
    import helpers
    out = {}
    for tag, strides in BIG.items():
        for branch in BRANCHES:
            for sin_res in (True, False):
                gen = _generator('9_16_26', strides, 96, '512_1', branch, sin_res)
                for precision in PRECISIONS:
                    for loss in LOSSES:
                        out[f'{tag}/{branch}/{"single" if sin_res else "multi"}/p{precision}/{loss}'] = _sizes(gen, loss, precision)
    for name, g in helpers.GEOS.items():
        gen = _generator(g['fc'], g['strides'], g['lower_width'], '32_1', 'ERB', True)
        out[f'geo/{name}/ERB/single/p2/Fusion6'] = _sizes(gen, 'Fusion6', 2)
    return out


def check():
    """Differences between the library and the fixture, one line each (empty: none)."""
    with open(PATH) as f:
        want = json.load(f)['cases']
    got = table()
    diff = [f'{k}: only in the {"fixture" if k in want else "library"}' for k in sorted(set(want) ^ set(got))]
    diff += [f'{k}: fixture {want[k]} library {got[k]}' for k in sorted(set(want) & set(got)) if want[k] != got[k]]
    return diff


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--check', action='store_true', help='compare instead of write; exit status 1 on a difference')
    args = ap.parse_args()
    if args.check:
        diff = check()
        print('\n'.join(diff) if diff else f'{PATH}: the library gives every size of the fixture')
        return 1 if diff else 0
    doc = {'what': 'bytes of orn_engine_ws_bytes (ws), orn_engine_batch_ws_bytes for 1 and 4 frames (batch) and '
                   'orn_engine_eval_frames_ws_bytes for 1 and 8 frames (eval); case = geometry/branch/heads/precision/loss; '
                   'error: the text behind ws = 0 (tools/make_golden_engine_ws.py)',
           'cases': table()}
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {PATH}: {len(doc["cases"])} cases')
    return 0


if __name__ == '__main__':
    sys.exit(main())
