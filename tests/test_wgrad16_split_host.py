"""The slab rule of the 16-bit weight gradient (orn_wgrad_bf16_split, csrc/orn_wgrad_bf16.hip) under a caller's cap, and the
workspace that has to hold its slabs (orn_wgrad_bf16_ws_floats), through orn_debug_wgrad16_split / _ws_floats (no GPU).

The rule is evaluated twice per step for a layer -- by the batched wgrad launch that writes the slabs and by the reduction launch
that reads them -- and the engine caps its last block (OrnWgradJob::smax).  A count that outgrows the workspace, or one that is not a
multiple of 8 (every problem of the batched launch starts on a multiple-of-8 work-group so that its XCD decode holds), would be a
silent change of the sum or a write beyond the slabs.  The workspace inequality holds in today's code; this test keeps it.  It also
pins the counts that the cases of tests/test_gpu_wgrad16_batch.py rely on."""
import itertools

import pytest

HS = (1, 2, 3, 7, 9, 17, 26, 33, 45, 64, 90, 135, 180, 270, 360, 540, 1080, 3997, 4000)
WS = (1, 5, 31, 32, 33, 63, 64, 65, 80, 97, 127, 160, 240, 320, 321, 480, 640, 959, 960)      # W % 32 in {0, 1, 31} among them
OS = (32, 96, 128, 384, 864, 1152, 2048)
PRODUCT = ((45, 80, 384), (90, 160, 384), (180, 320, 384), (360, 640, 384),                 # 720p L1..L4
           (45, 80, 864), (135, 240, 384), (270, 480, 384), (540, 960, 384))                 # 1080p L1..L4
SMALL = ((9, 33, 1152), (3, 5, 384), (17, 63, 864), (7, 97, 96), (33, 97, 128))              # the GPU cases' shapes that give 8 at every cap
PINNED = {      # (H, W, O) -> {smax: S}
    (64, 320, 128): {0: 24, 8: 8, 16: 16, 24: 24, 32: 32, 40: 40},
    (90, 160, 384): {0: 24, 8: 8, 16: 16, 24: 24, 32: 24, 40: 24},
    (26, 320, 384): {0: 16, 8: 8, 16: 16, 24: 16, 32: 16, 40: 16},
    (360, 640, 384): {0: 40, 24: 24},
}


@pytest.fixture(scope='module')
def L():
    import orn_amd
    from orn_amd import _build
    _build.build()
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_wgrad16_split', 'orn_debug_wgrad16_ws_floats'):
        assert hasattr(lib, name), name
    return lib


def _shapes():
    seen = set()
    for hwo in itertools.chain(PRODUCT, SMALL, PINNED, itertools.product(HS, WS, OS)):
        if hwo not in seen:
            seen.add(hwo)
            yield hwo


def test_split_under_every_cap_fits_the_workspace(L):
    n = 0
    for H, W, O in _shapes():
        ws = L.orn_debug_wgrad16_ws_floats(H, W, O)
        s0 = L.orn_debug_wgrad16_split(H, W, O, 0)
        for smax in range(0, 65):
            S = L.orn_debug_wgrad16_split(H, W, O, smax)
            at = f'H={H} W={W} O={O} smax={smax}: S={S}'
            assert S % 8 == 0 and 8 <= S <= 40, at
            if smax >= 8:                               # (smax / 8 * 8 is then at least 8)
                assert S <= smax // 8 * 8, at
            if 1 <= smax <= 7:
                assert S == s0, at + f', without a cap {s0}'
            assert S * (9 * O * 96 + O) <= ws, at + f' needs {S * (9 * O * 96 + O)} floats, the workspace has {ws}'
            n += 1
    assert n >= 65 * len(HS) * len(WS) * len(OS)


def test_split_values_the_gpu_cases_rely_on(L):
    for (H, W, O), row in PINNED.items():
        for smax, want in row.items():
            assert L.orn_debug_wgrad16_split(H, W, O, smax) == want, (H, W, O, smax)
    # a cap of 8 or more switches the "24 below 2000 K tiles" rule off: 64 x 320 x 128 rises above 24 only under a cap
    assert L.orn_debug_wgrad16_split(64, 320, 128, 48) == 40 and L.orn_debug_wgrad16_split(64, 320, 128, 7) == 24
    for H, W, O in SMALL:
        for smax in range(0, 65):
            assert L.orn_debug_wgrad16_split(H, W, O, smax) == 8, (H, W, O, smax)
