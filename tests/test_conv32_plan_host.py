"""The case table of tests/test_gpu_conv32_forms.py reaches the kernel forms it names (no GPU).

orn_debug_conv_f32_plan reports what the fp32 conv launchers select for a block, from the selection functions the launchers call
themselves.  Every case of conv32_cases.py is run through it: form, split counts and tile counts are asserted, and
orn_conv3x3_ps_silu_bwd_ws_bytes must cover every region the plan implies (dy, Wd, S wgrad slabs, the dbias partial rows of either
producer, the dgrad's channel-split slabs).  The forms the table is there for are listed once more at the end and each must be
reached by at least one case."""
import pytest

import conv32_cases as K


@pytest.fixture(scope='module')
def L():
    import orn_amd
    from orn_amd import _build
    _build.build()
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_conv_f32_plan', 'orn_debug_conv_fwd_f32', 'orn_debug_head_fwd_z', 'orn_debug_conv_bwd_f32_head_ws_bytes',
                 'orn_debug_conv_bwd_f32_head'):
        assert hasattr(lib, name), name
    return lib


def _align(n, a=256):
    return -(-n // a) * a


def _ids(cases):
    return ['x'.join(map(str, c[0])) for c in cases]


@pytest.mark.parametrize('shape,want,what', K.FWD_CASES + K.BWD_CASES, ids=_ids(K.FWD_CASES + K.BWD_CASES))
def test_case_reaches_its_form(L, shape, want, what):
    p = K.plan(L, *shape[:5])
    got = {k: p[k] for k in want}
    assert got == want, f'{shape}: {what}: plan {p}'


@pytest.mark.parametrize('shape,want,what', K.BWD_CASES, ids=_ids(K.BWD_CASES))
def test_workspace_covers_the_plan(L, shape, want, what):
    B, C, O, H, W, s = shape
    p = K.plan(L, B, C, O, H, W)
    HW = H * W
    need = _align(B * O * HW * 4)                                          # dy
    need += _align(O * C * 9 * 4)                                          # Wd
    need += _align(p[K.WG_S] * O * C * 9 * 4)                              # wgrad slabs
    need += _align(max(p[K.DB_ROWS], B * p[K.HDB_ROWS]) * O * 4)           # dbias partial rows, the producer with more of them
    need += _align(p[K.DG_NSPLIT] * B * C * HW * 4) if p[K.DG_NSPLIT] > 1 else 0   # dgrad channel-split slabs
    have = L.orn_conv3x3_ps_silu_bwd_ws_bytes(B, C, O, H, W)
    assert have >= need, (shape, have, need, p)
    assert p[K.DG_NSPLIT] * p[K.DG_CPS] >= O > (p[K.DG_NSPLIT] - 1) * p[K.DG_CPS]      # the splits cover C_in = O, none is empty
    assert p[K.WG_S] <= p[K.WG_KT]                                         # no slab without a K tile


@pytest.mark.parametrize('hw,blocks,what', K.HEAD_HW, ids=[f'{h}x{w}' for (h, w), _, _ in K.HEAD_HW])
@pytest.mark.parametrize('Cn', K.HEAD_CN)
def test_head_cases(L, Cn, hw, blocks, what):
    H, W = hw
    C, O = K.HEAD_C, 4 * Cn
    p = K.plan(L, 1, C, O, H, W)
    assert p[K.HDB_ROWS] == blocks, (what, p)
    assert p[K.HDB_RED] == (K.RED_TALL if blocks >= 32 else K.RED_ROWS)
    conv = L.orn_conv3x3_ps_silu_bwd_ws_bytes(1, C, O, H, W)
    assert conv >= _align(O * H * W * 4) + _align(O * C * 9 * 4) + _align(p[K.WG_S] * O * C * 9 * 4) + _align(blocks * O * 4)
    have = L.orn_debug_conv_bwd_f32_head_ws_bytes(C, O, H, W)
    assert have >= _align(conv) + _align((blocks + 1) * (3 * Cn + 3) * 4) + _align(O * C * 9 * 4), (have, conv)
    if blocks == 33:
        assert (3 * Cn + 3) % 32 != 0
    assert L.orn_debug_conv_bwd_f32_head_ws_bytes(C, O + 1, H, W) == 0 and L.orn_debug_conv_bwd_f32_head_ws_bytes(C, O, 0, W) == 0


def test_every_named_form_is_reached(L):
    fwd = [(K.plan(L, *c[0][:5]), c[0]) for c in K.FWD_CASES]
    bwd = [(K.plan(L, *c[0][:5]), c[0]) for c in K.BWD_CASES]

    def some(cases, pred):
        return any(pred(p, c) for p, c in cases)
    # forward: SMALL x (the stride-2 epilogue, the general one); both sides of the 256 work-group threshold
    for small in (0, 1):
        assert some(fwd, lambda p, c: p[K.FWD_SMALL] == small and c[5] == 2)
        assert some(fwd, lambda p, c: p[K.FWD_SMALL] == small and c[5] != 2)
    assert some(fwd, lambda p, c: p[K.FWD_SMALL] == 0 and p[K.FWD_WGS] == 256)
    assert some(fwd, lambda p, c: p[K.FWD_SMALL] == 1 and p[K.FWD_WGS] == 4 * 248)
    # dgrad: small unsplit / split; 8-row tiles split / 64 + tail / tail alone / plain; the split at exactly 256 work-groups of a
    # shape that would otherwise take the tail
    assert some(bwd, lambda p, c: p[K.DG_SMALL] == 1 and p[K.DG_NSPLIT] == 1)
    assert some(bwd, lambda p, c: p[K.DG_SMALL] == 1 and p[K.DG_NSPLIT] > 1 and c[2] % p[K.DG_CPS] % 8 != 0)
    assert some(bwd, lambda p, c: p[K.DG_SMALL] == 0 and p[K.DG_NSPLIT] == 2 and c[1] % 64 == 0)
    assert some(bwd, lambda p, c: p[K.DG_SMALL] == 0 and p[K.DG_NSPLIT] == 2 and c[1] % 64 == 32 and p[K.DG_L32] == 0)
    assert some(bwd, lambda p, c: p[K.DG_L64] == 1 and p[K.DG_L32] == 1 and c[1] == 96)
    assert some(bwd, lambda p, c: p[K.DG_L64] == 1 and p[K.DG_L32] == 1 and c[1] > 128)
    assert some(bwd, lambda p, c: p[K.DG_L64] == 0 and p[K.DG_L32] == 1)
    assert some(bwd, lambda p, c: p[K.DG_SMALL] == 0 and p[K.DG_NSPLIT] == 1 and p[K.DG_L32] == 0 and c[1] % 64 not in (0, 32))
    # wgrad: both forms with S == K tiles and with several K tiles per split; both reductions; ragged o tile; item tail
    for form in (1, 2):
        assert some(bwd, lambda p, c: p[K.WG_FORM] == form and p[K.WG_S] == p[K.WG_KT])
        assert some(bwd, lambda p, c: p[K.WG_FORM] == form and p[K.WG_S] < p[K.WG_KT])
    assert some(bwd, lambda p, c: p[K.WG_FORM] == 2 and 2 * p[K.WG_S] < p[K.WG_KT])          # three tiles in a split: the buffers turn over
    assert some(bwd, lambda p, c: p[K.WG_RED] == K.RED_TALL) and some(bwd, lambda p, c: p[K.WG_RED] == K.RED_ROWS)
    assert some(bwd, lambda p, c: p[K.WG_FORM] == 1 and c[2] % 64 != 0 and c[3] >= 9 and c[4] >= 65)
    assert some(bwd, lambda p, c: p[K.WG_FORM] == 1 and p[K.WG_ITEMS] % 8 != 0)
    assert some(bwd, lambda p, c: p[K.WG_FORM] == 1 and 9 * c[1] % 128 == 14)
    # conv dbias: several chunks with a ragged last one; batch 2; the tall reduction
    assert some(bwd, lambda p, c: p[K.DB_ROWS] > 1 and c[0] == 1 and c[3] * c[4] % 2048 != 0)
    assert some(bwd, lambda p, c: c[0] == 2)
    assert some(bwd, lambda p, c: p[K.DB_RED] == K.RED_TALL)


def test_plan_declines_bad_arguments(L):
    import ctypes
    out = (ctypes.c_int32 * K.PLAN_N)()
    assert L.orn_debug_conv_f32_plan(1, 8, 16, 4, 4, None) == -1
    for bad in [(0, 8, 16, 4, 4), (1, 0, 16, 4, 4), (1, 8, 0, 4, 4), (1, 8, 16, 0, 4), (1, 8, 16, 4, 0)]:
        assert L.orn_debug_conv_f32_plan(*bad, out) == -1, bad
