"""The case table of the fp32 conv kernel forms, shared by test_conv32_plan_host.py (which proves without a GPU that every case
reaches the form it names) and test_gpu_conv32_forms.py (which runs the cases).  A case is (B, C, O, H, W, s) and the values that
orn_debug_conv_f32_plan (include/orn_debug.h) must report for it: the launchers call the same selection functions, so a retuned
threshold fails here instead of silently moving a case to another kernel form."""
import ctypes

# indices of orn_debug_conv_f32_plan's out[18]
(FWD_SMALL, FWD_WGS, DG_SMALL, DG_NSPLIT, DG_CPS, DG_L64, DG_L32, DG_RED, DG_WGS, WG_FORM, WG_S, WG_KT, WG_ITEMS, WG_RED,
 DB_ROWS, DB_RED, HDB_ROWS, HDB_RED) = range(18)
PLAN_N = 18
RED_NONE, RED_ROWS, RED_TALL = 0, 1, 2


def plan(L, B, C, O, H, W):
    out = (ctypes.c_int32 * PLAN_N)()
    assert L.orn_debug_conv_f32_plan(B, C, O, H, W, out) == 0
    return list(out)


# ---- forward: k_conv3x3_f32<EPI_PS_SILU, SMALL>; SMALL = 1 below 256 work-groups of 64 channels x 8 x 32 pixels ---------------
FWD_CASES = [
    # (B, C, O, H, W, s), {plan index: value}, what it reaches
    ((1, 5, 8, 3, 5, 2), {FWD_SMALL: 1, FWD_WGS: 2}, 'small, s = 2: one tile, C < 8'),
    ((1, 9, 16, 9, 33, 2), {FWD_SMALL: 1, FWD_WGS: 10}, 'small, s = 2: one channel in the second chunk, W % 32 = 1, odd H'),
    ((1, 7, 36, 1, 1, 3), {FWD_SMALL: 1, FWD_WGS: 1}, 'small, general epilogue: 1 x 1 image'),
    ((2, 17, 25, 10, 35, 5), {FWD_SMALL: 1, FWD_WGS: 20}, 'small, general epilogue: batch 2, s = 5'),
    ((1, 8, 12, 7, 31, 1), {FWD_SMALL: 1, FWD_WGS: 4}, 'small, general epilogue: s = 1'),
    ((1, 8, 256, 256, 64, 2), {FWD_SMALL: 0, FWD_WGS: 256}, '8-row tiles, s = 2: exactly 256 work-groups'),
    ((1, 8, 256, 248, 64, 2), {FWD_SMALL: 1, FWD_WGS: 992}, '248 work-groups of 8 rows: small, the other side of the threshold'),
    ((1, 3, 36, 256, 256, 3), {FWD_SMALL: 0, FWD_WGS: 256}, '8-row tiles, general epilogue: O < 64'),
    ((2, 4, 288, 104, 64, 3), {FWD_SMALL: 0, FWD_WGS: 260}, '8-row tiles, general epilogue: O % 64 = 32 (masks, no tail form), batch 2'),
]
# the z-only and the a-only form through orn_debug_conv_fwd_f32 (indices into FWD_CASES)
FWD_ONE_OUTPUT = [5, 1]

# ---- backward through orn_conv3x3_ps_silu_bwd: dgrad = conv(dy, Wd) with C_in = O, O_out = C; wgrad; dbias -------------------
BWD_CASES = [
    ((1, 9, 16, 9, 33, 2), {DG_SMALL: 1, DG_NSPLIT: 1, DG_CPS: 16, DG_L64: 1, DG_L32: 0, DG_RED: RED_NONE,
                            WG_FORM: 1, WG_S: 6, WG_KT: 6},
     'dgrad small unsplit (O <= 16)'),
    ((1, 26, 104, 45, 80, 2), {DG_SMALL: 1, DG_NSPLIT: 7, DG_CPS: 16, DG_RED: RED_ROWS,
                               WG_FORM: 1, WG_S: 36, WG_KT: 36, WG_ITEMS: 144, WG_RED: RED_TALL, DB_ROWS: 2},
     'dgrad small, 7 splits of 16, the last 8 channels; wgrad form 1, ragged o tile beside interior tiles, tall reduction; '
     'dbias: two chunks, the second ragged'),
    ((1, 12, 36, 8, 64, 3), {DG_SMALL: 1, DG_NSPLIT: 3, DG_CPS: 16, DG_RED: RED_ROWS, WG_FORM: 1, WG_S: 4, WG_KT: 4},
     'dgrad small, last split 4 channels (chunk tail, cleft = 4); wgrad form 1, no interior tile'),
    ((1, 70, 130, 9, 65, 1), {DG_SMALL: 1, DG_NSPLIT: 9, DG_CPS: 16, DG_RED: RED_ROWS,
                              WG_FORM: 1, WG_S: 9, WG_KT: 9, WG_ITEMS: 135, WG_RED: RED_ROWS},
     'dgrad small, 9 splits, the last 2 channels; wgrad form 1, 135 items (not a multiple of 8)'),
    ((1, 64, 32, 256, 256, 2), {DG_SMALL: 0, DG_NSPLIT: 2, DG_CPS: 16, DG_L64: 1, DG_L32: 0, DG_RED: RED_ROWS, DG_WGS: 512,
                                WG_FORM: 1, DB_ROWS: 32, DB_RED: RED_TALL},
     'dgrad 8-row tiles split in 2; dbias: 32 chunks, tall reduction'),
    ((1, 96, 32, 256, 128, 2), {DG_SMALL: 0, DG_NSPLIT: 2, DG_CPS: 16, DG_L64: 1, DG_L32: 0, DG_RED: RED_ROWS, DG_WGS: 512},
     'dgrad 8-row tiles, exactly 256 work-groups with O_out % 64 = 32: the split wins over the tail'),
    ((1, 96, 16, 264, 128, 2), {DG_SMALL: 0, DG_NSPLIT: 1, DG_L64: 1, DG_L32: 1, DG_RED: RED_NONE, DG_WGS: 264},
     'dgrad 8-row tiles, 64 + 32 tail'),
    ((1, 160, 8, 176, 128, 2), {DG_SMALL: 0, DG_NSPLIT: 1, DG_L64: 1, DG_L32: 1, DG_RED: RED_NONE, DG_WGS: 264},
     'dgrad 8-row tiles, two 64-channel tiles + tail'),
    ((1, 32, 16, 264, 256, 2), {DG_SMALL: 0, DG_NSPLIT: 1, DG_L64: 0, DG_L32: 1, DG_RED: RED_NONE, DG_WGS: 264},
     'dgrad 8-row tiles, the tail alone'),
    ((1, 26, 16, 264, 256, 2), {DG_SMALL: 0, DG_NSPLIT: 1, DG_L64: 1, DG_L32: 0, DG_RED: RED_NONE, DG_WGS: 264},
     'dgrad 8-row tiles, plain with a ragged O_out'),
    ((1, 13, 40, 9, 65, 2), {WG_FORM: 1, WG_S: 9, WG_KT: 9},
     'wgrad form 1, exactly one interior K tile, its patch ends on the last row and column'),
    ((1, 48, 864, 45, 80, 3), {WG_FORM: 1, WG_S: 19, WG_KT: 36, WG_RED: RED_ROWS},
     'wgrad form 1, two K tiles per split in 17 of 19 splits'),
    ((1, 30, 64, 4, 32, 2), {WG_FORM: 1, WG_S: 1, WG_KT: 1, WG_ITEMS: 3}, 'wgrad form 1, n-tile clamp: 9 C % 128 = 14'),
    ((1, 32, 128, 3, 65, 2), {WG_FORM: 2, WG_S: 9, WG_KT: 9}, 'wgrad form 2, exactly one interior tile'),
    ((1, 32, 128, 2, 64, 2), {WG_FORM: 2, WG_S: 4, WG_KT: 4}, 'wgrad form 2, no interior tile'),
    ((1, 32, 128, 3, 64, 2), {WG_FORM: 2, WG_S: 6, WG_KT: 6},
     'wgrad form 2, W % 32 = 0: the middle row\'s tile at the right edge ends one column short of interior'),
    ((1, 64, 256, 5, 130, 2), {WG_FORM: 2, WG_S: 25, WG_KT: 25, WG_ITEMS: 100}, 'wgrad form 2, interior tiles in three rows'),
    ((2, 96, 384, 20, 97, 2), {WG_FORM: 2, WG_S: 56, WG_KT: 160, WG_ITEMS: 504, DB_ROWS: 2},
     'wgrad form 2, batch 2: splits of 2 and 3 K tiles, the double buffer turns over; dbias with B = 2'),
]

# ---- fused head backward through orn_debug_conv_bwd_f32_head: (C, Cn, H, W) low-res, O = 4 Cn; HDB_ROWS = work-groups ----------
HEAD_HW = [
    ((9, 25), 1, 'H W = 225 < 256: the second pixel of every thread is absent'),
    ((16, 32), 1, 'H W = 512: one full work-group'),
    ((19, 27), 2, 'H W = 513: one pixel in the second work-group'),
    ((130, 128), 33, '33 work-groups: k_head_partials_finish strides over rows, 3 Cn + 3 not a multiple of 32'),
]
HEAD_CN = [1, 3, 24]
HEAD_C = 6                     # input channels of the block below the head

# ---- z-input head forward: (B, C, Cn, H, W, s) of the conv forward (O = Cn s^2) that makes z and a = SiLU(z); the head sees Cn
# planes of H s x W s pixels
HEADZ_CASES = [
    ((2, 3, 1, 5, 6, 2), 'V = 4 (120 pixels), one head channel, batch 2'),
    ((2, 4, 24, 17, 17, 2), 'V = 4 (1156 pixels: two work-groups, the second ragged), 24 channels, batch 2'),
    ((2, 3, 1, 3, 5, 3), 'V = 1 (135 pixels), one head channel, batch 2'),
    ((2, 4, 24, 7, 5, 3), 'V = 1 (315 pixels: two work-groups), 24 channels, batch 2'),
]
