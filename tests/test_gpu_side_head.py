"""The side-head kernels of the multi-resolution generator (csrc/orn_side_head.hip; the fp32 layout's and the dW / db finish:
csrc/orn_side_head_f32.hip) elementwise against fp64, through the entry points of include/orn_debug.h (csrc/orn_debug.hip): the forward on a block's stored output, and the backward that ADDS its term to a gradient buffer
another kernel has already written.

The fp64 reference starts from the SAME stored inputs (the 16-bit z and gradient buffer, the fp32 w, b, out, dout), so what is
left is the kernel's fp32 arithmetic and, for a 16-bit target, its one final rounding:

    forward      |out - r64|  <=                 C_FWD * 2^-24 * (sum_c |w_kc a_c| + |b_k| + 1)
    accumulate   |new - r64|  <= u16 * |r64| + d16 + C_BWD * 2^-24 * (|old| + sum_k |gs w_kc du_k SiLU'(z_c)|)
    dW, db       max|g - r64| <= C_DW * max(max|r32 - r64|, 2^-24 max|r64|)          (the project's form; r32: the same sums in fp32)

u16 = 2^-11 (IEEE half), 2^-8 (bf16), 0 (fp32 target, whose rounding is one of the 2^-24 terms); d16 = 2^-25, half the smallest
IEEE-half subnormal, for that type only.  The constants are the next power of two at least twice the worst ratio measured over
every shape, dtype and activation below on an MI355X with the constant at 1 (the rule of DESIGN 4.11; DESIGN 4.12 has the table by
dtype):
    forward     0.92 (fp16, sigmoid, C = 1, 10x15)                                    -> C_FWD = 2
    accumulate  3.05 (fp32 target, tanh, C = 32, 20x30: du is a product of five fp32 factors; the 16-bit targets stay below 0.35,
                their final rounding dominates)                                       -> C_BWD = 8
    dW, db      2.89 (bf16, tanh, C = 32, 6x9: SiLU through v_exp_f32 / v_rcp_f32)    -> C_DW = 8
Each test prints its worst ratios before it asserts.
"""
import numpy as np
import pytest
import torch
from ctypes import c_float, c_size_t

from head_ref import BAND, banded, bands_intact, dsilu64, interior, silu64      # shared with test_gpu_head16.py

pytestmark = pytest.mark.gpu

C_FWD, C_BWD, C_DW = 2.0, 8.0, 8.0
CHANNELS = (1, 3, 26, 32, 96, 128)
SHAPES = ((2, 2, 2), (5, 5, 5), (10, 15, 5), (6, 9, 3), (20, 30, 2))
# beyond the issue's grid: channels past one 128-channel chunk (16-byte and element-wise form), and an image of several work-groups
# in every kernel (2300 pixels: 5 x 512 in the 16-bit backward, 2 x 2048 in the fp32 one, 36 x 64 in the forward)
EXTRA = ((160, 6, 9, 3), (131, 6, 9, 3), (32, 46, 50, 2), (26, 46, 50, 2))
CASES = tuple((C, H, W, s) for C in CHANNELS for (H, W, s) in SHAPES) + EXTRA
DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
U16 = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8, 'f32': 0.0}
D16 = {'f16': 2.0 ** -25, 'bf16': 0.0, 'f32': 0.0}
GS = {'f16': 1024.0, 'bf16': 1.0, 'f32': 1.0}
LW = 0.7


@pytest.fixture(scope='module')
def L():
    from orn_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, 'orn_debug_side_head_bwd_f32'), 'liborn.so has no side-head entry points'
    return _lib


def make_inputs(C, H, W, s, kind, seed):
    """Host tensors of one case.  x: what the block stored (16 bit: z [H,W,C]; fp32: the activation [C,H,W]); old: the gradient buffer
    as the block above left it (16 bit: padded, ring included; fp32: [C,H,W])."""
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[kind]
    w = (torch.rand(3, C, generator=g) * 2 - 1) / np.sqrt(C)
    b = (torch.rand(3, generator=g) * 2 - 1) * 0.1
    dout = torch.randn(3, H, W, generator=g) * 0.02
    if kind == 'f32':
        x = torch.randn(C, H, W, generator=g) * 1.5
        old = torch.randn(C, H, W, generator=g) * 0.02
    else:
        x = (torch.randn(H, W, C, generator=g) * 1.5).to(dt)
        old = (torch.randn(H // s + 2, W // s + 2, C * s * s, generator=g) * 0.02 * GS[kind]).to(dt)
    return x, w, b, dout, old


def ref_forward(x, w, b, sigmoid, kind, dtype=torch.float64):
    """(out [3,H,W], sum of |terms| [3,H,W], a [C,H,W]) in `dtype` from the stored x."""
    xd = x.to(dtype)
    a = xd if kind == 'f32' else silu64(xd).permute(2, 0, 1)
    wd, bd = w.to(dtype), b.to(dtype)
    u = torch.einsum('kc,chw->khw', wd, a) + bd[:, None, None]
    mag = torch.einsum('kc,chw->khw', wd.abs(), a.abs()) + bd.abs()[:, None, None] + 1
    out = torch.sigmoid(u) if sigmoid else (torch.tanh(u) + 1) * 0.5
    return out, mag, a


def ref_backward(x, w, out, dout, old, sigmoid, kind, C, H, W, s, dtype=torch.float64):
    """(new gradient values [C,H,W], sum of |terms| [C,H,W], dW [3,C], db [3]) in `dtype`, from the same stored inputs."""
    od, gd, wd = out.to(dtype), dout.to(dtype), w.to(dtype)
    du = gd * LW * (od * (1 - od) if sigmoid else 2 * od * (1 - od))
    xd = x.to(dtype)
    if kind == 'f32':
        a, fac, oldv = xd, torch.ones_like(xd), old.to(dtype)
    else:
        z = xd.permute(2, 0, 1)
        a, fac, oldv = silu64(z), dsilu64(z) * GS[kind], interior(old, C, H, W, s).to(dtype)
    term = torch.einsum('kc,khw->chw', wd, du) * fac
    mag = oldv.abs() + torch.einsum('kc,khw->chw', wd.abs(), du.abs()) * fac.abs()
    dw = torch.einsum('khw,chw->kc', du, a)
    db = du.sum(dim=(1, 2))
    return oldv + term, mag, dw, db


def run_case(L, C, H, W, s, kind, sigmoid, seed, misalign=False):
    """One case on the device, twice.  Returns the three ratios to the bounds at constant 1."""
    lib = L.lib()
    x, w, b, dout, old = make_inputs(C, H, W, s, kind, seed)
    dt = DTYPES[kind]
    st = L.stream()
    if misalign:                                    # z two bytes past a 16-byte boundary: the element-wise form at C % 8 == 0
        xbuf = torch.zeros(x.numel() + 9, dtype=dt, device='cuda')
        xg = xbuf[9:].view(x.shape)
        xg.copy_(x)
        assert xg.data_ptr() % 16 == 2
    else:
        xg = x.cuda()
    wg, bg, dg = w.cuda(), b.cuda(), dout.cuda()

    # ---- forward
    r_out, r_mag, _ = ref_forward(x, w, b, sigmoid, kind)
    outs = []
    for _ in range(2):
        obuf, og = banded((3, H, W), torch.float32)
        L.check(getattr(lib, f'orn_debug_side_head_fwd_{kind}')(L.ptr(xg), L.ptr(wg), L.ptr(bg), C, H, W, int(sigmoid), L.ptr(og), st),
                'side_head_fwd')
        torch.cuda.synchronize()
        assert bands_intact(obuf), 'forward wrote outside out'
        outs.append(og.cpu())
    assert torch.equal(outs[0], outs[1]), 'forward differs between two runs'
    assert torch.isfinite(outs[0]).all()
    rf = float(((outs[0].double() - r_out).abs() / (2.0 ** -24 * r_mag)).max())

    # ---- accumulating backward, on the fp32 image the forward produced
    out = outs[0]
    r_new, r_mag, r_dw, r_db = ref_backward(x, w, out, dout, old, sigmoid, kind, C, H, W, s)
    _, _, r32_dw, r32_db = ref_backward(x, w, out, dout, old, sigmoid, kind, C, H, W, s, torch.float32)
    og = out.cuda()
    nbytes = lib.orn_debug_side_head_bwd_ws_bytes(C, H, W)
    assert nbytes > 0
    res = []
    for _ in range(2):
        gbuf, gg = banded(tuple(old.shape), dt, old)
        wbuf, dwg = banded((3, C), torch.float32)
        bbuf, dbg = banded((3,), torch.float32)
        ws = torch.full((nbytes // 4,), float('nan'), device='cuda')
        if kind == 'f32':
            L.check(lib.orn_debug_side_head_bwd_f32(L.ptr(xg), L.ptr(wg), L.ptr(og), L.ptr(dg), C, H, W, int(sigmoid), c_float(LW),
                                                    L.ptr(gg), L.ptr(dwg), L.ptr(dbg), L.ptr(ws), c_size_t(nbytes), st), 'side_head_bwd_f32')
        else:
            L.check(getattr(lib, f'orn_debug_side_head_bwd_{kind}')(L.ptr(xg), L.ptr(wg), L.ptr(og), L.ptr(dg), C, H, W, int(sigmoid), s,
                                                                   c_float(LW), c_float(GS[kind]), L.ptr(gg), L.ptr(dwg), L.ptr(dbg),
                                                                   L.ptr(ws), c_size_t(nbytes), st), 'side_head_bwd')
        torch.cuda.synchronize()
        assert bands_intact(gbuf) and bands_intact(wbuf) and bands_intact(bbuf), 'backward wrote outside an output'
        res.append((gg.cpu(), dwg.cpu(), dbg.cpu()))
    for t0, t1 in zip(res[0], res[1]):
        assert torch.equal(t0.view(torch.int16 if t0.element_size() == 2 else torch.int32),
                           t1.view(torch.int16 if t1.element_size() == 2 else torch.int32)), 'backward differs between two runs'
    new, dw, db = res[0]
    assert torch.isfinite(new.float()).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
    if kind == 'f32':
        newv = new.double()
    else:
        # the one-pixel ring exactly as found
        ring = torch.ones(old.shape[:2], dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        assert torch.equal(new[ring].view(torch.int16), old[ring].view(torch.int16)), 'the ring of the padded buffer changed'
        newv = interior(new, C, H, W, s).double()
    err = (newv - r_new).abs() - U16[kind] * r_new.abs() - D16[kind]
    rb = float((err / (2.0 ** -24 * r_mag)).max())
    rw = 0.0
    for got, r64, r32 in ((dw, r_dw, r32_dw), (db, r_db, r32_db)):
        yard = max(float((r32.double() - r64).abs().max()), 2.0 ** -24 * float(r64.abs().max()))
        rw = max(rw, float((got.double() - r64).abs().max()) / yard)
    return rf, rb, rw, res[0], outs[0]


@pytest.mark.parametrize('sigmoid', [False, True], ids=['tanh', 'sigmoid'])
@pytest.mark.parametrize('kind', ['f16', 'bf16', 'f32'])
def test_side_head_against_fp64(L, kind, sigmoid):
    worst = [0.0, 0.0, 0.0]
    where = [None, None, None]
    for n, (C, H, W, s) in enumerate(CASES):
        r = run_case(L, C, H, W, s, kind, sigmoid, seed=1000 + n)[:3]
        for k in range(3):
            if r[k] > worst[k]:
                worst[k], where[k] = r[k], (C, H, W, s)
    print(f'\nside head {kind} {"sigmoid" if sigmoid else "tanh"}: worst ratio to the bound at constant 1: '
          f'forward {worst[0]:.3f} at {where[0]}, accumulate {worst[1]:.3f} at {where[1]}, dW/db {worst[2]:.3f} at {where[2]}')
    assert worst[0] <= C_FWD, (worst[0], where[0])
    assert worst[1] <= C_BWD, (worst[1], where[1])
    assert worst[2] <= C_DW, (worst[2], where[2])


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_both_access_forms_give_the_same_bits(L, kind):
    """C % 8 == 0 with z off a 16-byte boundary takes the element-wise form: same sums in the same order as the 16-byte form."""
    for (C, H, W, s) in ((32, 6, 9, 3), (96, 20, 30, 2), (160, 6, 9, 3)):
        a = run_case(L, C, H, W, s, kind, False, seed=7)
        b = run_case(L, C, H, W, s, kind, False, seed=7, misalign=True)
        assert torch.equal(a[4], b[4])
        for t0, t1 in zip(a[3], b[3]):
            assert torch.equal(t0.float(), t1.float())


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_ops_wrapper_forward(L, kind):
    """ops.side_head_fwd (what a caller outside the tests uses) reaches the same kernel: same bound."""
    from orn_amd import ops
    for C in (32, 96, 128):
        x, w, b, _, _ = make_inputs(C, 20, 30, 2, kind, seed=3)
        out = ops.side_head_fwd(x.cuda(), w.cuda(), b.cuda(), False)
        r, mag, _ = ref_forward(x, w, b, False, kind)
        assert float(((out.cpu().double() - r).abs() / (2.0 ** -24 * mag)).max()) <= C_FWD


def test_zero_weight_adds_an_exact_zero(L):
    """lw = 0: the gradient buffer keeps its bits (x + 0 rounds to x), dW and db are exactly 0."""
    from orn_amd import ops
    for kind in ('f16', 'bf16', 'f32'):
        C, H, W, s = 26, 10, 15, 5
        x, w, b, dout, old = make_inputs(C, H, W, s, kind, seed=11)
        xg = x.cuda()
        out = ops.side_head_fwd(xg, w.cuda(), b.cuda(), False)
        g = old.cuda().clone()
        dw, db = ops.side_head_bwd_(xg, w.cuda(), out, dout.cuda(), g, False, lw=0.0, sp=s, gs=GS[kind])
        assert torch.equal(g.cpu().float(), old.float())
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


def test_bad_arguments_are_refused(L):
    lib = L.lib()
    z = torch.zeros(4, 4, 8, dtype=torch.bfloat16, device='cuda')
    f = torch.zeros(3 * 16 + 3 * 8 + 64, device='cuda')
    assert lib.orn_debug_side_head_bwd_ws_bytes(0, 4, 4) == 0 and lib.orn_debug_side_head_bwd_ws_bytes(513, 4, 4) == 0
    rc = lib.orn_debug_side_head_bwd_bf16(L.ptr(z), L.ptr(f), L.ptr(f), L.ptr(f), 8, 4, 4, 0, 3, c_float(1), c_float(1), L.ptr(z), L.ptr(f),
                                          L.ptr(f), L.ptr(f), c_size_t(f.numel() * 4), L.stream())
    assert rc == -1 and 'stride' in L.last_error()
    rc = lib.orn_debug_side_head_bwd_bf16(L.ptr(z), L.ptr(f), L.ptr(f), L.ptr(f), 8, 4, 4, 0, 2, c_float(1), c_float(1), L.ptr(z), L.ptr(f),
                                          L.ptr(f), L.ptr(f), c_size_t(16), L.stream())
    assert rc == -2 and 'workspace' in L.last_error()
