"""The last stage's 16-bit head (k_head_fwd_nhwc_bf16, k_head_bwd_nhwc_bf16<C / 32>, csrc/orn_ops_bf16.hip) and the reduction of its
dW / db partials (head_finish_body, csrc/orn_wgrad_bf16.hip) elementwise against fp64, through the entry points of include/orn_debug.h,
which call the launchers the engine calls.  These are the head kernels of the step bench.py times.

The fp64 reference starts from the SAME stored inputs (the 16-bit z, the fp32 w, b, out, dout), so what is left is the kernel's fp32
arithmetic and the one rounding of dy to 16 bits:

    forward   |out - r64| <=                  C_FWD * 2^-24 * (sum_c |w_kc a_c| + |b_k| + 1)
    dy        |dy - r64|  <= u16 |r64| + d16 + C_DY * 2^-24 * sum_k |gs w_kc du_k SiLU'(z_c)|          du = dout * act'(out)
    dW, db    max|g - r64| <= C_DW * max(max|r32 - r64|, 2^-24 max|r64|)                  (r32: the same sums in fp32)

u16 = 2^-11 (IEEE half), 2^-8 (bf16); d16 = 2^-25 (IEEE half), 2^-134 (bf16): half the smallest subnormal.  The constants are the next
power of two at least twice the worst ratio measured over every case below on an MI355X with the constant at 1 (the rule of DESIGN
4.11; DESIGN 4.14 has the table by type):
    forward   0.85 (fp16, tanh, C = 32, 516x1024; bf16 0.82 there; the small images stay below 0.64)          -> C_FWD = 2
    dy        1.19 (fp16, tanh, C = 32, 258x256, sp 2; bf16 1.16 at C = 128, sigmoid; the small images stay below 0.84:
              the 16-bit rounding dominates, and millions of elements find a deeper tail of it than 40 thousand)     -> C_DY = 4
    dW, db    4.02 (fp16, sigmoid, C = 64, 20x30; bf16 3.03 there, tanh: SiLU through v_exp_f32 / v_rcp_f32)       -> C_DW = 16
gs = 1024 and gs = 2^20 give the same ratios (powers of two).  Each test prints its worst ratios before it asserts.

Mutations of the kernels, each built once on a scratch copy and run against this file (DESIGN 4.14 has the table): a prefetch
that reloads the current pixel fails the grid-stride tests alone (backward: dy 2.2e13, forward: 5.9e6 times the bound), a swapped
sub-pixel index every backward test (dy 5e11), a finish that drops its last row every dW / db (1.7e7), a rider test that misses its
work-group test_loss_rider (stats stay NaN); db taken from another `sub` lane passes, as it must: the four lanes of a pixel hold
the same du.

Shapes (H, W, sp): fewer pixels than one work-group (2,2,2); odd W (7,13,1); sp = 3 and 5 with H != W, where a swapped sub-pixel
index lands elsewhere; a ragged last work-group (20,30,2).  The backward walks a grid stride above 512 x 64 pixels: (128,256,2) is
exactly one pass, (130,256,2) gives some lanes a second pixel, (258,256,2) a third; the forward above 8192 x 64: 512x1024 is exactly
one pass, 516x1024 has a ragged second one.
"""
import numpy as np
import pytest
import torch
from ctypes import byref, c_float, c_int, c_size_t

from head_ref import banded, bands_intact, bits, dsilu64, interior_pc, silu64

pytestmark = pytest.mark.gpu

C_FWD, C_DY, C_DW = 2.0, 4.0, 16.0
DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16}
U16 = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
D16 = {'f16': 2.0 ** -25, 'bf16': 2.0 ** -134}
SUBNORMAL = {'f16': 2.0 ** -24, 'bf16': 2.0 ** -133}
# the gradient scales dypad travels with: bf16 1; IEEE half 1024 (the side-head test's) and 2^20 (the engine's default)
GSCALES = {'bf16': (1.0,), 'f16': (1024.0, 2.0 ** 20)}
BWD_CHANNELS = (32, 64, 96, 128)                    # the four instantiations of the backward
FWD_CHANNELS = BWD_CHANNELS + (160, 256)            # + the un-pipelined loop of the forward (C / 32 > 4)
SMALL = ((2, 2, 2), (5, 5, 5), (7, 13, 1), (6, 9, 3), (10, 15, 5), (20, 30, 2))
SPECIAL_AT = (20, 30, 2)                            # the small case that also carries the special values of z
BWD_STRIDE = ((128, 256, 2), (130, 256, 2), (258, 256, 2))
FWD_STRIDE = ((512, 1024), (516, 1024))
L2, FUSION6 = 0, 2                                  # loss ids of include/orn.h


@pytest.fixture(scope='module')
def L():
    from orn_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, 'orn_debug_head_bwd_f16'), 'liborn.so has no head16 entry points'
    return _lib


def make_inputs(kind, C, H, W, seed, special=False):
    """z [H W, C] (16 bit), w [3, C], b [3], dout [3, H W] at unit gradient scale"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(H * W, C, generator=g) * 1.5
    if special:                                     # 0, -0, the smallest subnormals, +-20: at the first, a middle and the last pixel
        sub = SUBNORMAL[kind]
        vals = torch.tensor([0.0, -0.0, sub, -sub, 20.0, -20.0, 0.0, -sub])
        for p, c0 in ((0, 0), (H * W // 2, 8), (H * W - 1, C - 8)):
            z[p, c0:c0 + 8] = vals
    z = z.to(DTYPES[kind])
    if special:
        assert float(z[0, 2]) == SUBNORMAL[kind] and bits(z[0:1, 1:2]).item() != 0 and float(z[0, 1]) == 0.0
    w = (torch.rand(3, C, generator=g) * 2 - 1) / np.sqrt(C)
    b = (torch.rand(3, generator=g) * 2 - 1) * 0.1
    dout = torch.randn(3, H * W, generator=g) * 0.02
    return z, w, b, dout


def act64(u, sigmoid):
    return torch.sigmoid(u) if sigmoid else (torch.tanh(u) + 1) * 0.5


def fwd_ref(z, w, b, chunk=1 << 16):
    """(u [P, 3], sum of |terms| + |b| + 1 [P, 3]) in fp64 from the stored z, in chunks of rows"""
    w64, b64 = w.double(), b.double()
    us, mags = [], []
    for p0 in range(0, z.shape[0], chunk):
        a = silu64(z[p0:p0 + chunk].double())
        us.append(a @ w64.t() + b64)
        mags.append(a.abs() @ w64.abs().t() + b64.abs() + 1)
    return torch.cat(us), torch.cat(mags)


def run_fwd(L, kind, zg, wg, bg, C, H, W, sigmoid):
    """The forward on the device, twice: out [3, H W] on the host."""
    lib, st = L.lib(), L.stream()
    outs = []
    for _ in range(2):
        obuf, og = banded((3, H * W), torch.float32)
        L.check(getattr(lib, f'orn_debug_head_fwd_{kind}')(L.ptr(zg), L.ptr(wg), L.ptr(bg), C, H, W, int(sigmoid), L.ptr(og), st), 'head_fwd')
        torch.cuda.synchronize()
        assert bands_intact(obuf), 'forward wrote outside out'
        outs.append(og.cpu())
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'forward differs between two runs'
    assert torch.isfinite(outs[0]).all()            # (every element written: the buffer started as NaN)
    return outs[0]


def fwd_ratio(out, u, mag, sigmoid):
    return float(((out.double().t() - act64(u, sigmoid)).abs() / (2.0 ** -24 * mag)).max())


def z_terms(z, dtype):
    """(SiLU(z), SiLU'(z)) [P, C] in `dtype`"""
    zd = z.to(dtype)
    return silu64(zd), dsilu64(zd)


def bwd_ref(terms, w, out, dout, gs, sigmoid, dtype=torch.float64):
    """(dy [P, C], sum of |terms| [P, C], dW [3, C], db [3]) in `dtype` from the stored inputs; dW, db un-scaled"""
    a, ds = terms
    o, g, wd = out.to(dtype).t(), dout.to(dtype).t(), w.to(dtype)
    du = g * gs * (o * (1 - o) if sigmoid else 2 * o * (1 - o))          # [P, 3]
    dy = (du @ wd) * ds
    mag = (du.abs() @ wd.abs()) * ds.abs()
    return dy, mag, (du.t() @ a) / gs, du.sum(dim=0) / gs


def run_bwd(L, kind, zg, wg, og, dg, C, H, W, s, sigmoid, gs, engine=False, target=None, loss_type=L2):
    """One backward call on NaN-seeded outputs and an exact-size NaN workspace.  dg: dout (written by the call when there is a target).
    Returns dict(dy [P, C] 16 bit, dw, db, flag, stats) on the host."""
    lib, st = L.lib(), L.stream()
    dt = DTYPES[kind]
    g = torch.Generator().manual_seed(99)
    old = (torch.randn(H // s + 2, W // s + 2, C * s * s, generator=g) * 0.5).to(dt)
    old[1:-1, 1:-1] = float('nan')                  # every interior element must be overwritten
    ybuf, yg = banded(tuple(old.shape), dt, old)
    wbuf, dwg = banded((3, C), torch.float32)
    bbuf, dbg = banded((3,), torch.float32)
    sbuf, sg = banded((8,), torch.float32)
    nbytes = lib.orn_debug_head16_bwd_ws_bytes(C) if target is None else lib.orn_debug_head16_bwd_rider_ws_bytes(C, H, W, loss_type)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), float('nan'), device='cuda')
    flag = c_int(-7)
    rc = getattr(lib, f'orn_debug_head_bwd_{kind}')(L.ptr(zg), L.ptr(wg), L.ptr(og), L.ptr(dg), C, H, W, int(sigmoid), s, c_float(gs), L.ptr(yg),
                                                    L.ptr(dwg), L.ptr(dbg), L.ptr(ws), c_size_t(nbytes), byref(flag) if engine else None,
                                                    L.ptr(target), loss_type, L.ptr(sg) if target is not None else None, st)
    L.check(rc, 'head_bwd')
    torch.cuda.synchronize()
    assert bands_intact(ybuf) and bands_intact(wbuf) and bands_intact(bbuf) and bands_intact(sbuf), 'backward wrote outside an output'
    new = yg.cpu()
    ring = torch.ones(old.shape[:2], dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert torch.equal(bits(new[ring]), bits(old[ring])), 'the ring of the padded buffer changed'
    return dict(dy=interior_pc(new, C, H, W, s), dw=dwg.cpu(), db=dbg.cpu(), flag=flag.value if engine else None, stats=sg.cpu())


def same_bits(a, b, what):
    for k in ('dy', 'dw', 'db'):
        assert torch.equal(bits(a[k]), bits(b[k])), f'{what}: {k} differs'


def bwd_case(L, kind, C, H, W, s, sigmoid, gs, zg, w, wg, out, og, dout_unit, t64, t32, saturated=None):
    """One backward case: the per-op form twice and the engine's form once (same bits, flag clear), then the ratios (dy, dW/db) to the
    bounds at constant 1.  dout_unit is scaled so that the scaled gradient has the same size under every gs."""
    dout = dout_unit * (min(gs, 1024.0) / gs)       # (a power of two: the engine's 2^20 meets gradients 2^-10 times as large)
    dg = dout.cuda()
    r_dy, r_mag, r_dw, r_db = bwd_ref(t64, w, out, dout, gs, sigmoid)
    assert float(r_dy.abs().max()) <= 2.0 ** 15, 'the case itself leaves the 16-bit range'
    _, _, r32_dw, r32_db = bwd_ref(t32, w, out, dout, gs, sigmoid, torch.float32)
    a = run_bwd(L, kind, zg, wg, og, dg, C, H, W, s, sigmoid, gs)
    b = run_bwd(L, kind, zg, wg, og, dg, C, H, W, s, sigmoid, gs)
    e = run_bwd(L, kind, zg, wg, og, dg, C, H, W, s, sigmoid, gs, engine=True)
    same_bits(a, b, 'two runs')
    same_bits(a, e, 'per-op form against the engine form')
    assert e['flag'] == 0
    dy = a['dy'].double()
    assert torch.isfinite(dy).all() and torch.isfinite(a['dw']).all() and torch.isfinite(a['db']).all()
    err = (dy - r_dy).abs() - U16[kind] * r_dy.abs() - D16[kind]
    rel = err / (2.0 ** -24 * r_mag)
    if saturated is not None:
        rel = rel[~saturated]
    ry = float(rel.max())
    rw = 0.0
    for got, r64, r32 in ((a['dw'], r_dw, r32_dw), (a['db'], r_db, r32_db)):
        yard = max(float((r32.double() - r64).abs().max()), 2.0 ** -24 * float(r64.abs().max()))
        rw = max(rw, float((got.double() - r64).abs().max()) / yard)
    return ry, rw, a, (r_dy, r_mag)


class Worst:
    def __init__(self, names):
        self.names, self.v, self.at = names, [float('-inf')] * len(names), [None] * len(names)

    def add(self, ratios, where):
        for k, r in enumerate(ratios):
            if not r <= self.v[k]:                  # (a NaN ratio is kept, and fails)
                self.v[k], self.at[k] = r, where

    def __str__(self):
        return ', '.join(f'{n} {v:.3f} at {a}' for n, v, a in zip(self.names, self.v, self.at))


def backward_cases(L, kind, C, shapes, seed0):
    worst = Worst(('dy', 'dW/db'))
    for n, (H, W, s) in enumerate(shapes):
        z, w, b, dout = make_inputs(kind, C, H, W, seed0 + 16 * n + C // 32, special=(H, W, s) == SPECIAL_AT)
        zg, wg, bg = z.cuda(), w.cuda(), b.cuda()
        t64, t32 = z_terms(z, torch.float64), z_terms(z, torch.float32)
        for sigmoid in (False, True):
            out = run_fwd(L, kind, zg, wg, bg, C, H, W, sigmoid)         # the backward runs on the fp32 image the forward produced
            og = out.cuda()
            for gs in GSCALES[kind]:
                ry, rw = bwd_case(L, kind, C, H, W, s, sigmoid, gs, zg, w, wg, out, og, dout, t64, t32)[:2]
                worst.add((ry, rw), (C, H, W, s, 'sigmoid' if sigmoid else 'tanh', gs))
    return worst


@pytest.mark.parametrize('C', BWD_CHANNELS)
@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_backward_against_fp64(L, kind, C):
    worst = backward_cases(L, kind, C, SMALL, 2000)
    print(f'\nhead16 backward {kind} C={C}: worst ratio to the bound at constant 1: {worst}')
    assert worst.v[0] <= C_DY, (worst.v[0], worst.at[0])
    assert worst.v[1] <= C_DW, (worst.v[1], worst.at[1])


@pytest.mark.parametrize('C', (32, 128))
@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_backward_grid_stride_against_fp64(L, kind, C):
    lib = L.lib()
    assert [lib.orn_debug_head16_bwd_blocks(H, W) for (H, W, _) in BWD_STRIDE] == [512, 512, 512]
    assert lib.orn_debug_head16_bwd_blocks(127, 256) == 508 and lib.orn_debug_head16_bwd_blocks(20, 30) == 10
    worst = backward_cases(L, kind, C, BWD_STRIDE, 3000)
    print(f'\nhead16 backward, grid stride, {kind} C={C}: worst ratio to the bound at constant 1: {worst}')
    assert worst.v[0] <= C_DY, (worst.v[0], worst.at[0])
    assert worst.v[1] <= C_DW, (worst.v[1], worst.at[1])


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_forward_against_fp64(L, kind):
    worst = Worst(('forward',))
    for C in FWD_CHANNELS:
        for n, (H, W, s) in enumerate(SMALL):
            z, w, b, _ = make_inputs(kind, C, H, W, 4000 + 16 * n + C // 32, special=(H, W, s) == SPECIAL_AT)
            zg, wg, bg = z.cuda(), w.cuda(), b.cuda()
            u, mag = fwd_ref(z, w, b)
            for sigmoid in (False, True):
                out = run_fwd(L, kind, zg, wg, bg, C, H, W, sigmoid)
                worst.add((fwd_ratio(out, u, mag, sigmoid),), (C, H, W, 'sigmoid' if sigmoid else 'tanh'))
    print(f'\nhead16 forward {kind}: worst ratio to the bound at constant 1: {worst}')
    assert worst.v[0] <= C_FWD, (worst.v[0], worst.at[0])


@pytest.mark.parametrize('C', (32, 96))
@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_forward_grid_stride_against_fp64(L, kind, C):
    worst = Worst(('forward',))
    for n, (H, W) in enumerate(FWD_STRIDE):
        z, w, b, _ = make_inputs(kind, C, H, W, 5000 + 16 * n + C // 32)
        zg, wg, bg = z.cuda(), w.cuda(), b.cuda()
        u, mag = fwd_ref(z, w, b)
        for sigmoid in (False, True):
            out = run_fwd(L, kind, zg, wg, bg, C, H, W, sigmoid)
            worst.add((fwd_ratio(out, u, mag, sigmoid),), (C, H, W, 'sigmoid' if sigmoid else 'tanh'))
    print(f'\nhead16 forward, grid stride, {kind} C={C}: worst ratio to the bound at constant 1: {worst}')
    assert worst.v[0] <= C_FWD, (worst.v[0], worst.at[0])


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_backward_saturated_z(L, kind):
    """|z| in {88, 100, the type's largest finite value}: outputs stay finite; z > 0 gives SiLU' = 1 within the dy bound; z < 0 gives
    |dy| <= 2^-100 sum_k |gs w du| -- fp32 may flush the tail of SiLU' to zero, it may not produce garbage."""
    C, H, W, s = 32, 6, 9, 3
    big = float(torch.finfo(DTYPES[kind]).max)
    vals = torch.tensor([88.0, -88.0, 100.0, -100.0, big, -big])
    z, w, b, dout = make_inputs(kind, C, H, W, 6000)
    z = z.float()
    for p, c0 in ((0, 0), (H * W // 2 + 1, 13), (H * W - 1, C - 6)):
        z[p, c0:c0 + 6] = vals
    z = z.to(DTYPES[kind])
    zf = z.double()
    assert float(zf.max()) == big and float(zf.min()) == -big
    sat = zf.abs() >= 88
    assert int(sat.sum()) == 18
    out = (torch.rand(3, H * W, generator=torch.Generator().manual_seed(6001)) * 0.8 + 0.1)      # (a head that has not saturated itself)
    zg, wg, og = z.cuda(), w.cuda(), out.cuda()
    t64, t32 = z_terms(z, torch.float64), z_terms(z, torch.float32)
    assert torch.isfinite(t64[0]).all() and torch.isfinite(t64[1]).all()
    for sigmoid in (False, True):
        for gs in GSCALES[kind]:
            ry, rw, got, (r_dy, r_mag) = bwd_case(L, kind, C, H, W, s, sigmoid, gs, zg, w, wg, out, og, dout, t64, t32, saturated=sat)
            dy = got['dy'].double()
            o, g = out.double().t(), (dout * (min(gs, 1024.0) / gs)).double().t()
            du = g * gs * (o * (1 - o) if sigmoid else 2 * o * (1 - o))
            lin, lin_abs = du @ w.double(), du.abs() @ w.double().abs()          # SiLU' = 1
            pos, neg = sat & (zf > 0), sat & (zf < 0)
            e_pos = ((dy - lin).abs() - U16[kind] * lin.abs() - D16[kind])[pos] / (2.0 ** -24 * lin_abs[pos])
            r_neg = dy.abs()[neg] / (2.0 ** -100 * lin_abs[neg])
            print(f'\nhead16 backward, saturated z, {kind} {"sigmoid" if sigmoid else "tanh"} gs={gs:g}: z > 0 ratio {float(e_pos.max()):.3f}, '
                  f'z < 0 |dy| / (2^-100 sum) {float(r_neg.max()):.3g}, the other elements {ry:.3f}')
            assert float(e_pos.max()) <= C_DY
            assert float(r_neg.max()) <= 1.0
            assert ry <= C_DY


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_nonfinite_gradient_raises_the_flag(L, kind):
    """One dout element at +inf: a plain non-finite value travels into dW / db, and the engine's finish raises the state's flag."""
    C, H, W, s = 64, 20, 30, 2
    z, w, b, dout = make_inputs(kind, C, H, W, 7000)
    zg, wg, bg = z.cuda(), w.cuda(), b.cuda()
    og = run_fwd(L, kind, zg, wg, bg, C, H, W, False).cuda()
    for gs in GSCALES[kind]:
        d = dout * (min(gs, 1024.0) / gs)
        assert run_bwd(L, kind, zg, wg, og, d.cuda(), C, H, W, s, False, gs, engine=True)['flag'] == 0
        d[1, 333] = float('inf')
        r = run_bwd(L, kind, zg, wg, og, d.cuda(), C, H, W, s, False, gs, engine=True)
        assert r['flag'] == 1
        assert not torch.isfinite(r['db'][1]) and torch.isfinite(r['db'][0]) and torch.isfinite(r['db'][2])


@pytest.mark.parametrize('loss_type', [L2, FUSION6], ids=['L2', 'Fusion6'])
@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_loss_rider(L, kind, loss_type):
    """With a target the loss's launches come first and write dout, and its last stage rides on the head backward as one more work-group:
    stats and dout as orn_loss_fwd_bwd leaves them, dypad / dw / db as a rider-less call on that dout, bit for bit."""
    lib, st = L.lib(), L.stream()
    gs = GSCALES[kind][0]
    for C, (H, W, s) in ((96, (20, 30, 2)), (32, (130, 256, 2))):
        z, w, b, _ = make_inputs(kind, C, H, W, 8000 + C)
        zg, wg, bg = z.cuda(), w.cuda(), b.cuda()
        og = run_fwd(L, kind, zg, wg, bg, C, H, W, False).cuda()
        target = torch.rand(3, H * W, generator=torch.Generator().manual_seed(8001)).cuda()
        nb = lib.orn_loss_ws_bytes_for(loss_type, 1, 3, H, W)
        lws = torch.full((nb // 4,), float('nan'), device='cuda')
        stats_ref = torch.full((8,), float('nan'), device='cuda')
        dout_ref = torch.full((3, H * W), float('nan'), device='cuda')
        L.check(lib.orn_loss_fwd_bwd(L.ptr(og), L.ptr(target), 1, 3, H, W, loss_type, c_float(gs), L.ptr(stats_ref), L.ptr(dout_ref), L.ptr(lws),
                                     c_size_t(nb), st), 'loss_fwd_bwd')
        torch.cuda.synchronize()
        assert torch.isfinite(stats_ref).all() and torch.isfinite(dout_ref).all()
        plain = run_bwd(L, kind, zg, wg, og, dout_ref, C, H, W, s, False, gs)
        for engine in (False, True):
            dbuf, dg = banded((3, H * W), torch.float32)
            r = run_bwd(L, kind, zg, wg, og, dg, C, H, W, s, False, gs, engine=engine, target=target, loss_type=loss_type)
            assert bands_intact(dbuf)
            assert torch.equal(bits(dg.cpu()), bits(dout_ref.cpu())), 'dout differs from orn_loss_fwd_bwd'
            assert torch.equal(bits(r['stats']), bits(stats_ref.cpu())), (r['stats'], stats_ref)
            same_bits(r, plain, f'rider (engine form: {engine}) against the rider-less call')
            assert r['flag'] in (None, 0)


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_forward_equals_the_side_head_forward(L, kind):
    """include/orn_debug.h: with C % 32 == 0 the side head's 16-bit forward has the summation order of this one -- same bits."""
    lib, st = L.lib(), L.stream()
    H, W = 20, 30
    differ = []
    for C in FWD_CHANNELS:
        z, w, b, _ = make_inputs(kind, C, H, W, 9000 + C)
        zg, wg, bg = z.cuda(), w.cuda(), b.cuda()
        for sigmoid in (False, True):
            out = run_fwd(L, kind, zg, wg, bg, C, H, W, sigmoid)
            side = torch.full((3, H * W), float('nan'), device='cuda')
            L.check(getattr(lib, f'orn_debug_side_head_fwd_{kind}')(L.ptr(zg), L.ptr(wg), L.ptr(bg), C, H, W, int(sigmoid), L.ptr(side), st),
                    'side_head_fwd')
            torch.cuda.synchronize()
            if not torch.equal(bits(out), bits(side.cpu())):
                differ.append((C, sigmoid, float((out - side.cpu()).abs().max())))
    print(f'\nhead16 forward against the side head forward, {kind}: differing cases {differ}')
    assert not differ


def test_bad_arguments_are_refused(L):
    lib = L.lib()
    assert lib.orn_debug_head16_bwd_ws_bytes(0) == 0 and lib.orn_debug_head16_bwd_ws_bytes(48) == 0
    assert lib.orn_debug_head16_bwd_ws_bytes(96) == 513 * (3 * 96 + 3) * 4
    assert lib.orn_debug_head16_bwd_blocks(0, 4) == 0 and lib.orn_debug_head16_bwd_blocks(4, -1) == 0
    assert lib.orn_debug_head16_bwd_rider_ws_bytes(96, 20, 30, 99) == 0 and lib.orn_debug_head16_bwd_rider_ws_bytes(48, 20, 30, L2) == 0
    z = torch.zeros(4, 4, 32, dtype=torch.bfloat16, device='cuda')
    y = torch.zeros(4, 4, 128, dtype=torch.bfloat16, device='cuda')
    nb = lib.orn_debug_head16_bwd_ws_bytes(32)
    f = torch.zeros(nb // 4, device='cuda')

    def call(zp, C, H, sp, nbytes):
        return lib.orn_debug_head_bwd_bf16(zp, L.ptr(f), L.ptr(f), L.ptr(f), C, H, 4, 0, sp, c_float(1), L.ptr(y), L.ptr(f), L.ptr(f), L.ptr(f),
                                           c_size_t(nbytes), None, None, L2, None, L.stream())
    assert call(L.ptr(z), 32, 4, 3, nb) == -1 and 'stride' in L.last_error()
    assert call(L.ptr(z), 32, 4, 2, 16) == -2 and 'workspace' in L.last_error()
    assert call(L.ptr(z), 48, 4, 2, nb) == -1 and 'C=48' in L.last_error()
    assert call(None, 32, 4, 2, nb) == -1 and 'null' in L.last_error()
    assert lib.orn_debug_head_fwd_bf16(L.ptr(z), L.ptr(f), L.ptr(f), 48, 4, 4, 0, L.ptr(f), L.stream()) == -1 and 'C=48' in L.last_error()
    assert lib.orn_debug_head_fwd_bf16(L.ptr(z), L.ptr(f), L.ptr(f), 0, 4, 4, 0, L.ptr(f), L.stream()) == -1
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0 and float(f.abs().max()) == 0.0       # nothing was launched
