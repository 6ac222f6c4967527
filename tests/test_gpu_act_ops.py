"""The per-op ABI twins with act = gelu -- orn_stem_*_act and orn_conv3x3_ps_silu_*_act in fp32 (through ops.StemFn / ops.ConvPsSiluFn)
and in both 16-bit builds -- against torch on the CPU in fp64, under the tolerances test_gpu_parity.py and test_gpu_bf16.py hold the swish
entries to.  Shapes (C, O, H, W, s): (8, 32, 5, 7, 2) and (96, 384, 9, 16, 2)."""
import math
from ctypes import c_size_t

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GELU = 1
SHAPES = [(8, 32, 5, 7, 2), (96, 384, 9, 16, 2)]


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _dgelu(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def test_stem_twins(orn):
    """test_gpu_parity.py::test_stem_fwd_bwd's tolerances."""
    g = torch.Generator().manual_seed(11)
    B, E, Hd, Nout = 2, 80, 32, 96
    embed = torch.randn(B, E, generator=g)
    ws = [torch.randn(Hd, E, generator=g) / math.sqrt(E), torch.randn(Hd, generator=g) * 0.1,
          torch.randn(Nout, Hd, generator=g) / math.sqrt(Hd), torch.randn(Nout, generator=g) * 0.1]
    dout = torch.randn(B, Nout, generator=g)
    dev = [w.cuda().requires_grad_(True) for w in ws]
    out = orn.ops.StemFn.apply(embed.cuda(), *dev, 'gelu')
    out.backward(dout.cuda())
    ref_w = [w.double().requires_grad_(True) for w in ws]
    ref = F.gelu(F.linear(F.gelu(F.linear(embed.double(), ref_w[0], ref_w[1])), ref_w[2], ref_w[3]))
    ref.backward(dout.double())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=2e-6)
    for a, b in zip(dev, ref_w):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=3e-5, atol=3e-6)
    swish = orn.ops.StemFn.apply(embed.cuda(), *[w.detach() for w in dev])
    assert not torch.allclose(swish, out.detach(), atol=1e-3)               # five arguments: still swish


@pytest.mark.parametrize('C,O,H,W,s', SHAPES)
def test_conv_fp32_twins(orn, C, O, H, W, s):
    """test_gpu_parity.py::test_conv_ps_silu_vs_oracle's tolerances."""
    g = torch.Generator().manual_seed(C + O)
    x = torch.randn(1, C, H, W, generator=g)
    wf = torch.randn(O, C, 3, 3, generator=g) / math.sqrt(9 * C)
    bf = torch.randn(O, generator=g) * 0.1
    da = torch.randn(1, O // (s * s), H * s, W * s, generator=g)
    dx, dw, db = (t.cuda().requires_grad_(True) for t in (x, wf, bf))
    out = orn.ops.ConvPsSiluFn.apply(dx, dw, db, s, 'gelu')
    out.backward(da.cuda())
    rx, rw, rb = (t.double().requires_grad_(True) for t in (x, wf, bf))
    ref = F.gelu(F.pixel_shuffle(F.conv2d(rx, rw, rb, padding=1), s))
    ref.backward(da.double())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(dx.grad.cpu().numpy(), rx.grad.numpy(), rtol=1e-4, atol=1e-4)
    scale = float(rw.grad.abs().max())
    np.testing.assert_allclose(dw.grad.cpu().numpy(), rw.grad.numpy(), rtol=1e-4, atol=2e-5 * scale)
    np.testing.assert_allclose(db.grad.cpu().numpy(), rb.grad.numpy(), rtol=1e-4, atol=2e-5 * float(rb.grad.abs().max()))
    four = orn.ops.ConvPsSiluFn.apply(dx.detach(), dw.detach(), db.detach(), s)      # four arguments keep working: swish
    np.testing.assert_allclose(four.cpu().numpy(), F.silu(F.pixel_shuffle(F.conv2d(rx, rw, rb, padding=1), s)).detach().numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
def test_conv_16bit_twins(orn, half):
    """test_gpu_bf16.py::test_bf16_block_fwd_bwd with act = gelu at (96, 384, 9, 16, 2), its tolerances unchanged (the 16-bit hooks take
    C = 96 only: the (8, 32, 5, 7, 2) shape is the fp32 twins')."""
    C, O, H, W, s = SHAPES[1]
    L, P, st = orn._lib.lib(), orn._lib.ptr, orn._lib.stream
    rnd = lambda t: t.to(torch.bfloat16 if half == 'bf16' else torch.float16).to(torch.float32)       # noqa: E731
    fwd_fn = L.orn_conv3x3_ps_silu_fwd_bf16_act if half == 'bf16' else L.orn_conv3x3_ps_silu_fwd_f16_act
    bwd_fn = L.orn_conv3x3_ps_silu_bwd_bf16_act if half == 'bf16' else L.orn_conv3x3_ps_silu_bwd_f16_act
    tol = 5e-3 if half == 'bf16' else 1e-3
    gen = torch.Generator().manual_seed(C + O + H * W)
    x = rnd(torch.randn(1, C, H, W, generator=gen))
    wf = rnd(torch.randn(O, C, 3, 3, generator=gen) / math.sqrt(9 * C))
    bf = torch.randn(O, generator=gen) * 0.1
    Cn = O // (s * s)
    da = torch.randn(1, Cn, H * s, W * s, generator=gen)
    rx, rw, rb = (t.double().requires_grad_(True) for t in (x, wf, bf))
    y = F.conv2d(rx, rw, rb, padding=1)
    zr = F.pixel_shuffle(y, s)
    ar = F.gelu(zr)
    nb = L.orn_conv3x3_ps_silu_bf16_ws_bytes(C, O, H, W, s)
    ws = torch.zeros(nb, dtype=torch.uint8, device='cuda')
    xd, wd, bd = x.cuda(), wf.cuda(), bf.cuda()
    z = torch.empty(1, Cn, H * s, W * s, device='cuda')
    a = torch.empty_like(z)
    orn._lib.check(fwd_fn(P(xd), P(wd), P(bd), C, O, H, W, s, P(z), P(a), P(ws), c_size_t(nb), st(), GELU))
    np.testing.assert_allclose(z.cpu().numpy(), zr.detach().numpy(), rtol=tol, atol=tol)
    np.testing.assert_allclose(a.cpu().numpy(), ar.detach().numpy(), rtol=tol, atol=tol)
    zq = rnd(zr.detach().float()).double()
    dz = rnd((da.double() * _dgelu(zq)).float()).double()
    dy = F.pixel_unshuffle(dz, s)
    gx, gw = torch.autograd.grad(y, (rx, rw), dy)
    gb = dy.sum(dim=(0, 2, 3))
    dx = torch.empty(1, C, H, W, device='cuda')
    dwf = torch.empty(O, C, 3, 3, device='cuda')
    dbf = torch.empty(O, device='cuda')
    zd, dad = zr.detach().float().cuda().contiguous(), da.cuda()
    orn._lib.check(bwd_fn(P(xd), P(wd), P(zd), P(dad), C, O, H, W, s, P(dx), P(dwf), P(dbf), P(ws), c_size_t(nb), st(), GELU))
    torch.cuda.synchronize()
    np.testing.assert_allclose(dwf.cpu().numpy(), gw.numpy(), rtol=2e-3, atol=2e-3 * float(gw.abs().max()))
    np.testing.assert_allclose(dbf.cpu().numpy(), gb.numpy(), rtol=2e-3, atol=2e-3 * float(gb.abs().max()))
    np.testing.assert_allclose(dx.cpu().numpy(), gx.numpy(), rtol=2e-3, atol=2e-3 * float(gx.abs().max()))
