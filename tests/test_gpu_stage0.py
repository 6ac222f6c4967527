"""The fp32 front of the 16-bit engine, elementwise against a float64 reference: the fused first block (k_stage0_fwd, k_stage0_bwd
of orn_stage0.hip) and the B == 1 stem backward that sums the block's per-work-group dx slabs (orn_stem_l2_block / k_stem_bwd_l2,
k_linear_silu_bwd_w_slabs), through the test entry points of include/orn_debug.h; and the workspace of orn_stem_bwd.

The engine reaches the fused block at three shapes only (C = 26 or 48, s = 5 or 4, W = 16, Cn = 96) and judges it by norms over a
whole network.  The cases below are the smallest shapes that reach each edge of the two kernels: C16 = 16 / 32 / 48 / 64 with and
without a ragged last batch of channels, s = 1 (the divide-by-one path of s0_div), Cn and O not a multiple of 16, W not a multiple
of 4 (a lane's four pixels in two rows, the row wrap of the dW loop), one wave and sixteen, Cn < Cp and Cn = Cp, 1 / 3 / 9 input
slabs, and the three product shapes (one of them beyond 64 KB of LDS).

Reference: float64 on the CPU (conv2d, pixel_shuffle, unfold, conv_transpose2d, closed forms), from the identical fp32 inputs; it
does not use liborn.  Per element, never as a norm, with A the same linear operation on the absolute values (float64):
    fp32 outputs          |k - r| <= c * A                  (z, dwf, dbf, dx slabs summed, dx)
                          |k - r| <= c * A + extra          (the stem's dw0, db0, dw1, db1)
    16-bit xpad_next      |k - silu(r)| <= ulp16(silu(r)) + c' * A
extra: where SiLU'(z) = s (1 + z (1 - s)) multiplies an output elementwise (the stem's four outputs), its fp32 evaluation leaves an
error that does not scale with SiLU' itself -- the factor 1 + z (1 - s) cancels near z = -1.28, where A vanishes with it: with e
the relative error of s (expf, 1 + e^-z, reciprocal + one Newton step: below 5 * 2^-24) the computed value differs by at most
|SiLU'| (e + 3 * 2^-24) + |z| s (2 * 2^-24 (1 - s) + s e) < 2^-20 (1 + |z|) s.  That much, times the gradient |g| it multiplies,
is allowed apart instead of inflating c, as _run_dgrad of test_gpu_conv16_forms.py allows 2^-20 (1 + |z|) |g| (here times
s <= 1: the exact-mode SiLU' needs no more).  Outputs that sum over many SiLU' factors (dwf, dbf, dx; the upstream part of the
stem's dw0 / db0) get no allowance: there the error is covered by c * A.
c per output is C_TOL below: at most 3x the worst ratio measured on an MI355X, which stands in the comment beside it; every case
prints its own.  Each measured ratio is also asserted below (L + 2) * 2^-24, L the longest summation chain of that output
(9 * C16 forward, H*W for dW / dbias, 144 + slabs for dx; 16 + ceil(Nout / 16) for the stem's dw0 / db0, the slab count for
dw1 / db1): nothing loses more than its fp32 chain explains (the closest, dwf at H*W = 16, reaches 36 % of its cap).
The module's 59 tests run in about 3 s on one MI355X, none above 0.4 s.

Contract checks on every case:
  - the ring of xpad_next and its channels [Cn, Cp) hold a finite sentinel before and after the call;
  - a sentinel guard behind z, xpad_next, dwf, dbf, slabs, dx (and behind every stem output and the stem's workspace) is unchanged;
  - z, slabs, dwf, dbf (and the stem's outputs) start as NaN and are finite afterwards: every element a consumer reads is written;
  - channels [Cn, Cp) of dxn hold NaN and nothing leaks (the narrow dgrad form really leaves them unwritten);
  - z == NULL gives the same xpad_next bits; two runs are bit-identical.
"""
import functools
import math
from ctypes import c_float, c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = 7.0                     # finite sentinel, exact in bf16 and fp16
GUARD = 1024                   # elements of sentinel behind every output
NAN = float('nan')
DT = {'bf16': torch.bfloat16, 'fp16': torch.float16}
PREC = {'bf16': 1, 'fp16': 2}
EPS = 2.0 ** -24

# c of the bound above per output: at most 3x the worst ratio measured on an MI355X (the comment gives it).
C_TOL = {
    'fwd z':          1.35e-6,  # measured 4.52e-7 (C = 48, a chain of 432 products)
    'fwd xpad bf16':  4.6e-7,   # measured 1.54e-7
    'fwd xpad fp16':  4.6e-7,   # measured 1.55e-7
    'bwd dbf':        2.9e-7,   # measured 9.98e-8
    'bwd dwf':        1.1e-6,   # measured 3.83e-7 (H*W = 16, 3 slabs: a third of its cap)
    'bwd slabs':      5.3e-7,   # measured 1.79e-7
    'bwd dx':         5.3e-7,   # measured 1.79e-7
    'stem db1':       1.4e-7,   # measured 4.78e-8
    'stem dw1':       1.4e-7,   # measured 4.82e-8
    'stem db0':       2.1e-7,   # measured 7.25e-8
    'stem dw0':       2.1e-7,   # measured 7.26e-8
    'chain db1':      1.0e-8,   # measured 3.59e-9 (A of the chain is far above |dx|: the block's dx cancels)
    'chain dw1':      1.1e-8,   # measured 3.67e-9
    'chain db0':      0.0,      # measured 0: the whole difference lies inside the SiLU' allowance of pre1
    'chain dw0':      0.0,      # measured 0: as db0
}
WORST = {}                     # output -> worst measured ratio of this run


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_stage0_supported', 'orn_debug_stage0_slabs', 'orn_debug_stage0_fwd', 'orn_debug_stage0_bwd',
                 'orn_debug_stem_bwd_slabs', 'orn_stem_bwd_ws_bytes'):
        assert hasattr(lib, name), name
    torch.set_num_threads(16)
    return lib


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    torch.cuda.synchronize()


def _err():
    import orn_amd
    return orn_amd._lib.last_error()


# ---- the kernels under test (one thin call each) -----------------------------------------------------------------------------
def k_supported(L, C, O, H, W, s):
    return L.orn_debug_stage0_supported(C, O, H, W, s)


def k_slabs(L, O, s):
    return L.orn_debug_stage0_slabs(O, s)


def k_fwd(L, x, wf, bf, C, O, H, W, s, z, xpad, Cp, half):
    return L.orn_debug_stage0_fwd(_p(x), _p(wf), _p(bf), C, O, H, W, s, _p(z), _p(xpad), Cp, PREC[half], _st())


def k_bwd(L, x, wf, z, dxn, nslab, Cp, inv_gs, C, O, H, W, s, slabs, dx, dwf, dbf):
    return L.orn_debug_stage0_bwd(_p(x), _p(wf), _p(z), _p(dxn), nslab, Cp, c_float(inv_gs), C, O, H, W, s, _p(slabs), _p(dx),
                                  _p(dwf), _p(dbf), _st())


def k_stem_slabs(L, embed, w1, pre1, h1, pre2, slabs, nslab, E, Hd, Nout, dw0, db0, dw1, db1, ws, ws_bytes):
    return L.orn_debug_stem_bwd_slabs(_p(embed), _p(w1), _p(pre1), _p(h1), _p(pre2), _p(slabs), nslab, E, Hd, Nout, _p(dw0), _p(db0),
                                      _p(dw1), _p(db1), _p(ws), ws_bytes, _st())


def k_stem_bwd(L, embed, w1, pre1, h1, pre2, dh2, E, Hd, Nout, dw0, db0, dw1, db1, ws):
    return L.orn_stem_bwd(_p(embed), _p(w1), _p(pre1), _p(h1), _p(pre2), _p(dh2), 1, E, Hd, Nout, _p(dw0), _p(db0), _p(dw1), _p(db1),
                          _p(ws), _st())


def k_ws_bytes(L, B, Hd, Nout):
    return L.orn_stem_bwd_ws_bytes(B, Hd, Nout)


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _ulp16(r, half):
    e = torch.floor(torch.log2(r.abs().clamp_min(1e-300)))
    if half == 'bf16':
        return torch.exp2(e.clamp_min(-126) - 7)
    return torch.exp2(e.clamp_min(-14) - 10)


def _silu(z):
    return z * torch.sigmoid(z)


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _silu_grad_allow(z):
    """Allowance for the fp32 evaluation of SiLU'(z) = s (1 + z (1 - s)), per unit of the gradient it multiplies (module
    docstring)."""
    return 2.0 ** -20 * (1 + z.abs()) * torch.sigmoid(z)


def _guarded(n, dtype=torch.float32, fill=NAN):
    """Flat buffer of n elements of `fill` + GUARD elements of sentinel behind; returns (whole buffer, view of the n elements)."""
    buf = torch.full((n + GUARD,), SENT, dtype=dtype, device=DEV)
    buf[:n] = fill
    return buf, buf[:n]


def _guard_ok(buf, n, what):
    g = buf[n:].float()
    assert bool((g == SENT).all()), f'{what}: {int((g != SENT).sum())} guard elements behind the output were written'


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _scales(n, gen, lo=-1.5, hi=1.5):
    return torch.exp2(torch.rand(n, generator=gen) * (hi - lo) + lo)


def _first_bad(bad, k, r, what):
    i = int(torch.nonzero(bad.flatten())[0])
    return (f'{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at flat index {i} (shape {tuple(bad.shape)}): '
            f'kernel {float(k.flatten()[i])!r} reference {float(r.flatten()[i])!r}')


def _check32(k, r, A, name, what, chain, extra=None):
    """fp32 output k against r: |k - r| <= c * A + extra; the measured ratio below (chain + 2) * 2^-24."""
    k = k.double().cpu().reshape(r.shape)
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    ex = torch.zeros_like(d) if extra is None else extra
    ratio = float(((d - ex).clamp_min(0) / A.clamp_min(1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f'RATIO {name} {what} {ratio:.3e} (cap {(chain + 2) * EPS:.3e})')
    bad = d > C_TOL[name] * A + ex
    assert not bool(bad.any()), _first_bad(bad, k, r, f'{name} {what}')
    assert ratio < (chain + 2) * EPS, f'{name} {what}: ratio {ratio:.3e} above the chain cap {(chain + 2) * EPS:.3e}'


def _check16(k, r, A, half, name, what, chain):
    """16-bit output k against r: |k - r| <= ulp16(r) + c * A; the measured ratio is the part beyond half an ulp."""
    k = k.double().cpu().reshape(r.shape)
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    u = _ulp16(r, half)
    ratio = float(((d - u / 2).clamp_min(0) / A.clamp_min(1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f'RATIO {name} {what} {ratio:.3e} (cap {(chain + 2) * EPS:.3e})')
    bad = d > u + C_TOL[name] * A
    assert not bool(bad.any()), _first_bad(bad, k, r, f'{name} {what}')
    assert ratio < (chain + 2) * EPS, f'{name} {what}: ratio {ratio:.3e} above the chain cap {(chain + 2) * EPS:.3e}'


# ---- the fused first block -----------------------------------------------------------------------------------------------------
CASES = [
    # C, Cn, s, H, W, Cp, nslab, inv_gs                the smallest shape that reaches each edge
    (1, 1, 2, 4, 4, 96, 1, 1.0),                     # one wave, O = 4 < 16, Cn < 16
    (16, 16, 1, 4, 4, 96, 3, 2.0 ** -20),            # s = 1: the divide-by-one path
    (17, 24, 2, 4, 4, 96, 9, 1.0 / 3),               # C16 = 32 ragged, Cn = 24 ragged
    (17, 24, 2, 4, 4, 24, 3, 1.0),                   # the same with Cp = Cn
    (33, 8, 3, 4, 8, 96, 1, 2.0 ** -20),             # C16 = 48, O = 72
    (64, 16, 2, 4, 4, 96, 9, 1.0),                   # maximum C
    (5, 3, 3, 8, 6, 96, 3, 1.0 / 3),                 # W % 4 != 0, W + 2 = 8
    (7, 16, 2, 16, 5, 96, 9, 2.0 ** -20),            # W = 5
    (3, 8, 2, 8, 14, 96, 1, 1.0 / 3),                # W % 4 = 2, W + 2 = 16
    (4, 16, 2, 1, 16, 96, 3, 1.0),                   # one row
    (4, 8, 2, 64, 4, 96, 9, 1.0 / 3),                # tall, sixteen waves
    (8, 16, 2, 16, 16, 96, 3, 2.0 ** -20),           # sixteen waves
    (26, 96, 5, 9, 16, 96, 3, 1.0 / 3),              # 720p
    (48, 96, 5, 9, 16, 96, 9, 2.0 ** -20),           # 1080p: more than 64 KB of LDS, the attribute path
    (26, 96, 4, 2, 16, 96, 1, 1.0),                  # the 2_16_26 fit
]
CHAIN_CASE = CASES[12]


def _case_id(c):
    return 'C%d-Cn%d-s%d-%dx%d-Cp%d-n%d' % c[:7]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Seeded fp32 inputs of a case (on the device) and the forward's float64 reference r, A [O][H][W] (CPU); shared by the tests
    of the case and left unchanged."""
    C, Cn, s, H, W, Cp, nslab, inv_gs = case
    O = Cn * s * s
    gen = torch.Generator().manual_seed(C * 7919 + Cn * 131 + s * 17 + H * 5 + W)
    x = (torch.randn(C, H, W, generator=gen) + 0.25) * _scales(C, gen)[:, None, None]
    wf = (torch.randn(O, C, 3, 3, generator=gen) + 0.2) / math.sqrt(9 * C)
    wf = wf * _scales(O, gen, -1, 1)[:, None, None, None] * _scales(C, gen, -1, 1)[None, :, None, None]
    bf = torch.randn(O, generator=gen) * 0.3
    # the next block's dgrad slabs, each at another scale, times 1 / inv_gs; channels [Cn, Cp) are never written by its narrow form
    dxn = torch.full((nslab, H * s, W * s, Cp), NAN)
    ig = float(np.float32(inv_gs))
    dxn[..., :Cn] = (torch.randn(nslab, H * s, W * s, Cn, generator=gen) + 0.1) * _scales(nslab, gen, -3, 3)[:, None, None, None] / ig
    x64, w64, b64 = x.double(), wf.double(), bf.double()
    r = F.conv2d(x64[None], w64, b64, padding=1)[0]
    A = F.conv2d(x64[None].abs(), w64.abs(), b64.abs(), padding=1)[0]
    return dict(x=x.to(DEV), wf=wf.to(DEV), bf=bf.to(DEV), dxn=dxn.to(DEV), x64=x64, w64=w64, r=r, A=A, ig=ig)


def _run_fwd(L, case, half, keep_z=True):
    C, Cn, s, H, W, Cp = case[:6]
    O, inp = Cn * s * s, _inputs(case)
    nz, na = O * H * W, (H * s + 2) * (W * s + 2) * Cp
    zbuf, z = _guarded(nz) if keep_z else (None, None)
    abuf, a = _guarded(na, DT[half], fill=SENT)
    rc = k_fwd(L, inp['x'], inp['wf'], inp['bf'], C, O, H, W, s, z, a, Cp, half)
    assert rc == 0, _err()
    _sync()
    _guard_ok(abuf, na, 'xpad_next')
    if keep_z:
        _guard_ok(zbuf, nz, 'z')
    return z, a.view(H * s + 2, W * s + 2, Cp)


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_stage0_fwd(L, case, half):
    C, Cn, s, H, W, Cp = case[:6]
    O, ss, HW, inp = Cn * s * s, s * s, H * W, _inputs(case)
    assert k_supported(L, C, O, H, W, s) == 1
    z, a = _run_fwd(L, case, half)
    z2, a2 = _run_fwd(L, case, half)
    _, a3 = _run_fwd(L, case, half, keep_z=False)
    assert torch.equal(_bits(z), _bits(z2)) and torch.equal(_bits(a), _bits(a2)), 'two runs differ'
    assert torch.equal(_bits(a), _bits(a3)), 'z == NULL changes xpad_next'
    ring = torch.cat([a[0].flatten(), a[-1].flatten(), a[:, 0].flatten(), a[:, -1].flatten()]).float()
    assert bool((ring == SENT).all()), f'xpad_next: {int((ring != SENT).sum())} ring elements written'
    assert bool((a[..., Cn:].float() == SENT).all()), 'xpad_next: channels [Cn, Cp) written'
    where = f'{_case_id(case)} {half}'
    # z [s^2][H*W][Cn]: element (sub, px, n) = conv channel n * s^2 + sub
    r, A = (t.view(Cn, ss, HW).permute(1, 2, 0) for t in (inp['r'], inp['A']))
    _check32(z, r, A, 'fwd z', where, chain=9 * ((C + 15) // 16 * 16))
    rs, As = (F.pixel_shuffle(t[None], s)[0].permute(1, 2, 0) for t in (inp['r'], inp['A']))     # [H*s][W*s][Cn]
    _check16(a[1:-1, 1:-1, :Cn], _silu(rs), As, half, f'fwd xpad {half}', where, chain=9 * ((C + 15) // 16 * 16))


def _bwd_ref(case, z):
    """float64 backward of the block from its fp32 inputs and the kernel's own z: {output: (r, A)}."""
    C, Cn, s, H, W, Cp, nslab, _ = case
    O, ss, HW, inp = Cn * s * s, s * s, H * W, _inputs(case)
    d = inp['dxn'][..., :Cn].double().cpu()
    G, AG = (F.pixel_unshuffle(t.permute(2, 0, 1)[None], s)[0] for t in (d.sum(0), d.abs().sum(0)))   # [O][H][W], o = n s^2 + i s + j
    zc = z.double().cpu().view(ss, HW, Cn).permute(2, 0, 1).reshape(O, H, W)
    sg, ig = _silu_grad(zc), inp['ig']
    dy, Ady = G * ig * sg, AG * ig * sg.abs()
    xcol = F.unfold(inp['x64'][None], 3, padding=1)[0]                                              # [C*9][HW], row c * 9 + tap
    return {'dbf': (dy.sum((1, 2)), Ady.sum((1, 2))),
            'dwf': (dy.view(O, HW) @ xcol.T, Ady.view(O, HW) @ xcol.abs().T),
            'dx': (F.conv_transpose2d(dy[None], inp['w64'], padding=1)[0], F.conv_transpose2d(Ady[None], inp['w64'].abs(), padding=1)[0])}


def _run_bwd(L, case, z, with_dx):
    C, Cn, s, H, W, Cp, nslab, inv_gs = case
    O, inp = Cn * s * s, _inputs(case)
    nwg = k_slabs(L, O, s)
    assert nwg == s * s * -(-Cn // 16)
    n = C * H * W
    sbuf, slabs = _guarded(nwg * n)
    wbuf, dwf = _guarded(O * C * 9)
    bbuf, dbf = _guarded(O)
    xbuf, dx = _guarded(n) if with_dx else (None, None)
    rc = k_bwd(L, inp['x'], inp['wf'], z, inp['dxn'], nslab, Cp, inp['ig'], C, O, H, W, s, slabs, dx, dwf, dbf)
    assert rc == 0, _err()
    _sync()
    for buf, m, what in ((sbuf, nwg * n, 'slabs'), (wbuf, O * C * 9, 'dwf'), (bbuf, O, 'dbf')) + (((xbuf, n, 'dx'),) if with_dx else ()):
        _guard_ok(buf, m, what)
    return slabs.view(nwg, n), dx, dwf, dbf


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_stage0_bwd(L, case):
    C, Cn, s, H, W, Cp, nslab, inv_gs = case
    O, HW = Cn * s * s, H * W
    assert k_supported(L, C, O, H, W, s) == 1
    z, _ = _run_fwd(L, case, 'fp16')
    assert bool(torch.isfinite(z).all()), 'z: elements the backward reads were not written'
    slabs, _, dwf, dbf = _run_bwd(L, case, z, with_dx=False)
    slabs2, dx, dwf2, dbf2 = _run_bwd(L, case, z, with_dx=True)
    assert bool(torch.isfinite(slabs).all()), 'slabs: elements the consumer reads were not written (or NaN leaked from dxn)'
    for p, q, what in ((slabs, slabs2, 'slabs'), (dwf, dwf2, 'dwf'), (dbf, dbf2, 'dbf')):
        assert torch.equal(_bits(p), _bits(q)), f'{what}: two runs differ'
    ref = _bwd_ref(case, z)
    where = _case_id(case) + f' inv_gs={inv_gs:.3g}'
    _check32(dbf, *ref['dbf'], 'bwd dbf', where, chain=HW)
    _check32(dwf, *ref['dwf'], 'bwd dwf', where, chain=HW)
    nwg = slabs.shape[0]
    _check32(slabs.double().sum(0), *ref['dx'], 'bwd slabs', where, chain=144 + nwg)
    _check32(dx, *ref['dx'], 'bwd dx', where, chain=144 + nwg)


def test_stage0_rejects_unsupported_shapes(L):
    """A shape the fused block declines returns ORN_E_ARG with a text that names stage0, and launches nothing."""
    big = torch.full((1 << 20,), SENT, device=DEV)
    half = torch.full((1 << 20,), SENT, dtype=torch.float16, device=DEV)
    for C, Cn, s, H, W in [(4, 4, 2, 1, 6),        # H*W = 6
                           (65, 4, 2, 4, 4),       # C = 65
                           (4, 4, 2, 16, 3)]:      # W = 3 (H*W = 48)
        O = Cn * s * s
        assert k_supported(L, C, O, H, W, s) == 0
        assert k_fwd(L, big, big, big, C, O, H, W, s, big, half, 96, 'fp16') == -1, (C, Cn, s, H, W)
        assert 'stage0' in _err(), _err()
        assert k_bwd(L, big, big, big, big, 1, 96, 1.0, C, O, H, W, s, big, big, big, big) == -1, (C, Cn, s, H, W)
        assert 'stage0' in _err(), _err()
    assert k_slabs(L, 0, 2) == 0 and k_slabs(L, 16, 0) == 0 and k_slabs(L, 2400, 5) == 150
    _sync()
    assert bool((big == SENT).all()) and bool((half.float() == SENT).all())


# ---- the stem backward on slabs ----------------------------------------------------------------------------------------------
def _stem_inputs(E, Hd, Nout, nslab, seed):
    gen = torch.Generator().manual_seed(seed)
    t = dict(embed=torch.randn(E, generator=gen), w1=(torch.randn(Nout, Hd, generator=gen) + 0.1) / math.sqrt(Hd),
             pre1=torch.randn(Hd, generator=gen) * 2 + 0.3, h1=torch.randn(Hd, generator=gen) + 0.25,
             pre2=torch.randn(Nout, generator=gen) * 2 + 0.3)
    if nslab:          # each slab at another scale
        t['slabs'] = (torch.randn(nslab, Nout, generator=gen) + 0.1) * _scales(nslab, gen, -3, 3)[:, None]
    return t


def _stem_ref(t, G, AG):
    """float64 stem backward at B = 1 from the upstream gradient G [Nout] (AG: the A of it), by the formulas above OrnStemL2Job
    (orn_common.h): {output: (r, A, extra)}; extra is the allowance for the SiLU' that multiplies the output elementwise."""
    embed, w1, pre1, h1, pre2 = (t[k].double().cpu() for k in ('embed', 'w1', 'pre1', 'h1', 'pre2'))
    sg2 = _silu_grad(pre2)
    d2, Ad2, Ed2 = G * sg2, AG * sg2.abs(), _silu_grad_allow(pre2) * G.abs()
    dh1, Adh1 = w1.T @ d2, w1.abs().T @ Ad2
    sg1 = _silu_grad(pre1)
    d1, Ad1, Ed1 = dh1 * sg1, Adh1 * sg1.abs(), _silu_grad_allow(pre1) * dh1.abs()
    return {'db1': (d2, Ad2, Ed2), 'dw1': tuple(torch.outer(v, h1.abs() if i else h1) for i, v in enumerate((d2, Ad2, Ed2))),
            'db0': (d1, Ad1, Ed1), 'dw0': tuple(torch.outer(v, embed.abs() if i else embed) for i, v in enumerate((d1, Ad1, Ed1)))}


def _stem_outputs(E, Hd, Nout):
    return {k: _guarded(n) for k, n in (('dw0', Hd * E), ('db0', Hd), ('dw1', Nout * Hd), ('db1', Nout))}


def _stem_check(out, E, Hd, Nout, ref, prefix, where, chain_l2, chain_w0):
    for k, n in (('dw0', Hd * E), ('db0', Hd), ('dw1', Nout * Hd), ('db1', Nout)):
        _guard_ok(out[k][0], n, k)
        r, A, ex = ref[k]
        _check32(out[k][1], r, A, f'{prefix} {k}', where, chain=chain_w0 if k in ('dw0', 'db0') else chain_l2, extra=ex)


def _run_stem_slabs(L, t, slabs, nslab, E, Hd, Nout):
    nb = k_ws_bytes(L, 1, Hd, Nout)
    assert nb % 4 == 0 and nb >= 4 * (Nout + 2 * Hd + max(256, -(-Nout // 16)) * Hd)
    wsbuf, ws = _guarded(nb // 4)
    out = _stem_outputs(E, Hd, Nout)
    d = {k: v.to(DEV) for k, v in t.items() if k != 'slabs'}
    rc = k_stem_slabs(L, d['embed'], d['w1'], d['pre1'], d['h1'], d['pre2'], slabs, nslab, E, Hd, Nout, out['dw0'][1], out['db0'][1],
                      out['dw1'][1], out['db1'][1], ws, nb)
    assert rc == 0, _err()
    _sync()
    _guard_ok(wsbuf, nb // 4, 'ws')
    return out


STEM_CASES = [
    # Nout, Hd, E, nslab
    (15, 8, 80, 1),            # less than one work-group of 16 rows
    (16, 300, 130, 2),
    (17, 8, 130, 63),          # one row in the second work-group; one lane without a slab
    (2065, 300, 130, 65),      # every size ragged: Nout % 16 = 1, Hd beyond 256 threads, E beyond 128, one slab in the second round
    (4112, 8, 80, 64),         # 257 partial rows: beyond the 256 of the batched form
    (4112, 300, 80, 150),
    (2065, 8, 80, 150),
]


@pytest.mark.parametrize('Nout,Hd,E,nslab', STEM_CASES)
def test_stem_bwd_slabs(L, Nout, Hd, E, nslab):
    t = _stem_inputs(E, Hd, Nout, nslab, seed=Nout * 31 + Hd * 7 + E + nslab)
    out = _run_stem_slabs(L, t, t['slabs'].to(DEV), nslab, E, Hd, Nout)
    out2 = _run_stem_slabs(L, t, t['slabs'].to(DEV), nslab, E, Hd, Nout)
    for k in out:
        assert torch.equal(_bits(out[k][1]), _bits(out2[k][1])), f'{k}: two runs differ'
    s64 = t['slabs'].double()
    ref = _stem_ref(t, s64.sum(0), s64.abs().sum(0))
    _stem_check(out, E, Hd, Nout, ref, 'stem', f'Nout={Nout} Hd={Hd} E={E} nslab={nslab}', nslab, 16 + -(-Nout // 16))


def test_stem_bwd_slabs_rejects_a_short_workspace(L):
    big = torch.full((1 << 16,), SENT, device=DEV)
    nb = k_ws_bytes(L, 1, 8, 4112)
    assert k_stem_slabs(L, big, big, big, big, big, big, 1, 80, 8, 4112, big, big, big, big, big, nb - 4) == -2
    assert 'stem_bwd_slabs' in _err(), _err()
    _sync()
    assert bool((big == SENT).all())


def test_stage0_slabs_into_stem_bwd(L):
    """The engine's hand-off: the slabs orn_debug_stage0_bwd leaves with dx == NULL go straight into the stem backward, which sums
    them; against the float64 chain from the block's inputs."""
    case = CHAIN_CASE
    C, Cn, s, H, W, Cp, nslab, inv_gs = case
    O, E, Hd, Nout = Cn * s * s, 80, 64, C * H * W
    z, _ = _run_fwd(L, case, 'fp16')
    slabs, _, _, _ = _run_bwd(L, case, z, with_dx=False)
    nwg = k_slabs(L, O, s)
    assert nwg == 150 and tuple(slabs.shape) == (nwg, Nout)
    t = _stem_inputs(E, Hd, Nout, 0, seed=99)
    out = _run_stem_slabs(L, t, slabs, nwg, E, Hd, Nout)
    r, A = (v.reshape(-1) for v in _bwd_ref(case, z)['dx'])
    _stem_check(out, E, Hd, Nout, _stem_ref(t, r, A), 'chain', _case_id(case), 144 + nwg, 144 + nwg + 16 + -(-Nout // 16))


# ---- the workspace of orn_stem_bwd -------------------------------------------------------------------------------------------
WS_CASES = [(4112, 8), (6912, 32)]      # (Nout, Hd): 257 and 432 partial rows at B = 1; the second is the 1080p stem's Nout


@pytest.mark.parametrize('Nout,Hd', WS_CASES)
def test_stem_bwd_stays_inside_its_workspace(L, Nout, Hd):
    """orn_stem_bwd at B = 1 with a workspace of exactly orn_stem_bwd_ws_bytes: the cdiv(Nout, 16) rows of partial sums stay inside
    it (a library that sized 256 rows wrote (cdiv(Nout, 16) - 256) * Hd floats beyond; the guard keeps such a write inside the
    test's own allocation)."""
    E, rows = 80, -(-Nout // 16)
    nb = k_ws_bytes(L, 1, Hd, Nout)
    assert nb == 4 * (Nout + 2 * Hd + rows * Hd)
    n, g = nb // 4, max(GUARD, rows * Hd)
    buf = torch.full((n + g,), SENT, device=DEV)
    buf[:n] = NAN
    t = _stem_inputs(E, Hd, Nout, 1, seed=Nout + Hd)
    d = {k: v.to(DEV) for k, v in t.items()}
    out = _stem_outputs(E, Hd, Nout)
    rc = k_stem_bwd(L, d['embed'], d['w1'], d['pre1'], d['h1'], d['pre2'], d['slabs'], E, Hd, Nout, out['dw0'][1], out['db0'][1],
                    out['dw1'][1], out['db1'][1], buf)
    assert rc == 0, _err()
    _sync()
    assert bool((buf[n:] == SENT).all()), f'ws: {int((buf[n:] != SENT).sum())} floats written beyond orn_stem_bwd_ws_bytes'
    G = t['slabs'][0].double()
    _stem_check(out, E, Hd, Nout, _stem_ref(t, G, G.abs()), 'stem', f'orn_stem_bwd Nout={Nout} Hd={Hd}', 1,
                16 + rows)


@pytest.mark.parametrize('Nout,Hd', WS_CASES)
def test_stem_fn_backward_at_large_nout(L, Nout, Hd):
    """ops.StemFn (the eager model path) at the same sizes against float64 autograd; tolerances of test_stem_fwd_bwd
    (test_gpu_parity.py), the same comparison at Nout = 3744."""
    from orn_amd import ops
    E = 80
    gen = torch.Generator().manual_seed(Nout * 3 + Hd)
    e = torch.randn(1, E, generator=gen)
    w0 = torch.randn(Hd, E, generator=gen) / math.sqrt(E)
    b0 = torch.randn(Hd, generator=gen) * 0.1
    w1 = torch.randn(Nout, Hd, generator=gen) / math.sqrt(Hd)
    b1 = torch.randn(Nout, generator=gen) * 0.1
    dh2 = torch.randn(1, Nout, generator=gen)
    ref_in = [v.double().requires_grad_(True) for v in (w0, b0, w1, b1)]
    ref = F.silu(F.linear(F.silu(F.linear(e.double(), ref_in[0], ref_in[1])), ref_in[2], ref_in[3]))
    (ref * dh2.double()).sum().backward()
    dev_in = [v.to(DEV).requires_grad_(True) for v in (w0, b0, w1, b1)]
    out = ops.StemFn.apply(e.to(DEV), *dev_in)
    (out * dh2.to(DEV)).sum().backward()
    _sync()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=2e-6)
    for a, b, name in zip(dev_in, ref_in, ('w0', 'b0', 'w1', 'b1')):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=3e-5, atol=3e-6, err_msg=name)
