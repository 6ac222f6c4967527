"""Every kernel form of the three 16-bit conv launchers, elementwise against a float64 reference.

The forward (orn_launch_conv_bf16_fwd), the dgrad (orn_launch_conv_bf16_dgrad) and the wgrad (orn_launch_wgrad_bf16) each pick a
kernel form from the shape and the arguments they are given.  The cases below reach every form through the test entry points of
include/orn_debug.h (and orn_wgrad_nhwc_{bf16,f16}), in both builds, on the engine's own channels-last buffers, at every shape
the 720p and 1080p products run, on both sides of each selection threshold and at the tile edges.  Each case names the form its
launcher predicate selects.

Reference: float64 on the CPU (torch conv2d), from the identical 16-bit-rounded operands; it does not use liborn.  Per element,
never as a norm, with A the same linear operation on the absolute values of the operands (float64):
    16-bit outputs   |k - r| <= ulp16(r) + c * A        (z, apad, dyprev: the epilogue's cast is a round-to-nearest-even)
    fp32 outputs     |k - r| <= c * A                   (dx slabs, dwf, dbf)
c is per form and per build, at most 3x the worst ratio measured on an MI355X (C_TOL below holds both).  For a 16-bit output the
measured ratio is (|k - r| - ulp16(r) / 2)+ / A, the part of the error that the final rounding cannot explain.  Every measured
ratio is below 2^-16 (the largest, 2.1e-7, is the fp32 hand-off's sum of up to 9 partial slabs): no form loses more than a few
bits of its fp32 accumulator.  The module runs in about 40 s on one MI355X.

Contract checks on every case:
  - rings: the padding ring of every padded output (apad, dyprev) is pre-filled with a finite sentinel and still holds it after
    the call: no epilogue writes a ring (the next block's conv relies on the zeros the engine put there once);
  - exact sizes: every output has a sentinel-filled guard behind it that stays unchanged (dwf / dbf at C < 96 included);
  - slack: the readable slack orn.h allows behind wb / wd (96 * C elements) and dypad (128 elements) holds NaN, and every output
    is finite and correct; the wgrad's slab workspace starts as NaN too (every slab the reduction reads must be written);
  - fp16 overflow: a dgrad output beyond the half range comes out as +-inf (the engine's non-finite guard needs that), exactly
    where the reference exceeds it.
"""
import math
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

# the wgrad's operands, fp64 accumulation and per-element check are shared with test_gpu_wgrad16_batch.py
from wgrad16_ref import DT, FAST_C, check32, wgrad_channels, wgrad_ref
from wgrad16_ref import oprime as _oprime, padded as _padded, rand as _rand, scales as _scales

pytestmark = pytest.mark.gpu

TH, TW = 8, 32                 # pixel tile of the conv kernels (CB_TH x CB_TW, C2_TH x C2_TW)
SENT = 7.0                     # finite sentinel, exact in bf16 and fp16
GUARD = 1024                   # elements of sentinel behind every output

# c of the bound above, per form and build: at most 3x the worst ratio measured on an MI355X (the comment gives it).
C_TOL = {                      # worst measured (MI355X, this module): bf16 / fp16
    'fwd':          {'bf16': 3.4e-7, 'fp16': 3.2e-7},     # 1.17e-7 / 1.09e-7 (apad / z)
    'fwd2':         {'bf16': 2.6e-7, 'fp16': 3.4e-7},     # 8.71e-8 / 1.15e-7 (z)
    'dgrad2':       {'bf16': 1.2e-7, 'fp16': 1.0e-7},     # 4.26e-8 / 3.57e-8 (beside the SiLU' allowance of _run_dgrad)
    'dgrad_split':  {'bf16': 5.9e-8, 'fp16': 4.7e-8},     # 1.99e-8 / 1.57e-8
    'dgrad_f32':    {'bf16': 6.2e-7, 'fp16': 5.5e-7},     # 2.07e-7 / 1.85e-7
    'wgrad':        {'bf16': 3.1e-7, 'fp16': 4.1e-7},     # 1.06e-7 (dbf) / 1.39e-7 (dwf, 3 x 5 image at 8 slabs)
}
WORST = {}                     # form, half -> worst measured ratio of this run (printed per case)


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_conv_fwd_bf16', 'orn_debug_conv_fwd_f16', 'orn_debug_conv_dgrad_bf16', 'orn_debug_conv_dgrad_f16'):
        assert hasattr(lib, name), name
    torch.set_num_threads(16)
    return lib


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _err(L):
    import orn_amd
    return orn_amd._lib.last_error()


def _fn(L, kind, half):
    return getattr(L, f'orn_debug_conv_{kind}_{"bf16" if half == "bf16" else "f16"}')


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


def _guarded(n, dtype, fill=SENT):
    """Flat buffer of n elements + GUARD elements of sentinel behind; returns (whole buffer, view of the n elements)."""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device='cuda')
    return buf, buf[:n]


def _guard_ok(buf, n, what):
    g = buf[n:].float()
    assert bool((g == SENT).all()), f'{what}: {int((g != SENT).sum())} guard elements behind the output were written'


def _tile_rows(H, seed, th=TH):
    """Row ranges (of th rows) to compare: all of them on small images; else the first, the last (ragged) and a seeded sample
    of at least 5 % of the interior tile rows."""
    n = -(-H // th)
    if n <= 12:
        idx = list(range(n))
    else:
        g = torch.Generator().manual_seed(seed)
        inner = torch.randperm(n - 2, generator=g)[:max(1, math.ceil(0.05 * (n - 2)))] + 1
        idx = sorted({0, n - 1, *inner.tolist()})
    return [(i * th, min(H, (i + 1) * th)) for i in idx]


def _record(form, half, ratio, what):
    key = (form, half)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f'RATIO {form} {half} {what} {ratio:.3e}')


def _check16(k, r, A, half, form, what, gain=1.0, extra=0.0):
    """16-bit output k against the fp64 reference r: |k - r| <= ulp16(r) + c * gain * A (+ extra, see _run_dgrad)."""
    k = k.double()
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    u = _ulp16(r, half)
    ratio = float(((d - u / 2 - extra).clamp_min(0) / (gain * A).clamp_min(1e-300)).max())
    _record(form, half, ratio, what)
    bound = u + C_TOL[form][half] * gain * A + extra
    bad = d > bound
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at flat index {i} '
                             f'(shape {tuple(bad.shape)}): kernel {float(k.flatten()[i])!r} reference {float(r.flatten()[i])!r}')


def _check32(k, r, A, half, form, what):
    """fp32 output k against r: |k - r| <= c * A."""
    check32(k, r, A, C_TOL[form][half], what, record=lambda ratio: _record(form, half, ratio, what))


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _weights(O, c_real, s, half, gen):
    """PyTorch-layout wf [O][c_real][3][3] (16-bit-rounded, as k_prep_weights_bf16 casts it), bf [O], and the kernels' layouts
    made by a mirror of k_prep_weights_bf16: wb [9][O'][96], wd [9][96][O'] (taps flipped), bias' [O'], channels >= c_real zero
    (as in the engine's workspace).  wb and wd carry 96 * 96 elements of NaN slack behind them (orn.h)."""
    wf = (torch.randn(O, c_real, 3, 3, generator=gen, device='cuda') + 0.2) / math.sqrt(9 * c_real)
    wf = wf * _scales(O, gen, -1, 1)[:, None, None, None] * _scales(c_real, gen, -1, 1)[None, :, None, None]
    wf = wf.to(DT[half])
    bf = torch.randn(O, generator=gen, device='cuda') * 0.3
    op = _oprime(O, s)
    n = 9 * O * FAST_C
    slack = FAST_C * FAST_C
    wb_buf = torch.full((n + slack,), float('nan'), dtype=DT[half], device='cuda')
    wd_buf = torch.full((n + slack,), float('nan'), dtype=DT[half], device='cuda')
    wb = wb_buf[:n].view(9, O, FAST_C)
    wd = wd_buf[:n].view(9, FAST_C, O)
    wb.zero_()
    wd.zero_()
    wt = wf.reshape(O, c_real, 9).permute(2, 0, 1)            # [tap][o][c]
    wb[:, op, :c_real] = wt
    wd.view(9, FAST_C, O)[:, :c_real, :].index_copy_(2, op, wt.flip(0).permute(0, 2, 1).contiguous())
    bias_p = torch.empty(O, device='cuda')
    bias_p[op] = bf
    return wf, bf, wb_buf, wd_buf, bias_p


def _conv_ref(xs, w, b=None):
    """fp64 conv (padding 0) of a padded channels-last slab xs [h+2][W+2][c] with w [O][c][3][3]: value and A, both [O][h][W]."""
    x = xs.permute(2, 0, 1)[None]
    r = F.conv2d(x, w, b)[0]
    A = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs())[0]
    return r, A


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _run_fwd(L, half, H, W, O, s, c_real, apad, form, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    Cn, Hs, Ws = O // (s * s), H * s, W * s
    xbuf, xpad = _padded(H, W, FAST_C, c_real, half, gen)
    wf, bf, wb_buf, _, bias_p = _weights(O, c_real, s, half, gen)
    nz = Hs * Ws * Cn
    zbuf, z = _guarded(nz, DT[half])
    na = (Hs + 2) * (Ws + 2) * Cn
    abuf, a = _guarded(na, DT[half]) if apad else (None, None)
    rc = _fn(L, 'fwd', half)(_p(xpad), _p(wb_buf), _p(bias_p), H, W, FAST_C, O, s, _p(z), _p(a), c_real, _st())
    assert rc == 0, _err(L)
    torch.cuda.synchronize()
    _guard_ok(zbuf, nz, 'z')
    z = z.view(Hs, Ws, Cn)
    if apad:
        _guard_ok(abuf, na, 'apad')
        a = a.view(Hs + 2, Ws + 2, Cn)
        ring = torch.cat([a[0].flatten(), a[-1].flatten(), a[:, 0].flatten(), a[:, -1].flatten()]).float()
        assert bool((ring == SENT).all()), f'apad: {int((ring != SENT).sum())} ring elements written'
    w64, b64 = wf.double().cpu(), bf.double().cpu()
    for h0, h1 in _tile_rows(H, seed):
        xs = xpad[h0:h1 + 2, :, :c_real].double().cpu()
        r, A = _conv_ref(xs, w64, b64)                                   # [O][h][W], PyTorch channel order
        r = F.pixel_shuffle(r[None], s)[0].permute(1, 2, 0)               # [h*s][Ws][Cn]
        A = F.pixel_shuffle(A[None], s)[0].permute(1, 2, 0)
        where = f'{form} {half} H={H} W={W} O={O} s={s} c_real={c_real} rows {h0}..{h1}'
        _check16(z[h0 * s:h1 * s].cpu(), r, A, half, form, 'z ' + where)
        if apad:
            # apad = round16(silu(v32)) with v32 the fp32 value z was rounded from; |silu'| <= 1.1 carries the error of v32
            ra = _silu(r)
            _check16(a[1 + h0 * s:1 + h1 * s, 1:Ws + 1].cpu(), ra, A, half, form, 'apad ' + where, gain=1.1)


FWD_CASES = [
    # H, W, O, s, c_real, apad, form -- form selected by orn_launch_conv_bf16_fwd (orn_conv_fwd_bf16.hip) from ptiles = tiles of 8 x 32
    # product shapes (bench.layer_geo): 720p L1..L4, 1080p L1..L4
    (45, 80, 384, 2, 26, True, 'fwd'),        # 720p L1: apad && c_real <= 32 -> narrow k_conv_fwd_nhwc_bf16<..,32,true>
    (90, 160, 384, 2, 96, True, 'fwd'),       # 720p L2: 60 tiles < 400 with apad -> first form (N tiles split: cost model)
    (180, 320, 384, 2, 96, True, 'fwd'),      # 720p L3: 230 tiles < 400 -> first form, N tiles whole
    (360, 640, 384, 2, 96, False, 'fwd2'),    # 720p L4: z only, 900 tiles >= 128 -> k_conv2_nhwc<2>
    (45, 80, 864, 3, 48, True, 'fwd'),        # 1080p L1: c_real 48 > 32 -> first form, ragged last 128-channel N tile
    (135, 240, 384, 2, 96, True, 'fwd'),      # 1080p L2: 136 tiles < 400 -> first form
    (270, 480, 384, 2, 96, True, 'fwd2'),     # 1080p L3: 510 tiles >= 400 with apad -> k_conv2_nhwc<1>
    (540, 960, 384, 2, 96, False, 'fwd2'),    # 1080p L4: k_conv2_nhwc<2>
    # thresholds
    (1009, 31, 384, 2, 96, False, 'fwd'),     # 127 tiles (H % 8 = 1, W % 32 = 31), z only -> first form <..,3,96,false>
    (121, 225, 384, 2, 96, False, 'fwd2'),    # 128 tiles (H % 8 = 1, W % 32 = 1) -> k_conv2_nhwc<2>
    (151, 641, 384, 2, 96, True, 'fwd'),      # 399 tiles with apad -> first form
    (153, 639, 384, 2, 96, True, 'fwd2'),     # 400 tiles with apad -> k_conv2_nhwc<1>
    (13, 37, 384, 2, 32, True, 'fwd'),        # c_real 32 -> narrow form
    (13, 37, 384, 2, 33, True, 'fwd'),        # c_real 33 -> full-K first form
    (136, 320, 384, 2, 96, True, 'fwd'),      # 170 tiles: cost_whole 3 > cost_split 2.6 -> one N tile per work-group
    (152, 288, 384, 2, 96, True, 'fwd'),      # 171 tiles: cost_whole 3 <= cost_split 3.9 -> N tiles whole
    # tile edges, O and s
    (5, 7, 384, 2, 96, True, 'fwd'),          # image smaller than one tile
    (17, 33, 864, 3, 96, True, 'fwd'),        # H % 8 = 1, W % 32 = 1, ragged 128-channel N tile, s = 3
    (9, 33, 1152, 3, 96, False, 'fwd'),       # O = 1152 (Cn = 128), z only
    (63, 513, 1152, 3, 96, False, 'fwd2'),    # 136 tiles, O = 1152 -> k_conv2_nhwc<2>, 12 N tiles
    (23, 95, 96, 1, 96, True, 'fwd'),         # s = 1
    (127, 255, 864, 3, 96, True, 'fwd'),      # 128 tiles with apad (< 400) -> first form, ragged N tile, s = 3
    # O % 96 != 0 (in orn.h's contract, not the engine's): fwd2 declines, the first form runs; 600 tiles >= 512 keep the 3 N tiles
    # whole and cut the last partial round (600 - 512 tiles) into single N tiles (n_full)
    (237, 625, 320, 2, 96, True, 'fwd'),
    (237, 625, 320, 2, 96, False, 'fwd'),
]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('H,W,O,s,c_real,apad,form', FWD_CASES)
def test_conv16_fwd_form(L, half, H, W, O, s, c_real, apad, form):
    _run_fwd(L, half, H, W, O, s, c_real, apad, form, seed=H * 7919 + W * 31 + O + s + c_real + 2 * apad)


# ---- dgrad ------------------------------------------------------------------------------------------------------------------
def _run_dgrad(L, half, H, W, O, sp, mode, c_real, form, seed, boost=None):
    """mode 'fused': zprev + dyprev (k_conv2_nhwc<0> or, below 128 tiles, split + k_dgrad_finish with dx_f32 as scratch);
    'f32': dx_f32 output slabs (the fp32 hand-off of the first 16-bit layer)."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    C = FAST_C
    dbuf, dypad = _padded(H, W, O, O, half, gen, slack=128)
    if boost is not None:                                  # fp16 overflow case: a block of dy set to a large constant
        (r0, r1, c0, c1), v = boost
        dypad[1 + r0:1 + r1, 1 + c0:1 + c1] = v
    # (the dgrad sums over every o': s = 1 keeps o' = o, any other permutation would do)
    wf, _, _, wd_buf, _ = _weights(O, c_real, 1, half, gen)
    tiles = -(-W // TW) * -(-H // TH)
    Q = O // 96 if (tiles < 128 and O // 96 > 1) else 1                   # orn_dgrad_f32_slabs
    st = _st()
    fn = _fn(L, 'dgrad', half)
    if mode == 'fused':
        zprev = (torch.randn(H, W, C, generator=gen, device='cuda') * 2 + 0.3).to(DT[half])
        Hp, Wp, Cp = H // sp, W // sp, C * sp * sp
        npv = (Hp + 2) * (Wp + 2) * Cp
        pbuf, dyprev = _guarded(npv, DT[half])
        scratch = torch.full((Q * H * W * C,), float('nan'), device='cuda') if Q > 1 else None
        rc = fn(_p(dypad), _p(wd_buf), H, W, O, C, _p(zprev), _p(dyprev), sp, _p(scratch), c_real, st)
        assert rc == 0, _err(L)
        torch.cuda.synchronize()
        _guard_ok(pbuf, npv, 'dyprev')
        dyprev = dyprev.view(Hp + 2, Wp + 2, Cp)
        ring = torch.cat([dyprev[0].flatten(), dyprev[-1].flatten(), dyprev[:, 0].flatten(), dyprev[:, -1].flatten()]).float()
        assert bool((ring == SENT).all()), f'dyprev: {int((ring != SENT).sum())} ring elements written'
        # un-shuffle view: [Hp][sp][Wp][sp][C] of the interior, channel (i*sp + j)*96 + c <- pixel (ph*sp + i, pw*sp + j)
        inner = dyprev[1:Hp + 1, 1:Wp + 1].view(Hp, Wp, sp, sp, C).permute(0, 2, 1, 3, 4).reshape(H, W, C)
    else:
        ns = Q * H * W * C
        xbuf, dx = _guarded(ns, torch.float32)
        rc = fn(_p(dypad), _p(wd_buf), H, W, O, C, None, None, 1, _p(dx), c_real, st)
        assert rc == 0, _err(L)
        torch.cuda.synchronize()
        _guard_ok(xbuf, ns, 'dx_f32')
        dx = dx.view(Q, H, W, C)
        narrow = Q > 1 and c_real <= 32
        if narrow:                              # the all-taps N = 32 form writes channels [0, 32) of each slab only
            assert bool((dx[..., 32:] == SENT).all()), 'dx_f32: the narrow form wrote channels >= 32'
            assert bool((dx[..., c_real:32] == 0).all()), 'dx_f32: channels c_real..31 (zero weights) not zero'
        else:
            assert bool((dx[..., c_real:] == 0).all()), 'dx_f32: channels >= c_real (zero weights) not zero'
    # reference: dx = conv2d(dy, flipped transposed weights) on the padded dy slab (o in PyTorch order)
    op = _oprime(O, 1).cpu()
    wflip = wf.double().cpu().flip(2, 3).transpose(0, 1).contiguous()   # [c][o][3][3]
    got = []
    for h0, h1 in _tile_rows(H, seed):
        ds = dypad[h0:h1 + 2].double().cpu()[:, :, op]                    # o' -> o (s = 1 here: identity)
        r, A = _conv_ref(ds, wflip)                                       # [c][h][W]
        r, A = r.permute(1, 2, 0), A.permute(1, 2, 0)                     # [h][W][c]
        where = f'{form} {half} H={H} W={W} O={O} sp={sp} c_real={c_real} rows {h0}..{h1}'
        if mode == 'fused':
            zp = zprev[h0:h1].double().cpu()
            sg = _silu_grad(zp)
            # the epilogue evaluates SiLU'(z) = s (1 + z (1 - s)) in fp32 with the fast exp and reciprocal: an error of a few
            # 2^-24 times (1 + |z|) that does not scale with SiLU' itself (1 + z (1 - s) cancels near its root z = -1.28), so it
            # is allowed apart, times |dx|, instead of inflating c
            rr, AA, k = r * sg, A * sg.abs(), inner[h0:h1].cpu().double()
            extra = 2.0 ** -20 * (1 + zp.abs()) * r.abs()
            if boost is not None:
                got.append((k, rr, AA, extra))
                continue
            _check16(k, rr, AA, half, form, 'dyprev ' + where, extra=extra)
        else:
            k = dx[:, h0:h1, :, :c_real].double().cpu().sum(0)
            _check32(k, r[..., :c_real], A[..., :c_real], half, form, 'dx_f32 ' + where)
    if boost is not None:
        return tuple(torch.cat([g[i] for g in got]) for i in range(4)) + (f'{form} fp16 H={H} W={W} O={O} sp={sp}',)


DGRAD_CASES = [
    # H, W, O, sp, mode, c_real, form -- form selected by orn_launch_conv_bf16_dgrad (orn_conv_bf16.hip)
    # product shapes: the dgrad of 720p L2..L4 and 1080p L2..L4 into the block below (sp = that block's stride), the fp32 hand-off
    # of L1 (layer ff)
    (90, 160, 384, 2, 'fused', 96, 'dgrad_split'),    # 720p L2: 60 tiles < 128 -> k_conv_nhwc_bf16<8,1,1,3,2,96,false> + k_dgrad_finish
    (180, 320, 384, 2, 'fused', 96, 'dgrad2'),        # 720p L3: k_conv2_nhwc<0>
    (360, 640, 384, 2, 'fused', 96, 'dgrad2'),        # 720p L4
    (135, 240, 384, 3, 'fused', 96, 'dgrad2'),        # 1080p L2: 136 tiles, sp = 3 (H % 8 = 7)
    (270, 480, 384, 2, 'fused', 96, 'dgrad2'),        # 1080p L3
    (540, 960, 384, 2, 'fused', 96, 'dgrad2'),        # 1080p L4
    (45, 80, 384, 1, 'f32', 26, 'dgrad_f32'),         # 720p L1: qsplit (18 tiles, 4 chunks), c_real 26 -> narrow <8,1,1,1,2,96,true>
    (45, 80, 864, 1, 'f32', 48, 'dgrad_f32'),         # 1080p L1: qsplit, 9 chunks, c_real 48 -> EPI_B_DGRAD_F32 <8,1,1,3,..>
    # thresholds
    (1010, 30, 384, 2, 'fused', 96, 'dgrad_split'),   # 127 tiles -> split + finish
    (122, 226, 384, 2, 'fused', 96, 'dgrad2'),        # 128 tiles -> k_conv2_nhwc<0>
    (1009, 31, 384, 1, 'f32', 96, 'dgrad_f32'),       # 127 tiles -> qsplit: 4 slabs
    (121, 225, 384, 1, 'f32', 96, 'dgrad_f32'),       # 128 tiles -> one slab
    (13, 37, 384, 1, 'f32', 32, 'dgrad_f32'),         # c_real 32 -> narrow
    (13, 37, 384, 1, 'f32', 33, 'dgrad_f32'),         # c_real 33 -> full
    (13, 37, 96, 1, 'f32', 26, 'dgrad_f32'),          # O = 96: one chunk, no qsplit -> full form even at c_real 26
    # tile edges, O and sp
    (6, 6, 864, 3, 'fused', 96, 'dgrad_split'),       # image smaller than one tile, 9 chunks, sp = 3
    (9, 33, 1152, 3, 'fused', 96, 'dgrad_split'),     # H % 8 = 1, W % 32 = 1, 12 chunks
    (16, 62, 384, 1, 'fused', 96, 'dgrad_split'),     # sp = 1
    (129, 255, 864, 3, 'fused', 96, 'dgrad2'),        # 136 tiles, H % 8 = 1, W % 32 = 31, sp = 3, O = 864
    (128, 256, 1152, 1, 'fused', 96, 'dgrad2'),       # sp = 1, O = 1152
]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('H,W,O,sp,mode,c_real,form', DGRAD_CASES)
def test_conv16_dgrad_form(L, half, H, W, O, sp, mode, c_real, form):
    _run_dgrad(L, half, H, W, O, sp, mode, c_real, form, seed=H * 7919 + W * 31 + O + sp + c_real)


@pytest.mark.parametrize('H,W,form', [(64, 512, 'dgrad2'), (16, 64, 'dgrad_split')])
def test_conv16_dgrad_fp16_overflow_is_inf(L, H, W, form):
    """A block of dy set to 2^14 drives part of dx * SiLU'(z) beyond the half range: exactly the elements whose reference
    exceeds it by a margin come out as +-inf (the cast rounds to nearest, so 65520 and above overflow), every element below it
    by the margin is finite and within the bound; the few elements inside the margin are not asserted."""
    k, r, A, extra, where = _run_dgrad(L, 'fp16', H, W, 384, 2, 'fused', 96, form, seed=H + W, boost=((4, 10, 8, 40), 16384.0))
    over, under = r.abs() > 65520 * (1 + 1e-3), r.abs() < 65520 * (1 - 1e-3)
    assert int(over.sum()) >= 100, int(over.sum())
    assert bool((torch.isinf(k[over]) & (torch.sign(k[over]) == torch.sign(r[over]))).all()), \
        f'{where}: {int((~torch.isinf(k[over])).sum())} of {int(over.sum())} overflowing elements are not +-inf'
    assert bool(torch.isfinite(k[under]).all()), f'{where}: {int((~torch.isfinite(k[under])).sum())} spurious non-finite'
    assert int((~over & ~under).sum()) < int(over.sum())
    assert float(r[under].abs().max()) > 1e4
    _check16(k[under], r[under], A[under], 'fp16', form, 'dyprev (overflow case) ' + where, extra=extra[under])


# ---- wgrad ------------------------------------------------------------------------------------------------------------------
def _wgrad_split(H, W, O):
    """Mirror of orn_wgrad_bf16_split (no caller cap): the slab count the hook runs with."""
    n_ktiles = -(-H // 2) * -(-W // 32)
    S = min(40, (512 // (3 * -(-O // 128))) // 8 * 8)
    if n_ktiles < 2000 and S > 24:
        S = 24
    S = min(S, (n_ktiles // 8) // 8 * 8)
    return max(S, 8)


def _run_wgrad(L, half, H, W, C, O, s, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    xbuf, xpad = _padded(H, W, FAST_C, C, half, gen)
    dbuf, dypad = _padded(H, W, O, O, half, gen, slack=128)
    nbytes = L.orn_wgrad_nhwc_bf16_ws_bytes(H, W, O)
    slabs = torch.full((nbytes // 4,), float('nan'), device='cuda')
    nw = O * C * 9
    wbuf, dwf = _guarded(nw, torch.float32)
    bbuf, dbf = _guarded(O, torch.float32)
    fn = L.orn_wgrad_nhwc_bf16 if half == 'bf16' else L.orn_wgrad_nhwc_f16
    rc = fn(_p(xpad), _p(dypad), H, W, C, O, s, _p(slabs), _p(dwf), _p(dbf), _st())
    assert rc == 0, _err(L)
    torch.cuda.synchronize()
    _guard_ok(wbuf, nw, 'dwf')
    _guard_ok(bbuf, O, 'dbf')
    dwf = dwf.view(O, C, 3, 3)
    # output channels compared: all of them below ~50 M pixel-channel products, else the first 16 and last 16 o' (the ragged
    # last 128-channel tile) and a seeded sample of 32 more (all C and taps of each)
    sel = wgrad_channels(H, W, O, s, seed)
    r, A, rb, Ab = wgrad_ref(xpad, dypad, H, W, C, O, s, sel)
    where = f'wgrad {half} H={H} W={W} C={C} O={O} s={s} S={_wgrad_split(H, W, O)}'
    _check32(dwf.reshape(O, C, 9)[sel].cpu(), r, A, half, 'wgrad', 'dwf ' + where)
    # dbf[o] = sum of dy over pixels, channel o' of o
    _check32(dbf.cpu(), rb, Ab, half, 'wgrad', 'dbf ' + where)


WGRAD_CASES = [
    # H, W, C, O, s -- slab count S from orn_wgrad_bf16_split: min(40, (512 / (3 * ceil(O/128))) / 8 * 8), 24 below 2000 K tiles
    # of 2 x 32 pixels, at most (K tiles / 8) / 8 * 8, at least 8
    (45, 80, 26, 384, 2),       # 720p L1 (C = 26): 69 K tiles -> by_work 8
    (90, 160, 96, 384, 2),      # 720p L2: 225 K tiles -> 24
    (180, 320, 96, 384, 2),     # 720p L3: 900 -> 24
    (360, 640, 96, 384, 2),     # 720p L4: 3600 -> 40
    (45, 80, 48, 864, 3),       # 1080p L1 (C = 48): ragged 128-channel O tile, by_work 8
    (135, 240, 96, 384, 2),     # 1080p L2: 544 -> 24
    (270, 480, 96, 384, 2),     # 1080p L3: 2025 -> 40
    (540, 960, 96, 384, 2),     # 1080p L4: 8100 -> 40
    (3, 5, 96, 384, 2),         # 2 K tiles: the 8-slab floor (slabs without a K tile), odd H, image below one tile
    (26, 320, 96, 384, 2),      # 130 K tiles: by_work cap 16
    (3997, 31, 96, 384, 2),     # 1999 K tiles -> 24 slabs (odd H, W % 32 = 31)
    (4000, 32, 96, 384, 2),     # 2000 K tiles -> 40 slabs
    (9, 33, 96, 1152, 3),       # O = 1152: 9 O tiles -> 16 slabs cap, by_work 8
    (17, 63, 26, 864, 3),       # C = 26 with a ragged O tile, H % 8 = 1
    (7, 97, 48, 96, 1),         # s = 1, O = 96 (one ragged O tile), W % 32 = 1
]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('H,W,C,O,s', WGRAD_CASES)
def test_conv16_wgrad_form(L, half, H, W, C, O, s):
    _run_wgrad(L, half, H, W, C, O, s, seed=H * 7919 + W * 31 + O + s + C)


# ---- rejections -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('half', ['bf16', 'fp16'])
def test_conv16_launchers_reject_out_of_contract_arguments(L, half):
    """Each launcher returns ORN_E_ARG and names itself for arguments outside its contract, and launches nothing: the buffers
    (big enough for every shape tried) keep their sentinel."""
    big = torch.full((1 << 24,), SENT, dtype=DT[half], device='cuda')
    outz = torch.full((1 << 22,), SENT, dtype=DT[half], device='cuda')
    outf = torch.full((1 << 24,), SENT, device='cuda')
    bias = torch.zeros(2048, device='cuda')
    st = _st()
    fwd, dgr = _fn(L, 'fwd', half), _fn(L, 'dgrad', half)
    wg = L.orn_wgrad_nhwc_bf16 if half == 'bf16' else L.orn_wgrad_nhwc_f16
    for Cin, O, s, c_real in [(48, 384, 2, 48), (192 + 1, 384, 2, 96), (96, 100, 2, 96), (96, 160, 4, 96), (96, 384, 0, 96)]:
        assert fwd(_p(big), _p(big), _p(bias), 8, 8, Cin, O, s, _p(outz), _p(outz), c_real, st) == -1, (Cin, O, s)
        assert 'conv_bf16_fwd' in _err(L), _err(L)
    for H, W, O, C, sp, fused, dx in [(8, 8, 384, 48, 2, True, False), (8, 8, 200, 96, 2, True, False),
                                      (8, 8, 320, 96, 2, False, True), (9, 8, 384, 96, 2, True, False),
                                      (8, 9, 384, 96, 2, True, False), (9, 8, 384, 96, 2, True, True),
                                      (64, 512, 384, 96, 2, True, True)]:   # split epilogue at >= 128 tiles
        rc = dgr(_p(big), _p(big), H, W, O, C, _p(big) if fused else None, _p(outz) if fused else None, sp,
                 _p(outf) if dx else None, 96, st)
        assert rc == -1, (H, W, O, C, sp, fused, dx)
        assert 'conv_bf16_dgrad' in _err(L), _err(L)
    for C, O, s in [(97, 384, 2), (0, 384, 2), (96, 100, 2), (96, 384, 3)]:
        assert wg(_p(big), _p(big), 8, 8, C, O, s, _p(outf), _p(outf), _p(outf), st) == -1, (C, O, s)
        assert 'wgrad_bf16' in _err(L), _err(L)
    torch.cuda.synchronize()
    assert bool((outz.float() == SENT).all()) and bool((outf == SENT).all())
