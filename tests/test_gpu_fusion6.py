"""k_fusion6 (every form the launcher picks: <GRAD, TC_NONE / TC_READ / TC_FILL, L2T>), k_loss_grad and the finalize stage
(csrc/orn_loss.hip on the tile machine of csrc/orn_ssim_tile.h) elementwise against a float64 reference, through
orn_debug_loss_launch -- orn_launch_loss itself, with the frame table, the device frame index and the cached target maps the engine
gives it -- orn_debug_loss_layout and orn_loss_target_stats.

Shapes (H x W, msssim_levels_ref.BWD_SHAPES), the smallest reaching each edge of the 16x64 tiling with its 10 + 10 pixel apron:
  11x11 one valid pixel, scalar loads; 11x12 float4 loads with x0 - 12 < 0; 16x64 exactly one image tile; 17x65 2x2 tiles, three
  of which own no map pixel yet receive a full gradient from their apron; 26x74 the valid map exactly one tile; 26x75 and 27x75
  mixed parities; 30x78 even width on the scalar path; 32x128 float4, exactly 2x2 tiles; 43x139 and 42x140 3x3 tiles with an interior
  tile, scalar and float4
Planes (B, Ch): (1, 1), (1, 3), (2, 3), (1, 64).  Inputs: the suite's pair (every plane its own noise), the nearly flat pair, and the
tied pair (p = t on a checkerboard of one plane: sign(d) = 0 there).

Cases:
  structural term  loss SSIM (w_l1 = w_l2 = 0: no pixel term sets the error floor): dpred, part_ssim, part_l1 by the rule; without
                   dpred (GRAD = false) the same partials and stats, bit for bit
  pixel terms      Fusion6 (L1 sign) and Fusion1 (L2T): dpred by the rule.  On the tied pixels the L1 term is exactly 0 whatever its
                   scale: Fusion6's dpred there equals Fusion5's bit for bit (the same w_struct = 0.3, hence the same g_ssim, and a
                   pixel term of g_l1 * 0 against g_l2 * 0) -- the exact form chosen; the rule's reference (sign(0) = 0) holds too
  TC_FILL          orn_loss_target_stats on a 3-frame, 3-channel table, every element of [n][2][Ch][Hv][Wv] written, by the rule
  TC_READ          that table at frame_idx = 2, then 0 (B = 1, Ch = 3, the engine's form), the other frames' maps NaN: dpred, both
                   partials and stats bit-equal to TC_NONE on that frame, and by the rule; Fusion6 and Fusion1; without dpred too
  addressing       W % 4 == 0: frame_stride = 3HW (float4), 3HW + 4 (float4, padded), 3HW + 1 (scalar); at 32x128 and 16x64 also pred
                   offset by one float (scalar): each bit-equal to the aligned result
  loss_scale 256   dpred and stats[0] exactly 256 times the scale-1 results, stats[1..4] unchanged
  finalize         stats[0..4] by the documented formula in double from the kernel's OWN partials, 2^-23 relative (PSNR 1e-5):
                   Fusion6's hard-coded branch, the generic one (Fusion1, Fusion9, SSIM), L2, L1, Fusion7 / 8.  On the suite's and the
                   tied pair: the bound is relative to the loss, which the kernel forms in fp32 from the fp32 s -- for the flat pair
                   (1 - s ~ 1e-3, L1 ~ 1e-3) the rounding of s alone is 2^-25 / 1e-3 of the loss
  k_loss_grad      L2, L1, Fusion7, Fusion8 with and without dpred at 11x11, 17x65, 30x78, 32x128: dpred within 2^-23 relative per
                   element of g_l2 d + g_l1 sign(d) in double with the launcher's fp32 scales; part_l1 by the rule; stats as above;
                   the tied pixels of L1 exactly 0

Reference and tolerance rule: tests/fusion6_ref.py (float64 with the fp32 taps; E = max(max|r32 - r64|, 2^-24 max|r64|),
max|k - r64| <= c E).  tests/test_fusion6_host.py shows that this comparator rejects eight kinds of mutant with the c below.

Worst ratio max|k - r64| / E measured on an MI355X per kind, and the c it fixes (the smallest power of two >= twice the ratio):
    kind            worst ratio   c    where
    tmaps           2.502         8    11x11, frame 1 of the table, G*t         the TC_FILL output
    ssim part       3.452         8    17x65, 1x3 planes, the suite's pair      the SSIM tile partials
    dpred struct    1.601         4    11x11, 1x3 planes, the tied pair         dpred of the structural term alone
    dpred pixel     1.896         4    27x75, Fusion1, frame 2 of the table     dpred with a pixel term (TC_NONE and TC_READ)
    pix part        1.734         4    43x139, 1x3 planes, the suite's pair     the {|d|, d^2} tile partials of both kernels
None is above 4; the flat pair passes under the same c (its E is measured on its own inputs): at worst 3.189 (ssim part, 11x12, one
plane), 1.538 (dpred pixel), 1.536 (dpred struct), 1.000 (pix part).  The finalize stage reaches 0.993 of
its 2^-23 (Fusion9, the tied pair, 1x3x11x11), dpred of k_loss_grad 0.500 of its 2^-23.
The module's 186 tests run in 3.0 s on one MI355X, none above 0.2 s.

Every output buffer starts as NaN between two sentinel bands that must stay untouched; every case runs twice and must give the
same bits."""
from ctypes import c_float, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import fusion6_ref as Q
import msssim_levels_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = 7.0
GUARD = 1024                   # floats: keeps the payload 16-byte aligned
NAN = float('nan')
F64, F32 = Q.F64, Q.F32
ids = dict(ids=lambda s: 'x'.join(map(str, s)))


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_loss_launch', 'orn_debug_loss_layout', 'orn_loss_target_stats'):
        assert hasattr(lib, name), name
    torch.set_num_threads(16)
    return lib


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _err():
    import orn_amd
    return orn_amd._lib.last_error()


def guarded(n):
    """(buffer, payload): n NaN floats between two sentinel bands"""
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV)
    buf[GUARD:GUARD + n] = NAN
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def judge(kind, name, k, r64, r32):
    r = R.ratio(k, r64, r32)
    print(f'{kind:12s} {name}: ratio {r:.3f} (c = {Q.C[kind]:g})')
    assert r <= Q.C[kind], (kind, name, r)


_ARENAS = {}


def arena(sizes):
    """A fresh device buffer  band | payload 0 | band | payload 1 | band ...  (NaN payloads padded to whole float4s between sentinel
    bands), the payloads' offsets and the pristine host copy to compare the bands with"""
    if sizes not in _ARENAS:
        parts, offs = [torch.full((GUARD,), SENT)], []
        for n in sizes:
            offs.append(sum(x.numel() for x in parts))
            parts += [torch.full((-(-n // 4) * 4,), NAN), torch.full((GUARD,), SENT)]
        host = torch.cat(parts)
        _ARENAS[sizes] = (host.to(DEV), offs, host)
    dev, offs, host = _ARENAS[sizes]
    return dev.clone(), offs, host


class Out:
    """what one launch left (host copies): dpred [P][H][W] (NaN without the gradient), part_ssim [P][tiles], part_l1 [P][tiles][2],
    stats [8]"""

    def same(self, o, grad=True):
        return ((not grad or same_bits(self.dpred, o.dpred)) and same_bits(self.part_ssim, o.part_ssim) and same_bits(self.part_l1, o.part_l1)
                and same_bits(self.stats, o.stats))


def layout(L, B, Ch, H, W):
    lay = (c_int64 * 4)()
    assert L.orn_debug_loss_layout(B, Ch, H, W, lay) == 0, _err()
    tw, th, off_pl, total = lay
    assert (tw, th) == (-(-W // R.TW), -(-H // R.TH))
    return tw * th, off_pl, total


def launch(L, loss, pred, frames, B, Ch, H, W, fidx=None, stride=0, tstats=None, scale=1.0, grad=True):
    """One orn_debug_loss_launch on device tensors.  Checked here for every call: the sentinel bands, that every output element is
    written and finite, and that nothing else is."""
    lid, _, _, w_struct = Q.LOSSES[loss]
    P = B * Ch
    tiles, off_pl, total = layout(L, B, Ch, H, W)
    ws_bytes = L.orn_loss_ws_bytes_for(lid, B, Ch, H, W)
    assert ws_bytes == total * 4 and off_pl >= P * tiles and total >= off_pl + 2 * P * tiles
    buf, (o_ws, o_d, o_s), pristine = arena((total, P * H * W, 8))
    base = buf.data_ptr()
    rc = L.orn_debug_loss_launch(_p(pred), _p(frames), _p(fidx), c_size_t(stride), B, Ch, H, W, lid, c_float(scale), _p(tstats),
                                 c_void_p(base + 4 * o_s), c_void_p(base + 4 * o_d) if grad else None, c_void_p(base + 4 * o_ws), ws_bytes, _st())
    host = buf.cpu()                                               # (synchronises)
    assert rc == 0, _err()
    o = Out()
    ws = host[o_ws:o_ws + total]
    o.dpred, o.stats = host[o_d:o_d + P * H * W].view(P, H, W), host[o_s:o_s + 8]
    o.part_ssim, o.part_l1 = ws[:P * tiles].view(P, tiles), ws[off_pl:off_pl + 2 * P * tiles].view(P, tiles, 2)
    assert bool(torch.isfinite(o.part_l1).all()) and bool(torch.isfinite(o.stats).all()), (loss, H, W)
    assert bool(torch.isfinite(o.dpred).all()) if grad else bool(torch.isnan(o.dpred).all())
    # the structural kinds write every SSIM partial, the others none; nothing else changed: the rest of the workspace, the padding and
    # the sentinel bands hold the bits they started with
    assert bool(torch.isfinite(o.part_ssim).all()) if w_struct else bool(torch.isnan(o.part_ssim).all())
    left = host.clone()
    for t in (o.dpred, o.stats, o.part_ssim, o.part_l1):
        t.fill_(NAN)
    assert same_bits(host, pristine), (loss, H, W)
    host.copy_(left)
    return o


def twice(L, *a, **k):
    o, o2 = launch(L, *a, **k), launch(L, *a, **k)
    assert o.same(o2, k.get('grad', True))
    return o


def check_stats(o, loss, P, H, W, scale=1.0, name=''):
    """stats[0..4] against the documented formula in double from the kernel's own partials"""
    w_struct = Q.LOSSES[loss][3]
    want = Q.stats_from_partials(o.part_ssim if w_struct else None, o.part_l1, loss, P, H, W, scale)
    got = o.stats.double().cpu().numpy()
    rel = np.abs(got[:4] - want[:4]) / np.maximum(np.abs(want[:4]), 1e-300)
    print(f'stats {loss} {name}: relative error {rel.max() / 2.0 ** -23:.3f} x 2^-23, psnr {abs(got[4] - want[4]) / abs(want[4]):.2e}')
    assert (np.abs(got[:4] - want[:4]) <= 2.0 ** -23 * np.abs(want[:4])).all(), (loss, name, got, want)
    assert abs(got[4] - want[4]) <= 1e-5 * abs(want[4]), (loss, name, got, want)
    assert (got[5:] == 0).all()


_DEVICE = {}


def on_device(kind, P, H, W):
    key = (kind, P, H, W)
    if key not in _DEVICE:
        cs = Q.case(kind, P, H, W)
        _DEVICE[key] = (cs, cs['p'].to(DEV), cs['t'].to(DEV))
    return _DEVICE[key]


# ---- the structural term alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', Q.PLANES, **ids)
@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_structural_term(L, shape, planes):
    (H, W), (B, Ch) = shape, planes
    P = B * Ch
    for kind in Q.KINDS:
        cs, p, t = on_device(kind, P, H, W)
        name = f'{kind} {B}x{Ch}x{H}x{W}'
        o = twice(L, 'SSIM', p, t, B, Ch, H, W)
        r64, r32 = cs['ref'][F64], cs['ref'][F32]
        judge('dpred struct', name, o.dpred, Q.dpred_ref(cs, 'SSIM', F64), Q.dpred_ref(cs, 'SSIM', F32))
        judge('ssim part', name, o.part_ssim, r64['part_ssim'], r32['part_ssim'])
        judge('pix part', name, o.part_l1, r64['part_l1'], r32['part_l1'])
        assert o.same(launch(L, 'SSIM', p, t, B, Ch, H, W, grad=False), grad=False)


# ---- the pixel-term forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', Q.PLANES, **ids)
@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_pixel_term_forms(L, shape, planes):
    (H, W), (B, Ch) = shape, planes
    P = B * Ch
    for kind in Q.KINDS:
        cs, p, t = on_device(kind, P, H, W)
        out = {}
        for loss in ('Fusion6', 'Fusion1'):
            out[loss] = o = twice(L, loss, p, t, B, Ch, H, W)
            judge('dpred pixel', f'{loss} {kind} {B}x{Ch}x{H}x{W}', o.dpred, Q.dpred_ref(cs, loss, F64), Q.dpred_ref(cs, loss, F32))
            judge('ssim part', f'{loss} {kind} {B}x{Ch}x{H}x{W}', o.part_ssim, cs['ref'][F64]['part_ssim'], cs['ref'][F32]['part_ssim'])
        assert same_bits(out['Fusion6'].part_ssim, out['Fusion1'].part_ssim) and same_bits(out['Fusion6'].part_l1, out['Fusion1'].part_l1)
        if kind == 'tied':
            m = Q.tied_mask(P, H, W)
            f5 = launch(L, 'Fusion5', p, t, B, Ch, H, W)
            assert same_bits(out['Fusion6'].dpred[m], f5.dpred[m])
            assert not same_bits(out['Fusion6'].dpred[~m], f5.dpred[~m])


# ---- the cached target maps --------------------------------------------------------------------------------------------------
_TABLE = {}


def table_run(L, H, W):
    """orn_loss_target_stats on the 3-frame table, twice, checked for coverage; the device copies of the case"""
    if (H, W) not in _TABLE:
        tc = Q.table_case(H, W)
        frames, pred = tc['frames'].to(DEV), tc['pred'].to(DEV)
        n = 3 * 2 * 3 * (H - 10) * (W - 10)
        assert L.orn_loss_target_stats_bytes(3, 3, H, W) == 4 * n
        runs = []
        for _ in range(2):
            bt, ts = guarded(n)
            rc = L.orn_loss_target_stats(_p(frames), 3, 3, H, W, _p(ts), _st())
            torch.cuda.synchronize()
            assert rc == 0, _err()
            assert guards_intact(bt) and bool(torch.isfinite(ts).all())
            runs.append(ts)
        assert same_bits(*runs)
        _TABLE[H, W] = (tc, frames, pred, runs[0].view(3, 2, 3, H - 10, W - 10))
    return _TABLE[H, W]


@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_target_stats_fill(L, shape):
    H, W = shape
    tc, _, _, ts = table_run(L, H, W)
    judge('tmaps', f'{H}x{W}', ts, tc['tstats'][F64], tc['tstats'][F32])
    for k in range(3):                                             # per frame and map too: a slip must not hide behind the largest map
        for m in range(2):
            judge('tmaps', f'{H}x{W} frame {k} map {m}', ts[k, m], tc['tstats'][F64][k, m], tc['tstats'][F32][k, m])


@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_target_stats_read(L, shape):
    H, W = shape
    tc, frames, pred, ts = table_run(L, H, W)
    for k in (2, 0):
        cs = tc['frame'][k]
        fidx = torch.tensor([k], dtype=torch.int32, device=DEV)
        only = torch.full_like(ts, NAN)                            # the other frames' maps are NaN: a frame slip cannot stay finite
        only[k] = ts[k]
        for loss in ('Fusion6', 'Fusion1'):
            name = f'{loss} {H}x{W} frame {k}'
            o = twice(L, loss, pred[k], frames, 1, 3, H, W, fidx=fidx, stride=3 * H * W, tstats=only)
            none = launch(L, loss, pred[k], frames, 1, 3, H, W, fidx=fidx, stride=3 * H * W)
            assert o.same(none), name
            assert none.same(launch(L, loss, pred[k], frames[k], 1, 3, H, W)), name
            judge('dpred pixel', name, o.dpred, Q.dpred_ref(cs, loss, F64), Q.dpred_ref(cs, loss, F32))
            judge('ssim part', name, o.part_ssim, cs['ref'][F64]['part_ssim'], cs['ref'][F32]['part_ssim'])
            judge('pix part', name, o.part_l1, cs['ref'][F64]['part_l1'], cs['ref'][F32]['part_l1'])
            check_stats(o, loss, 3, H, W, name=name)
            for ts_k in (only, None):                              # GRAD = false, TC_READ and TC_NONE: the same partials and stats
                assert o.same(launch(L, loss, pred[k], frames, 1, 3, H, W, fidx=fidx, stride=3 * H * W, tstats=ts_k, grad=False), grad=False), name


# ---- frame addressing and the load path --------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [s for s in Q.SHAPES if s[1] % 4 == 0], **ids)
def test_frame_addressing(L, shape):
    H, W = shape
    tc, frames, pred, ts = table_run(L, H, W)
    n = 3 * H * W
    cs = tc['frame'][2]
    fidx = torch.tensor([2], dtype=torch.int32, device=DEV)
    variants = [(n, 0), (n + 4, 0), (n + 1, 0)] + ([(n, 1), (n + 4, 1)] if shape in ((32, 128), (16, 64)) else [])
    for loss, tstats in (('Fusion6', None), ('Fusion6', ts), ('Fusion1', ts), ('L1', None), ('Fusion7', None)):
        base = launch(L, loss, pred[2], frames[2], 1, 3, H, W)                  # aligned, no table: float4 where the kernel has it
        for stride, shift in variants:
            tab = torch.full((3 * stride + 4,), NAN, device=DEV)                # the slack between the frames stays NaN
            for k in range(3):
                tab[k * stride:k * stride + n] = frames[k].flatten()
            pbuf = torch.full((n + 4,), NAN, device=DEV)
            pbuf[shift:shift + n] = pred[2].flatten()
            assert tab.data_ptr() % 16 == 0 and pbuf.data_ptr() % 16 == 0
            o = launch(L, loss, pbuf[shift:shift + n], tab, 1, 3, H, W, fidx=fidx, stride=stride, tstats=tstats)
            assert o.same(base), (loss, stride, shift)
        if Q.LOSSES[loss][3]:
            judge('dpred pixel', f'{loss} {H}x{W} aligned', base.dpred, Q.dpred_ref(cs, loss, F64), Q.dpred_ref(cs, loss, F32))


# ---- loss_scale --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_loss_scale_is_a_plain_factor(L, shape):
    H, W = shape
    cs, p, t = on_device('pair', 3, H, W)
    for loss in ('Fusion6', 'Fusion1', 'Fusion7'):
        one, big = launch(L, loss, p, t, 1, 3, H, W), launch(L, loss, p, t, 1, 3, H, W, scale=256.0)
        assert torch.equal(big.dpred, 256.0 * one.dpred) and float(big.stats[0]) == 256.0 * float(one.stats[0]), loss
        assert same_bits(big.stats[1:], one.stats[1:]) and same_bits(big.part_l1, one.part_l1), loss


# ---- the finalize stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', Q.PLANES, **ids)
@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_finalize_from_the_kernels_own_partials(L, shape, planes):
    (H, W), (B, Ch) = shape, planes
    P = B * Ch
    for kind in ('pair', 'tied'):
        cs, p, t = on_device(kind, P, H, W)
        for loss, scale in (('Fusion6', 1.0), ('Fusion1', 1.0), ('Fusion9', 1.0), ('SSIM', 1.0), ('Fusion6', 256.0)):
            check_stats(launch(L, loss, p, t, B, Ch, H, W, scale=scale), loss, P, H, W, scale, f'{kind} {B}x{Ch}x{H}x{W}')


# ---- k_loss_grad -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', Q.PLANES, **ids)
@pytest.mark.parametrize('shape', Q.GRAD_SHAPES, **ids)
def test_loss_grad(L, shape, planes):
    (H, W), (B, Ch) = shape, planes
    P = B * Ch
    for kind in Q.KINDS:
        cs, p, t = on_device(kind, P, H, W)
        for loss, scale in (('L2', 1.0), ('L1', 1.0), ('Fusion7', 1.0), ('Fusion8', 1.0), ('Fusion7', 256.0)):
            name = f'{loss} {kind} {B}x{Ch}x{H}x{W}'
            o = twice(L, loss, p, t, B, Ch, H, W, scale=scale)
            want = Q.loss_grad_ref(cs['p'], cs['t'], loss, scale)
            err = (o.dpred.double().cpu() - want).abs()
            print(f'{name}: worst relative error {float((err / want.abs().clamp_min(1e-300)).max()) / 2.0 ** -23:.3f} x 2^-23')
            assert bool((err <= 2.0 ** -23 * want.abs()).all()), name
            judge('pix part', name, o.part_l1, cs['ref'][F64]['part_l1'], cs['ref'][F32]['part_l1'])
            assert o.same(launch(L, loss, p, t, B, Ch, H, W, scale=scale, grad=False), grad=False), name
            if kind != 'flat':
                check_stats(o, loss, P, H, W, scale, name)
            if kind == 'tied' and loss == 'L1':
                m = Q.tied_mask(P, H, W)
                assert bool((o.dpred[m] == 0).all()) and bool((o.dpred[~m] != 0).all())


def test_the_entries_decline_what_they_do_not_take(L):
    H = W = 11
    x = torch.rand(3, H, W, device=DEV)
    bo, out = guarded(3 * H * W)
    bs, stats = guarded(8)
    tiles, off_pl, total = layout(L, 1, 3, H, W)
    bw, ws = guarded(total)

    def call(pred=x, frames=x, B=1, Ch=3, h=H, w=W, lid=2, tstats=None, st=stats, wsp=ws, nbytes=total * 4):
        return L.orn_debug_loss_launch(_p(pred), _p(frames), None, c_size_t(0), B, Ch, h, w, lid, c_float(1.0), _p(tstats), _p(st), _p(out),
                                       _p(wsp), nbytes, _st())

    bad = [call(pred=None), call(frames=None), call(st=None), call(wsp=None), call(B=0), call(Ch=0), call(h=0), call(B=2, Ch=40000),
           call(lid=15), call(lid=-1), call(lid=12), call(lid=1, tstats=x), call(h=10), call(w=10)]
    assert 'loss' in _err()
    assert bad == [-1] * len(bad), bad
    assert call(nbytes=total * 4 - 4) == -2 and 'debug_loss_launch' in _err()
    lay = (c_int64 * 4)()
    assert L.orn_debug_loss_layout(1, 3, H, W, None) == -1 and L.orn_debug_loss_layout(0, 3, H, W, lay) == -1
    assert 'debug_loss_layout' in _err()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(stats).all())
    assert guards_intact(bo) and guards_intact(bw) and guards_intact(bs)
