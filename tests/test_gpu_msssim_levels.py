"""The eleven launches of the MS-SSIM losses (Fusion10 / 11 / 12) one by one against a float64 reference: k_msssim_level (orn_loss.hip),
k_msssim_coef and the three gradient forms of k_msssim_level_bwd plus its partials-only form (orn_loss_msssim.hip), through
orn_debug_msssim_level_fwd / _bwd and orn_debug_loss_msssim_layout of include/orn_debug.h.  The public entry takes nothing below
161 px, so levels 1..4 only ever see what pooling leaves (81x89, 41x45, 21x23, 11x12 ...); the entries take any H, W >= 11 and
build the kernel argument with the function the product launcher uses.

Shapes (H x W), the smallest reaching each edge of the 16x64 tiling and of the pooling:
  forward   11x11 one valid pixel; 11x12 two valid columns (the product's smallest level 4); 26x74 the valid map exactly one tile;
            27x75 two tile rows and columns with a remainder of 1 and ph = pw = 1, a pooled pixel straddling each tile boundary;
            27x76 mixed parity; 32x128 all even; 43x139 and 42x140 3x3 tiles with an interior tile
  backward  11x11; 11x12 (the float4 path with x0 - 12 < 0); 16x64 and 17x65 (one image tile exactly, and plus 1); 26x74; 26x75
            (even x odd); 27x75; 30x78 (even width, scalar path); 32x128 (float4, exactly 2x2 tiles); 43x139; 42x140 -- so every
            parity of (H, W) meets the pool adjoint; each with and without gnext, each of the three gradient forms, and the
            level-0 forms also through a three-frame table at frame_idx = 2 with frame_stride % 4 == 0 and != 0
  planes    1, 3 and 64, every plane its own noise and its own k
  chain     orn_loss_fwd_bwd at 1x3x161x177 and 2x3x163x201: every pooled plane, every level's gradient and dpred, read through
            the layout entry, for the suite's pair, a nearly flat pair and a pair on the relu branch

Reference and tolerance rule: tests/msssim_levels_ref.py (float64 with the fp32 taps; E = max(max|r32 - r64|, 2^-24 max|r64|),
max|k - r64| <= c E).  Pooled planes: 2^-22 relative per level.  Coefficients and value: the documented formula in double from
the kernel's OWN partials, 2^-23 relative (the final cast), which separates k_msssim_coef from the error of the maps.
tests/test_msssim_levels_host.py shows that this comparator rejects seven mutants with the c below.

Worst ratio max|k - r64| / E measured on an MI355X per kind, and the c it fixes (the smallest power of two >= twice the ratio):
    kind            worst ratio   c    where
    fwd part        3.337         8    27x75, 1 plane           {ssim, cs} tile partials of k_msssim_level
    bwd g           2.101         8    11x11, 3 planes, form 0  g of the three gradient forms of k_msssim_level_bwd
    bwd part        1.734         4    43x139, 3 planes         {|d|, d^2} tile partials of the level-0 forms
    chain g         1.185         4    1x3x161x177, level 4     the level gradients of a product call
    chain dpred     1.128         4    1x3x161x177              dpred of a product call
The module's 70 tests run in 3.5 s on one MI355X, none above 0.4 s.

Every output buffer starts as NaN between two sentinel bands that must stay untouched; every case runs twice and must give the
same bits."""
from ctypes import c_float, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import msssim_levels_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = 7.0
GUARD = 1024                   # floats: keeps the payload 16-byte aligned
NAN = float('nan')
F64, F32 = torch.float64, torch.float32
FUSION10, W_L1, W_STRUCT = 12, 0.7, 0.3


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_msssim_level_fwd', 'orn_debug_msssim_level_bwd', 'orn_debug_msssim_level_fwd_tiles',
                 'orn_debug_msssim_level_bwd_tiles', 'orn_debug_loss_msssim_layout'):
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
    print(f'{kind:12s} {name}: ratio {r:.3f} (c = {R.C[kind]:g})')
    assert r <= R.C[kind], (kind, name, r)


# ---- the kernels under test (one thin call each) -----------------------------------------------------------------------------
def k_level_fwd(L, x, y, P, H, W, part, nx, ny):
    return L.orn_debug_msssim_level_fwd(_p(x), _p(y), P, H, W, _p(part), _p(nx), _p(ny), _st())


def k_level_bwd(L, form, x, y, k, gnext, fidx, fstride, P, H, W, g_l1, g_l2, g, part):
    return L.orn_debug_msssim_level_bwd(form, _p(x), _p(y), _p(k), _p(gnext), _p(fidx), c_size_t(fstride), P, H, W, c_float(g_l1),
                                        c_float(g_l2), _p(g), _p(part), _st())


def k_loss(L, p, t, B, H, W, stats, dpred, ws, ws_bytes):
    return L.orn_loss_fwd_bwd(_p(p), _p(t), B, 3, H, W, FUSION10, c_float(1.0), _p(stats), _p(dpred), _p(ws), ws_bytes, _st())


# ---- one forward level -------------------------------------------------------------------------------------------------------
def run_fwd(L, x, y, P, H, W, pool=True):
    tiles = L.orn_debug_msssim_level_fwd_tiles(H, W)
    assert tiles == -(-(H - 10) // R.TH) * -(-(W - 10) // R.TW)
    no = P * R.pooled(H) * R.pooled(W)
    bp, part = guarded(P * tiles * 2)
    bx, nx = guarded(no)
    by, ny = guarded(no)
    rc = k_level_fwd(L, x, y, P, H, W, part, nx if pool else None, ny if pool else None)
    torch.cuda.synchronize()
    assert rc == 0, _err()
    assert guards_intact(bp) and guards_intact(bx) and guards_intact(by)
    return part.view(P, tiles, 2), nx.view(P, R.pooled(H), R.pooled(W)), ny.view(P, R.pooled(H), R.pooled(W))


@pytest.mark.parametrize('P', R.PLANES)
@pytest.mark.parametrize('shape', R.FWD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_level_forward(L, shape, P):
    H, W = shape
    x, y = R.planes_pair(P, H, W)
    part64, nx64, ny64 = R.fwd_ref(x, y, F64)
    part32, _, _ = R.fwd_ref(x, y, F32)
    dx, dy = x.to(DEV), y.to(DEV)
    part, nx, ny = run_fwd(L, dx, dy, P, H, W)
    again = run_fwd(L, dx, dy, P, H, W)
    assert all(same_bits(a, b) for a, b in zip((part, nx, ny), again))
    # every pooled element is written (no NaN left; each has one owner tile, whose patch alone holds all of its inputs) and right
    assert bool(torch.isfinite(nx).all()) and bool(torch.isfinite(ny).all()) and bool(torch.isfinite(part).all())
    assert R.pooled_ok(nx, nx64) and R.pooled_ok(ny, ny64)
    judge('fwd part', f'{H}x{W} P={P}', part, part64, part32)
    alone, nx0, ny0 = run_fwd(L, dx, dy, P, H, W, pool=False)      # the last level's form: nothing pooled, the same partials
    assert same_bits(alone, part) and bool(torch.isnan(nx0).all()) and bool(torch.isnan(ny0).all())


# ---- one backward level ------------------------------------------------------------------------------------------------------
def run_bwd(L, form, case, P, H, W, with_gnext, table_stride=0):
    x, k, gn = (case[n].to(DEV) for n in ('x', 'k', 'gnext'))
    n = P * H * W
    if table_stride:             # the target as frame 2 of a three-frame table; the other frames and the slack hold NaN
        y = torch.full((3 * table_stride,), NAN, device=DEV)
        y[2 * table_stride:2 * table_stride + n] = case['y'].to(DEV).flatten()
        fidx = torch.tensor([2], dtype=torch.int32, device=DEV)
    else:
        y, fidx = case['y'].to(DEV), None
    tiles = L.orn_debug_msssim_level_bwd_tiles(H, W)
    assert tiles == -(-H // R.TH) * -(-W // R.TW)
    bg, g = guarded(n)
    bp, part = guarded(P * tiles * 2)
    rc = k_level_bwd(L, form, x, y, k, gn if with_gnext else None, fidx, table_stride, P, H, W, case['g_l1'], case['g_l2'], g, part)
    torch.cuda.synchronize()
    assert rc == 0, _err()
    assert guards_intact(bg) and guards_intact(bp)
    return g.view(P, H, W), part.view(P, tiles, 2)


@pytest.mark.parametrize('P', R.PLANES)
@pytest.mark.parametrize('shape', R.BWD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_level_backward(L, shape, P):
    H, W = shape
    case = R.bwd_case(P, H, W)
    ref = case['ref']
    n4 = -(-P * H * W // 4) * 4
    for form in (0, 1, 2):
        for with_gnext in (False, True):
            name = f'{H}x{W} P={P} form {form} gnext {int(with_gnext)}'
            g, part = run_bwd(L, form, case, P, H, W, with_gnext)
            g2, part2 = run_bwd(L, form, case, P, H, W, with_gnext)
            assert same_bits(g, g2) and bool(torch.isfinite(g).all())
            judge('bwd g', name, g, R.bwd_ref(case, form, with_gnext, F64), R.bwd_ref(case, form, with_gnext, F32))
            if form < 2:
                assert bool(torch.isnan(part).all())               # only the level-0 forms write partials
                continue
            assert same_bits(part, part2)
            judge('bwd part', name, part, ref[F64]['part'], ref[F32]['part'])
            for stride in (n4 + 4, n4 + 5):                        # a multiple of 4, and not: the scalar path at any width
                gt, pt = run_bwd(L, form, case, P, H, W, with_gnext, table_stride=stride)
                assert same_bits(gt, g) and same_bits(pt, part), (name, stride)
    # the level-0 form without the gradient writes the partials of the form with it, and nothing else
    g, part = run_bwd(L, 2, case, P, H, W, True)
    for stride in (0, n4 + 4, n4 + 5):
        g3, part3 = run_bwd(L, 3, case, P, H, W, True, table_stride=stride)
        assert bool(torch.isnan(g3).all()) and same_bits(part3, part)


def test_the_entries_decline_what_they_do_not_take(L):
    x = torch.rand(2, 11, 11, device=DEV)
    bo, out = guarded(2 * 11 * 11)
    k = torch.ones(2, device=DEV)
    bad = [k_level_fwd(L, x, x, 2, 10, 11, out, None, None), k_level_fwd(L, x, x, 0, 11, 11, out, None, None),
           k_level_fwd(L, x, x, 2, 11, 11, None, None, None), k_level_fwd(L, x, x, 2, 11, 11, out, out, None),
           k_level_bwd(L, 4, x, x, k, None, None, 0, 2, 11, 11, 0.0, 0.0, out, out),
           k_level_bwd(L, 1, x, x, k, None, None, 0, 2, 11, 10, 0.0, 0.0, out, out),
           k_level_bwd(L, 1, x, x, None, None, None, 0, 2, 11, 11, 0.0, 0.0, out, out),
           k_level_bwd(L, 2, x, x, k, None, None, 0, 2, 11, 11, 0.0, 0.0, out, None),
           k_level_bwd(L, 0, x, x, k, None, k, 0, 2, 11, 11, 0.0, 0.0, out, out),
           k_level_bwd(L, 1, x, x, k, None, None, 0, 70000, 11, 11, 0.0, 0.0, out, out)]
    assert 'debug_msssim_level_bwd' in _err()
    lay = (c_int64 * 44)()
    bad += [L.orn_debug_loss_msssim_layout(2, 1, 3, 161, 177, lay), L.orn_debug_loss_msssim_layout(FUSION10, 1, 3, 160, 177, lay),
            L.orn_debug_loss_msssim_layout(FUSION10, 22, 3, 161, 177, lay)]
    assert 'debug_loss_msssim_layout' in _err()
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert bool(torch.isnan(out).all()) and guards_intact(bo)
    assert L.orn_debug_msssim_level_fwd_tiles(10, 64) == 0 and L.orn_debug_msssim_level_bwd_tiles(64, 10) == 0


# ---- the whole chain ---------------------------------------------------------------------------------------------------------
_CHAIN = {}
PAIRS = {'pair': R.make_pair, 'flat': R.flat_pair, 'relu': R.relu_pair}


def chain_run(L, shape, kind):
    """One orn_loss_fwd_bwd(Fusion10) call (run twice, same bits) with every intermediate read back through the layout entry."""
    if (shape, kind) in _CHAIN:
        return _CHAIN[shape, kind]
    B, H, W = shape
    P = 3 * B
    p, t = PAIRS[kind](*shape)
    lay = (c_int64 * 44)()
    assert L.orn_debug_loss_msssim_layout(FUSION10, B, 3, H, W, lay) == 0, _err()
    lay = list(lay)
    ws_bytes = L.orn_loss_ws_bytes_for(FUSION10, B, 3, H, W)
    assert lay[43] * 4 == ws_bytes
    runs = []
    for _ in range(2):
        bw, ws = guarded(ws_bytes // 4)
        bd, dpred = guarded(P * H * W)
        stats = torch.full((8,), NAN, device=DEV)
        rc = k_loss(L, p.to(DEV), t.to(DEV), B, H, W, stats, dpred, ws, ws_bytes)
        torch.cuda.synchronize()
        assert rc == 0, _err()
        assert guards_intact(bw) and guards_intact(bd)
        runs.append((ws, dpred, stats))
    assert all(same_bits(a, b) for a, b in zip(*runs))
    ws, dpred, stats = (a.cpu() for a in runs[0])
    out = dict(p=p, t=t, dpred=dpred.view(P, H, W), stats=stats, x=[None], y=[None], g=[None], part=[], k=[], nblk=[])
    for l in range(5):
        h, w, ox, oy, opart, nblk, og, ok = lay[8 * l:8 * l + 8]
        assert (h, w) == ((H, W) if l == 0 else (R.pooled(out['hw'][0]), R.pooled(out['hw'][1])))
        out['hw'] = (h, w)
        if l:
            out['x'].append(ws[ox:ox + P * h * w].view(P, h, w))
            out['y'].append(ws[oy:oy + P * h * w].view(P, h, w))
            out['g'].append(ws[og:og + P * h * w].view(P, h, w))
        out['part'].append(ws[opart:opart + P * nblk * 2].view(P, nblk, 2).double().numpy())
        out['k'].append(ws[ok:ok + P].double().numpy())
        out['nblk'].append(nblk)
    out['val'] = float(ws[lay[40]])
    out['part_l1'] = ws[lay[41]:lay[41] + P * lay[42] * 2].view(P, lay[42], 2)
    _CHAIN[shape, kind] = out
    return out


_REF = {}


def chain_refs(shape, kind):
    if (shape, kind) not in _REF:
        p, t = PAIRS[kind](*shape)
        _REF[shape, kind] = (R.chain_ref(p, t, W_L1, W_STRUCT, F64), R.chain_ref(p, t, W_L1, W_STRUCT, F32))
    return _REF[shape, kind]


@pytest.mark.parametrize('kind', ['pair', 'flat'])
@pytest.mark.parametrize('shape', R.CHAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_chain_wiring(L, shape, kind):
    """Level order, buffer offsets and the k row per level: every intermediate of a product call against the float64 chain."""
    out = chain_run(L, shape, kind)
    r64, r32 = chain_refs(shape, kind)
    assert r64['v'].min() > 0.05                                   # no level mean near the relu's kink
    for l in (1, 2, 3, 4):
        assert R.pooled_ok(out['x'][l], r64['x'][l], l) and R.pooled_ok(out['y'][l], r64['y'][l], l), l
        judge('chain g', f'{kind} {shape} level {l}', out['g'][l], r64['g'][l], r32['g'][l])
    judge('chain dpred', f'{kind} {shape}', out['dpred'], r64['dpred'], r32['dpred'])
    judge('bwd part', f'{kind} {shape} chain', out['part_l1'], R.pixel_parts(out['p'].view(-1, *shape[1:]), out['t'].view(-1, *shape[1:]), F64),
          R.pixel_parts(out['p'].view(-1, *shape[1:]), out['t'].view(-1, *shape[1:]), F32))
    assert float(out['stats'][3]) == out['val']


@pytest.mark.parametrize('kind', ['pair', 'flat', 'relu'])
@pytest.mark.parametrize('shape', R.CHAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_coefficients_from_the_kernels_own_partials(L, shape, kind):
    """k[l][p] and the value against the documented formula in double, evaluated from the partials the level kernels left."""
    out = chain_run(L, shape, kind)
    _, H, W = shape
    nmap, v, h, w = [], [], H, W
    for l in range(5):
        nmap.append(float(np.float32(h - 10) * np.float32(w - 10)))
        assert out['nblk'][l] == -(-(h - 10) // R.TH) * -(-(w - 10) // R.TW)
        v.append(out['part'][l][:, :, 0 if l == 4 else 1].sum(1) / nmap[-1])
        h, w = R.pooled(h), R.pooled(w)
    val, k = R.coefficients(np.stack(v), W_STRUCT, nmap)
    got = np.stack(out['k'])
    print(f'{kind} {shape}: worst relative k error {np.abs(got - k).max() / max(np.abs(k).max(), 1e-300):.3g}')
    assert (np.abs(got - k) <= 2.0 ** -23 * np.abs(k)).all()
    assert abs(out['val'] - val) <= 2.0 ** -23 * abs(val)
    if kind == 'relu':
        assert (got == 0).all() and out['val'] == 0.0


@pytest.mark.parametrize('shape', R.CHAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_chain_on_the_relu_branch(L, shape):
    """A negative CS mean at level 0: value 0, every coefficient 0, every level gradient exactly 0 and dpred exactly
    float(w_l1 / n) sign(p - t), as orn.h documents (autograd gives NaN there)."""
    out = chain_run(L, shape, 'relu')
    B, H, W = shape
    x, y = out['p'].view(-1, H, W).double(), out['t'].view(-1, H, W).double()
    for l in range(5):
        s, c = R.maps(x, y, R.win(F64))
        v = (s if l == 4 else c).mean((1, 2))
        assert bool((v < -0.05).all()) if l == 0 else bool((v > 0.9).all()), (l, v)
        x, y = R.pool(x), R.pool(y)
    assert out['val'] == 0.0 and float(out['stats'][3]) == 0.0
    for l in (1, 2, 3, 4):
        assert torch.equal(out['x'][l], out['y'][l])
        assert bool((out['g'][l] == 0).all()), l
    g_l1 = np.float32(W_L1 / (3 * B * H * W))
    want = torch.sign(out['p'] - out['t']).view(-1, H, W) * float(g_l1)
    assert torch.equal(out['dpred'], want)
