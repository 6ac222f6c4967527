"""Reference, inputs, comparator and mutants shared by tests/test_gpu_msssim_levels.py (the kernels on the GPU) and
tests/test_msssim_levels_host.py (the comparator against mutants, no GPU).

Reference: the operation of one MS-SSIM level (oracle.cpu_ref.ssim_maps, avg_pool2d, autograd) on the CPU in float64, filtered
with the fp32 Gaussian taps of pytorch_msssim promoted to float64 -- the window the package and liborn both use, whatever the
dtype of the image.  Every function takes the dtype to evaluate in: float64 gives r64, float32 gives r32, the same formulas in
fp32 in torch's summation order.

Tolerance rule (ratio / accept): E = max(max|r32 - r64|, 2^-24 max|r64|) per compared tensor; a result k passes when
max|k - r64| <= c E.  The error of a correct fp32 evaluation depends on conditioning (sigma^2 = G*x^2 - mu^2 cancels), so E is
measured on the case's own inputs instead of fixed.  C holds c per kind of tensor."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref

TH, TW = 16, 64                                   # the tile of every loss kernel
MS_W = np.array(cpu_ref._MS_WEIGHTS, dtype=np.float32)       # the kernels hold the level weights as fp32 constants

# c of the tolerance rule per kind: the smallest power of two that is at least twice the worst ratio max|k - r64| / E measured on
# an MI355X (the table in tests/test_gpu_msssim_levels.py); the rule allows no c above 8.
C = {
    'fwd part': 8.0,        # measured 3.337 (27x75, 1 plane)
    'bwd g': 8.0,           # measured 2.101 (11x11, 3 planes, the SSIM form with gnext)
    'bwd part': 4.0,        # measured 1.734 (43x139, 3 planes)
    'chain g': 4.0,         # measured 1.185 (1x3x161x177, level 4)
    'chain dpred': 4.0,     # measured 1.128 (1x3x161x177)
}

FWD_SHAPES = [(11, 11), (11, 12), (26, 74), (27, 75), (27, 76), (32, 128), (43, 139), (42, 140)]
# the issue's list plus 26x75: the only (even, odd) size, so that every parity of (H, W) meets the pool's adjoint
BWD_SHAPES = [(11, 11), (11, 12), (16, 64), (17, 65), (26, 74), (26, 75), (27, 75), (30, 78), (32, 128), (43, 139), (42, 140)]
PLANES = [1, 3, 64]
CHAIN_SHAPES = [(1, 161, 177), (2, 163, 201)]


def taps32():
    """pytorch_msssim _fspecial_gauss_1d(11, 1.5) in fp32, operation by operation as liborn's orn_gauss_taps forms it: fp32
    argument, correctly rounded exp, fp32 sum in index order, fp32 divide."""
    c = np.arange(11, dtype=np.float32) - np.float32(5)
    a = -(c * c) / np.float32(2.0 * 1.5 * 1.5)
    g = np.exp(a.astype(np.float64)).astype(np.float32)
    s = np.float32(0)
    for v in g:
        s = np.float32(s + v)
    return (g / s).astype(np.float32)


def win(dtype):
    return torch.from_numpy(taps32()).to(dtype)


def pooled(n):
    return (n + 2 * (n % 2)) // 2


def make_pair(B, H, W):
    """The inputs of tests/test_gpu_loss_types.py: target = uniform noise under a 5x5 box filter, pred = target + 0.1 randn."""
    gen = torch.Generator().manual_seed(H * W + B)
    u = torch.rand(B, 3, H + 4, W + 4, generator=gen)
    t = F.avg_pool2d(u, 5, stride=1)
    p = (t + 0.1 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    return p.contiguous(), t.contiguous()


def planes_pair(P, H, W):
    """P planes [P][H][W] of make_pair (every plane its own noise, so a plane-index slip shows)."""
    p, t = make_pair(-(-P // 3), H, W)
    return p.reshape(-1, H, W)[:P].contiguous(), t.reshape(-1, H, W)[:P].contiguous()


def flat_pair(B, H, W):
    """Nearly flat: 0.5 + 1e-3 noise on both sides, sigma^2 far below C2 -- the ill-conditioned case."""
    gen = torch.Generator().manual_seed(7 * H + W + B)
    t = 0.5 + 1e-3 * torch.randn(B, 3, H, W, generator=gen)
    p = t + 1e-3 * torch.randn(B, 3, H, W, generator=gen)
    return p.contiguous(), t.contiguous()


def relu_pair(B, H, W, a=0.25):
    """p, t = clamp(s +- a * checker), s smooth.  The 2x2 pool cancels the checkerboard exactly wherever no clamp acts (s stays
    inside [a, 1 - a]), so levels 1..4 see p == t, and level 0 sees sigma_pt = sigma_s^2 - a^2 < 0: a negative CS mean."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    s = torch.stack([0.5 + 0.125 * torch.sin(0.05 * yy + 0.3 * c + b) * torch.cos(0.04 * xx) for b in range(B) for c in range(3)])
    s = (s.view(B, 3, H, W) * 1024).round() / 1024               # 10 fractional bits: s +- a and the pool's sums are exact in fp32
    chk = 1 - 2 * ((yy + xx) % 2)
    if H % 2 and W % 2:
        chk[0, 0] = 0            # with both sizes odd the padded pool forms its corner from this pixel alone: nothing to cancel with
    return (s + a * chk).clamp(0, 1).contiguous(), (s - a * chk).clamp(0, 1).contiguous()


# ---- one level ---------------------------------------------------------------------------------------------------------------
def maps(x, y, w):
    """ssim_map, cs_map [P][H-10][W-10] of planes x, y [P][H][W]"""
    s, c = cpu_ref.ssim_maps(x[None], y[None], 1.0, win=w)
    return s[0], c[0]


def _filt(x, wv, wh):
    P = x.shape[0]
    out = F.conv2d(x[None], wv.view(1, 1, -1, 1).repeat(P, 1, 1, 1), groups=P)
    return F.conv2d(out, wh.view(1, 1, 1, -1).repeat(P, 1, 1, 1), groups=P)[0]


def _maps_windows(x, y, wv, wh):
    m, mu = _filt(x, wv, wh), _filt(y, wv, wh)
    sp, st, spt = _filt(x * x, wv, wh) - m * m, _filt(y * y, wv, wh) - mu * mu, _filt(x * y, wv, wh) - m * mu
    cs = (2 * spt + 0.03 ** 2) / (sp + st + 0.03 ** 2)
    return (2 * m * mu + 0.01 ** 2) / (m * m + mu * mu + 0.01 ** 2) * cs, cs


def maps_tap_dropped(where):
    """MUTANT: the weakest tap (the last one) missing in the last valid column ('col') or row ('row') of both maps."""
    def fn(x, y, w):
        full = maps(x, y, w)
        wd = w.clone()
        wd[-1] = 0
        if where == 'col':
            edge = _maps_windows(x[:, :, -11:], y[:, :, -11:], w, wd)
            return tuple(torch.cat([f[:, :, :-1], e], 2) for f, e in zip(full, edge))
        edge = _maps_windows(x[:, -11:], y[:, -11:], wd, w)
        return tuple(torch.cat([f[:, :-1], e], 1) for f, e in zip(full, edge))
    return fn


def tile_sums(m):
    """[P][tiles] sums of m [P][h][w] over its 16x64 tiles, tile rows first"""
    P, h, w = m.shape
    nh, nw = -(-h // TH), -(-w // TW)
    z = m.new_zeros(P, nh * TH, nw * TW)
    z[:, :h, :w] = m
    return z.view(P, nh, TH, nw, TW).sum((2, 4)).reshape(P, nh * nw)


def pool(x):
    return F.avg_pool2d(x[None], 2, padding=(x.shape[1] % 2, x.shape[2] % 2))[0]


def pool_boundary_row_from_neighbour(x):
    """MUTANT of pool: the first pooled row owned by the second tile row reads its inputs one row further down."""
    H, pw = x.shape[1], x.shape[2] % 2
    out = pool(x).clone()
    if H - 10 > TH:                                   # a second tile row exists
        ph = H % 2
        yo = TH // 2 + ph                             # its inputs are rows 2 yo - ph and the next one
        xp = F.pad(x[:, 2 * yo - ph + 1:2 * yo - ph + 3], (pw, 0))
        out[:, yo] = 0.25 * (xp[:, :, 0::2] + xp[:, :, 1::2]).sum(1)
    return out


def fwd_ref(x32, y32, dtype, maps_fn=maps):
    """part [P][tiles][2] = {ssim, cs} tile sums of the valid map, and the pooled planes"""
    x, y = x32.to(dtype), y32.to(dtype)
    s, c = maps_fn(x, y, win(dtype))
    return torch.stack([tile_sums(s), tile_sums(c)], 2), pool(x), pool(y)


def unit_grads(x32, y32, dtype, maps_fn=maps):
    """d(sum of the map over the plane) / dx per plane, for the SSIM map and the CS map: [P][H][W] each"""
    x, y = x32.to(dtype).requires_grad_(True), y32.to(dtype)
    s, c = maps_fn(x, y, win(dtype))
    gs, = torch.autograd.grad(s.sum(), x, retain_graph=True)
    gc, = torch.autograd.grad(c.sum(), x)
    return gs, gc


def pool_adjoint(gnext32, H, W, dtype):
    """gradient of (avg_pool2d(x, 2, padding = size % 2) * gnext).sum() with respect to x [P][H][W], by autograd"""
    x = torch.zeros(gnext32.shape[0], H, W, dtype=dtype, requires_grad=True)
    g, = torch.autograd.grad((pool(x) * gnext32.to(dtype)).sum(), x)
    return g


def pool_adjoint_indexed(gnext32, H, W, dtype, ph, pw, off=0):
    """MUTANTS of the adjoint: 0.25 * gnext[(y + ph + off) >> 1][(x + pw) >> 1] with a wrong ph or a shifted parity"""
    g = gnext32.to(dtype)
    yi = ((torch.arange(H) + ph + off) >> 1).clamp(0, g.shape[1] - 1)
    xi = ((torch.arange(W) + pw) >> 1).clamp(0, g.shape[2] - 1)
    return 0.25 * g[:, yi][:, :, xi]


def pixel_term(x32, y32, g_l1, g_l2, dtype):
    d = x32.to(dtype) - y32.to(dtype)
    return g_l1 * torch.sign(d) + g_l2 * d


def pixel_parts(x32, y32, dtype):
    """[P][tiles][2] = {sum |d|, sum d^2} over the 16x64 tiles of the image"""
    d = x32.to(dtype) - y32.to(dtype)
    return torch.stack([tile_sums(d.abs()), tile_sums(d * d)], 2)


def level_grad(unit, k32, adj, pix, dtype):
    """g = k[plane] * unit + adjoint of the level above + pixel term (either may be None), formed in dtype"""
    g = k32.to(dtype).view(-1, 1, 1) * unit
    if adj is not None:
        g = g + adj
    if pix is not None:
        g = g + pix
    return g


_BWD = {}


def bwd_case(P, H, W):
    """Inputs and both references of the backward forms at one (planes, shape), computed once and never modified: planes, a
    distinct k per plane, gnext and the pixel scales sized so that each term weighs in the sum, and per dtype the unit gradients
    of both maps, the pool adjoint, the pixel term and the pixel partials."""
    key = (P, H, W)
    if key not in _BWD:
        x, y = planes_pair(P, H, W)
        gen = torch.Generator().manual_seed(1000 * H + W + P)
        ref = {}
        for dt in (torch.float64, torch.float32):
            gs, gc = unit_grads(x, y, dt)
            ref[dt] = {'ssim': gs, 'cs': gc}
        s = float(ref[torch.float64]['cs'].abs().mean())
        k = -(1 + 0.5 * torch.arange(P, dtype=torch.float32) / P)
        gnext = (4 * s * torch.randn(P, pooled(H), pooled(W), generator=gen)).float()
        g_l1, g_l2 = float(np.float32(0.5 * s)), float(np.float32(2 * s))
        for dt in (torch.float64, torch.float32):
            ref[dt]['adj'] = pool_adjoint(gnext, H, W, dt)
            ref[dt]['pix'] = pixel_term(x, y, g_l1, g_l2, dt)
            ref[dt]['part'] = pixel_parts(x, y, dt)
        _BWD[key] = dict(x=x, y=y, k=k, gnext=gnext, g_l1=g_l1, g_l2=g_l2, ref=ref)
    return _BWD[key]


def bwd_ref(case, form, with_gnext, dtype, unit=None, k=None, adj=None):
    """reference gradient of one form (0 SSIM map, 1 CS map, 2 CS map at level 0) in dtype; unit / k / adj: a mutant's"""
    r = case['ref'][dtype]
    unit = r['ssim' if form == 0 else 'cs'] if unit is None else unit
    adj = (r['adj'] if adj is None else adj) if with_gnext else None
    return level_grad(unit, case['k'] if k is None else k, adj, r['pix'] if form == 2 else None, dtype)


# ---- the whole chain ---------------------------------------------------------------------------------------------------------
def coefficients(v, w_struct_scaled, nmap):
    """value and k[5][P] of the coefficient kernel from the level means v [5][P] (float64): the documented formula in double,
    the weights and w_struct * loss_scale rounded to fp32 first as the kernel holds them"""
    w = MS_W.astype(np.float64)[:, None]
    prod = np.prod(np.power(np.maximum(v, 0.0), w), 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        c = -float(np.float32(w_struct_scaled)) * w * prod[None] / v / v.shape[1] / np.asarray(nmap, np.float64)[:, None]
    return prod.mean(), np.where(v > 0, c, 0.0)


def chain_ref(p32, t32, w_l1, w_struct, dtype, wrong_gnext_at_3=False):
    """The MS-SSIM loss of orn_loss_fwd_bwd in dtype (coefficients in double, as the kernel): pooled planes [(x_l, y_l)], level
    gradients g[l], dpred = g[0] + float(w_l1 / n) sign(p - t), the value and k.  wrong_gnext_at_3 (MUTANT): level 3 takes the
    start of its own gradient buffer, read with level 4's geometry, where level 4's gradient belongs."""
    H, W = p32.shape[-2:]
    xs, ys = [p32.reshape(-1, H, W).to(dtype)], [t32.reshape(-1, H, W).to(dtype)]
    for _ in range(4):
        xs.append(pool(xs[-1]))
        ys.append(pool(ys[-1]))
    P = xs[0].shape[0]
    v, unit, nmap = [], [], []
    for l in range(5):
        x = xs[l].detach().requires_grad_(True)
        s, c = maps(x, ys[l], win(dtype))
        m = s if l == 4 else c
        unit.append(torch.autograd.grad(m.sum(), x)[0])
        v.append(m.detach().double().mean((1, 2)).numpy())
        nmap.append(float(m.shape[1] * m.shape[2]))
    val, k = coefficients(np.stack(v), w_struct, nmap)
    k32 = torch.from_numpy(k.astype(np.float32))
    g = [None] * 5
    for l in (4, 3, 2, 1, 0):
        adj = None
        if l < 4:
            gn = g[l + 1]
            if wrong_gnext_at_3 and l == 3:
                gn = (k32[3].to(dtype).view(-1, 1, 1) * unit[3]).reshape(P, -1)[:, :g[4][0].numel()].reshape(g[4].shape)
            adj = pool_adjoint(gn.float() if dtype == torch.float32 else gn, xs[l].shape[1], xs[l].shape[2], dtype)
        g[l] = level_grad(unit[l], k32[l], adj, None, dtype)
    g_l1 = float(np.float32(w_l1 / (P * H * W)))
    dpred = g[0] + g_l1 * torch.sign(xs[0] - ys[0])
    return dict(x=xs, y=ys, g=g, dpred=dpred, val=val, k=k, v=np.stack(v), g_l1=g_l1)


# ---- the comparator ----------------------------------------------------------------------------------------------------------
def _np(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def ratio(k, r64, r32):
    """max|k - r64| / E with E = max(max|r32 - r64|, 2^-24 max|r64|); NaN if k holds one"""
    k, r64, r32 = _np(k), _np(r64), _np(r32)
    E = max(np.abs(r32 - r64).max(), 2.0 ** -24 * np.abs(r64).max())
    err = np.abs(k - r64).max()
    if E == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return float(err / E)


def accept(k, r64, r32, kind):
    return bool(ratio(k, r64, r32) <= C[kind])


def pooled_ok(k, r64, levels=1):
    """a pooled plane against float64: three fp32 additions of non-negative values and an exact scaling per level lose at most
    3 * 2^-24 < 2^-22 relative, and non-negative inputs carry a relative error through the next level's sums unchanged"""
    k, r64 = _np(k), _np(r64)
    return bool((np.abs(k - r64) <= levels * 2.0 ** -22 * np.abs(r64)).all())
