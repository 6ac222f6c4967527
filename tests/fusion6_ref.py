"""Reference, inputs, comparator constants and mutants shared by tests/test_gpu_fusion6.py (k_fusion6, k_loss_grad and the finalize
stage on the GPU) and tests/test_fusion6_host.py (the comparator against mutants, no GPU).  Built on tests/msssim_levels_ref.py: its
window, maps, inputs and the tolerance rule  E = max(max|r32 - r64|, 2^-24 max|r64|), max|k - r64| <= c E.

Every reference takes the dtype to evaluate in: float64 gives r64, float32 gives r32 (the fp32 taps promoted either way).
  target maps    G*t and G*t^2 on the valid map (H-10) x (W-10): what orn_loss_target_stats caches per frame
  SSIM partials  the SSIM map summed per tile of the IMAGE's tiling, ceil(H/16) x ceil(W/64): a tile owns the valid-map pixels whose
                 coordinates fall inside it, so the trailing tiles own nothing and hold 0
  dpred          loss_scale * (w_l1 d mean|d| + w_l2 d mse + w_struct d (1 - mean ssim)) / d pred, each of the three terms by autograd
                 (autograd of the weighted sum is this combination: the backward pass is linear in the weights), sign(0) = 0
  pixel partials {sum |d|, sum d^2} per image tile (msssim_levels_ref.pixel_parts)
References are computed once per case (case, table_case) and never modified."""
import numpy as np
import torch

import msssim_levels_ref as R

F64, F32 = torch.float64, torch.float32
TH, TW = R.TH, R.TW
C1, C2 = 0.01 ** 2, 0.03 ** 2

# c of the tolerance rule per kind: the smallest power of two that is at least twice the worst ratio max|k - r64| / E measured on
# an MI355X (the table in tests/test_gpu_fusion6.py); the rule allows no c above 8.
C = {
    'tmaps': 8.0,           # measured 2.502 (11x11, frame 1 of the table, G*t)
    'ssim part': 8.0,       # measured 3.452 (17x65, 1x3 planes, the suite's pair)
    'dpred struct': 4.0,    # measured 1.601 (11x11, 1x3 planes, the tied pair)
    'dpred pixel': 4.0,     # measured 1.896 (27x75, Fusion1 through the table at frame 2)
    'pix part': 4.0,        # measured 1.734 (43x139, 1x3 planes, the suite's pair)
}

SHAPES = R.BWD_SHAPES
PLANES = [(1, 1), (1, 3), (2, 3), (1, 64)]                 # (B, Ch)
KINDS = ('pair', 'flat', 'tied')
GRAD_SHAPES = [(11, 11), (17, 65), (30, 78), (32, 128)]    # k_loss_grad
# name: (loss id of include/orn.h, w_l1, w_l2, w_struct) -- orn_loss_spec_of; tests/test_fusion6_host.py checks them against the library
LOSSES = {'L2': (0, 0.0, 1.0, 0.0), 'L1': (1, 1.0, 0.0, 0.0), 'Fusion6': (2, 0.7, 0.0, 0.3), 'SSIM': (3, 0.0, 0.0, 1.0),
          'Fusion1': (4, 0.0, 0.3, 0.7), 'Fusion5': (8, 0.0, 0.7, 0.3), 'Fusion7': (9, 0.3, 0.7, 0.0), 'Fusion8': (10, 0.5, 0.5, 0.0),
          'Fusion9': (11, 0.9, 0.0, 0.1), 'Fusion10': (12, 0.7, 0.0, 0.3)}


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def flat_planes(P, H, W):
    p, t = R.flat_pair(-(-P // 3), H, W)
    return p.reshape(-1, H, W)[:P].contiguous(), t.reshape(-1, H, W)[:P].contiguous()


def tied_plane(P):
    return min(1, P - 1)


def tied_mask(P, H, W):
    """[P][H][W] bool: the checkerboard of plane tied_plane(P) on which tied_pair sets p = t"""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    m = torch.zeros(P, H, W, dtype=torch.bool)
    m[tied_plane(P)] = (yy + xx) % 2 == 0
    return m


def tied_pair(P, H, W):
    """planes_pair with p set equal to t on a checkerboard of one plane: d = 0 there, so sign(d) = 0 and the L1 pixel term is 0"""
    p, t = R.planes_pair(P, H, W)
    p = torch.where(tied_mask(P, H, W), t, p)
    return p.contiguous(), t.contiguous()


PAIRS = {'pair': R.planes_pair, 'flat': flat_planes, 'tied': tied_pair}


# ---- the reference -----------------------------------------------------------------------------------------------------------
def target_maps(t32, dtype, drop=None):
    """G*t, G*t^2 [P][H-10][W-10] of planes t [P][H][W].  drop (MUTANT): 'col' / 'row' -- the weakest tap missing in the last valid
    column / row."""
    t, w = t32.to(dtype), R.win(dtype)
    out = [R._filt(t, w, w), R._filt(t * t, w, w)]
    if drop:
        wd = w.clone()
        wd[-1] = 0
        for k, x in enumerate((t, t * t)):
            if drop == 'col':
                out[k] = torch.cat([out[k][:, :, :-1], R._filt(x[:, :, -11:], w, wd)], 2)
            else:
                out[k] = torch.cat([out[k][:, :-1], R._filt(x[:, -11:], wd, w)], 1)
    return out[0], out[1]


def tstats_ref(frames32, dtype, drop=None):
    """[n][2][Ch][H-10][W-10] of a frame table [n][Ch][H][W]: the layout of orn_loss_target_stats"""
    n, Ch, H, W = frames32.shape
    mu, tt = target_maps(frames32.reshape(n * Ch, H, W), dtype, drop)
    return torch.stack([mu.view(n, Ch, H - 10, W - 10), tt.view(n, Ch, H - 10, W - 10)], 1)


def image_tile_sums(m, H, W):
    """[P][tiles] sums of a valid map m [P][H-10][W-10] over the 16x64 tiles of the IMAGE, tile rows first"""
    P, h, w = m.shape
    nh, nw = -(-H // TH), -(-W // TW)
    z = m.new_zeros(P, nh * TH, nw * TW)
    z[:, :h, :w] = m
    return z.view(P, nh, TH, nw, TW).sum((2, 4)).reshape(P, nh * nw)


def ssim_map(p, t, w, maps_fn=R.maps):
    return maps_fn(p, t, w)[0]


def ssim_map_from(p, t, mu, tt, w):
    """The SSIM map with the target's two filtered maps handed in (TC_READ): mu = G*t, tt = G*t^2"""
    m, qq, rr = R._filt(p, w, w), R._filt(p * p, w, w), R._filt(p * t, w, w)
    sp, st, spt = qq - m * m, tt - mu * mu, rr - m * mu
    return (2 * m * mu + C1) / (m * m + mu * mu + C1) * ((2 * spt + C2) / (sp + st + C2))


def term_grads(p32, t32, dtype, map_of=None):
    """by autograd: d mean|d| / dp, d mse / dp, d (1 - mean ssim) / dp [P][H][W], and the SSIM map.  map_of(p, t, w): a mutant's map"""
    p, t = p32.to(dtype, copy=True).requires_grad_(True), t32.to(dtype)      # (a copy: the case's own input stays a plain tensor)
    d = p - t
    g1, = torch.autograd.grad(d.abs().mean(), p, retain_graph=True)
    g2, = torch.autograd.grad((d * d).mean(), p)
    s = (map_of or ssim_map)(p, t, R.win(dtype))
    gs, = torch.autograd.grad(1 - s.mean(), p)
    return dict(l1=g1, l2=g2, struct=gs, map=s.detach())


def combine(terms, loss, scale=1.0):
    _, w1, w2, ws = LOSSES[loss]
    g = None
    for wt, name in ((w1, 'l1'), (w2, 'l2'), (ws, 'struct')):
        if wt:
            g = wt * terms[name] if g is None else g + wt * terms[name]
    return g * scale


def _make_case(p, t):
    P, H, W = p.shape
    ref = {}
    for dt in (F64, F32):
        r = term_grads(p, t, dt)
        r['part_ssim'] = image_tile_sums(r['map'], H, W)
        r['part_l1'] = R.pixel_parts(p, t, dt)
        ref[dt] = r
    return dict(p=p, t=t, P=P, H=H, W=W, ref=ref)


_CASES = {}


def case(kind, P, H, W):
    """Inputs and both references at one (input kind, planes, shape), computed once and never modified"""
    key = (kind, P, H, W)
    if key not in _CASES:
        _CASES[key] = _make_case(*PAIRS[kind](P, H, W))
    return _CASES[key]


def dpred_ref(cs, loss, dtype, scale=1.0):
    return combine(cs['ref'][dtype], loss, scale)


_TABLES = {}


def table_case(H, W):
    """A 3-frame, 3-channel table (every frame its own noise) with a prediction per frame: frames [3][3][H][W], the table of target
    maps per dtype, and a case per frame"""
    if (H, W) not in _TABLES:
        p, t = R.make_pair(3, H, W)
        _TABLES[H, W] = dict(frames=t, pred=p, tstats={dt: tstats_ref(t, dt) for dt in (F64, F32)},
                             frame={k: _make_case(p[k], t[k]) for k in (0, 2)})
    return _TABLES[H, W]


# ---- the finalize stage and k_loss_grad: closed forms in double --------------------------------------------------------------
def scales(loss, P, H, W, loss_scale=1.0):
    """g_l1, g_l2, g_ssim as orn_launch_loss forms them: in double, then rounded to fp32"""
    _, w1, w2, ws = LOSSES[loss]
    n, nmap = float(P) * H * W, float(P) * max(H - 10, 0) * max(W - 10, 0)
    ls = float(np.float32(loss_scale))
    return (float(np.float32(w1 * ls / n)), float(np.float32(2.0 * w2 * ls / n)), float(np.float32(ws * ls / nmap)) if nmap else 0.0)


def stats_from_partials(part_ssim, part_l1, loss, P, H, W, loss_scale=1.0):
    """stats[0..4] = {loss * loss_scale, L1, MSE, s, PSNR} by the documented formula of orn_loss_finalize_block in double from the
    kernel's own tile partials (part_ssim None: a loss without the SSIM term, s = 0); the weights rounded to fp32 as the kernel
    holds them"""
    _, w1, w2, ws = (float(np.float32(v)) for v in LOSSES[loss])
    n, nmap = float(P) * H * W, float(P) * (H - 10) * (W - 10)
    pl = R._np(part_l1)
    l1, mse = pl[..., 0].sum() / n, pl[..., 1].sum() / n
    ss = R._np(part_ssim).sum() / nmap if part_ssim is not None else 0.0
    val = {'L2': mse, 'L1': l1}.get(loss, w1 * l1 + w2 * mse + ws * (1.0 - ss))
    return np.array([val * float(np.float32(loss_scale)), l1, mse, ss, -10.0 * np.log10(mse)])


def loss_grad_ref(p32, t32, loss, loss_scale=1.0):
    """dpred of k_loss_grad by its formula in double with the launcher's fp32-rounded scales: g_l2 d + g_l1 sign(d)"""
    P, H, W = p32.shape
    g_l1, g_l2, _ = scales(loss, P, H, W, loss_scale)
    d = p32.double() - t32.double()
    return g_l2 * d + g_l1 * torch.sign(d)


# ---- mutants (float64) -------------------------------------------------------------------------------------------------------
def part_ssim_row17_twice(smap, H, W):
    """MUTANT: the map row at tile-local row 17 of the 26-row column pass (valid-map row 16 th + 7) counted twice in its tile's sum"""
    extra = torch.zeros_like(smap)
    rows = list(range(7, smap.shape[1], TH))
    extra[:, rows] = smap[:, rows]
    return image_tile_sums(smap, H, W) + image_tile_sums(extra, H, W)


def struct_grad_without_apron(p32, t32):
    """MUTANT of d (1 - mean ssim) / dp: every image tile forms its gradient from its OWN part of the derivative maps alone (the
    derivative maps zeroed outside it), so nothing arrives from the neighbours' apron"""
    p, t = p32.double().requires_grad_(True), t32.double()
    P, H, W = p.shape
    s = ssim_map(p, t, R.win(F64))
    g = torch.zeros_like(p)
    for y0 in range(0, H, TH):
        for x0 in range(0, W, TW):
            own = s[:, y0:y0 + TH, x0:x0 + TW]
            if own.numel():
                gi, = torch.autograd.grad(own.sum(), p, retain_graph=True)
                g[:, y0:y0 + TH, x0:x0 + TW] = gi[:, y0:y0 + TH, x0:x0 + TW]
    return -g / s[0].numel() / P


def struct_grad_from(p32, t32, mu, tt):
    """d (1 - mean ssim) / dp in float64 with the target's filtered maps handed in (MUTANTS: another frame's, or the two exchanged)"""
    p, t = p32.double().requires_grad_(True), t32.double()
    s = ssim_map_from(p, t, mu.double(), tt.double(), R.win(F64))
    g, = torch.autograd.grad(1 - s.mean(), p)
    return g


def with_struct(terms, struct):
    out = dict(terms)
    out['struct'] = struct
    return out
