"""Every kernel form of the fp32 block path and the fp32 engine's fused head backward, elementwise against a float64 reference.

orn_launch_conv3x3_f32 and orn_launch_conv_bwd_f32 (orn_conv_f32.hip) pick a kernel form from the shape: 2-row or 8-row tiles, the
input channels split over partial slabs or not, a 32-channel tail launch, the first or the second wgrad form with one or several K
tiles per split, one of two row reductions.  The 16-bit engines run them for every block they keep unfused, the fp32 engine for
all, and the 16-bit modes are credited against it.  The cases of conv32_cases.py reach every form through the public C ABI and the
test entry points of include/orn_debug.h; each case first asserts through orn_debug_conv_f32_plan that it reaches the form it names
(tests/test_conv32_plan_host.py proves the same table without a GPU).  k_head_bwd_fused_f32, k_head_partials_finish and the
z-input head forward run on their own here, through orn_debug_conv_bwd_f32_head and orn_debug_head_fwd_z.

Reference: float64 on the CPU (torch conv2d, pixel_shuffle, the conv's autograd formulas) from the identical fp32 inputs; it uses no
liborn function.  Every element of every output is compared, never a norm.  With A the same linear operation applied in float64
to the absolute values of the operands:
    z, dx, dwf, dbf, head dw / db     |k - r| <= c * A         (dy is internal: da * SiLU'(z), or (W^T du) * SiLU'(z) with
                                                                du = dout * act'(out), in float64; A from |dy|, |W|^T |du|, ...)
    a                                 |a - SiLU64(z of the kernel)| <= n fp32 ulps of the result
    head output of the z-input form   |k - r| <= c * A_u * max|act'| + n ulps,  n = 4 fixed beforehand: expf / tanhf are good to
                                      2 ulps, the divide or the (t + 1) / 2 behind them adds at most 2 more roundings
c and n are per form, at most 3x the worst ratio measured on an MI355X (C_TOL, N_TOL below hold both figures).  Every measured c is
below 2^-16, as for the 16-bit forms with the same fp32 accumulators (test_gpu_conv16_forms.py): the largest, 6.1e-7, is z of the stride-2 forward on 8-row tiles.

Contract checks on every case: the backward's workspace is exactly *_ws_bytes long, NaN-filled before every call (every slab,
partial row and dy element that is read must have been written) with a sentinel guard behind it; every output is NaN-seeded, comes
back fully finite and sits in front of a sentinel guard that stays untouched; every input has NaN behind it (nothing past the
end of an input may reach an output: a channel mask dropped from a staging load shows here); every call runs twice and is bit-identical (the
reductions are in fixed order); dx == NULL leaves dwf and dbf bit-equal.  The module runs in about 5 s on one MI355X.
"""
from ctypes import c_size_t, c_void_p

import pytest
import torch
import torch.nn.functional as F

import conv32_cases as K

pytestmark = pytest.mark.gpu

SENT = 7.0                     # finite sentinel
GUARD = 1024                   # elements of sentinel behind every output and workspace
NAN = float('nan')
INVESTIGATE = 2.0 ** -16       # a measured c above this is a finding, not a constant to record

# c of the bounds above per form: at most 3x the worst ratio measured on an MI355X (the comment gives it)
C_TOL = {
    'fwd_small_s2':      1.2e-6,     # 4.10e-7
    'fwd_small_gen':     8.1e-7,     # 2.70e-7
    'fwd_8row_s2':       1.8e-6,     # 6.15e-7
    'fwd_8row_gen':      1.1e-6,     # 3.98e-7
    'dgrad_small':       7.3e-7,     # 2.46e-7
    'dgrad_small_split': 6.5e-7,     # 2.19e-7
    'dgrad_8row_split':  1.3e-6,     # 4.36e-7
    'dgrad_8row_tail':   1.4e-6,     # 4.81e-7
    'dgrad_8row_plain':  1.1e-6,     # 3.89e-7
    'wgrad1':            8.2e-7,     # 2.77e-7
    'wgrad2':            5.9e-7,     # 1.97e-7
    'dbias':             2.2e-7,     # 7.65e-8
    'head_dx':           1.2e-6,     # 4.19e-7
    'head_dwf':          3.6e-7,     # 1.20e-7
    'head_dbf':          1.5e-7,     # 5.31e-8
    'head_dw':           1.3e-7,     # 4.60e-8
    'head_db':           1.1e-7,     # 3.90e-8
    'head_chain':        2.3e-7,     # 7.72e-8
    'headz':             1.5e-7,     # 5.32e-8
}
# n (fp32 ulps) of the SiLU epilogue per forward form, same rule; headz: fixed beforehand (docstring)
N_TOL = {
    'fwd_small_s2':      7.4,        # 2.50
    'fwd_small_gen':     6.5,        # 2.18
    'fwd_8row_s2':       7.3,        # 2.44
    'fwd_8row_gen':      7.2,        # 2.42
    'headz':             4.0,        # not measured: see above
}
WORST = {}


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_conv_f32_plan', 'orn_debug_conv_fwd_f32', 'orn_debug_head_fwd_z', 'orn_debug_conv_bwd_f32_head_ws_bytes',
                 'orn_debug_conv_bwd_f32_head'):
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


def _ids(cases):
    return ['x'.join(map(str, c[0])) for c in cases]


def _silu(z):
    return z * torch.sigmoid(z)


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _ulp32(r):
    e = torch.floor(torch.log2(r.abs().clamp_min(1e-300)))
    return torch.exp2(e.clamp_min(-126) - 23)


def _guarded(shape, fill=NAN):
    """Output of `shape`, filled with `fill`, with GUARD elements of sentinel behind: (whole buffer, view)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + GUARD,), SENT, device='cuda')
    buf[:n] = fill
    return buf, buf[:n].view(shape)


def _finite(t, what):
    assert bool(torch.isfinite(t).all()), f'{what}: {int((~torch.isfinite(t)).sum())} of {t.numel()} outputs not finite (NaN-seeded: not written, or NaN read)'


def _guard_ok(buf, what):
    g = buf[-GUARD:]
    assert bool((g == SENT).all()), f'{what}: {int((g != SENT).sum())} guard elements behind it were written'


def _slack(t, n=4096):
    """The input t with n elements of NaN behind it: nothing past the end of an input may reach an output."""
    buf = torch.full((t.numel() + n,), NAN, device='cuda')
    buf[:t.numel()] = t.flatten()
    return buf[:t.numel()].view(t.shape)


def _rand(shape, gen, chan_scale, dim=1):
    """Seeded, not symmetric (a positive mean), a different scale per channel (dimension `dim`)."""
    sh = [1] * len(shape)
    sh[dim] = shape[dim]
    return (torch.randn(shape, generator=gen, device='cuda') + 0.25) * chan_scale.view(sh)


def _scales(n, gen, lo=-1.5, hi=1.5):
    return torch.exp2(torch.rand(n, generator=gen, device='cuda') * (hi - lo) + lo)


def _weights(O, C, gen):
    wf = (torch.randn(O, C, 3, 3, generator=gen, device='cuda') + 0.2) / (9 * C) ** 0.5
    wf = wf * _scales(O, gen, -1, 1)[:, None, None, None] * _scales(C, gen, -1, 1)[None, :, None, None]
    return wf.contiguous(), torch.randn(O, generator=gen, device='cuda') * 0.3


def _record(form, ratio, what):
    WORST[form] = max(WORST.get(form, 0.0), ratio)
    print(f'RATIO {form} {what} {ratio:.3e}')


def _fail(k, r, bad, what):
    i = int(torch.nonzero(bad.flatten())[0])
    raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at flat index {i} '
                         f'(shape {tuple(bad.shape)}): kernel {float(k.flatten()[i])!r} reference {float(r.flatten()[i])!r}')


def _check(k, r, A, form, what):
    """fp32 output k (every element) against the fp64 reference r: |k - r| <= c * A."""
    k = k.detach().double().cpu()
    assert k.shape == r.shape, (k.shape, r.shape)
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    _record(form, float((d / A.clamp_min(1e-300)).max()), what)
    bad = d > C_TOL[form] * A
    if bool(bad.any()):
        _fail(k, r, bad, what)


def _check_ulps(k, r, form, what, extra=None):
    """|k - r| <= n fp32 ulps of r (+ extra)."""
    k = k.detach().double().cpu()
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    u = _ulp32(r)
    if extra is None:
        _record(form + '/ulps', float((d / u).max()), what)
        bad = d > N_TOL[form] * u
    else:
        A = extra
        _record(form, float(((d - N_TOL[form] * u).clamp_min(0) / A.clamp_min(1e-300)).max()), what)
        _record(form + '/ulps', float((d / u).max()), what + ' (all of the error as ulps)')
        bad = d > C_TOL[form] * A + N_TOL[form] * u
    if bool(bad.any()):
        _fail(k, r, bad, what)


def _assert_plan(L, shape, want, what):
    p = K.plan(L, *shape[:5])
    got = {k: p[k] for k in want}
    assert got == want, f'{shape}: no longer reaches "{what}": plan {p}'
    return p


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _fwd_inputs(shape, seed):
    B, C, O, H, W, s = shape
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = _slack(_rand((B, C, H, W), gen, _scales(C, gen)), 8 * H * W + 4096)       # (a whole chunk of 8 channels)
    wf, bf = _weights(O, C, gen)
    return x, _slack(wf), _slack(bf)


def _fwd_call(L, fn, x, wf, bf, shape, want_z=True, want_a=True):
    B, C, O, H, W, s = shape
    osh = (B, O // (s * s), H * s, W * s)
    zb, z = _guarded(osh) if want_z else (None, None)
    ab, a = _guarded(osh) if want_a else (None, None)
    assert fn(_p(x), _p(wf), _p(bf), B, C, O, H, W, s, _p(z), _p(a), _st()) == 0, _err()
    torch.cuda.synchronize()
    for buf, t, name in ((zb, z, 'z'), (ab, a, 'a')):
        if buf is not None:
            _guard_ok(buf, name)
            _finite(t, name)
    return z, a


def _fwd_form(p, s):
    return ('fwd_small' if p[K.FWD_SMALL] else 'fwd_8row') + ('_s2' if s == 2 else '_gen')


@pytest.mark.parametrize('shape,want,what', K.FWD_CASES, ids=_ids(K.FWD_CASES))
def test_conv32_fwd_form(L, shape, want, what):
    B, C, O, H, W, s = shape
    form = _fwd_form(_assert_plan(L, shape, want, what), s)
    x, wf, bf = _fwd_inputs(shape, seed=sum(shape) * 7919 + O)
    z, a = _fwd_call(L, L.orn_conv3x3_ps_silu_fwd, x, wf, bf, shape)
    z2, a2 = _fwd_call(L, L.orn_conv3x3_ps_silu_fwd, x, wf, bf, shape)
    assert torch.equal(z, z2) and torch.equal(a, a2), 'two runs differ'
    x64, w64, b64 = x.double().cpu(), wf.double().cpu(), bf.double().cpu()
    r = F.pixel_shuffle(F.conv2d(x64, w64, b64, padding=1), s)
    A = F.pixel_shuffle(F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=1), s)
    where = f'{form} {shape}'
    _check(z, r, A, form, 'z ' + where)
    _check_ulps(a, _silu(z.double().cpu()), form, 'a ' + where)


@pytest.mark.parametrize('idx', K.FWD_ONE_OUTPUT, ids=[_ids(K.FWD_CASES)[i] for i in K.FWD_ONE_OUTPUT])
def test_conv32_fwd_one_output(L, idx):
    """The z-only form (a == NULL: the fp32 engine's last block) and the a-only form write the bits of the both-outputs call."""
    shape, want, what = K.FWD_CASES[idx]
    _assert_plan(L, shape, want, what)
    x, wf, bf = _fwd_inputs(shape, seed=sum(shape) * 7919 + shape[2])
    z, a = _fwd_call(L, L.orn_conv3x3_ps_silu_fwd, x, wf, bf, shape)
    z1, none = _fwd_call(L, L.orn_debug_conv_fwd_f32, x, wf, bf, shape, want_a=False)
    assert none is None and torch.equal(z1, z), 'z-only form differs'
    none, a1 = _fwd_call(L, L.orn_debug_conv_fwd_f32, x, wf, bf, shape, want_z=False)
    assert none is None and torch.equal(a1, a), 'a-only form differs'
    z2, a2 = _fwd_call(L, L.orn_debug_conv_fwd_f32, x, wf, bf, shape)
    assert torch.equal(z2, z) and torch.equal(a2, a)
    B, C, O, H, W, s = shape
    assert L.orn_debug_conv_fwd_f32(_p(x), _p(wf), _p(bf), B, C, O, H, W, s, None, None, _st()) == -1 and 'null' in _err()
    assert L.orn_debug_conv_fwd_f32(_p(x), _p(wf), _p(bf), B, C, O - 1, H, W, s, _p(z2), None, _st()) == -1
    torch.cuda.synchronize()
    assert torch.equal(z2, z)


# ---- backward ---------------------------------------------------------------------------------------------------------------
def _conv_bwd_ref(x64, w64, dy, Ady):
    """fp64 dx, dwf, dbf of y = conv2d(x, w, pad 1) for the output gradient dy, and the same sums over absolute values."""
    r = {'dx': torch.nn.grad.conv2d_input(x64.shape, w64, dy, padding=1),
         'dwf': torch.nn.grad.conv2d_weight(x64, w64.shape, dy, padding=1),
         'dbf': dy.sum((0, 2, 3))}
    A = {'dx': torch.nn.grad.conv2d_input(x64.shape, w64.abs(), Ady, padding=1),
         'dwf': torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, Ady, padding=1),
         'dbf': Ady.sum((0, 2, 3))}
    return r, A


def _ws(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    buf = torch.full((nbytes // 4 + GUARD,), SENT, device='cuda')
    return buf, buf[:nbytes // 4]


def _dgrad_form(p):
    if p[K.DG_SMALL]:
        return 'dgrad_small_split' if p[K.DG_NSPLIT] > 1 else 'dgrad_small'
    if p[K.DG_NSPLIT] > 1:
        return 'dgrad_8row_split'
    return 'dgrad_8row_tail' if p[K.DG_L32] else 'dgrad_8row_plain'


def _bwd_call(L, x, wf, z, da, shape, with_dx=True):
    B, C, O, H, W, s = shape
    nbytes = L.orn_conv3x3_ps_silu_bwd_ws_bytes(B, C, O, H, W)
    wsb, ws = _ws(nbytes)
    ws.fill_(NAN)
    xb, dx = _guarded((B, C, H, W)) if with_dx else (None, None)
    wb, dwf = _guarded((O, C, 3, 3))
    bb, dbf = _guarded((O,))
    rc = L.orn_conv3x3_ps_silu_bwd(_p(x), _p(wf), _p(z), _p(da), B, C, O, H, W, s, _p(dx), _p(dwf), _p(dbf), _p(ws), c_size_t(nbytes), _st())
    assert rc == 0, _err()
    torch.cuda.synchronize()
    for buf, t, name in ((wsb, None, 'workspace'), (xb, dx, 'dx'), (wb, dwf, 'dwf'), (bb, dbf, 'dbf')):
        if buf is not None:
            _guard_ok(buf, name)
        if t is not None:
            _finite(t, name)
    return dx, dwf, dbf


@pytest.mark.parametrize('shape,want,what', K.BWD_CASES, ids=_ids(K.BWD_CASES))
def test_conv32_bwd_form(L, shape, want, what):
    B, C, O, H, W, s = shape
    p = _assert_plan(L, shape, want, what)
    dform, wform = _dgrad_form(p), f'wgrad{p[K.WG_FORM]}'
    gen = torch.Generator(device='cuda').manual_seed(sum(shape) * 7919 + O)
    Cn = O // (s * s)
    x = _slack(_rand((B, C, H, W), gen, _scales(C, gen)), 8 * H * W + 4096)
    wf = _slack(_weights(O, C, gen)[0])
    z = _slack(torch.randn(B, Cn, H * s, W * s, generator=gen, device='cuda') * 2 + 0.3)
    da = _slack(_rand((B, Cn, H * s, W * s), gen, _scales(Cn, gen)))
    dx, dwf, dbf = _bwd_call(L, x, wf, z, da, shape)
    dx2, dwf2, dbf2 = _bwd_call(L, x, wf, z, da, shape)
    assert torch.equal(dx, dx2) and torch.equal(dwf, dwf2) and torch.equal(dbf, dbf2), 'two runs differ'
    none, dwf3, dbf3 = _bwd_call(L, x, wf, z, da, shape, with_dx=False)
    assert none is None and torch.equal(dwf, dwf3) and torch.equal(dbf, dbf3), 'dx == NULL changes dwf or dbf'
    z64, da64 = z.double().cpu(), da.double().cpu()
    sg = _silu_grad(z64)
    dy, Ady = F.pixel_unshuffle(da64 * sg, s), F.pixel_unshuffle(da64.abs() * sg.abs(), s)
    r, A = _conv_bwd_ref(x.double().cpu(), wf.double().cpu(), dy, Ady)
    where = f'{shape} S={p[K.WG_S]} nsplit={p[K.DG_NSPLIT]}'
    _check(dx, r['dx'], A['dx'], dform, f'dx {dform} {where}')
    _check(dwf, r['dwf'], A['dwf'], wform, f'dwf {wform} {where}')
    _check(dbf, r['dbf'], A['dbf'], 'dbias', f'dbf rows={p[K.DB_ROWS]} {where}')


def test_conv32_bwd_declines_a_short_workspace(L):
    shape = K.BWD_CASES[0][0]
    B, C, O, H, W, s = shape
    nbytes = L.orn_conv3x3_ps_silu_bwd_ws_bytes(B, C, O, H, W)
    out = torch.full((1 << 16,), SENT, device='cuda')
    rc = L.orn_conv3x3_ps_silu_bwd(_p(out), _p(out), _p(out), _p(out), B, C, O, H, W, s, _p(out), _p(out), _p(out), _p(out),
                                   c_size_t(nbytes - 4), _st())
    assert rc == -2 and 'workspace' in _err(), (rc, _err())
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- fused head backward ----------------------------------------------------------------------------------------------------
def _head_call(L, x, wf, z, hw, out, dout, C, O, H, W, sigmoid, preflip):
    Cn = O // 4
    nbytes = L.orn_debug_conv_bwd_f32_head_ws_bytes(C, O, H, W)
    wsb, ws = _ws(nbytes)
    ws.fill_(NAN)
    bufs = [_guarded((1, C, H, W)), _guarded((O, C, 3, 3)), _guarded((O,)), _guarded((3, Cn)), _guarded((3,))]
    dx, dwf, dbf, dw, db = (v for _, v in bufs)
    rc = L.orn_debug_conv_bwd_f32_head(_p(x), _p(wf), _p(z), _p(hw), _p(out), _p(dout), C, O, H, W, sigmoid, preflip, _p(dx), _p(dwf),
                                       _p(dbf), _p(dw), _p(db), _p(ws), c_size_t(nbytes), _st())
    assert rc == 0, _err()
    torch.cuda.synchronize()
    _guard_ok(wsb, 'workspace')
    for (buf, t), name in zip(bufs, ('dx', 'dwf', 'dbf', 'head dw', 'head db')):
        _guard_ok(buf, name)
        _finite(t, name)
    return dx, dwf, dbf, dw, db


def _unfused_chain(L, x, wf, z, hw, out, dout, C, O, H, W, sigmoid):
    """orn_head_bwd on a = SiLU(z) (float64, rounded once), then orn_conv3x3_ps_silu_bwd on its da."""
    Cn, Hs, Ws = O // 4, 2 * H, 2 * W
    a = _silu(z.double()).float().contiguous()
    nb = L.orn_head_bwd_ws_bytes(1, Cn, Hs, Ws)
    wsb, ws = _ws(nb)
    ws.fill_(NAN)
    da = torch.full((1, Cn, Hs, Ws), NAN, device='cuda')
    dw = torch.full((3, Cn), NAN, device='cuda')
    db = torch.full((3,), NAN, device='cuda')
    rc = L.orn_head_bwd(_p(a), _p(hw), _p(out), _p(dout), 1, Cn, Hs, Ws, sigmoid, _p(da), _p(dw), _p(db), _p(ws), c_size_t(nb), _st())
    assert rc == 0, _err()
    torch.cuda.synchronize()
    _guard_ok(wsb, 'head_bwd workspace')
    dx, dwf, dbf = _bwd_call(L, x, wf, z, da, (1, C, O, H, W, 2))
    return dx, dwf, dbf, dw, db


@pytest.mark.parametrize('sigmoid', [0, 1], ids=['tanh', 'sigmoid'])
@pytest.mark.parametrize('hw,blocks,what', K.HEAD_HW, ids=[f'{h}x{w}' for (h, w), _, _ in K.HEAD_HW])
@pytest.mark.parametrize('Cn', K.HEAD_CN)
def test_conv32_fused_head_bwd(L, Cn, hw, blocks, what, sigmoid):
    (H, W), C, O = hw, K.HEAD_C, 4 * Cn
    p = _assert_plan(L, (1, C, O, H, W), {K.HDB_ROWS: blocks}, what)
    gen = torch.Generator(device='cuda').manual_seed(H * 7919 + W * 31 + Cn * 3 + sigmoid)
    Hs, Ws = 2 * H, 2 * W
    x = _slack(_rand((1, C, H, W), gen, _scales(C, gen)), 8 * H * W + 4096)
    wf = _slack(_weights(O, C, gen)[0])
    z = _slack(torch.randn(1, Cn, Hs, Ws, generator=gen, device='cuda') * 2 + 0.3)
    hw_ = _slack((torch.randn(3, Cn, generator=gen, device='cuda') + 0.2) * _scales(Cn, gen, -1, 1)[None, :])
    u = torch.randn(3, Hs, Ws, generator=gen, device='cuda') * 1.5 + 0.2
    out = _slack(torch.sigmoid(u) if sigmoid else (torch.tanh(u) + 1) * 0.5)
    dout = _slack(_rand((3, Hs, Ws), gen, _scales(3, gen), dim=0))
    args = (L, x, wf, z, hw_, out, dout, C, O, H, W, sigmoid)
    got = _head_call(*args, 0)
    again = _head_call(*args, 0)
    flipped = _head_call(*args, 1)
    for g, g2, g3, name in zip(got, again, flipped, ('dx', 'dwf', 'dbf', 'head dw', 'head db')):
        assert torch.equal(g, g2), f'{name}: two runs differ'
        assert torch.equal(g, g3), f'{name}: preflip changes the result'
    # float64 reference
    z64, w64, o64, g64 = z.double().cpu(), hw_.double().cpu(), out.double().cpu(), dout.double().cpu()
    du = g64 * (o64 * (1 - o64) * (1 if sigmoid else 2))                        # [3][Hs][Ws]
    da, Ada = torch.einsum('kn,khw->nhw', w64, du)[None], torch.einsum('kn,khw->nhw', w64.abs(), du.abs())[None]
    sg = _silu_grad(z64)
    dy, Ady = F.pixel_unshuffle(da * sg, 2), F.pixel_unshuffle(Ada * sg.abs(), 2)
    r, A = _conv_bwd_ref(x.double().cpu(), wf.double().cpu(), dy, Ady)
    a64 = _silu(z64)[0]
    r['dw'], A['dw'] = torch.einsum('khw,nhw->kn', du, a64), torch.einsum('khw,nhw->kn', du.abs(), a64.abs())
    r['db'], A['db'] = du.sum((1, 2)), du.abs().sum((1, 2))
    where = f'Cn={Cn} {H}x{W} {"sigmoid" if sigmoid else "tanh"} blocks={blocks} S={p[K.WG_S]}'
    names = ('dx', 'dwf', 'dbf', 'dw', 'db')
    for k, name in zip(got, names):
        _check(k, r[name], A[name], 'head_' + name, f'{name} fused {where}')
    # the unfused chain computes the same five tensors: same rule, the chain's result in the reference's place
    chain = _unfused_chain(*args)
    for k, c, name in zip(got, chain, names):
        _check(k, c.double().cpu(), A[name], 'head_chain', f'{name} fused vs unfused {where}')


def test_conv32_fused_head_declines_bad_arguments(L):
    C, O, H, W = 6, 12, 9, 25
    nbytes = L.orn_debug_conv_bwd_f32_head_ws_bytes(C, O, H, W)
    buf = torch.full((1 << 18,), SENT, device='cuda')
    b = _p(buf)

    def call(C=C, O=O, H=H, W=W, x=b, ws=b, n=nbytes):
        return L.orn_debug_conv_bwd_f32_head(x, b, b, b, b, b, C, O, H, W, 0, 1, b, b, b, b, b, ws, c_size_t(n), _st())
    assert call(n=nbytes - 4) == -2 and 'workspace' in _err(), _err()
    for kw in (dict(x=None), dict(ws=None), dict(O=10), dict(C=0), dict(H=0), dict(O=4 * 513, n=1 << 20)):
        assert call(**kw) == -1, kw
        assert 'debug_conv_bwd_f32_head' in _err(), _err()
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- z-input head forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigmoid', [0, 1], ids=['tanh', 'sigmoid'])
@pytest.mark.parametrize('shape,what', K.HEADZ_CASES, ids=_ids(K.HEADZ_CASES))
def test_conv32_head_fwd_on_z(L, shape, what, sigmoid):
    """k_head_fwd<V, ZIN = true> forms SiLU(z) itself: bit for bit the output of orn_head_fwd on the a of the same conv forward."""
    B, C, Cn, H, W, s = shape
    Hs, Ws = H * s, W * s
    assert (Hs * Ws % 4 == 0) == what.startswith('V = 4')
    conv = (B, C, Cn * s * s, H, W, s)
    x, wf, bf = _fwd_inputs(conv, seed=sum(shape) * 7919 + sigmoid)
    z, a = _fwd_call(L, L.orn_conv3x3_ps_silu_fwd, x, wf, bf, conv)
    gen = torch.Generator(device='cuda').manual_seed(Cn + 5)
    hw_ = _slack((torch.randn(3, Cn, generator=gen, device='cuda') + 0.2) * _scales(Cn, gen, -1, 1)[None, :] / Cn ** 0.5)
    hb = _slack(torch.randn(3, generator=gen, device='cuda') * 0.3)
    outs = []
    for fn, src in ((L.orn_head_fwd, a), (L.orn_debug_head_fwd_z, z), (L.orn_debug_head_fwd_z, z)):
        ob, o = _guarded((B, 3, Hs, Ws))
        assert fn(_p(src), _p(hw_), _p(hb), B, Cn, Hs, Ws, sigmoid, _p(o), _st()) == 0, _err()
        torch.cuda.synchronize()
        _guard_ok(ob, 'head output')
        _finite(o, 'head output')
        outs.append(o)
    assert torch.equal(outs[1], outs[2]), 'two runs differ'
    assert torch.equal(outs[0], outs[1]), 'the head on z differs from the head on a = SiLU(z)'
    a64, w64, b64 = _silu(z.double().cpu()), hw_.double().cpu(), hb.double().cpu()
    u = torch.einsum('kn,bnhw->bkhw', w64, a64) + b64[None, :, None, None]
    Au = torch.einsum('kn,bnhw->bkhw', w64.abs(), a64.abs()) + b64.abs()[None, :, None, None]
    r = torch.sigmoid(u) if sigmoid else (torch.tanh(u) + 1) * 0.5
    _check_ulps(outs[1], r, 'headz', f'head on z {shape} {"sigmoid" if sigmoid else "tanh"}', extra=Au * (0.25 if sigmoid else 0.5))
    assert L.orn_debug_head_fwd_z(None, _p(hw_), _p(hb), B, Cn, Hs, Ws, sigmoid, _p(outs[1]), _st()) == -1
    assert L.orn_debug_head_fwd_z(_p(z), _p(hw_), _p(hb), B, 513, Hs, Ws, sigmoid, _p(outs[1]), _st()) == -1


def test_conv32_worst_ratios_are_recorded(L):
    """Runs last: prints the worst ratio per form of this run (the table DESIGN.md quotes); no constant is above 2^-16."""
    for form in sorted(WORST):
        print(f'WORST {form} {WORST[form]:.3e}')
    for form, c in C_TOL.items():
        assert c <= INVESTIGATE, form
