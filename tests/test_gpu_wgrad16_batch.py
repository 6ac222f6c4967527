"""The two weight-gradient launches of every 16-bit training step, run as the engine runs them and compared per element with float64:
k_wgrad_nhwc_bf16_all<ACT> (several layers as one multi-problem launch, the head's dW / db finish and the stem backward's first
kernel as trailing work-groups) and k_wgrad_bf16_reduce_all<ACT> (every layer's slab reduction in grid y, the stem backward's last
kernel as one more y slice), csrc/orn_wgrad_bf16.hip, through orn_debug_wgrad16_step_{bf16,f16} (include/orn_debug.h), which calls
the OrnHalfOps members the engine's fast_weight_grads and side_branch_backward call.

What the per-op tests cannot see and this one pins: the walk over start[] and the two rider ranges behind it; the caller's slab cap
(OrnWgradJob::smax, evaluated once by the launch that writes the slabs and once by the one that reads them); the scale-state path
of the reduction (1 / gs from the device, the non-finite flag); layers of different O sharing one grid x; the stem slice's idle half;
riders behind several hundred wgrad work-groups.

Reference and bound, dwf / dbf: those of test_conv16_wgrad_form (tests/wgrad16_ref.py) -- float64 on the CPU from the identical
16-bit-rounded operands, per element |k - r| <= c * A with A the same sum on absolute values, both divided by gs.  c = C_TOL below:
the per-op module's C_TOL['wgrad'] (the bodies are the same).  WORST_MEASURED holds the worst ratio measured on an MI355X per
build over every case of this module; by the module's rule c is at most 3x that and below 2^-16, so the per-op values stand.  The
worst, 1.29e-7 (bf16) and 1.50e-7 (fp16), is dwf of the 3 x 5 image at 8 slabs (most of them without a K tile), as in the per-op
module.  The capped layer itself (64 x 320 x 128 alone): 4.9e-8 / 4.1e-8 / 7.6e-8 / 6.9e-8 / 7.8e-8 at 8 / 16 / 24 / 32 / 40 slabs
(bf16), 4.8e-8 / 4.7e-8 / 6.8e-8 / 6.4e-8 / 7.3e-8 (fp16); the 720p last block at the engine's cap of 24: 6.9e-8 / 8.6e-8 (dbf).  No
slab count loses more than the uncapped ones do.
Riders: |k - r| <= (L + 2) * 2^-24 * A (+ the allowance for the activation derivative where it multiplies the output), L the
length of the output's summation chain (DESIGN 4.3's rule, nothing measured): head finish ceil(blocks / 256) + 8 (a lane's rows, then
the 8-level tree); stem dw1 / db1 the slab count, dw0 / db0 16 + ceil(Nout / 16).  The swish allowance is test_gpu_stage0.py's; the
gelu one is 2^-21 (1 + |z|) |g|: tests/test_gpu_act_eval.py holds gelu' to 5.9 * 2^-24 (1 + |z|).

Bit identities, on top of the comparison: smax = 0, gs = 1 without a state equals orn_wgrad_nhwc_{bf16,f16} on the same buffers;
the head rider equals the finish launch of orn_debug_head_bwd_*; the stem rider equals orn_debug_stem_bwd_slabs_act; side = 1
equals side = 0; the state form equals the by-value form; two caps that give the same slab count give the same bits; every case runs
twice.  Contract: every output is NaN-seeded between sentinel guards; each job's slab workspace is NaN-seeded, sized by
orn_debug_wgrad16_ws_floats, and keeps the seed's bit pattern behind S * (9 * O * 96 + O) floats (and its guard); dypad carries 128
NaN elements of slack.

Cases (H, W, C, O, s): the smallest that reach each edge -- see the tables below.  Output channels are sampled in the one
product-shape case (360 x 640) only.  The module's 116 tests (both builds) run in 7.4 s on one MI355X, none above 1.1 s (the
product shape's float64 reference).

Mutations of the real source, each built once on a scratch copy and run against this file on an MI355X: the
reduction told smax = 0 while the launch uses the cap fails test_slab_caps at 64 x 320 x 128 and the product shape (4 tests); a
problem decoded eight work-groups off (clamped into its range: the unclamped form writes past the slabs) fails every test with a
job (60); the scale state dropped for the second layer of the reduction, and for the stem jobs, each fail the four non-finite
cases that depend on it.
"""
import itertools
import math
from ctypes import byref, c_float, c_int, c_size_t, c_void_p

import pytest
import torch

import test_gpu_stage0 as S0            # the float64 stem reference (_stem_inputs, _stem_ref) and its SiLU' allowance
from wgrad16_ref import DT, FAST_C, check32, padded, wgrad_channels, wgrad_ref

pytestmark = pytest.mark.gpu

SENT = 7.0
GUARD = 1024
NAN_BITS = 0x7FC00000            # what torch.full(nan) stores: the slab seed
EPS = 2.0 ** -24
SWISH, GELU = 0, 1
HALVES = ('bf16', 'fp16')
SUFFIX = {'bf16': 'bf16', 'fp16': 'f16'}
C_TOL = {'bf16': 3.1e-7, 'fp16': 4.1e-7}           # test_gpu_conv16_forms.C_TOL['wgrad']
WORST_MEASURED = {'bf16': 1.288e-7, 'fp16': 1.503e-7}      # MI355X, this module: 3x these is 3.9e-7 / 4.5e-7, not below C_TOL
WORST = {}

# the jobs of case 1, in the engine's order (largest first): S 16 / 144 work-groups; 9 O tiles / 216; slabs without a K tile / 72;
# ragged O tile with C = 26 / 168
CASE1 = ((26, 320, 96, 384, 2), (9, 33, 96, 1152, 3), (3, 5, 96, 384, 2), (17, 63, 26, 864, 3))
EIGHT = ((7, 97, 48, 96, 1), (3, 5, 96, 384, 2), (33, 97, 96, 128, 2))
GRID = ((7, 97, 48, 96, 1), (13, 37, 26, 384, 2), (9, 33, 96, 1152, 3))          # O = 96 / 384 / 1152, C = 48 / 26 / 96
CAPS = {(64, 320, 96, 128, 2): (0, 7, 8, 16, 24, 32, 40, 48), (90, 160, 96, 384, 2): (0, 24, 40)}
SPLIT = {(64, 320, 128): {0: 24, 7: 24, 8: 8, 16: 16, 24: 24, 32: 32, 40: 40, 48: 40}, (90, 160, 384): {0: 24, 24: 24, 40: 24}}
STEMS = ((32, 15, 1), (33, 4112, 9), (512, 3744, 150))          # (Hd, Nout, nslab), E = 80
E = 80


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    for name in ('orn_debug_wgrad16_step_bf16', 'orn_debug_wgrad16_step_f16', 'orn_debug_wgrad16_split', 'orn_debug_wgrad16_ws_floats'):
        assert hasattr(lib, name), name
    torch.set_num_threads(16)
    return lib


def _lib():
    import orn_amd
    return orn_amd._lib


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _banded(n, fill=float('nan')):
    """(whole buffer, view of n floats): the view holds `fill`, GUARD sentinel floats stand on both sides of it."""
    buf = torch.full((n + 2 * GUARD,), SENT, device='cuda')
    v = buf[GUARD:GUARD + n]
    v.fill_(fill)
    return buf, v


def _bands_ok(buf, what):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    assert bool((g == SENT).all()), f'{what}: {int((g != SENT).sum())} guard elements around the buffer were written'


def _record(half, what, ratio):
    WORST[half] = max(WORST.get(half, 0.0), ratio)
    print(f'RATIO wgrad16_batch {half} {what} {ratio:.3e}')


# ---- operands and references, made once per (build, shape, seed) and never changed ---------------------------------------------
class Job:
    def __init__(self, half, shape, seed):
        self.half, self.shape, self.seed = half, shape, seed
        H, W, C, O, s = shape
        gen = torch.Generator(device='cuda').manual_seed(seed)
        self.xbuf, self.xpad = padded(H, W, FAST_C, C, half, gen)
        self.dbuf, self.dypad = padded(H, W, O, O, half, gen, slack=128)
        self._ref = self._perop = None

    def ref(self):
        if self._ref is None:
            H, W, C, O, s = self.shape
            sel = wgrad_channels(H, W, O, s, self.seed)
            self._ref = (sel,) + wgrad_ref(self.xpad, self.dypad, H, W, C, O, s, sel)
        return self._ref

    def perop(self, L):
        """dwf, dbf bits of orn_wgrad_nhwc_{bf16,f16} on the same buffers."""
        if self._perop is None:
            H, W, C, O, s = self.shape
            slabs = torch.full((L.orn_wgrad_nhwc_bf16_ws_bytes(H, W, O) // 4,), float('nan'), device='cuda')
            dwf, dbf = torch.full((O * C * 9,), float('nan'), device='cuda'), torch.full((O,), float('nan'), device='cuda')
            fn = L.orn_wgrad_nhwc_bf16 if self.half == 'bf16' else L.orn_wgrad_nhwc_f16
            assert fn(_p(self.xpad), _p(self.dypad), H, W, C, O, s, _p(slabs), _p(dwf), _p(dbf), _st()) == 0, _lib().last_error()
            torch.cuda.synchronize()
            self._perop = (dwf.cpu(), dbf.cpu())
        return self._perop


_JOBS = {}


def job(half, shape, seed=0):
    key = (half, shape, seed)
    if key not in _JOBS:
        _JOBS[key] = Job(half, shape, 1000003 * seed + shape[0] * 7919 + shape[1] * 31 + shape[2] + shape[3] + shape[4])
    return _JOBS[key]


class Head:
    """The head finish's partials as the head backward leaves them: [blocks][3 C + 3] from an 8 x 8 blocks image at sp = 1, with the
    dw / db bits of the backward's own finish launch (per-op form) at the same gs."""
    def __init__(self, L, half, C, blocks, gs):
        H, W = 8, 8 * blocks
        assert L.orn_debug_head16_bwd_blocks(H, W) == blocks
        g = torch.Generator().manual_seed(C * 1009 + blocks)
        z = (torch.randn(H * W, C, generator=g) * 1.5).to(DT[half]).cuda()
        w = ((torch.rand(3, C, generator=g) * 2 - 1) / math.sqrt(C)).cuda()
        out = (torch.rand(3, H * W, generator=g) * 0.9 + 0.05).cuda()
        dout = (torch.randn(3, H * W, generator=g) * 0.02 * (min(gs, 1024.0) / gs)).cuda()
        dypad = torch.zeros((H + 2) * (W + 2) * C, dtype=DT[half], device='cuda')
        nb = L.orn_debug_head16_bwd_ws_bytes(C)
        ws = torch.full((nb // 4,), float('nan'), device='cuda')
        dw, db = torch.full((3 * C,), float('nan'), device='cuda'), torch.full((3,), float('nan'), device='cuda')
        fn = getattr(L, f'orn_debug_head_bwd_{SUFFIX[half]}')
        rc = fn(_p(z), _p(w), _p(out), _p(dout), C, H, W, 1, 1, c_float(gs), _p(dypad), _p(dw), _p(db), _p(ws), c_size_t(nb), None, None, 0,
                None, _st())
        assert rc == 0, _lib().last_error()
        torch.cuda.synchronize()
        self.C, self.blocks, self.gs = C, blocks, gs
        self.partial = ws[:blocks * (3 * C + 3)].clone()
        assert bool(torch.isfinite(self.partial).all())
        self.dw, self.db = dw.cpu(), db.cpu()
        p64 = self.partial.double().cpu().view(blocks, 3 * C + 3)
        self.r, self.A = p64.sum(0) / gs, p64.abs().sum(0) / gs
        self.chain = -(-blocks // 256) + 8


_HEADS = {}


def head(L, half, C, blocks, gs=1.0):
    key = (half, C, blocks, gs)
    if key not in _HEADS:
        _HEADS[key] = Head(L, half, C, blocks, gs)
    return _HEADS[key]


def _gelu_grad(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _stem_ref(t, G, AG, act):
    """{output: (r, A, extra)} of the B == 1 stem backward in float64: test_gpu_stage0's reference for swish; the same formulas with
    gelu' and its allowance (module docstring) for gelu."""
    if act == SWISH:
        return S0._stem_ref(t, G, AG)
    embed, w1, pre1, h1, pre2 = (t[k].double().cpu() for k in ('embed', 'w1', 'pre1', 'h1', 'pre2'))
    allow = lambda z: 2.0 ** -21 * (1 + z.abs())
    g2 = _gelu_grad(pre2)
    d2, Ad2, Ed2 = G * g2, AG * g2.abs(), allow(pre2) * G.abs()
    dh1, Adh1 = w1.T @ d2, w1.abs().T @ Ad2
    g1 = _gelu_grad(pre1)
    d1, Ad1, Ed1 = dh1 * g1, Adh1 * g1.abs(), allow(pre1) * dh1.abs()
    return {'db1': (d2, Ad2, Ed2), 'dw1': tuple(torch.outer(v, h1.abs() if i else h1) for i, v in enumerate((d2, Ad2, Ed2))),
            'db0': (d1, Ad1, Ed1), 'dw0': tuple(torch.outer(v, embed.abs() if i else embed) for i, v in enumerate((d1, Ad1, Ed1)))}


class Stem:
    def __init__(self, L, Hd, Nout, nslab, act):
        self.Hd, self.Nout, self.nslab, self.act = Hd, Nout, nslab, act
        self.t = S0._stem_inputs(E, Hd, Nout, nslab, seed=Nout * 31 + Hd * 7 + E + nslab)
        self.d = {k: v.cuda() for k, v in self.t.items()}
        s64 = self.t['slabs'].double()
        self.ref = _stem_ref(self.t, s64.sum(0), s64.abs().sum(0), act)
        self.chain = {'dw1': nslab, 'db1': nslab, 'dw0': 16 + -(-Nout // 16), 'db0': 16 + -(-Nout // 16)}
        self.sizes = {'dw0': Hd * E, 'db0': Hd, 'dw1': Nout * Hd, 'db1': Nout}
        self.ws_bytes = L.orn_stem_bwd_ws_bytes(1, Hd, Nout)
        # the same backward as two launches of its own (orn_debug_stem_bwd_slabs_act)
        out = {k: torch.full((n,), float('nan'), device='cuda') for k, n in self.sizes.items()}
        ws = torch.full((self.ws_bytes // 4,), float('nan'), device='cuda')
        d = self.d
        rc = L.orn_debug_stem_bwd_slabs_act(_p(d['embed']), _p(d['w1']), _p(d['pre1']), _p(d['h1']), _p(d['pre2']), _p(d['slabs']), nslab, E, Hd,
                                            Nout, _p(out['dw0']), _p(out['db0']), _p(out['dw1']), _p(out['db1']), _p(ws), self.ws_bytes, _st(), act)
        assert rc == 0, _lib().last_error()
        torch.cuda.synchronize()
        self.two_launches = {k: v.cpu() for k, v in out.items()}


_STEMS = {}


def stem(L, shape, act=SWISH):
    key = (shape, act)
    if key not in _STEMS:
        _STEMS[key] = Stem(L, *shape, act)
    return _STEMS[key]


# ---- one call of the entry ------------------------------------------------------------------------------------------------------
def run_step(L, half, specs, hd=None, stm=None, gs=1.0, use_state=0, side=0, partial=None, stem_slabs=None, dypads=None):
    """specs: [(Job, smax)].  NaN-seeded guarded outputs and slab workspaces; returns dict(jobs=[(dwf, dbf)], head=(dw, db),
    stem={name: tensor}, flag) on the host after the contract checks.  partial / stem_slabs / dypads[i]: replacement inputs (the
    non-finite cases)."""
    M = _lib()
    n = len(specs)
    arr = (M.Wgrad16Job * max(n, 1))()
    keep = []
    for i, (jb, smax) in enumerate(specs):
        H, W, C, O, s = jb.shape
        nfl = L.orn_debug_wgrad16_ws_floats(H, W, O)
        sbuf, slabs = _banded(nfl)
        wbuf, dwf = _banded(O * C * 9)
        bbuf, dbf = _banded(O)
        dyp = jb.dypad if dypads is None or dypads[i] is None else dypads[i]
        arr[i] = M.Wgrad16Job(jb.xpad.data_ptr(), dyp.data_ptr(), H, W, C, O, s, smax, slabs.data_ptr(), dwf.data_ptr(), dbf.data_ptr())
        keep.append((sbuf, slabs, wbuf, dwf, bbuf, dbf))
    hs = hk = None
    if hd is not None:
        hwbuf, hdw = _banded(3 * hd.C)
        hbbuf, hdb = _banded(3)
        part = hd.partial if partial is None else partial
        hs = M.Wgrad16Head(part.data_ptr(), hd.blocks, hd.C, hdw.data_ptr(), hdb.data_ptr())
        hk = (hwbuf, hdw, hbbuf, hdb)
    ss = sk = None
    if stm is not None:
        sk = {k: _banded(nn) for k, nn in stm.sizes.items()}
        sk['ws'] = _banded(stm.ws_bytes // 4)
        d = stm.d
        sl = d['slabs'] if stem_slabs is None else stem_slabs
        ss = M.Wgrad16Stem(*(d[k].data_ptr() for k in ('embed', 'w1', 'pre1', 'h1', 'pre2')), sl.data_ptr(), stm.nslab, E, stm.Hd, stm.Nout,
                           *(sk[k][1].data_ptr() for k in ('dw0', 'db0', 'dw1', 'db1', 'ws')), stm.ws_bytes)
    flag = c_int(-7)
    fn = getattr(L, f'orn_debug_wgrad16_step_{SUFFIX[half]}')
    rc = fn(n, arr, byref(hs) if hs is not None else None, byref(ss) if ss is not None else None, c_float(gs), use_state, side,
            stm.act if stm is not None else SWISH, byref(flag) if use_state else None, _st())
    assert rc == 0, _lib().last_error()
    torch.cuda.synchronize()
    res = dict(jobs=[], head=None, stem=None, flag=flag.value if use_state else None)
    for (jb, smax), (sbuf, slabs, wbuf, dwf, bbuf, dbf) in zip(specs, keep):
        H, W, C, O, s = jb.shape
        what = f'{jb.shape} smax={smax}'
        _bands_ok(sbuf, 'slabs ' + what)
        _bands_ok(wbuf, 'dwf ' + what)
        _bands_ok(bbuf, 'dbf ' + what)
        used = L.orn_debug_wgrad16_split(H, W, O, smax) * (9 * O * 96 + O)
        assert used <= slabs.numel(), what
        tail = _bits(slabs[used:])
        assert bool((tail == NAN_BITS).all()), f'slabs {what}: {int((tail != NAN_BITS).sum())} floats behind the {used} of its slab count were written'
        assert bool(torch.isnan(jb.dbuf[-128:].float()).all()), 'the slack behind dypad changed'
        res['jobs'].append((dwf.cpu(), dbf.cpu()))
    if hk is not None:
        _bands_ok(hk[0], 'head dw')
        _bands_ok(hk[2], 'head db')
        res['head'] = (hk[1].cpu(), hk[3].cpu())
    if sk is not None:
        for k, (buf, v) in sk.items():
            _bands_ok(buf, 'stem ' + k)
        res['stem'] = {k: sk[k][1].cpu() for k in stm.sizes}
    return res


def same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a['jobs'], b['jobs'])):
        assert torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[1]), _bits(y[1])), f'{what}: job {i} differs'
    if a['head'] is not None:
        assert torch.equal(_bits(a['head'][0]), _bits(b['head'][0])) and torch.equal(_bits(a['head'][1]), _bits(b['head'][1])), f'{what}: head'
    if a['stem'] is not None:
        for k in a['stem']:
            assert torch.equal(_bits(a['stem'][k]), _bits(b['stem'][k])), f'{what}: stem {k}'


def check_job(half, jb, smax, out, gs=1.0, skip_o=None, where=''):
    """dwf / dbf of one job against float64, every element (the sampled channels of the product shape); skip_o: an output channel
    that an injected non-finite element reaches."""
    H, W, C, O, s = jb.shape
    sel, r, A, rb, Ab = jb.ref()
    dwf, dbf = out[0].view(O, C, 9)[sel], out[1]
    keep_w, keep_b = torch.ones(len(sel), dtype=torch.bool), torch.ones(O, dtype=torch.bool)
    if skip_o is not None:
        keep_w, keep_b = sel != skip_o, torch.arange(O) != skip_o
    what = f'{where} {jb.shape} smax={smax}'
    check32(dwf[keep_w], r[keep_w] / gs, A[keep_w] / gs, C_TOL[half], 'dwf ' + what, record=lambda q: _record(half, 'dwf ' + what, q))
    check32(dbf[keep_b], rb[keep_b] / gs, Ab[keep_b] / gs, C_TOL[half], 'dbf ' + what, record=lambda q: _record(half, 'dbf ' + what, q))


def check_perop_bits(L, jb, out, what):
    pw, pb = jb.perop(L)
    assert torch.equal(_bits(out[0]), _bits(pw)), f'{what} {jb.shape}: dwf differs from orn_wgrad_nhwc'
    assert torch.equal(_bits(out[1]), _bits(pb)), f'{what} {jb.shape}: dbf differs from orn_wgrad_nhwc'


def _chain_check(k, r, A, chain, what, extra=None, keep=None):
    k = k.double().reshape(r.shape)
    ex = torch.zeros_like(r) if extra is None else extra
    if keep is not None:
        k, r, A, ex = k[keep], r[keep], A[keep], ex[keep]
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    ratio = float(((d - ex).clamp_min(0) / A.clamp_min(1e-300)).max())
    print(f'RATIO rider {what} {ratio:.3e} (bound {(chain + 2) * EPS:.3e})')
    bad = d > (chain + 2) * EPS * A + ex
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements beyond ({chain} + 2) * 2^-24 * A; worst ratio {ratio:.3e}'


def check_head(hd, out, where='', skip_col=None):
    n = 3 * hd.C + 3
    keep = None if skip_col is None else torch.arange(n) != skip_col
    _chain_check(torch.cat([out[0], out[1]]), hd.r, hd.A, hd.chain, f'head finish C={hd.C} blocks={hd.blocks} gs={hd.gs} {where}', keep=keep)


def check_head_bits(hd, out):
    assert torch.equal(_bits(out[0]), _bits(hd.dw)) and torch.equal(_bits(out[1]), _bits(hd.db)), 'head rider differs from the finish launch'


def check_stem(stm, out, where='', only_rows_but=None):
    """only_rows_but: a row o of the second layer that an injected element reaches -- dw1 / db1 without it, dw0 / db0 not at all."""
    for k in ('dw1', 'db1') + (() if only_rows_but is not None else ('dw0', 'db0')):
        r, A, ex = stm.ref[k]
        keep = None
        if only_rows_but is not None:
            keep = torch.arange(stm.Nout) != only_rows_but
        _chain_check(out[k], r, A, stm.chain[k], f'stem {k} Hd={stm.Hd} Nout={stm.Nout} nslab={stm.nslab} act={stm.act} {where}', extra=ex, keep=keep)


def check_stem_bits(stm, out):
    for k, v in stm.two_launches.items():
        assert torch.equal(_bits(out[k]), _bits(v)), f'stem rider {k} differs from orn_debug_stem_bwd_slabs_act'


def run_case(L, half, specs, hd=None, stm=None, where='', perop=True):
    """A clean case at gs = 1 without a state: twice, side = 1, every output against float64 and against its own launch."""
    a = run_step(L, half, specs, hd, stm)
    same_bits(a, run_step(L, half, specs, hd, stm), where + ' two runs')
    same_bits(a, run_step(L, half, specs, hd, stm, side=1), where + ' side = 1')
    for (jb, smax), out in zip(specs, a['jobs']):
        check_job(half, jb, smax, out, where=where)
        if perop and smax == 0:
            check_perop_bits(L, jb, out, where)
    if hd is not None:
        check_head(hd, a['head'], where)
        check_head_bits(hd, a['head'])
    if stm is not None:
        check_stem(stm, a['stem'], where)
        check_stem_bits(stm, a['stem'])
    return a


# ---- 1. decode across problems ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['engine', 'reverse'])
@pytest.mark.parametrize('half', HALVES)
def test_decode_across_problems(L, half, order):
    shapes = CASE1 if order == 'engine' else CASE1[::-1]
    run_case(L, half, [(job(half, sh), 0) for sh in shapes], where=f'case 1 {order}')


# ---- 2. one to eight problems ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 8])
@pytest.mark.parametrize('half', HALVES)
def test_one_to_eight_problems(L, half, n):
    specs = [(job(half, EIGHT[i % 3], seed=i), 0) for i in range(n)]
    assert len({id(j) for j, _ in specs}) == n
    run_case(L, half, specs, where=f'case 2 n={n}')


# ---- 3. slab caps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(CAPS), ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('half', HALVES)
def test_slab_caps(L, half, shape):
    jb = job(half, shape)
    before, after = job(half, (3, 5, 96, 384, 2), seed=11), job(half, (7, 97, 48, 96, 1), seed=12)
    by_S = {}
    for smax in CAPS[shape]:
        S = L.orn_debug_wgrad16_split(shape[0], shape[1], shape[3], smax)
        assert S == SPLIT[shape[0], shape[1], shape[3]][smax], (shape, smax, S)
        alone = run_step(L, half, [(jb, smax)])
        same_bits(alone, run_step(L, half, [(jb, smax)]), f'cap {smax} two runs')
        check_job(half, jb, smax, alone['jobs'][0], where=f'case 3 alone S={S}')
        three = run_step(L, half, [(before, 0), (jb, smax), (after, 0)])
        same_bits(three, run_step(L, half, [(before, 0), (jb, smax), (after, 0)]), f'cap {smax} of three, two runs')
        for (j, c), out in zip([(before, 0), (jb, smax), (after, 0)], three['jobs']):
            check_job(half, j, c, out, where=f'case 3 of three S={S}')
        for j, out in ((before, three['jobs'][0]), (after, three['jobs'][2])):
            check_perop_bits(L, j, out, f'beside cap {smax}')
        assert torch.equal(_bits(three['jobs'][1][0]), _bits(alone['jobs'][0][0])) and torch.equal(_bits(three['jobs'][1][1]), _bits(alone['jobs'][0][1])), \
            f'cap {smax}: the job between two others differs from the job alone'
        if S in by_S:
            same_bits(by_S[S][1], alone, f'caps {by_S[S][0]} and {smax} both give {S} slabs')
        else:
            by_S[S] = (smax, alone)
    check_perop_bits(L, jb, by_S[SPLIT[shape[0], shape[1], shape[3]][0]][1]['jobs'][0], 'smax = 0')


@pytest.mark.parametrize('half', HALVES)
def test_slab_cap_product_shape(L, half):
    """The engine's own capped layer: the last block of the 720p product at ORN_LAST_SMAX = 24 (40 slabs without the cap); output
    channels sampled as test_conv16_wgrad_form samples them."""
    shape = (360, 640, 96, 384, 2)
    assert L.orn_debug_wgrad16_split(360, 640, 384, 24) == 24 and L.orn_debug_wgrad16_split(360, 640, 384, 0) == 40
    jb = Job(half, shape, 360 * 7919 + 640 * 31 + 96 + 384 + 2)             # (not cached: 180 MB of operands)
    a = run_step(L, half, [(jb, 24)])
    same_bits(a, run_step(L, half, [(jb, 24)]), 'product shape, two runs')
    check_job(half, jb, 24, a['jobs'][0], where='case 3 product S=24')


# ---- 4. reduction grid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', list(itertools.permutations(range(3))), ids=lambda o: ''.join(map(str, o)))
@pytest.mark.parametrize('half', HALVES)
def test_reduction_grid(L, half, order):
    run_case(L, half, [(job(half, GRID[i]), 0) for i in order], where=f'case 4 order {order}')


# ---- 5. riders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 255, 256, 257, 512])
@pytest.mark.parametrize('C', [32, 96, 128])
@pytest.mark.parametrize('half', HALVES)
def test_head_rider_alone(L, half, C, blocks):
    run_case(L, half, [], hd=head(L, half, C, blocks), where='head alone')


@pytest.mark.parametrize('act', [SWISH, GELU])
@pytest.mark.parametrize('shape', STEMS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('half', HALVES)
def test_stem_rider_alone(L, half, shape, act):
    run_case(L, half, [], stm=stem(L, shape, act), where='stem alone')


@pytest.mark.parametrize('act', [SWISH, GELU])
@pytest.mark.parametrize('shape', STEMS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('half', HALVES)
def test_riders_together_without_jobs(L, half, shape, act):
    run_case(L, half, [], hd=head(L, half, 96, 257), stm=stem(L, shape, act), where='both riders, n = 0')


@pytest.mark.parametrize('act', [SWISH, GELU])
@pytest.mark.parametrize('shape', STEMS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('half', HALVES)
def test_riders_behind_jobs(L, half, shape, act):
    """Both riders behind the 600 work-groups of case 1; the stem slice of the reduction at ceil(Hd / 2) * 256 = 4096 .. 65536 threads
    beside layers of 331776 .. 995328: far below the grid that the layers size."""
    run_case(L, half, [(job(half, sh), 0) for sh in CASE1], hd=head(L, half, 96, 512), stm=stem(L, shape, act), where='riders behind case 1')


@pytest.mark.parametrize('act', [SWISH, GELU])
@pytest.mark.parametrize('half', HALVES)
def test_stem_slice_sizes_the_reduction_grid(L, half, act):
    """ceil(512 / 2) * 256 = 65536 threads of the stem slice against a layer of 9 * 32 * 96 = 27648: grid x comes from the stem, and
    the layer's work-groups beyond its own size return early."""
    run_case(L, half, [(job(half, (3, 5, 96, 32, 2)), 0)], stm=stem(L, STEMS[2], act), where='stem sizes grid x')


# ---- 6. scale state --------------------------------------------------------------------------------------------------------------
THREE = ((7, 97, 48, 96, 1), (33, 97, 96, 128, 2), (3, 5, 96, 384, 2))


@pytest.mark.parametrize('gs', [1.0, 2.0 ** 10, 2.0 ** 20])
@pytest.mark.parametrize('half', HALVES)
def test_scale_state(L, half, gs):
    specs = [(job(half, sh, seed=20 + i), 0) for i, sh in enumerate(THREE)]
    hd, stm = head(L, half, 96, 257, gs), stem(L, STEMS[1])
    a = run_step(L, half, specs, hd, stm, gs=gs, use_state=1)
    assert a['flag'] == 0
    same_bits(a, run_step(L, half, specs, hd, stm, gs=gs, use_state=1), 'state form, two runs')
    same_bits(a, run_step(L, half, specs, hd, stm, gs=gs, use_state=0), 'state form against 1 / gs by value')
    for (jb, smax), out in zip(specs, a['jobs']):
        check_job(half, jb, smax, out, gs=gs, where=f'case 6 gs={gs}')
        if gs == 1.0:
            check_perop_bits(L, jb, out, 'state form')
    check_head(hd, a['head'], 'state form')
    check_head_bits(hd, a['head'])
    check_stem(stm, a['stem'], 'state form')
    check_stem_bits(stm, a['stem'])


@pytest.mark.parametrize('value', [float('inf'), float('nan')], ids=['inf', 'nan'])
@pytest.mark.parametrize('where', ['dypad', 'partial', 'stem'])
@pytest.mark.parametrize('half', HALVES)
def test_nonfinite_raises_the_flag(L, half, where, value):
    """One bad element in the middle job's dypad, in the head partials or in a dy slab of the stem raises the flag of the scale state;
    every output it does not reach is still within bound.  Without a state the same inputs run and return 0."""
    gs = 2.0 ** 10
    specs = [(job(half, sh, seed=20 + i), 0) for i, sh in enumerate(THREE)]
    hd, stm = head(L, half, 96, 257, gs), stem(L, STEMS[1])
    kw, skip_o, skip_col, skip_row = {}, None, None, None
    if where == 'dypad':
        H, W, C, O, s = THREE[1]
        bad = specs[1][0].dbuf.clone()
        op_bad = 77
        bad[:(H + 2) * (W + 2) * O].view(H + 2, W + 2, O)[1 + H // 2, 1 + W // 2, op_bad] = value
        kw['dypads'] = [None, bad, None]
        Cn, s2 = O // (s * s), s * s
        skip_o = (op_bad % Cn) * s2 + op_bad // Cn              # o of o' = (o % s2) * Cn + o / s2
    elif where == 'partial':
        bad = hd.partial.clone()
        skip_col = 3 * hd.C + 1
        bad.view(hd.blocks, 3 * hd.C + 3)[100, skip_col] = value
        kw['partial'] = bad
    else:
        bad = stm.d['slabs'].clone()
        skip_row = 2000
        bad[4, skip_row] = value
        kw['stem_slabs'] = bad
    a = run_step(L, half, specs, hd, stm, gs=gs, use_state=1, **kw)
    assert a['flag'] == 1, f'a {value} in {where} did not raise the flag'
    b = run_step(L, half, specs, hd, stm, gs=gs, use_state=0, **kw)              # launches and returns 0 (asserted inside)
    for res in (a, b):
        for i, ((jb, smax), out) in enumerate(zip(specs, res['jobs'])):
            check_job(half, jb, smax, out, gs=gs, skip_o=skip_o if i == 1 else None, where=f'{value} in {where}')
        check_head(hd, res['head'], f'{value} in {where}', skip_col=skip_col)
        check_stem(stm, res['stem'], f'{value} in {where}', only_rows_but=skip_row)
    if where == 'dypad':
        O, C = THREE[1][3], THREE[1][2]
        assert not bool(torch.isfinite(a['jobs'][1][1][skip_o])) and not bool(torch.isfinite(a['jobs'][1][0].view(O, C, 9)[skip_o]).any())
    elif where == 'partial':
        assert not bool(torch.isfinite(torch.cat(a['head'])[skip_col]))
    else:
        assert not bool(torch.isfinite(a['stem']['db1'][skip_row])) and not bool(torch.isfinite(a['stem']['db0']).any())


# ---- 7. rejections ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('half', HALVES)
def test_rejections(L, half):
    """Bad arguments return ORN_E_ARG (a short stem workspace ORN_E_WS) with a text and launch nothing: every buffer keeps its
    sentinel, the flag word is not written."""
    M = _lib()
    big16 = torch.full((1 << 22,), SENT, dtype=DT[half], device='cuda')
    bigf = torch.full((1 << 24,), SENT, device='cuda')
    fn = getattr(L, f'orn_debug_wgrad16_step_{SUFFIX[half]}')
    p16, pf = big16.data_ptr(), bigf.data_ptr()

    def mk_job(**kw):
        f = dict(xpad=p16, dypad=p16, H=8, W=8, C=96, O=384, s=2, smax=0, slabs=pf, dwf=pf, dbf=pf)
        f.update(kw)
        return M.Wgrad16Job(*(f[k] for k in ('xpad', 'dypad', 'H', 'W', 'C', 'O', 's', 'smax', 'slabs', 'dwf', 'dbf')))

    def mk_head(**kw):
        f = dict(partial=pf, blocks=4, C=96, dw=pf, db=pf)
        f.update(kw)
        return M.Wgrad16Head(*(f[k] for k in ('partial', 'blocks', 'C', 'dw', 'db')))

    def mk_stem(**kw):
        f = dict(embed=pf, w1=pf, pre1=pf, h1=pf, pre2=pf, dh2_slabs=pf, nslab=2, E=80, Hd=8, Nout=64, dw0=pf, db0=pf, dw1=pf, db1=pf, ws=pf,
                 ws_bytes=L.orn_stem_bwd_ws_bytes(1, 8, 64))
        f.update(kw)
        return M.Wgrad16Stem(*(f[k] for k in ('embed', 'w1', 'pre1', 'h1', 'pre2', 'dh2_slabs', 'nslab', 'E', 'Hd', 'Nout', 'dw0', 'db0', 'dw1',
                                              'db1', 'ws', 'ws_bytes')))

    def call(jobs=(), n=None, hd=None, stm=None, gs=1.0, use_state=0, act=SWISH, flag=None, null_jobs=False):
        arr = (M.Wgrad16Job * max(len(jobs), 1))(*jobs)
        return fn(len(jobs) if n is None else n, None if null_jobs else arr, byref(hd) if hd is not None else None,
                  byref(stm) if stm is not None else None, c_float(gs), use_state, 0, act, flag, _st())

    flag = c_int(-7)
    ok = mk_job()
    arg = [
        ('jobs', dict(jobs=[ok] * 8, n=9)), ('jobs', dict(jobs=[ok], n=-1)), ('null pointer', dict(n=1, null_jobs=True)),
        ('null pointer', dict(jobs=[ok], use_state=1, flag=None)),
        ('gradient scale', dict(jobs=[ok], gs=0.0)), ('gradient scale', dict(jobs=[ok], gs=-1.0)), ('gradient scale', dict(jobs=[ok], gs=float('nan'))),
        ('unknown activation', dict(jobs=[ok], act=2)), ('unknown activation', dict(jobs=[ok], act=-1)),
        ('wgrad_bf16: unsupported', dict(jobs=[ok, mk_job(C=97)])), ('wgrad_bf16: unsupported', dict(jobs=[mk_job(C=0)])),
        ('wgrad_bf16: unsupported', dict(jobs=[mk_job(O=100)])), ('wgrad_bf16: unsupported', dict(jobs=[mk_job(s=3)])),
        ('bad sizes', dict(jobs=[mk_job(s=0)])), ('bad sizes', dict(jobs=[mk_job(H=0)])), ('bad sizes', dict(jobs=[mk_job(W=-1)])),
        ('head finish', dict(hd=mk_head(blocks=0))), ('head finish', dict(hd=mk_head(C=0))),
        ('stem sizes', dict(stm=mk_stem(nslab=0))), ('stem sizes', dict(stm=mk_stem(Nout=0))),
    ]
    for f in ('xpad', 'dypad', 'slabs', 'dwf', 'dbf'):
        arg.append(('null pointer', dict(jobs=[ok, mk_job(**{f: None})])))
    for f in ('partial', 'dw', 'db'):
        arg.append(('null pointer', dict(hd=mk_head(**{f: None}))))
    for f in ('embed', 'w1', 'pre1', 'h1', 'pre2', 'dh2_slabs', 'dw0', 'db0', 'dw1', 'db1', 'ws'):
        arg.append(('null pointer', dict(jobs=[ok], stm=mk_stem(**{f: None}))))
    for text, kw in arg:
        if 'flag' not in kw:
            kw = dict(kw, use_state=kw.get('use_state', 1), flag=byref(flag))
        assert call(**kw) == -1, (text, kw)
        assert text in M.last_error(), (text, M.last_error())
    assert call(jobs=[ok], stm=mk_stem(ws_bytes=L.orn_stem_bwd_ws_bytes(1, 8, 64) - 4), use_state=1, flag=byref(flag)) == -2
    assert 'stem workspace' in M.last_error(), M.last_error()
    torch.cuda.synchronize()
    assert flag.value == -7
    assert bool((big16.float() == SENT).all()) and bool((bigf == SENT).all())

