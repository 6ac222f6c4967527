"""The merge backward of the 16-bit engine modes (ERB), elementwise against a float64 reference.

Both 16-bit modes (fp16 and bf16) compute the gradients of w1, w2, w3 and of the 1x3 / 3x1 slices on IEEE-half operand copies
(csrc/orn_merge_h16.hip, orn_merge_pack.h, the tail k_merge_bwd_tail_all): G = dL/dWf times 2^14 rounded to half (Gh, GT),
half copies of T, W1, W3^T and W2, then dW3 = G T^T and dT = W3^T G, then dW2 = dT W1 and the 9 dW1 partials W2 dT, dT carried
in half at the 2^14 scale.  The kernel-level cases reach it through orn_debug_merge_h16_bwd (include/orn_debug.h), which runs
the engine's own launchers in the engine's order; the engine-level cases check its wiring (which half copies are refreshed,
when, on which stream) from the gradients a TrainEngine leaves in its arena.

Reference: float64 on the CPU from the identically rounded operands (Gh = (G 2^14).half(), Th = T.half(), W1h, W3h, W2h =
.half() of the parameters); it does not use liborn.  Operand rounding is then no error; what remains is accumulation, plus
dT's one rounding to half.  Per element, never as a norm, with A the same contraction over absolute values (float64):
    dW3            |k - r| <= c A
    dW2, dW1       |k - r| <= c A + R                              (r, A from dTh, the reference's half dT; R below)
    d1x3, d3x1, db1x3, db3x1: bit-equal to the slices of G and to dbf.
dT's rounding: the kernel rounds to half an fp32 sum that lies within e = 2^-16 A_T + 2^-22 |dT| of the exact dT (A_T: the dT
contraction over absolute values; 2^-16 is ~170x the worst ratio measured on the same GEMM for dW3).  Where dT - e and dT + e
round to the same half, the kernel's dT is that half exactly; elsewhere it is one of the two, and R adds |hi - lo| of such
elements through the second contraction.  This is sharper than a blanket 2^-11 |dT| allowance: a W1 or W2 copy rounded toward
zero fails it.  c is per output, at most 3x the worst ratio (|k - r| - R)+ / A measured on an MI355X (C_TOL), and below 2^-14
for every output: operands rounded toward zero (up to 2^-10 relative) or a dropped 16-deep K step fail it.  The module runs in
about 8 s on one MI355X.

Contract checks on every kernel-level case: a guard of 1,024 sentinel floats behind every output stays unchanged; the outputs
start as NaN, and every one is finite when the flag is clear (every element is written, nothing non-finite is).
Overflow: the flag must rise for a G whose scaled half copy overflows (exactly at the rounding boundary 65520 2^-14), for a NaN
or inf in G, and for a dT beyond half range while every |G| < 4 (|W3^T dWf| > 4: the detector in k_mgemm_h16).
"""
import math
from ctypes import byref, c_int, c_void_p

import pytest
import torch

from helpers import GEOS, small_engine

pytestmark = pytest.mark.gpu

GS = 2.0 ** 14                 # MH_GS: the scale of the gradient-side half copies
SENT = 7.0
GUARD = 1024
KEYS = dict(w3x3='rbr_3x3_branch.weight', b3x3='rbr_3x3_branch.bias', w3x1='rbr_3x1_branch.weight', b3x1='rbr_3x1_branch.bias',
            w1x3='rbr_1x3_branch.weight', b1x3='rbr_1x3_branch.bias', w1='rbr_1x1_3x3_1x1_branch_1x1_1.weight',
            w2='rbr_1x1_3x3_1x1_branch_3x3.weight', w3='rbr_1x1_3x3_1x1_branch_1x1_2.weight')

# c per output: at most 3x the worst ratio measured on an MI355X (this module, kernel and engine cases together), and < 2^-14.
C_TOL = {                      # worst measured (MI355X; kernel cases / engine cases, fp16 and bf16 engines alike)
    'dW3': 1.1e-6,             # 3.85e-7 (dT near the half range: one column of G 100x the rest) / 6.6e-8 (720p fp16, layer 1)
    'dW2': 3.4e-7,             # 1.14e-7 (pack boundary, C = 17, O = 65) / 0 (every difference within dT's rounding allowance)
    'dW1': 1.2e-7,             # 4.2e-8 (C = 3, O = 1) / 0
}
WORST = {}
E_DT = 2.0 ** -16              # a priori bound of the dT GEMM's fp32 accumulation error, in units of its A (see the docstring)

PLANS = {
    '720p': [(26, 650), (26, 384), (96, 384), (96, 384), (96, 384)],
    '1080p': [(48, 1200), (48, 864), (96, 384), (96, 384), (96, 384)],
    # the layers of test_gpu_pipeline.GEOS
    'c96x2': [(96, 384), (96, 384)],
    'narrow_first': [(26, 650), (26, 384), (96, 384), (96, 384)],
    'stride3': [(26, 650), (26, 864), (96, 384)],
    # C at the r16 padding of E = 9C and of C, and the r32 padding of K2 = 2C
    'edge_c': [(1, 33), (15, 33), (16, 33), (17, 33)],
    # O at the 32x32 GEMM tiles and the 64x64 pack transposes, several shapes per set (table decoding across layers)
    'edge_o_a': [(3, 1), (3, 31), (5, 32), (3, 33)],
    'edge_o_b': [(2, 63), (3, 64), (7, 65), (1, 1)],
    # per-wave K of the dW3 / dT GEMMs (MH_KB = 8 steps of 16): 56 -> r16(9C) = 512 and O = 512: 128 per wave exactly;
    # O = 650 and 9C = 864: 128 plus a tail (the last wave of O = 650: exactly 128); 1200: two batches plus a tail
    'k_ranges': [(56, 512), (96, 650), (11, 120), (8, 1200)],
}


@pytest.fixture(scope='module')
def L():
    import orn_amd
    lib = orn_amd._lib.lib()
    assert hasattr(lib, 'orn_debug_merge_h16_bwd')
    torch.set_num_threads(16)
    return lib


def _err():
    import orn_amd
    return orn_amd._lib.last_error()


# ---- reference ---------------------------------------------------------------------------------------------------------------
def _h(t):
    return t.float().half().double()


def reference(G, dbf, T, w1, w2, w3):
    """float64 on the CPU, from the half operand copies the kernels read.  -> dict of (value, A, allowance for dT's rounding or
    None) per output, plus the slices and max |dT|."""
    O, C = G.shape[0], G.shape[1]
    E = 9 * C
    Gh = _h(G.reshape(O, E) * GS)                          # [O][E], scaled
    Th = _h(T.reshape(O, E))
    W3h = _h(w3.reshape(O, O))                            # [o][m]
    W1h = _h(w1.reshape(2 * C, C))                        # [k][c]
    W2h = _h(w2.reshape(O, 2 * C, 9))                     # [m][k][ij]
    out = {'dW3': (Gh @ Th.T / GS, Gh.abs() @ Th.abs().T / GS, None)}
    dT = (W3h.T @ Gh).reshape(O, C, 9)                    # [m][c][ij], scaled
    AT = (W3h.abs().T @ Gh.abs()).reshape(O, C, 9)
    # dT's rounding to half: the kernel rounds an fp32 sum within e of dT; where dT - e and dT + e round alike, so does it
    e = E_DT * AT + 2.0 ** -22 * dT.abs()
    lo, hi = (dT - e).half().double(), (dT + e).half().double()
    dTh = torch.where(lo == hi, lo, dT.half().double())
    amb = (hi - lo).abs()
    # dW2[m][k][ij] = sum_c dT[m][c][ij] W1h[k][c]
    out['dW2'] = (torch.einsum('mci,kc->mki', dTh, W1h) / GS, torch.einsum('mci,kc->mki', dTh.abs(), W1h.abs()) / GS,
                  torch.einsum('mci,kc->mki', amb, W1h.abs()) / GS)
    # dW1[k][c] = sum_{m,ij} W2h[m][k][ij] dT[m][c][ij]
    out['dW1'] = (torch.einsum('mki,mci->kc', W2h, dTh) / GS, torch.einsum('mki,mci->kc', W2h.abs(), dTh.abs()) / GS,
                  torch.einsum('mki,mci->kc', W2h.abs(), amb) / GS)
    g = G.reshape(O, C, 3, 3)
    out['d1x3'] = g[:, :, 1, :].contiguous()
    out['d3x1'] = g[:, :, :, 1].contiguous()
    out['dT_max'] = float(dT.abs().max()) / GS
    return out


def _record(name, ratio, what):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f'RATIO {name} {what} {ratio:.3e}')


def check_layer(k, ref, what):
    """k: dict of the kernel's outputs (CPU float32) for one layer; ref: reference()."""
    for name in ('dW3', 'dW2', 'dW1'):
        r, A, amb = ref[name]
        kk = k[name].double().reshape(r.shape)
        assert bool(torch.isfinite(kk).all()), f'{what} {name}: {int((~torch.isfinite(kk)).sum())} non-finite'
        d = (kk - r).abs()
        if amb is not None:
            d = (d - amb).clamp_min(0)
        ratio = float((d / A.clamp_min(1e-300)).max()) if bool((A > 0).any()) else 0.0
        _record(name, ratio, what)
        bad = d > C_TOL[name] * A
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            pytest.fail(f'{what} {name}: {int(bad.sum())} of {bad.numel()} elements out of bound (c = {C_TOL[name]:.1e}, '
                        f'worst ratio {ratio:.3e}); first at {i}: kernel {kk.flatten()[i].item():.9e} ref '
                        f'{r.flatten()[i].item():.9e} A {A.flatten()[i].item():.3e}')
    for name in ('d1x3', 'd3x1'):
        assert torch.equal(k[name].reshape(ref[name].shape), ref[name]), f'{what} {name}: not the slice of G'
    for name in ('db1x3', 'db3x1'):
        assert torch.equal(k[name], k['dbf']), f'{what} {name}: not dbf'


# ---- kernel-level: orn_debug_merge_h16_bwd -----------------------------------------------------------------------------------
OUTS = ('dW3', 'dW2', 'dW1', 'd1x3', 'd3x1', 'db1x3', 'db3x1')


def _out_sizes(C, O):
    return dict(dW3=O * O, dW2=O * 2 * C * 9, dW1=2 * C * C, d1x3=O * C * 3, d3x1=O * C * 3, db1x3=O, db3x1=O)


def run_kernel(L, layers):
    """layers: list of dicts of CPU float32 tensors G, dbf, T, w1, w2, w3.  -> (flag, list of dicts of CPU outputs)."""
    n = len(layers)
    co = (c_int * (2 * n))()
    ins = (c_void_p * (6 * n))()
    outs = (c_void_p * (7 * n))()
    keep, bufs = [], []
    for i, l in enumerate(layers):
        O, C = l['G'].shape[0], l['G'].shape[1]
        co[2 * i], co[2 * i + 1] = C, O
        for j, key in enumerate(('G', 'dbf', 'T', 'w1', 'w2', 'w3')):
            t = l[key].float().contiguous().cuda()
            keep.append(t)
            ins[6 * i + j] = t.data_ptr()
        b = {}
        for j, (name, cnt) in enumerate(_out_sizes(C, O).items()):
            buf = torch.full((cnt + GUARD,), SENT, device='cuda')
            buf[:cnt] = float('nan')
            b[name] = (buf, cnt)
            outs[7 * i + j] = buf.data_ptr()
        bufs.append(b)
    flag = c_int(-1)
    torch.cuda.synchronize()
    rc = L.orn_debug_merge_h16_bwd(n, co, ins, outs, byref(flag), c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _err()
    torch.cuda.synchronize()
    res = []
    for i, b in enumerate(bufs):
        o = {}
        for name, (buf, cnt) in b.items():
            g = buf[cnt:]
            assert bool((g == SENT).all()), f'layer {i} {name}: {int((g != SENT).sum())} guard elements written'
            o[name] = buf[:cnt].cpu()
        o['dbf'] = layers[i]['dbf'].float().flatten()
        res.append(o)
    return flag.value, res


def make_layer(C, O, seed, g_lo=1e-6, g_hi=1e-2):
    """Seeded operands: G at realistic scales (a per-row scale log-uniform in [g_lo, g_hi]) with exact zeros and elements whose
    scaled half copy is subnormal (|G| < 2^-28); parameters at the model's initial scales; T ~ 0.05."""
    gen = torch.Generator().manual_seed(seed)
    rs = torch.exp(torch.rand(O, 1, 1, 1, generator=gen) * math.log(g_hi / g_lo) + math.log(g_lo))
    G = torch.randn(O, C, 3, 3, generator=gen) * rs
    u = torch.rand(O, C, 3, 3, generator=gen)
    G[u < 0.05] = 0.0
    sub = (u >= 0.05) & (u < 0.08)
    G[sub] = torch.randn(int(sub.sum()), generator=gen) * 2.0 ** -31
    return dict(G=G, dbf=torch.randn(O, generator=gen) * 1e-3, T=(torch.randn(O, C, 3, 3, generator=gen) + 0.1) * 0.05,
                w1=(torch.rand(2 * C, C, 1, 1, generator=gen) * 2 - 1) / math.sqrt(C),
                w2=(torch.rand(O, 2 * C, 3, 3, generator=gen) * 2 - 1) / math.sqrt(18 * C),
                w3=(torch.rand(O, O, 1, 1, generator=gen) * 2 - 1) / math.sqrt(O))


def _check_all(L, layers, what):
    flag, res = run_kernel(L, layers)
    assert flag == 0, f'{what}: flag raised on in-range data'
    for i, (l, k) in enumerate(zip(layers, res)):
        check_layer(k, reference(**l), f'{what} layer {i} (C={l["G"].shape[1]}, O={l["G"].shape[0]})')
    return res


@pytest.mark.parametrize('plan', sorted(PLANS))
def test_merge16_bwd_elementwise(L, plan):
    """Every plan in one call (one merge set), as the engine builds it."""
    layers = [make_layer(C, O, seed=100 * k + len(plan)) for k, (C, O) in enumerate(PLANS[plan])]
    _check_all(L, layers, plan)


def test_merge16_bwd_scales_per_set(L):
    """The same layer at the smallest and at the largest realistic gradient scale, and an all-zero G, in one set."""
    layers = [make_layer(26, 384, 7, 1e-6, 2e-6), make_layer(26, 384, 8, 5e-3, 1e-2), make_layer(17, 65, 9)]
    layers[2]['G'].zero_()
    _check_all(L, layers, 'scales')


def test_merge16_pack_overflow_boundary(L):
    """D: the pack's half copy of G overflows exactly from 65520 2^-14 (round to nearest: 65520 is the tie above 65504)."""
    edge = torch.tensor(65520.0 / GS)
    below = torch.nextafter(edge, torch.tensor(0.0))
    for v, want in ((edge, 1), (-edge, 1), (below, 0), (-below, 0)):
        lay = make_layer(17, 65, 3)
        lay['G'][5, 3, 1, 2] = v
        flag, res = run_kernel(L, [make_layer(15, 33, 4), lay])
        assert flag == want, (float(v), flag)
        if not want:
            for i, (l, k) in enumerate(zip([make_layer(15, 33, 4), lay], res)):
                check_layer(k, reference(**l), f'below the boundary, layer {i}')


@pytest.mark.parametrize('bad', ['nan', 'inf', '-inf'])
def test_merge16_nonfinite_gradient_raises_flag(L, bad):
    """E: a NaN or inf in G (second layer of the set, in a ragged edge tile) raises the flag."""
    lay = make_layer(17, 65, 5)
    lay['G'][64, 16, 2, 2] = float(bad)
    flag, _ = run_kernel(L, [make_layer(26, 384, 6), lay])
    assert flag == 1


def _dt_layer(C, O, g0):
    lay = make_layer(C, O, 11)
    lay['w3'][:, 0] = 1.0
    lay['G'][:, 0, 0, 0] = g0
    return lay


def test_merge16_dT_overflow_raises_flag(L):
    """F: dT = W3^T G beyond half range at the 2^14 scale while every |G| < 3.99 (the pack's check passes): w3[:, 0] = 1 and
    G[:, 0, 0, 0] = 0.02 at O = 384 put dT[0, (0, 0)] at 7.68, 2^14 times that is 125829 > 65504.  The flag must rise (before,
    dW2 and dW1 came out inf / NaN with the flag clear)."""
    lay = _dt_layer(26, 384, 0.02)
    assert float(lay['G'].abs().max()) < 3.99
    ref = reference(**lay)
    assert ref['dT_max'] * GS > 65520
    flag, _ = run_kernel(L, [make_layer(96, 384, 12), lay])
    assert flag == 1


def test_merge16_flag_clear_means_finite(L):
    """G: just inside half range (2^14 dT = 384 x half(170.4) = 65424 < 65504) the flag stays clear and every output is finite and
    within its bound."""
    lay = _dt_layer(26, 384, 0.0104)
    ref = reference(**lay)
    assert 60000 < ref['dT_max'] * GS < 65504
    flag, res = run_kernel(L, [lay])
    assert flag == 0
    check_layer(res[0], ref, 'dT near the half range')


# ---- engine level ------------------------------------------------------------------------------------------------------------
def _slot(eng, arena, i, key):
    off, n = eng.layout[f'layers.{i}.{KEYS[key]}']
    return arena[off:off + n]


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import engine, model  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


@pytest.mark.parametrize('mode', ['serial', 'pipelined'])
@pytest.mark.parametrize('prec', ['fp16', 'bf16'])
def test_engine_merge16_bwd_elementwise_at_720p(orn, prec, mode):
    """The engine's merge backward of step n = 3 (lr > 0: its half copies are those of parameters after two Adam updates), every
    layer of the 720p plan, against the reference built from the engine's own G and dbf of that step (grad arena) and the
    parameters P_2 it started from (taken from a second engine that ran the first 2 steps).  The last block's merge backward runs
    on the side stream in the pipelined form, the others on the caller's stream.  T is the oracle's merge forward of P_2; the
    engine's T is not exposed, so the merged kernel Wf the same launch writes must equal the oracle's bit for bit."""
    import bench
    from oracle import c_oracle
    n = 3
    graph = True if mode == 'serial' else None
    entries = [((2 * k + 1) % 6, k + 1, 5e-4 * (1.0 - 0.1 * k)) for k in range(n)]
    a = bench.make_engine(seed=7, precision=prec, cfg=bench.CONFIGS['720p'], frames=6)
    a.set_schedule(entries[:n - 1])
    a.run(n - 1, graph=graph)
    torch.cuda.synchronize()
    P = a.params.cpu()
    assert a.scale_state()['skipped'] == 0
    del a
    b = bench.make_engine(seed=7, precision=prec, cfg=bench.CONFIGS['720p'], frames=6)
    b.set_schedule(entries)
    b.run(n, graph=graph)
    torch.cuda.synchronize()
    s = b.scale_state()
    assert s['skipped'] == 0 and s['late_skipped'] == 0, s
    G = b.grads.cpu()
    nl = len(b.model.layers)
    for i in range(nl):
        p = {key: _slot(b, P, i, key).view(dict(b.model.named_parameters())[f'layers.{i}.{KEYS[key]}'].shape) for key in KEYS}
        wf, bf, T = c_oracle.merge_fwd(*(p[key].numpy() for key in ('w3x3', 'b3x3', 'w3x1', 'b3x1', 'w1x3', 'b1x3', 'w1', 'w2', 'w3')))
        ewf, _ = b.engine_fused_kernel(i)
        assert torch.equal(ewf.cpu(), torch.from_numpy(wf)), f'layer {i}: the engine merged other parameters than P_{n - 1}'
        O, C = p['w3x3'].shape[:2]
        lay = dict(G=_slot(b, G, i, 'w3x3').view(O, C, 3, 3), dbf=_slot(b, G, i, 'b3x3'), T=torch.from_numpy(T),
                   w1=p['w1'], w2=p['w2'], w3=p['w3'])
        assert float(lay['G'].abs().max()) > 0
        k = dict(dW3=_slot(b, G, i, 'w3'), dW2=_slot(b, G, i, 'w2'), dW1=_slot(b, G, i, 'w1'), d1x3=_slot(b, G, i, 'w1x3'),
                 d3x1=_slot(b, G, i, 'w3x1'), db1x3=_slot(b, G, i, 'b1x3'), db3x1=_slot(b, G, i, 'b3x1'), dbf=lay['dbf'])
        check_layer(k, reference(**lay), f'720p {prec} {mode} layer {i}')


def _scale_layer(eng, i, k):
    """w3 of layer i times 2^k, its w2 times 2^-k: T scales by 2^-k, Wf, the forward and G stay bit for bit, dT scales by 2^k."""
    with torch.no_grad():
        _slot(eng, eng.params, i, 'w3').mul_(2.0 ** k)
        _slot(eng, eng.params, i, 'w2').mul_(2.0 ** -k)


def test_engine_dT_overflow_skips_the_step(orn):
    """A dT beyond half range (|W3^T dWf| > 4 while every |dWf| < 4) through the engine (narrow_first, fp16).  k is picked from
    the unscaled step's max |dT| so that the scaled one lies in [8, 16).  The premise is asserted: the loss and G are bit-equal
    to the unscaled step's.  Serial: the step is skipped and counted, nothing moves.  Pipelined: on the last block (side stream)
    it is a late-only skip -- the lower blocks update, the last block and the head do not; on a lower block the step is skipped.
    Everything stays finite (before the dT detector, the scaled layer's w1 / w2 turned NaN)."""
    prec, geo = 'fp16', 'narrow_first'
    nl = len(GEOS[geo]['strides'])
    sched = [(1, 1, 5e-4)]

    def engine():
        eng = small_engine(orn, prec, 'ERB', geo)
        eng.set_schedule(sched)
        return eng
    ref = engine()
    ref.run(1, graph=False)
    torch.cuda.synchronize()
    loss0 = ref.stats(1)[0, 0].item()
    G0 = ref.grads.clone()
    P0 = ref.params.cpu()
    ks = {}
    for i in (nl - 2, nl - 1):
        Ol = _slot(ref, P0, i, 'b3x3').numel()
        g = _slot(ref, G0, i, 'w3x3').cpu().double().view(Ol, -1)
        assert float(g.abs().max()) < 4
        dT = _slot(ref, P0, i, 'w3').double().view(Ol, Ol).T @ g
        ks[i] = math.ceil(math.log2(8.0 / float(dT.abs().max())))
        assert float(_slot(ref, P0, i, 'w3').abs().max()) * 2.0 ** ks[i] < 60000      # W3's own half copy stays in range
    del ref

    def scaled_run(i, graph):
        eng = engine()
        _scale_layer(eng, i, ks[i])
        p0, m0, v0 = eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()
        eng.run(1, graph=graph)
        torch.cuda.synchronize()
        assert eng.stats(1)[0, 0].item() == loss0, 'premise: the scaled state computes the same loss'
        assert torch.equal(_slot(eng, eng.grads, i, 'w3x3'), _slot(eng, G0, i, 'w3x3')), 'premise: the same G'
        assert torch.isfinite(eng.params).all() and torch.isfinite(eng.adam_m).all() and torch.isfinite(eng.adam_v).all()
        return eng, p0, m0, v0

    for i in (nl - 2, nl - 1):
        eng, p0, m0, v0 = scaled_run(i, False)
        s = eng.scale_state()
        assert s['skipped'] == 1, (i, s)
        assert torch.equal(eng.params, p0) and torch.equal(eng.adam_m, m0) and torch.equal(eng.adam_v, v0), i
        del eng
    eng, p0, m0, v0 = scaled_run(nl - 2, None)
    s = eng.scale_state()
    assert s['skipped'] == 1 and s['late_skipped'] == 0, s
    assert torch.equal(eng.params, p0) and torch.equal(eng.adam_m, m0), 'pipelined, lower block'
    del eng
    eng, p0, m0, v0 = scaled_run(nl - 1, None)
    s = eng.scale_state()
    assert s['skipped'] == 0 and s['late_skipped'] == 1, s
    lo = min(off for key, (off, n) in eng.layout.items() if key.startswith(f'layers.{nl - 1}.') or key.startswith('head_layers.'))
    assert torch.equal(eng.params[lo:], p0[lo:]) and torch.equal(eng.adam_m[lo:], m0[lo:]), 'the last block and the head'
    assert not torch.equal(eng.params[:lo], p0[:lo]), 'the lower blocks took the step'
