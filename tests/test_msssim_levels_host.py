"""The comparator of tests/test_gpu_msssim_levels.py can fail (no GPU): on that test's own shapes and inputs it accepts r32, the
fp32 evaluation of the reference on the CPU, against r64, and rejects every float64 mutant below wherever the mutation changes
anything -- with the values of c that the GPU measurement fixed (msssim_levels_ref.C).

  forward partials   the weakest Gaussian tap dropped in the last valid column; in the last valid row
  pooled planes      the pooled row at the boundary of the first two tile rows taken one input row further down
  level gradients    the two tap mutants; ph ignored in the pool adjoint; its 0.25 applied at the wrong row parity; the k of planes
                     0 and 1 swapped
  whole chain        level 3's own gradient buffer fed where level 4's gradient belongs
Also: liborn's filter taps are bit for bit the reference's, and the relu-branch pair of the chain test does what it is built for."""
import ctypes

import numpy as np
import pytest
import torch

import msssim_levels_ref as R

F64, F32 = torch.float64, torch.float32
torch.set_num_threads(min(16, torch.get_num_threads()))


def test_library_taps_are_the_references():
    import orn_amd
    from orn_amd import _build
    _build.build()
    g = (ctypes.c_float * 11)()
    orn_amd._lib.lib().orn_debug_gauss_taps(g)
    assert np.array_equal(np.array(g, dtype=np.float32), R.taps32())
    assert abs(float(R.taps32().astype(np.float64).sum()) - 1.0) < 1e-6


@pytest.mark.parametrize('P', R.PLANES)
@pytest.mark.parametrize('shape', R.FWD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_comparator(shape, P):
    H, W = shape
    x, y = R.planes_pair(P, H, W)
    part64, nx64, _ = R.fwd_ref(x, y, F64)
    part32, nx32, _ = R.fwd_ref(x, y, F32)
    assert R.accept(part32, part64, part32, 'fwd part')
    assert R.pooled_ok(nx32, nx64)
    for where in ('col', 'row'):
        mut, _, _ = R.fwd_ref(x, y, F64, R.maps_tap_dropped(where))
        r = R.ratio(mut, part64, part32)
        print(f'tap dropped in the last {where}: ratio {r:.3g}')
        assert not R.accept(mut, part64, part32, 'fwd part'), (where, r)
    if H - 10 > R.TH:
        assert not R.pooled_ok(R.pool_boundary_row_from_neighbour(x.double()), nx64)


@pytest.mark.parametrize('P', R.PLANES)
@pytest.mark.parametrize('shape', R.BWD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_backward_comparator(shape, P):
    H, W = shape
    case = R.bwd_case(P, H, W)
    x, y, gn = case['x'], case['y'], case['gnext']
    assert R.accept(case['ref'][F32]['part'], case['ref'][F64]['part'], case['ref'][F32]['part'], 'bwd part')
    dropped = {w: R.unit_grads(x, y, F64, R.maps_tap_dropped(w)) for w in ('col', 'row')}
    for form in (0, 1, 2):
        for with_gnext in (False, True):
            r64, r32 = R.bwd_ref(case, form, with_gnext, F64), R.bwd_ref(case, form, with_gnext, F32)
            assert R.accept(r32, r64, r32, 'bwd g')
            mutants = {f'tap dropped in the last {w}': R.bwd_ref(case, form, with_gnext, F64, unit=dropped[w][0 if form == 0 else 1])
                       for w in ('col', 'row')}
            if P > 1:
                k = case['k'].clone()
                k[[0, 1]] = k[[1, 0]]
                mutants['k of planes 0 and 1 swapped'] = R.bwd_ref(case, form, with_gnext, F64, k=k)
            if with_gnext:
                if H % 2:
                    mutants['ph ignored'] = R.bwd_ref(case, form, True, F64, adj=R.pool_adjoint_indexed(gn, H, W, F64, 0, W % 2))
                mutants['0.25 at the wrong parity'] = R.bwd_ref(case, form, True, F64,
                                                                adj=R.pool_adjoint_indexed(gn, H, W, F64, H % 2, W % 2, off=1))
                right = R.pool_adjoint_indexed(gn, H, W, F64, H % 2, W % 2)
                assert torch.equal(right, case['ref'][F64]['adj'])          # the indexed form itself is the adjoint
            for name, m in mutants.items():
                r = R.ratio(m, r64, r32)
                assert not R.accept(m, r64, r32, 'bwd g'), (name, form, with_gnext, r)


_CHAIN = {}


def chain(shape, kind):
    if (shape, kind) not in _CHAIN:
        p, t = {'pair': R.make_pair, 'flat': R.flat_pair}[kind](*shape)
        _CHAIN[shape, kind] = (R.chain_ref(p, t, 0.7, 0.3, F64), R.chain_ref(p, t, 0.7, 0.3, F32),
                               R.chain_ref(p, t, 0.7, 0.3, F64, wrong_gnext_at_3=True))
    return _CHAIN[shape, kind]


@pytest.mark.parametrize('kind', ['pair', 'flat'])
@pytest.mark.parametrize('shape', R.CHAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_chain_comparator(shape, kind):
    r64, r32, mut = chain(shape, kind)
    for l in (1, 2, 3, 4):
        assert R.pooled_ok(r32['x'][l], r64['x'][l], l) and R.pooled_ok(r32['y'][l], r64['y'][l], l)
        assert R.accept(r32['g'][l], r64['g'][l], r32['g'][l], 'chain g')
    assert R.accept(r32['dpred'], r64['dpred'], r32['dpred'], 'chain dpred')
    assert torch.equal(mut['g'][4], r64['g'][4])
    for l in (3, 2, 1):
        assert not R.accept(mut['g'][l], r64['g'][l], r32['g'][l], 'chain g'), (l, R.ratio(mut['g'][l], r64['g'][l], r32['g'][l]))
    assert not R.accept(mut['dpred'], r64['dpred'], r32['dpred'], 'chain dpred')


@pytest.mark.parametrize('shape', R.CHAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_relu_pair_reaches_the_relu_branch(shape):
    """Level 0's CS mean is negative, levels 1..4 see p == t, and p != t but at the corner pixel (the sign term is +-1 there)."""
    p, t = R.relu_pair(*shape)
    assert int((p == t).sum()) == p.shape[0] * p.shape[1] and float(p.min()) > 0 and float(p.max()) < 1 and float(t.min()) > 0 and float(t.max()) < 1
    x, y = p.reshape(-1, *shape[1:]), t.reshape(-1, *shape[1:])
    for l in range(5):
        s, c = R.maps(x.double(), y.double(), R.win(F64))
        v = (s if l == 4 else c).mean((1, 2))
        print(l, v.tolist())
        assert bool((v < -0.05).all()) if l == 0 else bool((v > 0.9).all())
        x, y = R.pool(x), R.pool(y)               # in fp32, as the kernel pools
        assert torch.equal(x, y)
