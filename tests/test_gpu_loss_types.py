"""GPU tests of the losses of loss_fn (utils.py:139-189) beyond L2 / L1 / Fusion6: the SSIM family (SSIM, Fusion1-5, Fusion9), the
L1 + L2 mixes (Fusion7 / 8) and the MS-SSIM losses (Fusion10-12: five forward level launches, one coefficient launch, five backward
level launches, orn_loss_msssim.hip), through utils.loss_fn + backward and ops.loss_stats.

The oracle's loss_fn lacks most of these names, so the references are composed here in fp64 from cpu_ref.ssim, cpu_ref.ms_ssim, L1
and MSE with the reference's weights, and differentiated by autograd.  Inputs: target = uniform noise smoothed by a 5x5 box filter,
pred = (target + 0.1 * randn).clamp(0, 1), seeded per shape.  Tolerances are those of test_gpu_parity.test_loss_fwd_bwd."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# utils.py:142-172: name -> (weight of mean|p-t|, weight of mse, weight of (1 - s), s)
WEIGHTS = {
    'SSIM': (0.0, 0.0, 1.0, 'ssim'), 'Fusion1': (0.0, 0.3, 0.7, 'ssim'), 'Fusion2': (0.3, 0.0, 0.7, 'ssim'),
    'Fusion3': (0.0, 0.5, 0.5, 'ssim'), 'Fusion4': (0.5, 0.0, 0.5, 'ssim'), 'Fusion5': (0.0, 0.7, 0.3, 'ssim'),
    'Fusion7': (0.3, 0.7, 0.0, None), 'Fusion8': (0.5, 0.5, 0.0, None), 'Fusion9': (0.9, 0.0, 0.1, 'ssim'),
    'Fusion10': (0.7, 0.0, 0.3, 'ms_ssim'), 'Fusion11': (0.9, 0.0, 0.1, 'ms_ssim'), 'Fusion12': (0.8, 0.0, 0.2, 'ms_ssim'),
}
SSIM_FAMILY = ['SSIM', 'Fusion1', 'Fusion2', 'Fusion3', 'Fusion4', 'Fusion5', 'Fusion7', 'Fusion8', 'Fusion9']
MS_FAMILY = ['Fusion10', 'Fusion11', 'Fusion12']
# (2, 30, 37): ragged tiles, W % 4 != 0 (the scalar load path), two batches
SSIM_SHAPES = [(1, 45, 80), (2, 30, 37)]
# (1, 161, 177): odd at every level, the smallest legal size; (2, 163, 201): odd at level 0, six planes; (1, 176, 192): even down to
# 11 x 12, one valid column at level 4
MS_SHAPES = [(1, 161, 177), (2, 163, 201), (1, 176, 192)]


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def cu(t):
    return t.cuda().contiguous()


def make_pair(B, H, W):
    gen = torch.Generator().manual_seed(H * W + B)
    u = torch.rand(B, 3, H + 4, W + 4, generator=gen)
    t = F.avg_pool2d(u, 5, stride=1)                       # 5x5 box filter
    assert t.shape == (B, 3, H, W)
    p = (t + 0.1 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    return p.contiguous(), t.contiguous()


def composed_loss(name, p, t):
    """loss_fn of the reference for `name` in the dtype of p, and the structural value s it contains (None: none)."""
    from oracle import cpu_ref
    w1, w2, ws, kind = WEIGHTS[name]
    s = None
    if kind == 'ssim':
        s = cpu_ref.ssim(p, t, data_range=1, size_average=True)
    elif kind == 'ms_ssim':
        s = cpu_ref.ms_ssim(p, t, data_range=1, size_average=True)
    loss = 0.0
    if w1:
        loss = loss + w1 * torch.mean(torch.abs(p - t))
    if w2:
        loss = loss + w2 * F.mse_loss(p, t)
    if ws:
        loss = loss + ws * (1 - s)
    return loss, s


def ms_level_means(p, t):
    """[5][B][C] level means of the oracle's ms_ssim (cs at levels 0..3, ssim at level 4) before the relu."""
    from oracle import cpu_ref
    out = []
    for i in range(5):
        ssim_map, cs_map = cpu_ref.ssim_maps(p, t, 1.0)
        out.append(torch.flatten(cs_map if i < 4 else ssim_map, 2).mean(-1))
        if i < 4:
            pad = [s % 2 for s in p.shape[2:]]
            p, t = F.avg_pool2d(p, 2, padding=pad), F.avg_pool2d(t, 2, padding=pad)
    return torch.stack(out)


_REF = {}


def reference(name, shape):
    """fp64 loss, gradient and structural value of one (loss, shape), computed once and never modified."""
    key = (name, shape)
    if key not in _REF:
        p, t = make_pair(*shape)
        rp = p.double().requires_grad_(True)
        loss, s = composed_loss(name, rp, t.double())
        loss.backward()
        _REF[key] = types.SimpleNamespace(p=p, t=t, loss=loss.item(), grad=rp.grad.float().numpy(),
                                          s=None if s is None else s.item())
    return _REF[key]


def check_against(orn, name, shape):
    r = reference(name, shape)
    dp = cu(r.p).requires_grad_(True)
    args = types.SimpleNamespace(loss_type=name)
    loss = orn.utils.loss_fn(dp, cu(r.t), args)
    loss.backward()
    g = dp.grad.cpu().numpy()
    gmax = np.abs(r.grad).max()
    print(f'{name} {shape}: loss {loss.item():.8f} ref {r.loss:.8f}; grad max|ref| {gmax:.3e} max abs err {np.abs(g - r.grad).max():.3e}')
    assert abs(loss.item() - r.loss) <= 2e-6 + 1e-5 * abs(r.loss)
    np.testing.assert_allclose(g, r.grad, rtol=2e-3, atol=2e-4 * gmax)
    st, _ = orn.ops.loss_stats(cu(r.p), cu(r.t), name, want_grad=False)
    st = st.cpu()
    print(f'    stats[3] {st[3].item():.8f} ref {r.s}')
    if r.s is None:
        assert st[3].item() == 0.0
    else:
        assert abs(st[3].item() - r.s) <= 2e-5
    assert abs(st[0].item() - r.loss) <= 2e-6 + 1e-5 * abs(r.loss)
    d = (r.p - r.t).double()
    assert abs(st[1].item() - d.abs().mean().item()) <= 1e-6 and abs(st[2].item() - (d * d).mean().item()) <= 1e-6
    return r


@pytest.mark.parametrize('shape', SSIM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', SSIM_FAMILY)
def test_ssim_family_vs_oracle(orn, name, shape):
    """Loss, dL/dpred and stats[3] of the SSIM family and of Fusion7 / 8 against the composed fp64 reference."""
    check_against(orn, name, shape)


@pytest.mark.parametrize('shape', MS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', MS_FAMILY)
def test_msssim_family_vs_oracle(orn, name, shape):
    """Loss, dL/dpred and the MS-SSIM value of Fusion10-12 against fp64 autograd of cpu_ref.ms_ssim.  No level mean sits near the
    relu's kink (asserted on the oracle side), and stats[3] is the very value ops.ms_ssim returns for the pair."""
    r = check_against(orn, name, shape)
    v = ms_level_means(r.p.double(), r.t.double())
    print(f'    min level mean {v.min().item():.4f}')
    assert v.min().item() > 0.05
    st, _ = orn.ops.loss_stats(cu(r.p), cu(r.t), name, want_grad=True)
    ms = orn.ops.ms_ssim(cu(r.p), cu(r.t))
    assert st[3].item() == ms.item()


@pytest.mark.parametrize('shape', MS_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_msssim_loss_is_deterministic_and_grad_free_form_agrees(orn, shape):
    """Two consecutive calls give bit-identical dpred and stats (fixed-order sums, no atomics); want_grad=False returns the same
    stats as want_grad=True."""
    p, t = (cu(x) for x in make_pair(*shape))
    s1, g1 = orn.ops.loss_stats(p, t, 'Fusion10', want_grad=True)
    s2, g2 = orn.ops.loss_stats(p, t, 'Fusion10', want_grad=True)
    s3, g3 = orn.ops.loss_stats(p, t, 'Fusion10', want_grad=False)
    assert g3 is None
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    assert torch.equal(s1, s3)
    assert bool(torch.isfinite(g1).all())


def test_msssim_loss_scale_scales_the_gradient(orn):
    """loss_scale multiplies stats[0] and dpred (the coefficient launch carries it), nothing else."""
    p, t = (cu(x) for x in make_pair(*MS_SHAPES[0]))
    s1, g1 = orn.ops.loss_stats(p, t, 'Fusion12', want_grad=True)
    s4, g4 = orn.ops.loss_stats(p, t, 'Fusion12', want_grad=True, loss_scale=4.0)
    assert torch.equal(s4[1:5], s1[1:5]) and s4[0].item() == 4.0 * s1[0].item()
    np.testing.assert_allclose(g4.cpu().numpy(), 4.0 * g1.cpu().numpy(), rtol=1e-6, atol=0)


def test_msssim_loss_refuses_a_side_of_160(orn):
    p, t = (cu(x) for x in make_pair(1, 160, 200))
    with pytest.raises(orn._lib.OrnError) as ei:
        orn.ops.loss_stats(p, t, 'Fusion10')
    assert '160' in str(ei.value) and 'rc=-1' in str(ei.value)


def test_unbuilt_loss_types_raise(orn):
    p, t = (cu(x) for x in make_pair(1, 45, 80))
    for name in ('Fusion13', 'Fusion15'):
        with pytest.raises(NotImplementedError) as ei:
            orn.ops.loss_stats(p, t, name)
        assert 'Fusion12' in str(ei.value)
        with pytest.raises(NotImplementedError):
            orn.utils.loss_fn(p.clone().requires_grad_(True), t, types.SimpleNamespace(loss_type=name))


def test_target_statistics_cache_changes_nothing_for_fusion1(orn):
    """The target-statistics table (orn_loss_target_stats) serves the whole SSIM family: with Fusion1 (the L2-term variant of the
    kernel) stats, gradients and parameters after 4 steps are bit-identical with and without it."""
    from oracle import cpu_ref
    res = []
    for cache in (False, True):
        torch.manual_seed(1)
        gen = orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim='2_3_26', expansion=1, num_blocks=1, norm='none',
                                  act='swish', bias=True, reduction=2, conv_type='conv', stride_list=[5, 2, 2], sin_res=True,
                                  lower_width=96, sigmoid=False, deploy=False, branch_type='ERB')
        eng = orn.engine.TrainEngine(gen, loss_type='Fusion1', beta=0.5, precision='fp16', target_cache=cache)
        frames = cpu_ref.synthetic_video(5, eng.out_hw[0], eng.out_hw[1], seed=5)
        embeds = cpu_ref.positional_encoding(torch.tensor([k / 5 for k in range(5)]), 1.25, 40)
        eng.set_video(frames, embeds)
        assert (eng.tstats is not None) == cache
        eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(4)])
        eng.run(4, graph=True)
        torch.cuda.synchronize()
        res.append((eng.stats(4).clone(), eng.grads.clone(), eng.params.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0][:, 3].min()) > 0.0            # stats[3] carries the SSIM value
