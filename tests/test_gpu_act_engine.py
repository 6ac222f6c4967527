"""--act gelu through the mirror and every form of the engine.

(a) the four generators of tests/golden/act_gelu.npz: the mirror against the reference (test_tiny_generator_golden's tolerances),
    then the fp32 engine on the same state against the mirror;
(b) three optimiser steps of the tiny ERB and NeRV_vanilla fp32 engines against torch autograd in fp64 + Adam (F.gelu, default
    approximation): every tensor within 0.75 lr, test_gpu_branch_kinds.py's rule;
(c) the fp16 and bf16 engines against the fp32 engine at the two small fast-path geometries, with the tolerances of
    test_gpu_bf16.py::test_bf16_engine_vs_fp32_engine (the issue names test_gpu_precision.py, which compares no gradients at these
    geometries; test_gpu_bf16.py is where the swish engines are held to the fp32 engine, and its figures are taken unchanged);
(d) launch forms: pipelined == graph replay == eager, bit for bit; batch 1 == the single-frame step, batch 2 == the mean of its
    frames' gradients; the split step; a multi-resolution engine;
(e) decode_frames against the mirror's forward, and an ECB engine against a NeRV_vanilla engine handed its merged kernel;
(f) the command lines without --act."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import act_fixture

pytestmark = pytest.mark.gpu

SMALL = {'3_4_96': dict(fc='3_4_96', strides=(2, 2), lower_width=96), '2_3_26': dict(fc='2_3_26', strides=(5, 2, 2), lower_width=96)}


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _video(eng, n=5, seed=5):
    from oracle import cpu_ref
    frames = cpu_ref.synthetic_video(n, eng.out_hw[0], eng.out_hw[1], seed=seed)
    embeds = cpu_ref.positional_encoding(torch.tensor([k / n for k in range(n)]), 1.25, 40)
    eng.set_video(frames, embeds)
    return frames, embeds


def _slot(e, name):
    off, n = e.layout[name]
    return e.grads[off:off + n]


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', act_fixture.TAGS)
def test_fixture_generators_mirror_and_engine(orn, tag):
    g = act_fixture.load()
    kind, sr = tag[len('tiny_'):].rsplit('_sr', 1)
    gen = act_fixture.tiny_generator(kind, bool(int(sr)), 'gelu').cuda()
    n = int(g[f'{tag}/n_stages'][0])
    outs = gen(cu(g[f'{tag}/embed']))
    assert len(outs) == n
    losses = []
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), g[f'{tag}/img{i}'], rtol=1e-5, atol=2e-6)
        losses.append(torch.mean(torch.abs(o - cu(g[f'{tag}/target{i}']))))
    loss = sum(float(g['lw'][0]) * l_ for l_ in losses[:-1]) + losses[-1]
    assert abs(loss.item() - float(g[f'{tag}/loss'])) < 1e-6 * n
    loss.backward()
    mirror = {}
    for k, p in gen.named_parameters():
        r = g[f'{tag}/grad/{k}']
        np.testing.assert_allclose(p.grad.cpu().numpy(), r, rtol=2e-4, atol=2e-5 * max(np.abs(r).max(), 1e-6), err_msg=k)
        mirror[k] = p.grad.detach().clone()
    # the fp32 engine on the same state: one step at lr 0 leaves its gradients in the arena.  Its kernels are the per-op ones with the
    # stem riding on other launches and the head's backward fused into the last block's: same sums in another order
    eng = orn.engine.TrainEngine(gen, loss_type='L1', beta=0.5, precision='fp32', lw=float(g['lw'][0]))
    eng.set_video(cu(g[f'{tag}/target{n - 1}']), cu(g[f'{tag}/embed']),
                  stage_frames=[cu(g[f'{tag}/target{i}']) for i in range(n - 1)] if n > 1 else None)
    eng.set_schedule([(0, 1, 0.0)])
    eng.run(1, graph=False)
    torch.cuda.synchronize()
    assert abs(eng.stats(1)[0, 0].item() - float(g[f'{tag}/loss'])) < 1e-6 * n
    img = eng.decode(cu(g[f'{tag}/embed']))
    np.testing.assert_allclose(img.cpu().numpy(), g[f'{tag}/img{n - 1}'], rtol=1e-5, atol=2e-6)
    for k, m in mirror.items():
        r = m.flatten()
        assert torch.allclose(_slot(eng, k), r, rtol=2e-4, atol=2e-5 * max(r.abs().max().item(), 1e-6)), k


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def _forward64(sd, embed, kind, strides, fc):
    """The reference's training forward with F.gelu, on a state dict of any dtype (ERB: its branches summed on the activations --
    with no bias inside the 1x1 -> 3x3 -> 1x1 chain that is the merged conv exactly)."""
    fh, fw, fd = fc
    x = F.gelu(F.linear(F.gelu(F.linear(embed, sd['stem.0.weight'], sd['stem.0.bias'])), sd['stem.2.weight'], sd['stem.2.bias']))
    x = x.view(x.shape[0], fd, fh, fw)
    for i, s in enumerate(strides):
        def P(n):
            return sd[f'layers.{i}.{n}']
        if kind == 'NeRV_vanilla':
            y = F.conv2d(x, P('branch.weight'), P('branch.bias'), padding=1)
        else:
            y = F.conv2d(x, P('rbr_3x3_branch.weight'), P('rbr_3x3_branch.bias'), padding=1)
            y = y + F.conv2d(x, P('rbr_3x1_branch.weight'), P('rbr_3x1_branch.bias'), padding=(1, 0))
            y = y + F.conv2d(x, P('rbr_1x3_branch.weight'), P('rbr_1x3_branch.bias'), padding=(0, 1))
            t = F.conv2d(F.conv2d(x, P('rbr_1x1_3x3_1x1_branch_1x1_1.weight')), P('rbr_1x1_3x3_1x1_branch_3x3.weight'), padding=1)
            y = y + F.conv2d(t, P('rbr_1x1_3x3_1x1_branch_1x1_2.weight'))
        x = F.gelu(F.pixel_shuffle(y, s))
    n = len(strides) - 1
    return (torch.tanh(F.conv2d(x, sd[f'head_layers.{n}.weight'], sd[f'head_layers.{n}.bias'])) + 1) * 0.5


@pytest.mark.parametrize('kind', act_fixture.KINDS)
def test_three_steps_against_fp64_autograd(orn, kind):
    from oracle import cpu_ref
    gen = act_fixture.tiny_generator(kind, True, 'gelu')
    sd0 = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    frames = cpu_ref.synthetic_video(5, 12, 16, seed=3)
    embeds = cpu_ref.positional_encoding(torch.tensor([k / 5.0 for k in range(5)], dtype=torch.float32), 1.25, 40)
    eng = orn.engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5)
    eng.set_video(frames, embeds)
    entries = [(3, 1, 5e-4), (0, 2, 4e-4), (4, 3, 3e-4)]
    eng.set_schedule(entries)
    eng.run(3, graph=False)
    torch.cuda.synchronize()
    st = eng.stats(3).numpy()
    sd = {k: v.double() for k, v in sd0.items()}
    am = {k: torch.zeros_like(v) for k, v in sd.items()}
    av = {k: torch.zeros_like(v) for k, v in sd.items()}
    for i, (f, step, lr) in enumerate(entries):
        params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        out = _forward64(params, embeds[f:f + 1].double(), kind, [2, 2], (3, 4, 8))
        loss = cpu_ref.loss_fn(out, frames[f:f + 1].double(), 'Fusion6')
        loss.backward()
        assert abs(st[i, 0] - loss.item()) < 5e-5, (i, st[i], loss.item())
        with torch.no_grad():
            for k in sd:
                cpu_ref.adam_step(sd[k], params[k].grad, am[k], av[k], step, lr, 0.5)
    new = gen.state_dict()
    worst = max((new[k].cpu().double() - sd[k]).abs().max().item() for k in sd)
    print(f'{kind} gelu: worst parameter distance from the fp64 reference after 3 steps: {worst / 5e-4:.3f} lr')
    assert worst < 0.75 * 5e-4, worst
    # and the swish engine on the same start does something else: the activation is not ignored
    gen_s = act_fixture.tiny_generator(kind, True, 'swish')
    eng_s = orn.engine.TrainEngine(gen_s, loss_type='Fusion6', beta=0.5)
    eng_s.set_video(frames, embeds)
    eng_s.set_schedule(entries)
    eng_s.run(1, graph=False)
    torch.cuda.synchronize()
    assert eng_s.stats(1)[0, 0].item() != st[0, 0]        # (close at this init: both are near z / 2 around 0; measured 1.6e-5 apart)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def _one_step(orn, geo, kind, prec, sin_res=True, loss='Fusion6', lr=0.0):
    gen = act_fixture.tiny_generator(kind, sin_res, 'gelu', **SMALL[geo])
    eng = orn.engine.TrainEngine(gen, loss_type=loss, beta=0.5, precision=prec)
    _video(eng, 4)
    eng.set_schedule([(1, 1, lr)])
    eng.run(1, graph=False)
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize('prec', ['fp16', 'bf16'])
@pytest.mark.parametrize('geo,kind', [('3_4_96', 'ERB'), ('2_3_26', 'ERB'), ('3_4_96', 'NeRV_vanilla')])
def test_half_engines_against_the_fp32_engine(orn, geo, kind, prec):
    """test_gpu_bf16.py::test_bf16_engine_vs_fp32_engine with act = gelu, its tolerances unchanged: loss 3e-4 (fp16) / 2e-3 (bf16)
    relative, PSNR 0.01 / 0.05 dB, decode 4e-3 / 2e-2 abs, every gradient tensor 0.6 % / 3 % relative L2."""
    ref = _one_step(orn, geo, kind, 'fp32')
    eng = _one_step(orn, geo, kind, prec)
    sf, sb = ref.stats(1)[0], eng.stats(1)[0]
    tight = prec == 'fp16'
    assert eng.scale_state()['skipped'] == 0
    worst = max(float((_slot(eng, k) - _slot(ref, k)).norm() / (_slot(ref, k).norm() + 1e-30)) for k in ref.layout if _slot(ref, k).norm() > 0)
    dimg = (eng.decode(eng.embeds[2]) - ref.decode(ref.embeds[2])).abs().max().item()
    print(f'{geo} {kind} {prec}: loss {sb[0].item():.6f} vs {sf[0].item():.6f}, decode {dimg:.2e}, worst gradient rel-L2 {worst:.2e}')
    assert abs(sb[0] - sf[0]) <= (3e-4 if tight else 2e-3) * abs(sf[0]), (sb, sf)
    assert abs(sb[4] - sf[4]) <= (0.01 if tight else 0.05), (sb, sf)
    assert dimg < (4e-3 if tight else 2e-2)
    assert worst < (6e-3 if tight else 3e-2), worst


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_pipelined_graph_and_eager_steps_are_the_same_bits(orn, prec):
    outs = []
    for mode in (True, None, False):
        gen = act_fixture.tiny_generator('ERB', True, 'gelu', **SMALL['2_3_26'])
        eng = orn.engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5, precision=prec)
        _video(eng, 4)
        eng.set_schedule([(k % 4, k + 1, 5e-4) for k in range(5)])
        eng.run(5, graph=mode)
        torch.cuda.synchronize()
        assert eng.scale_state()['skipped'] == 0
        outs.append((eng.params.clone(), eng.stats(5).clone()))
    for p, s in outs[1:]:
        assert torch.equal(p, outs[0][0]) and torch.equal(s, outs[0][1])


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_batched_step(orn, prec):
    def engine():
        gen = act_fixture.tiny_generator('NeRV_vanilla', True, 'gelu', **SMALL['3_4_96'])
        eng = orn.engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5, precision=prec)
        _video(eng, 4)
        return eng
    single = []
    for f in (3, 1):
        e = engine()
        e.set_schedule([(f, 1, 0.0)])
        e.run(1, graph=False)
        torch.cuda.synchronize()
        single.append(e.grads.clone())
    e1 = engine()
    e1.set_schedule([(3, 1, 0.0)])
    e1.run_batched(1, 1)
    torch.cuda.synchronize()
    assert torch.equal(e1.grads, single[0])                               # batch 1: the bits of the single-frame step
    e2 = engine()
    e2.set_schedule([(3, 1, 0.0), (1, 1, 0.0)])
    e2.run(1, batch=2)
    torch.cuda.synchronize()
    assert torch.equal(e2.grads, (single[0] + single[1]) * 0.5)           # vanilla: every slot is written directly; (g0 + g1) * (1 / 2)


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_multi_resolution_engine_graph_is_eager(orn, prec):
    """A head and a loss at every stage (sin_res=False), gelu: graph replay == one call per step, and the side stages train."""
    outs = []
    for mode in (True, False):
        gen = act_fixture.tiny_generator('ERB', False, 'gelu', **SMALL['3_4_96'])
        eng = orn.engine.TrainEngine(gen, loss_type='L1', beta=0.5, precision=prec, lw=0.7)      # (6 x 8 side stage: no SSIM window fits)
        _video(eng, 4)
        eng.set_schedule([(k % 4, k + 1, 5e-4) for k in range(4)])
        p0 = eng.params.clone()
        eng.run(4, graph=mode)
        torch.cuda.synchronize()
        assert eng.scale_state()['skipped'] == 0
        off, n = eng.layout['head_layers.0.weight']
        assert not torch.equal(eng.params[off:off + n], p0[off:off + n])
        outs.append((eng.params.clone(), eng.stats(4).clone(), eng.stage_stats(4).clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


def test_split_step_matches_the_built_in_loss(orn):
    res = []
    for split in (False, True):
        gen = act_fixture.tiny_generator('ERB', True, 'gelu', **SMALL['3_4_96'])
        eng = orn.engine.TrainEngine(gen, loss_type='L2', beta=0.5, precision='fp16')
        _video(eng, 4)
        eng.set_schedule([(k % 4, k + 1, 5e-4) for k in range(3)])
        if split:
            eng.run_with(lambda p, t: F.mse_loss(p, t), 3)
        else:
            eng.run(3, graph=False)
        torch.cuda.synchronize()
        res.append((eng.params.clone(), eng.stats(3)[:, 0].clone()))
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-5, atol=1e-7)
    # the caller's dLoss/dpred is torch's 2 (p - t) / N, the kernel's its own product: a few fp32 ulps of the gradient, then three Adam steps
    assert (res[0][0] - res[1][0]).abs().max().item() < 0.05 * 5e-4


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_decode_frames_against_the_mirror(orn, prec):
    gen = act_fixture.tiny_generator('ERB', True, 'gelu', **SMALL['3_4_96']).cuda()
    eng = orn.engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5, precision=prec)
    frames, embeds = _video(eng, 4)
    with torch.no_grad():
        want = torch.cat([gen(embeds[k:k + 1].cuda())[0] for k in range(4)])
    out = eng.decode_frames(f32=True)
    torch.cuda.synchronize()
    tol = 2e-6 if prec == 'fp32' else 4e-3        # fp16: test_gpu_bf16.py's decode tolerance (11-bit activations, an image in [0, 1])
    assert (out['img'] - want).abs().max().item() < tol
    # the output stage against the engine's own head forward, which tests/test_gpu_act_forms.py pins to fp64: the same bits
    for k in range(4):
        assert torch.equal(out['img'][k:k + 1], eng.decode(embeds[k])), k
    # bytes and PSNR against the MIRROR's image, not the engine's: a byte may differ only where the mirror's x * 255 + 0.5 lies within
    # tol * 255 of an integer, and then by one; the PSNR is that of the mirror's image to what tol moves an mse (2 tol sqrt(mse) + tol^2)
    v = want * 255.0 + 0.5
    q = torch.clamp(v, 0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    diff = (out['rgb8'].int() - q.int()).abs()
    near = ((v - torch.round(v)).abs() <= tol * 255.0 + 1e-4).permute(0, 2, 3, 1)
    assert int(diff.max()) <= 1 and bool((diff[~near] == 0).all()), (int(diff.max()), int((diff[~near] != 0).sum()))
    assert torch.equal(out['rgb8'], torch.clamp(out['img'] * 255.0 + 0.5, 0, 255).to(torch.uint8).permute(0, 2, 3, 1))
    mse = ((want - frames.cuda()) ** 2).mean(dim=(1, 2, 3))
    dmse = 2 * tol * mse.sqrt() + tol * tol
    lo, hi = -10.0 * torch.log10(mse + dmse), -10.0 * torch.log10((mse - dmse).clamp_min(1e-30))
    psnr = out['stats'][:, 1]
    assert bool(((psnr >= lo - 1e-3) & (psnr <= hi + 1e-3)).all()), (psnr, lo, hi)
    sw = act_fixture.tiny_generator('ERB', True, 'swish', **SMALL['3_4_96'])
    es = orn.engine.Decoder(sw, precision=prec)
    other = es.decode_frames(embeds=embeds, frames=frames, f32=True)['img']
    assert (other - out['img']).abs().max().item() > 1e-4                 # the decode evaluates the activation it was given


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_ecb_engine_is_the_vanilla_engine_on_its_merged_kernel(orn, prec):
    gen = act_fixture.tiny_generator('ECB', True, 'gelu')
    eng = orn.engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5, precision=prec)
    _video(eng, 5)
    rows = [0, 2, 4]
    bytes_k = eng.decode_frames(rows=rows, stats=False)['rgb8'].clone()
    fused = [eng.engine_fused_kernel(i) for i in range(len(gen.layers))]
    van = act_fixture.tiny_generator('NeRV_vanilla', True, 'gelu')
    sd = {k: v.detach().clone() for k, v in gen.state_dict().items() if not k.startswith('layers.')}
    for i, (wf, bf_) in enumerate(fused):
        sd[f'layers.{i}.branch.weight'], sd[f'layers.{i}.branch.bias'] = wf, bf_
    van.load_state_dict(sd)
    veng = orn.engine.TrainEngine(van, loss_type='Fusion6', beta=0.5, precision=prec)
    _video(veng, 5)
    assert torch.equal(veng.decode_frames(rows=rows, stats=False)['rgb8'], bytes_k)
    for e in (eng, veng):
        e.set_schedule([(3, 1, 5e-4)])
        e.run(1, graph=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.stats(1), veng.stats(1))
    for name in [k for k in eng.layout if not k.startswith('layers.')]:
        assert torch.equal(_slot(eng, name), _slot(veng, name)), name
    for i in range(len(gen.layers)):
        assert torch.equal(_slot(eng, f'layers.{i}.rbr_3x3_branch.weight'), _slot(veng, f'layers.{i}.branch.weight')), i


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
CLI = ('-e 2 --lower_width 8 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 --reduction 2 '
       '--fc_hw_dim 3_4_8 --expansion 1 --single_res --loss Fusion6 --warmup 0.2 --lr_type cosine --strides 2 2 --conv_type conv -b 1 '
       '--lr 0.0005 --norm none --outf gelu_t --branch_type ERB --synthetic 6 --precision fp32').split()


def test_cli_without_act_trains_and_evaluates_with_gelu(orn, tmp_path, monkeypatch):
    from orn_amd import main_eval, main_train
    monkeypatch.chdir(tmp_path)
    args = main_train.parse_args(CLI)
    assert args.act == 'gelu'
    best = main_train.train(args)['synthetic0']
    assert math.isfinite(best) and best > 5.0
    outf = tmp_path / 'result' / 'gelu_t'
    assert (outf / 'model_latest.pth').exists() and (outf / 'model_latest_deploy.pth').exists()
    ck = torch.load(outf / 'model_latest.pth', map_location='cpu', weights_only=True)
    assert not any('act' in k for k in ck)                                 # a checkpoint stores no activation
    mirror = main_eval.main(CLI + ['--act', 'gelu'])
    native = main_eval.main(CLI + ['--act', 'gelu', '--decoder', 'engine'])
    assert abs(mirror - native) < 1e-3 and abs(mirror - best) < 3.0
    swish = main_eval.main(CLI + ['--act', 'swish'])
    assert swish != mirror                                                 # evaluation must be given the --act the fit used
