"""GPU tests of the multi-resolution engine (include/orn.h, N8): a head and a loss at every stage, the objective of
main_train.py:239-250, sum_{i < n-1} lw * loss(out_i, target_i) + loss(out_{n-1}, target_{n-1}).

Geometries: fc 2_3_26, strides 5 2 2, lower_width 96 -> stages 10x15 (26 channels, an fp32 block in every precision), 20x30 and 40x60
(96 channels, 16-bit blocks in the 16-bit modes); fc 3_4_26 for the SSIM losses (smallest stage 15x20: the 11x11 window fits)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multires_fixture as mf

pytestmark = pytest.mark.gpu

FC, FC_SSIM, STRIDES = '2_3_26', '3_4_26', [5, 2, 2]
N_FRAMES = 5
PRECS = ('fp32', 'fp16', 'bf16')


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _generator(bt, sin_res, fc=FC, strides=STRIDES, lower_width=96):
    return mf.tiny_generator(bt, sin_res=sin_res, strides=strides, fc=fc, lower_width=lower_width)


_VIDEO = {}


def _video(hw, n=N_FRAMES):
    """Seeded frames and embeddings of one size, made once and never modified."""
    if (hw, n) not in _VIDEO:
        from oracle import cpu_ref
        _VIDEO[(hw, n)] = (cpu_ref.synthetic_video(n, hw[0], hw[1], seed=5),
                           cpu_ref.positional_encoding(torch.tensor([k / n for k in range(n)]), 1.25, 40))
    return _VIDEO[(hw, n)]


def _engine(orn, gen, prec, loss='L2', lw=1.0, n=N_FRAMES):
    eng = orn.engine.TrainEngine(gen, loss_type=loss, beta=0.5, precision=prec, lw=lw)
    eng.set_video(*_video(tuple(eng.out_hw), n))
    return eng


def _single_twin(multi, bt, fc=FC, strides=STRIDES):
    """A single-resolution generator holding the tensors the two share: stem, blocks and the last head."""
    single = _generator(bt, True, fc, strides)
    msd = multi.state_dict()
    single.load_state_dict({k: msd[k].detach().clone() for k in single.state_dict()})
    return single


def _slot(eng, arena, name):
    off, n = eng.layout[name]
    return arena[off:off + n]


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(eng, entries, form):
    eng.set_schedule(entries)
    eng.run(len(entries), graph={'eager': False, 'graph': True}[form])
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 1. lw = 0: the single-resolution engine's bits
@pytest.mark.parametrize('form', ['eager', 'graph'])
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('bt', ['NeRV_vanilla', 'ERB'])
def test_zero_weight_is_the_single_resolution_engine(orn, bt, prec, form):
    """Adding an exact zero changes nothing: after one step and after three, parameters, gradients, Adam moments of every shared tensor
    and the step records are those of a single-resolution engine; the side heads get gradients of exactly 0 and keep their bits."""
    multi = _generator(bt, False)
    single = _single_twin(multi, bt)
    em = _engine(orn, multi, prec, 'L2', lw=0.0)
    es = _engine(orn, single, prec, 'L2')
    side0 = {k: _slot(em, em.params, k).clone() for k in em.layout if k not in es.layout}
    assert sorted(side0) == ['head_layers.0.bias', 'head_layers.0.weight', 'head_layers.1.bias', 'head_layers.1.weight']
    entries = [(3, 1, 5e-4), (0, 2, 4e-4), (4, 3, 3e-4)]
    done = 0
    for upto in (1, 3):
        for e in (em, es):
            _run(e, [entries[i] for i in range(done, upto)], form)
        done = upto
        for arena in ('params', 'grads', 'adam_m', 'adam_v'):
            for k in es.layout:
                assert bits_equal(_slot(em, getattr(em, arena), k), _slot(es, getattr(es, arena), k)), (upto, arena, k)
        n = upto - (0 if upto == 1 else 1)
        assert bits_equal(em.stats(n), es.stats(n)), (upto, em.stats(n), es.stats(n))
        for k, p0 in side0.items():
            assert float(_slot(em, em.grads, k).abs().max()) == 0.0, k
            assert bits_equal(_slot(em, em.params, k), p0), k
        assert em.scale_state()['skipped'] == 0 and es.scale_state()['skipped'] == 0
    ss = em.stage_stats(1)[0]
    assert torch.isfinite(ss).all() and float(ss[:, 0].min()) > 0            # the side losses were computed (and weighted by 0)


# ---------------------------------------------------------------- 2. the reference fixture
@pytest.mark.parametrize('loss', ['L2', 'L1'])
@pytest.mark.parametrize('kind', mf.KINDS)
def test_against_the_reference_fixture(orn, kind, loss):
    """Every stage's image, its pooled target, the loss sum and every gradient of the reference's multi-resolution generator
    (tests/golden/multires.npz, lw = 0.7), under the rule of test_gpu_parity.test_tiny_generator_golden: images rtol 1e-5 / atol 2e-6,
    loss 1e-6, gradients rtol 2e-4 / atol 2e-5 max|g|.  Images through the eager mirror (the engine keeps its own inside its
    workspace); targets, per-stage losses, loss sum and gradients from one fp32 engine step at lr 0."""
    g = mf.load()
    tag = f'tiny_{kind}'
    lw = float(g['lw'][0])
    gen = mf.tiny_generator(kind)
    gen.load_state_dict({k: torch.from_numpy(g[f'{tag}/sd/{k}']) for k in g[f'{tag}/keys']})
    embed = torch.from_numpy(g[f'{tag}/embed'])
    eng = orn.engine.TrainEngine(gen, loss_type=loss, beta=0.5, precision='fp32', lw=lw)
    eng.set_video(torch.from_numpy(g[f'{tag}/data']), embed)
    assert torch.equal(eng.stage_frames[0].cpu(), torch.from_numpy(g[f'{tag}/target0']))     # adaptive_avg_pool2d, bit for bit
    assert torch.equal(eng.frames.cpu(), torch.from_numpy(g[f'{tag}/target1']))
    with torch.no_grad():
        outs = gen(embed.cuda())
    assert len(outs) == 2
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.cpu().numpy(), g[f'{tag}/img{i}'], rtol=1e-5, atol=2e-6)
    _run(eng, [(0, 1, 0.0)], 'eager')
    st, ss = eng.stats(1)[0], eng.stage_stats(1)[0]
    assert abs(float(st[0]) - float(g[f'{tag}/{loss}/loss'])) < 1e-6
    for i in range(2):
        assert abs(float(ss[i, 0]) - float(g[f'{tag}/{loss}/loss{i}'])) < 1e-6, i
    for k, p in gen.named_parameters():
        r = g[f'{tag}/{loss}/grad/{k}']
        got = _slot(eng, eng.grads, k).view(p.shape).cpu().numpy()
        np.testing.assert_allclose(got, r, rtol=2e-4, atol=2e-5 * max(np.abs(r).max(), 1e-6), err_msg=k)


# ---------------------------------------------------------------- 3. / 4. fp64 autograd on a plain-torch multi-branch forward
def _fp64_losses(sd, embed, frame, fc, strides, bt, loss, lw):
    """(weighted loss sum, [loss_i], [out_i]) in the dtype of sd: the oracle's forward with a head on every stage's activation, the
    targets pooled from the fp32 frame as the reference pools them."""
    from oracle import cpu_ref
    _, inter = cpu_ref.generator_forward(sd, embed, fc, strides, bt, return_intermediates=True)
    outs = [cpu_ref.head_forward(a, sd[f'head_layers.{i}.weight'], sd[f'head_layers.{i}.bias']) for i, a in enumerate(inter[1:])]
    targets = [F.adaptive_avg_pool2d(frame, o.shape[-2:]).to(o.dtype) for o in outs]
    losses = [cpu_ref.loss_fn(o, t, loss) for o, t in zip(outs, targets)]
    total = sum(l_ * (lw if i < len(losses) - 1 else 1) for i, l_ in enumerate(losses))
    return total, losses, outs


_REF = {}


def _fp64_grads(bt, loss, fc, sin_res, lw, frame_idx, sd0):
    key = (bt, loss, fc, sin_res, lw, frame_idx)
    if key not in _REF:
        hw = tuple(int(x) * 20 for x in fc.split('_')[:2])
        frames, embeds = _video(hw)
        params = {k: v.detach().double().requires_grad_(True) for k, v in sd0.items()}
        if sin_res:
            from oracle import cpu_ref
            out = cpu_ref.generator_forward(params, embeds[frame_idx:frame_idx + 1].double(), fc, STRIDES, bt)[0]
            total = cpu_ref.loss_fn(out, frames[frame_idx:frame_idx + 1].double(), loss)
            losses = [total]
        else:
            total, losses, _ = _fp64_losses(params, embeds[frame_idx:frame_idx + 1].double(), frames[frame_idx:frame_idx + 1], fc, STRIDES, bt, loss, lw)
        total.backward()
        _REF[key] = (total.item(), [l_.item() for l_ in losses], {k: p.grad for k, p in params.items()})
    return _REF[key]


def _grad_figures(eng, ref):
    """max|g - g64| / max|g64| and the relative L2 distance, per tensor."""
    out = {}
    for k, r in ref.items():
        got = _slot(eng, eng.grads, k).cpu().double()
        out[k] = (float((got - r.flatten()).abs().max() / r.abs().max()), float((got - r.flatten()).norm() / r.norm()))
    return out


@pytest.mark.parametrize('loss,fc', [('L2', FC), ('Fusion6', FC_SSIM)])
@pytest.mark.parametrize('prec', PRECS)
def test_one_step_against_fp64_autograd(orn, prec, loss, fc):
    """lw = 0.7, one step at lr 0, ERB: the loss sum, every stage's loss and every gradient tensor against fp64 autograd.
    fp32 engine: the project's fp32 parity rule (loss 5e-5 relative, relative L2 per gradient tensor below 2e-3).
    16-bit engines: max|g - g64| / max|g64| per tensor against the same figure of the SINGLE-resolution engine of that precision and
    geometry on its own fp64 reference -- a code path this feature leaves alone -- times two: one more 16-bit rounding per stage enters
    dz.  A side head has no single-resolution counterpart: it is held to twice the worst figure of the single-resolution tensors.
    Measured on an MI355X (worst multi / single ratio over the shared tensors; side heads against the worst single figure):
    see DESIGN 4.12."""
    lw, f = 0.7, 3
    multi = _generator('ERB', False, fc)
    sd0 = {k: v.detach().clone() for k, v in multi.state_dict().items()}
    em = _engine(orn, multi, prec, loss, lw=lw)
    _run(em, [(f, 1, 0.0)], 'eager')
    total, losses, ref = _fp64_grads('ERB', loss, fc, False, lw, f, sd0)
    st, ss = em.stats(1)[0], em.stage_stats(1)[0]
    tol_loss = 5e-5 if prec == 'fp32' else 3e-4
    assert abs(float(st[0]) - total) <= tol_loss * abs(total), (float(st[0]), total)
    for i, l_ in enumerate(losses):
        assert abs(float(ss[i, 0]) - l_) <= tol_loss * abs(l_), (i, float(ss[i, 0]), l_)
    assert set(ref) == set(em.layout) and em.scale_state()['skipped'] == 0
    fm = _grad_figures(em, ref)
    if prec == 'fp32':
        worst = max(fm.items(), key=lambda kv: kv[1][1])
        print(f'\nmulti-res fp32 {loss}: worst relative L2 gradient distance {worst[1][1]:.2e} at {worst[0]}')
        assert worst[1][1] < 2e-3, worst
        return
    single = _single_twin(multi, 'ERB', fc)
    ssd0 = {k: v.detach().clone() for k, v in single.state_dict().items()}
    es = _engine(orn, single, prec, loss)
    _run(es, [(f, 1, 0.0)], 'eager')
    fs = _grad_figures(es, _fp64_grads('ERB', loss, fc, True, 1.0, f, ssd0)[2])
    cap = max(v[0] for v in fs.values())
    ratios = {k: fm[k][0] / (fs[k][0] if k in fs else cap) for k in fm}
    worst = max(ratios.items(), key=lambda kv: kv[1])
    print(f'\nmulti-res {prec} {loss}: max|g - g64| / max|g64| relative to the single-resolution engine: worst {worst[1]:.2f} at {worst[0]}; '
          f'side heads ' + ', '.join(f'{k} {ratios[k]:.2f}' for k in sorted(ratios) if k not in fs))
    for k, r in ratios.items():
        assert r <= 2.0, (k, r, fm[k], fs.get(k, cap))


@pytest.mark.parametrize('bt', ['NeRV_vanilla', 'ERB'])
def test_three_steps_against_fp64_adam(orn, bt):
    """Three optimiser steps of the fp32 engine (Fusion6, lw = 0.7) against fp64 autograd + Adam: every tensor, the side heads'
    included, within 0.75 lr (the rule of test_gpu_branch_kinds.test_three_steps_against_fp64_multi_branch)."""
    from oracle import cpu_ref
    lw = 0.7
    gen = _generator(bt, False, FC_SSIM)
    sd0 = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    eng = _engine(orn, gen, 'fp32', 'Fusion6', lw=lw)
    frames, embeds = _video(tuple(eng.out_hw))
    entries = [(3, 1, 5e-4), (0, 2, 4e-4), (4, 3, 3e-4)]
    _run(eng, entries, 'eager')
    st = eng.stats(3).numpy()
    sd = {k: v.double() for k, v in sd0.items()}
    am = {k: torch.zeros_like(v) for k, v in sd.items()}
    av = {k: torch.zeros_like(v) for k, v in sd.items()}
    for i, (f, step, lr) in enumerate(entries):
        params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        total, _, _ = _fp64_losses(params, embeds[f:f + 1].double(), frames[f:f + 1], FC_SSIM, STRIDES, bt, 'Fusion6', lw)
        total.backward()
        assert abs(st[i, 0] - total.item()) < 5e-5 * 3, (i, st[i], total.item())
        with torch.no_grad():
            for k in sd:
                cpu_ref.adam_step(sd[k], params[k].grad, am[k], av[k], step, lr, 0.5)
    new = gen.state_dict()
    worst = max((float((new[k].cpu().double() - sd[k]).abs().max()), k) for k in sd)
    print(f'\n{bt}: worst parameter distance from fp64 autograd + Adam after 3 multi-resolution steps: {worst[0] / 5e-4:.3f} lr at {worst[1]}')
    for k in sd:
        assert float((new[k].cpu().double() - sd[k]).abs().max()) < 0.75 * 5e-4, k
    assert eng.scale_state()['skipped'] == 0


# ---------------------------------------------------------------- 5. the batched step
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_batch_of_two_is_the_mean_of_two_steps(orn, prec):
    """-b 2 (vanilla: every slot, the side heads' included, is written directly): the gradient is (g0 + g1) * 0.5 in fp32, bit for bit,
    of the two single-frame multi-resolution gradients (the rule of test_gpu_batch.test_batch_gradient_is_the_ordered_fp32_sum), and
    the per-stage ring holds the two frames' values."""
    rows, g, ss1 = [3, 1], [], []
    for f in rows:
        e = _engine(orn, _generator('NeRV_vanilla', False), prec, 'L2', lw=0.7)
        _run(e, [(f, 1, 0.0)], 'eager')
        g.append(e.grads.clone())
        ss1.append(e.stage_stats(1)[0])
    eng = _engine(orn, _generator('NeRV_vanilla', False), prec, 'L2', lw=0.7)
    eng.set_schedule([(f, 1, 0.0) for f in rows])
    eng.run(1, batch=2)
    torch.cuda.synchronize()
    want = (g[0] + g[1]) * 0.5
    for k in eng.layout:
        assert bits_equal(_slot(eng, eng.grads, k), _slot(eng, want, k)), k
    assert float(_slot(eng, eng.grads, 'head_layers.0.weight').abs().max()) > 0
    ss = eng.stage_stats(2)
    for j in range(2):
        assert bits_equal(ss[j], ss1[j]), (j, ss[j], ss1[j])
    st = eng.stats(1)[0]
    lsum = [float(torch.tensor(0.7) * s[0, 0] + torch.tensor(0.7) * s[1, 0] + s[2, 0]) for s in ss1]
    assert abs(float(st[0]) - 0.5 * (lsum[0] + lsum[1])) < 1e-6 * abs(float(st[0]))


# ---------------------------------------------------------------- 6. another block kind
def test_acb_side_heads_equal_the_vanilla_engine_on_the_merged_kernel(orn):
    """The merge side is untouched: an ACB engine's step (lw = 0.7) gives the side heads the gradients of a vanilla engine that is
    handed the merged kernels, bit for bit."""
    gen = _generator('ACB', False)
    eng = _engine(orn, gen, 'fp16', 'L2', lw=0.7)
    eng.decode_frames(rows=[0], stats=False)
    fused = [eng.engine_fused_kernel(i) for i in range(3)]
    van = _generator('NeRV_vanilla', False)
    sd = {k: v.detach().clone() for k, v in gen.state_dict().items() if not k.startswith('layers.')}
    for i, (wf, bf_) in enumerate(fused):
        sd[f'layers.{i}.branch.weight'], sd[f'layers.{i}.branch.bias'] = wf, bf_
    van.load_state_dict(sd)
    veng = _engine(orn, van, 'fp16', 'L2', lw=0.7)
    for e in (eng, veng):
        _run(e, [(2, 1, 5e-4)], 'eager')
    assert eng.scale_state()['skipped'] == 0
    for k in [k for k in eng.layout if not k.startswith('layers.')]:
        assert bits_equal(_slot(eng, eng.grads, k), _slot(veng, veng.grads, k)), k
    assert float(_slot(eng, eng.grads, 'head_layers.1.weight').abs().max()) > 0
    assert bits_equal(eng.stage_stats(1), veng.stage_stats(1))


# ---------------------------------------------------------------- 7. decode
@pytest.mark.parametrize('prec', PRECS)
def test_decode_is_the_last_stage(orn, prec):
    """decode_frames of a multi-resolution engine and of the decode-only engine of its model: the bytes of a single-resolution
    engine holding the same shared tensors (no side head runs)."""
    multi = _generator('ERB', False)
    single = _single_twin(multi, 'ERB')
    rows = [0, 2, 4]
    em, es = _engine(orn, multi, prec), _engine(orn, single, prec)
    want = es.decode_frames(rows=rows, f32=True)
    got = em.decode_frames(rows=rows, f32=True)
    for k in ('rgb8', 'img', 'stats'):
        assert torch.equal(got[k], want[k]), k
    dec = orn.engine.Decoder(multi, precision=prec)
    assert dec.desc.multi_res == 0
    assert torch.equal(dec.decode_frames(rows=rows, embeds=em.embeds, stats=False)['rgb8'], want['rgb8'])


# ---------------------------------------------------------------- 8. the guard
@pytest.mark.parametrize('prec', PRECS)
def test_a_side_head_out_of_range_skips_the_step(orn, prec):
    """A side head's bias at +inf: tanh hides it (out = 1, du = 0, every gradient finite), the flag of the head's pre-activation does
    not.  The step is skipped and counted; parameters and moments keep their bits."""
    eng = _engine(orn, _generator('ERB', False), prec, 'L2', lw=0.7)
    _run(eng, [(1, 1, 5e-4)], 'eager')
    assert eng.scale_state()['skipped'] == 0
    with torch.no_grad():
        _slot(eng, eng.params, 'head_layers.1.bias')[0] = float('inf')
    before = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
    _run(eng, [(2, 2, 5e-4)], 'eager')
    s = eng.scale_state()
    assert s['skipped'] == 1 and s['flag'] == 1, s
    for a, b in zip(before, (eng.params, eng.adam_m, eng.adam_v)):
        assert bits_equal(a, b)
    assert eng.applied_steps() == 1


def test_refusals_name_the_stage(orn):
    """An MS-SSIM loss at 40x60 is refused at creation as before (the output); an SSIM loss whose window does not fit stage 0
    (10x15) names that stage; the split step is refused."""
    with pytest.raises(orn.OrnError, match='stage 0 .10x15.'):
        orn.engine.TrainEngine(_generator('ERB', False), loss_type='Fusion6', precision='fp16')
    with pytest.raises(orn.OrnError, match='MS-SSIM'):
        orn.engine.TrainEngine(_generator('ERB', False), loss_type='Fusion10', precision='fp16')
    big = _generator('NeRV_vanilla', False, '21_21_26', [4, 2], 96)              # stages 84x84, 168x168
    with pytest.raises(orn.OrnError, match='stage 0 .84x84.*MS-SSIM'):
        orn.engine.TrainEngine(big, loss_type='Fusion10', precision='fp32')
    eng = _engine(orn, _generator('ERB', False), 'fp32')
    eng.set_schedule([(0, 1, 5e-4)])
    with pytest.raises(orn.OrnError, match='split step'):
        eng.forward_step()


# ---------------------------------------------------------------- 9. a short fit
def test_short_fit_fp16_follows_fp32(orn):
    """30 epochs of 8 frames, lw = 1, Fusion6: the last epoch's last-stage train PSNR of the fp16 engine within 0.05 dB of the fp32
    engine's; no step skipped."""
    psnr = {}
    for prec in ('fp32', 'fp16'):
        eng = _engine(orn, _generator('ERB', False, FC_SSIM), prec, 'Fusion6', lw=1.0, n=8)
        g = torch.Generator()
        step = 0
        for epoch in range(30):
            g.manual_seed(100 + epoch)
            order = torch.randperm(8, generator=g).tolist()
            entries = []
            for f in order:
                step += 1
                entries.append((f, step, 5e-4))
            eng.set_schedule(entries)
            eng.run(8)
        torch.cuda.synchronize()
        psnr[prec] = float(eng.stats(8)[:, 4].mean())
        assert eng.scale_state()['skipped'] == 0 and eng.scale_state()['late_skipped'] == 0
        ss = eng.stage_stats(8)
        assert torch.equal(ss[:, 2, 1], eng.stats(8)[:, 4])                # the last stage's column is the record's PSNR
    print(f'\nshort multi-resolution fit: last-epoch last-stage PSNR fp32 {psnr["fp32"]:.4f} dB, fp16 {psnr["fp16"]:.4f} dB')
    assert abs(psnr['fp16'] - psnr['fp32']) <= 0.05, psnr


# ---------------------------------------------------------------- 10. the CLIs
CLI = ('-e 2 --lower_width 8 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 --reduction 2 '
       '--fc_hw_dim 3_4_8 --expansion 1 --loss L2 --warmup 0.2 --lr_type cosine --strides 2 2 2 --conv_type conv -b 1 --lw 0.5 '
       '--lr 0.0005 --norm none --act swish --outf multires_t --branch_type ERB --synthetic 6 --precision fp32 --eval_freq 1').split()


def test_cli_trains_and_evaluates_without_single_res(orn, tmp_path, monkeypatch):
    import re
    from orn_amd import checkpoint, main_eval, main_train
    monkeypatch.chdir(tmp_path)
    assert not main_train.parse_args(CLI).single_res and main_train.parse_args(CLI).lw == 0.5
    main_train.train(main_train.parse_args(CLI))
    outf = tmp_path / 'result' / 'multires_t'
    log = (outf / 'rank0.txt').read_text()
    cols = re.findall(r'PSNR: \[([0-9.]+), ([0-9.]+), ([0-9.]+)\], best: ([0-9.]+)', log)
    assert len(cols) == 2, log
    assert all(abs(float(c[2]) - float(c[3])) < 0.011 or float(c[3]) > float(c[2]) for c in cols)     # best follows the last stage
    for name in ('model_latest.pth', 'model_latest_deploy.pth'):
        sd = checkpoint.load_state_dict_file(str(outf / name))
        for i in range(3):
            assert f'head_layers.{i}.weight' in sd and f'head_layers.{i}.bias' in sd, (name, i)
    p_eager = main_eval.main(CLI)
    p_engine = main_eval.main(CLI + ['--decoder', 'engine'])
    assert 5.0 < p_engine < 60.0 and abs(p_eager - p_engine) < 0.01, (p_eager, p_engine)
    m = re.findall(r'Eval best_PSNR at epoch2:\tcurrent: ([0-9.]+)', log)
    assert m and abs(float(m[0]) - p_engine) < 0.02, (m, p_engine)                                       # the last stage's PSNR
