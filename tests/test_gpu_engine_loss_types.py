"""GPU tests of the engine trained with the losses beyond L2 / L1 / Fusion6 (include/orn.h ORN_LOSS_*): one step of Fusion10 (the
MS-SSIM loss: 5 + 1 + 5 launches inside the step) and of Fusion1 (the L2-term variant of the SSIM kernel) against the CPU oracle,
the three forms of the step against each other, the workspace, and main_train --loss_type Fusion10.

Geometry: fc 5_6_26, strides 5 2 2 2, lower_width 96 -> 200 x 240 (the one of test_gpu_eval_frames: the smallest of the bench's
layer pattern above pytorch_msssim's 160; pyramid level 3 has 25 rows, an odd size).  3 frames, ERB."""
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEO = dict(fc='5_6_26', strides=[5, 2, 2, 2], lower_width=96)
N_FRAMES = 3
# utils.py:150,168
WEIGHTS = {'Fusion1': (0.0, 0.3, 0.7, 'ssim'), 'Fusion10': (0.7, 0.0, 0.3, 'ms_ssim')}


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine, main_train  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _generator(orn):
    return orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=GEO['fc'], expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=GEO['strides'], sin_res=True,
                               lower_width=GEO['lower_width'], sigmoid=False, deploy=False, branch_type='ERB')


_SETUP = {}


def _setup(orn):
    """Seeded model state, video and embeddings, made once and never modified."""
    if not _SETUP:
        from oracle import cpu_ref
        torch.manual_seed(1)
        gen = _generator(orn)
        _SETUP['sd'] = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        _SETUP['frames'] = cpu_ref.synthetic_video(N_FRAMES, 200, 240, seed=5)
        _SETUP['embeds'] = cpu_ref.positional_encoding(torch.tensor([k / N_FRAMES for k in range(N_FRAMES)]), 1.25, 40)
    return _SETUP


def _engine(orn, loss_type, prec):
    s = _setup(orn)
    gen = _generator(orn)
    gen.load_state_dict(s['sd'])
    eng = orn.engine.TrainEngine(gen, loss_type=loss_type, beta=0.5, precision=prec)
    assert tuple(eng.out_hw) == (200, 240)
    eng.set_video(s['frames'], s['embeds'])
    return eng


def _composed_loss(name, p, t):
    from oracle import cpu_ref
    w1, w2, ws, kind = WEIGHTS[name]
    s = cpu_ref.ssim(p, t, data_range=1, size_average=True) if kind == 'ssim' else cpu_ref.ms_ssim(p, t, data_range=1, size_average=True)
    loss = ws * (1 - s)
    if w1:
        loss = loss + w1 * torch.mean(torch.abs(p - t))
    if w2:
        loss = loss + w2 * F.mse_loss(p, t)
    return loss


_ORACLE = {}


def _oracle_step(orn, name):
    """Loss, PSNR and every gradient tensor of one step on frame 1 by autograd over the oracle's forward, once per loss."""
    if name not in _ORACLE:
        from oracle import cpu_ref
        s = _setup(orn)
        params = {k: v.detach().clone().requires_grad_(True) for k, v in s['sd'].items()}
        out = cpu_ref.generator_forward(params, s['embeds'][1:2], GEO['fc'], GEO['strides'], 'ERB')[0]
        target = s['frames'][1:2]
        loss = _composed_loss(name, out, target)
        loss.backward()
        psnr = cpu_ref.psnr_fn([out], [target])
        _ORACLE[name] = dict(loss=loss.item(), psnr=psnr.item(), ref={k: p.grad for k, p in params.items() if p.grad is not None})
    return _ORACLE[name]


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('name', ['Fusion10', 'Fusion1'])
def test_one_step_vs_oracle(orn, name, prec):
    """lr 0: loss, PSNR and every gradient tensor of the arena against the oracle, with the tolerances of
    test_gpu_parity._check_full_step (relative L2 per tensor)."""
    o = _oracle_step(orn, name)
    eng = _engine(orn, name, prec)
    eng.set_schedule([(1, 1, 0.0)])
    eng.run(1, graph=False if prec == 'fp32' else None)
    torch.cuda.synchronize()
    st = eng.stats(1)[0].numpy()
    grads = {k: eng.grads[off:off + n].clone().cpu() for k, (off, n) in eng.layout.items()}
    ref = o['ref']
    tol_loss, tol_psnr, tol_g = {'fp32': (5e-5, 1e-3, 2e-3), 'fp16': (3e-4, 0.01, 1e-2)}[prec]
    rel = sorted(((float((grads[k] - ref[k].flatten()).norm() / (ref[k].norm() + 1e-30)), k) for k in ref), reverse=True)
    print(f'{name} {prec}: loss {st[0]:.7f} ref {o["loss"]:.7f}; psnr {st[4]:.4f} ref {o["psnr"]:.4f}; worst grads {rel[:3]}')
    assert abs(st[0] - o['loss']) <= tol_loss * abs(o['loss']), (st[0], o['loss'])
    assert abs(st[4] - o['psnr']) < tol_psnr, (st[4], o['psnr'])
    assert set(ref) == set(eng.layout)
    assert rel[0][0] < tol_g, rel[:8]
    s = eng.scale_state()
    assert s['skipped'] == 0 and s['late_skipped'] == 0, s


def test_forms_of_the_step_agree(orn):
    """Fusion10, fp16, 4 steps with lr > 0: train_step one at a time, the pipelined call and the hipGraph replay leave bit-identical
    parameter arenas and equal stats rings; no step is skipped."""
    res, p0 = [], None
    for graph in (False, None, True):
        eng = _engine(orn, 'Fusion10', 'fp16')
        p0 = eng.params.clone()
        eng.set_schedule([(k % N_FRAMES, k + 1, 5e-4) for k in range(4)])
        eng.run(4, graph=graph)
        torch.cuda.synchronize()
        s = eng.scale_state()
        assert s['skipped'] == 0 and s['late_skipped'] == 0, (graph, s)
        st = eng.stats(4).clone()
        assert bool(torch.isfinite(st).all())
        assert float(st[:, 3].min()) > 0.0 and float(st[:, 3].max()) < 1.0        # the MS-SSIM value of each step
        res.append((eng.params.clone(), st))
        del eng
    assert not torch.equal(res[0][0], p0)                                         # the steps did move the parameters
    for p, st in res[1:]:
        assert torch.equal(p, res[0][0])
        assert torch.equal(st, res[0][1])


def test_msssim_descriptor_needs_more_workspace(orn):
    """orn_engine_ws_bytes of an MS-SSIM descriptor exceeds the Fusion6 one of the same model (pyramids, level gradients,
    coefficients); an SSIM-family descriptor needs exactly the Fusion6 workspace."""
    from ctypes import byref
    L = orn._lib.lib()
    gen = _generator(orn)
    layout, total = orn.engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    sizes = {}
    for name in ('Fusion6', 'Fusion1', 'Fusion10'):
        d = orn.engine.build_desc(gen, layout, total, name, precision=2)
        sizes[name] = L.orn_engine_ws_bytes(byref(d))
    assert sizes['Fusion10'] > sizes['Fusion6'] > 0
    assert sizes['Fusion1'] == sizes['Fusion6']
    # pytorch_msssim's limit holds for the engine too: the same layer pattern with a 120 x 160 output
    small = orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim='3_4_26', expansion=1, num_blocks=1, norm='none',
                                act='swish', bias=True, reduction=2, conv_type='conv', stride_list=GEO['strides'], sin_res=True,
                                lower_width=GEO['lower_width'], sigmoid=False, deploy=False, branch_type='ERB')
    layout, total = orn.engine.arena_layout([(k, tuple(p.shape)) for k, p in small.named_parameters()])
    assert L.orn_engine_ws_bytes(byref(orn.engine.build_desc(small, layout, total, 'Fusion6', precision=2))) > 0
    assert L.orn_engine_ws_bytes(byref(orn.engine.build_desc(small, layout, total, 'Fusion10', precision=2))) == 0
    assert '160' in orn._lib.last_error()


def test_train_cli_with_fusion10(tmp_path, monkeypatch):
    """main_train --loss_type Fusion10 on synthetic frames at the 200 x 240 geometry: the run completes, logs PSNR per epoch and
    MS-SSIM per evaluation, and the fit improves."""
    from orn_amd import main_train
    flags = ('-e 4 --lower_width 96 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 512_1 '
             '--reduction 2 --fc_hw_dim 5_6_26 --expansion 1 --single_res --loss_type Fusion10 --warmup 0.2 --lr_type cosine '
             '--strides 5 2 2 2 --conv_type conv -b 1 --lr 0.0005 --norm none --act swish --outf f10_t --branch_type ERB '
             '--synthetic 12 --eval_freq 2').split()
    monkeypatch.chdir(tmp_path)
    best = main_train.train(main_train.parse_args(flags))
    assert list(best) == ['synthetic0']
    log = (tmp_path / 'result' / 'f10_t' / 'rank0.txt').read_text()
    psnr = [float(x) for x in re.findall(r'Epoch\[\d+/4\], lr:\S+ PSNR: ([0-9.]+)', log)]
    ms = [float(x) for x in re.findall(r'train MS-SSIM ([0-9.]+)', log)]
    print(psnr, ms)
    assert len(psnr) == 4 and len(ms) >= 2
    assert psnr[-1] > psnr[0]
    assert all(0.0 < m <= 1.0 for m in ms)
    assert 'steps skipped' not in log
