"""GPU tests of the split step (orn_engine_step_forward / orn_engine_step_backward; TrainEngine.forward_step, backward_step,
step_with, run_with), of orn_amd.custom_losses and of main_train --custom_loss.

Geometries, lower_width 96, stem 32_1, three synthetic frames: A = fc 2_3_26, strides 5 2 2 -> 40 x 60 (one ragged 16x64 tile column,
a ragged last tile row); B = fc 2_4_26 -> 40 x 80 (two tile columns, the second ragged).  Both widths are multiples of 4 (the loss
stage's float4 form); a dpred that starts 4 bytes off a 16-byte boundary takes its scalar form.  Blocks 1 and 2 run on the 16-bit
kernels in the 16-bit modes, block 0 on the fp32 first block."""
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEOS = {'A': dict(fc='2_3_26', strides=[5, 2, 2], hw=(40, 60)), 'B': dict(fc='2_4_26', strides=[5, 2, 2], hw=(40, 80))}
N_FRAMES = 3
LR = 5e-4


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine, main_train, custom_losses  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _generator(orn, geo, branch):
    g = GEOS[geo]
    return orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=g['fc'], expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=g['strides'], sin_res=True,
                               lower_width=96, sigmoid=False, deploy=False, branch_type=branch)


_SETUP = {}


def _setup(orn, geo, branch):
    """Seeded model state, video and embeddings per (geometry, branch), made once and never modified."""
    key = (geo, branch)
    if key not in _SETUP:
        from oracle import cpu_ref
        torch.manual_seed(1)
        gen = _generator(orn, geo, branch)
        H, W = GEOS[geo]['hw']
        _SETUP[key] = dict(sd={k: v.detach().clone() for k, v in gen.state_dict().items()},
                           frames=cpu_ref.synthetic_video(N_FRAMES, H, W, seed=5),
                           embeds=cpu_ref.positional_encoding(torch.tensor([k / N_FRAMES for k in range(N_FRAMES)]), 1.25, 40))
    return _SETUP[key]


def _engine(orn, geo, branch, prec, loss_type='Fusion6'):
    s = _setup(orn, geo, branch)
    gen = _generator(orn, geo, branch)
    gen.load_state_dict(s['sd'])
    eng = orn.engine.TrainEngine(gen, loss_type=loss_type, beta=0.5, precision=prec)
    assert tuple(eng.out_hw) == GEOS[geo]['hw']
    eng.set_video(s['frames'], s['embeds'])
    return eng


def _fusion6_seam_step(orn, eng, frame, spoil=None, misalign=False):
    """One split step fed by the library's own Fusion6 kernel (ops.loss_stats): what a built-in step computes, through the seam."""
    pred = eng.forward_step()
    stats, g = orn.ops.loss_stats(pred, eng.frames[frame:frame + 1], 'Fusion6', want_grad=True)
    loss = stats[0]
    if misalign:                                            # same values, 4 bytes past a 16-byte boundary: the scalar loads
        buf = torch.empty(g.numel() + 4, device=g.device)
        assert buf.data_ptr() % 16 == 0
        buf[1:1 + g.numel()].copy_(g.reshape(-1))
        g = buf[1:1 + g.numel()].view(g.shape)
        assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    if spoil == 'dpred':
        g.view(-1)[-1] = float('nan')                       # the last pixel of the last plane
    if spoil == 'loss':
        loss = loss * float('nan')
    eng.backward_step(g, loss)


# ---- 1. the seam adds no arithmetic ---------------------------------------------------------------------------------
@pytest.mark.parametrize('geo,branch,prec,misalign', [('A', 'ERB', 'fp32', False), ('A', 'ERB', 'fp16', False), ('B', 'ERB', 'fp32', False),
                                                      ('B', 'ERB', 'fp16', False), ('A', 'NeRV_vanilla', 'fp16', False),
                                                      ('A', 'ERB', 'fp16', True)])
def test_seam_with_builtin_loss_matches_builtin_step(orn, geo, branch, prec, misalign):
    """Four steps, lr 5e-4.  X: forward_step -> ops.loss_stats(..., 'Fusion6') -> backward_step.  Y: a Fusion6 engine, run(4,
    graph=False).  Same loss kernel, same launches behind it: parameters, Adam moments and gradients equal bit for bit, stats column
    0 equal.  Columns 1 / 2 (L1, MSE) come from another kernel's per-tile fp32 sums of at most 1024 non-negative terms: two such sums
    differ by at most 2 * 1023 * 2^-24 = 1.2e-4 relative, bound 2e-4; PSNR within 1e-3 dB (2e-4 relative in MSE is 8.7e-4 dB)."""
    entries = [(k % N_FRAMES, k + 1, LR) for k in range(4)]
    X = _engine(orn, geo, branch, prec)
    p0 = X.params.clone()
    X.set_schedule(entries)
    for f, _, _ in entries:
        _fusion6_seam_step(orn, X, f, misalign=misalign)
    Y = _engine(orn, geo, branch, prec)
    Y.set_schedule(entries)
    Y.run(4, graph=False)
    torch.cuda.synchronize()
    assert X.global_step == Y.global_step == 4
    for name in ('params', 'adam_m', 'adam_v', 'grads'):
        a, b = getattr(X, name), getattr(Y, name)
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert not torch.equal(X.params, p0)
    sx, sy = X.stats(4).double(), Y.stats(4).double()
    rel = ((sx[:, 1:3] - sy[:, 1:3]).abs() / sy[:, 1:3].abs()).max().item()
    dpsnr = (sx[:, 4] - sy[:, 4]).abs().max().item()
    print(f'{geo} {branch} {prec}: L1/MSE rel {rel:.2e}, PSNR diff {dpsnr:.2e} dB')
    assert torch.equal(sx[:, 0], sy[:, 0]), (sx[:, 0], sy[:, 0])
    assert rel <= 2e-4
    assert dpsnr <= 1e-3
    assert torch.equal(sx[:, 3], torch.zeros(4, dtype=torch.float64))      # no structural term is known to the seam
    assert torch.equal(sx[:, 5:], sy[:, 5:])                                # lr, frame, step
    for e in (X, Y):
        s = e.scale_state()
        assert s['skipped'] == 0 and s['late_skipped'] == 0, s
    assert X.applied_steps() == 4


# ---- 2. an autograd loss against the oracle ---------------------------------------------------------------------------
def _freq_l1_ref(p, t):
    """utils.py:174-178 of the reference at batch 1, on whatever device and dtype p has."""
    pf = torch.fft.fft2(p, dim=(-2, -1))
    tf = torch.fft.fft2(t, dim=(-2, -1))
    return F.l1_loss(torch.stack([pf.real, pf.imag], -1), torch.stack([tf.real, tf.imag], -1))


def _fusion_freq_ref(p, t, kind='ssim'):
    from oracle import cpu_ref
    s = cpu_ref.ssim(p, t, data_range=1, size_average=True) if kind == 'ssim' else cpu_ref.ms_ssim(p, t, data_range=1, size_average=True)
    return 60 * (0.7 * torch.mean(torch.abs(p - t)) + 0.3 * (1 - s)) + _freq_l1_ref(p, t)


_ORACLE = {}


def _oracle_step(orn):
    """Loss, PSNR and every gradient tensor of one step on frame 1 (geometry A, ERB): autograd over the oracle's forward."""
    if not _ORACLE:
        from oracle import cpu_ref
        s = _setup(orn, 'A', 'ERB')
        params = {k: v.detach().clone().requires_grad_(True) for k, v in s['sd'].items()}
        out = cpu_ref.generator_forward(params, s['embeds'][1:2], GEOS['A']['fc'], GEOS['A']['strides'], 'ERB')[0]
        target = s['frames'][1:2]
        loss = _fusion_freq_ref(out, target)
        loss.backward()
        _ORACLE.update(loss=loss.item(), psnr=cpu_ref.psnr_fn([out], [target]).item(),
                       ref={k: p.grad for k, p in params.items() if p.grad is not None})
    return _ORACLE


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_step_with_autograd_loss_vs_oracle(orn, prec):
    """lr 0, one step of step_with(fusion_freq_ssim): loss, PSNR and every gradient tensor of the arena against autograd over
    cpu_ref.generator_forward with the same objective composed on the CPU; the tolerances of test_gpu_engine_loss_types."""
    o = _oracle_step(orn)
    eng = _engine(orn, 'A', 'ERB', prec, loss_type='L2')
    eng.set_schedule([(1, 1, 0.0)])
    ret = eng.step_with(orn.custom_losses.fusion_freq_ssim)
    torch.cuda.synchronize()
    st = eng.stats(1)[0].numpy()
    assert float(ret) == float(st[0])
    grads = {k: eng.grads[off:off + n].clone().cpu() for k, (off, n) in eng.layout.items()}
    ref = o['ref']
    tol_loss, tol_psnr, tol_g = {'fp32': (5e-5, 1e-3, 2e-3), 'fp16': (3e-4, 0.01, 1e-2)}[prec]
    rel = sorted(((float((grads[k] - ref[k].flatten()).norm() / (ref[k].norm() + 1e-30)), k) for k in ref), reverse=True)
    print(f'{prec}: loss {st[0]:.7f} ref {o["loss"]:.7f}; psnr {st[4]:.4f} ref {o["psnr"]:.4f}; worst grads {rel[:3]}')
    assert abs(st[0] - o['loss']) <= tol_loss * abs(o['loss']), (st[0], o['loss'])
    assert abs(st[4] - o['psnr']) < tol_psnr, (st[4], o['psnr'])
    assert set(ref) == set(eng.layout)
    assert rel[0][0] < tol_g, rel[:8]
    s = eng.scale_state()
    assert s['skipped'] == 0 and s['late_skipped'] == 0, s


# ---- 3. custom_losses at loss level ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,shape', [('freq_l1', (1, 3, 40, 60)), ('freq_l1', (2, 3, 30, 37)), ('fusion_freq_ssim', (1, 3, 40, 60)),
                                        ('fusion_freq_ssim', (2, 3, 30, 37)), ('fusion_freq_msssim', (1, 3, 161, 177))])
def test_custom_losses_vs_fp64(orn, name, shape):
    """Value (5e-5 relative) and gradient (2e-3 relative L2) against the same objective composed in fp64 on the CPU."""
    g = torch.Generator().manual_seed(11)
    t = torch.rand(*shape, generator=g)
    p = (t + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    ref_fn = {'freq_l1': _freq_l1_ref, 'fusion_freq_ssim': _fusion_freq_ref,
              'fusion_freq_msssim': lambda a, b: _fusion_freq_ref(a, b, 'ms_ssim')}[name]
    p64 = p.double().requires_grad_(True)
    ref = ref_fn(p64, t.double())
    (gref,) = torch.autograd.grad(ref, p64)
    pd = p.cuda().requires_grad_(True)
    val = getattr(orn.custom_losses, name)(pd, t.cuda())
    assert val.numel() == 1
    (gd,) = torch.autograd.grad(val, pd)
    rel_v = abs(val.item() - ref.item()) / abs(ref.item())
    rel_g = float((gd.cpu().double() - gref).norm() / gref.norm())
    print(f'{name} {shape}: value {val.item():.7f} ref {ref.item():.7f} rel {rel_v:.2e}; gradient rel-L2 {rel_g:.2e}')
    assert rel_v <= 5e-5
    assert rel_g <= 2e-3


def test_fft_names_stay_refused(orn):
    for name in ('Fusion13', 'Fusion15'):
        with pytest.raises(NotImplementedError):
            orn._lib.loss_id(name)


# ---- 4. the guard ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['dpred', 'loss', 'raise'])
def test_nonfinite_or_abandoned_step_is_skipped(orn, how):
    """A dpred with one NaN in its last pixel, a NaN loss, and a loss function that raises: parameters and moments bit-unchanged,
    `skipped` + 1; the next step with a clean gradient applies."""
    eng = _engine(orn, 'A', 'ERB', 'fp16')
    eng.set_schedule([(k % N_FRAMES, k + 1, LR) for k in range(3)])
    _fusion6_seam_step(orn, eng, 0)                                         # a clean step first: the moments are not zero
    torch.cuda.synchronize()
    before = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
    assert eng.scale_state()['skipped'] == 0
    if how == 'raise':
        def bad(pred, target):
            raise RuntimeError('objective failed')
        with pytest.raises(RuntimeError, match='objective failed'):
            eng.step_with(bad)
    else:
        _fusion6_seam_step(orn, eng, 1, spoil=how)
    torch.cuda.synchronize()
    for t, b in zip((eng.params, eng.adam_m, eng.adam_v), before):
        assert torch.equal(t, b)
    assert eng.scale_state()['skipped'] == 1
    assert eng.global_step == 2 and eng.applied_steps() == 1
    _fusion6_seam_step(orn, eng, 2)
    torch.cuda.synchronize()
    assert not torch.equal(eng.params, before[0])
    assert bool(torch.isfinite(eng.params).all())
    assert eng.scale_state()['skipped'] == 1
    assert eng.applied_steps() == 2
    st = eng.stats(3)
    assert st[:, 6].tolist() == [0.0, 1.0, 2.0] and st[:, 7].tolist() == [1.0, 2.0, 2.0]      # Adam's count leaves the skipped step out


# ---- 5. state -----------------------------------------------------------------------------------------------------------
def test_open_step_state(orn):
    eng = _engine(orn, 'A', 'ERB', 'fp16')
    H, W = eng.out_hw
    order = [2, 0, 1, 2]
    eng.set_schedule([(f, k + 1, LR) for k, f in enumerate(order)])
    g0 = torch.zeros(1, 3, H, W, device=eng.device)
    with pytest.raises(orn.OrnError, match='no open step'):
        eng.backward_step(g0)
    pred = eng.forward_step()
    assert tuple(pred.shape) == (1, 3, H, W) and pred.dtype == torch.float32
    assert eng.ws.data_ptr() <= pred.data_ptr() < eng.ws.data_ptr() + eng.ws.numel()      # a view, not a copy
    for call in (lambda: eng.run(1), lambda: eng.run(1, graph=False), lambda: eng.decode_frames(rows=[0], rgb8=False),
                 lambda: eng.decode(eng.embeds[0]), eng.forward_step):
        with pytest.raises(orn.OrnError, match='split step is open'):
            call()
    transposed = torch.zeros(1, 3, W, H, device=eng.device).transpose(2, 3)          # the right shape, not contiguous
    for bad in (g0.cpu(), g0.double(), g0[:, :, :, :W - 4], g0[0, 0], transposed):
        with pytest.raises(orn.OrnError):
            eng.backward_step(bad)
    stats, g = orn.ops.loss_stats(pred, eng.frames[order[0]:order[0] + 1], 'Fusion6')
    eng.backward_step(g, stats[0])                                          # still open after the refused calls
    eng.step_with(lambda p, t: (p - t).abs().mean())
    assert eng.global_step == 2
    eng.decode_frames(rows=[0], rgb8=False)
    eng.run(2)                                                              # continues at entry 2
    torch.cuda.synchronize()
    st = eng.stats(4)
    assert st[:, 6].tolist() == [float(f) for f in order]
    assert st[:, 7].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert eng.global_step == 4 and eng.scale_state()['skipped'] == 0
    with pytest.raises(orn.OrnError, match='used up'):
        eng.forward_step()


# ---- 6. CLI -------------------------------------------------------------------------------------------------------------
CLI = ('-e 4 --lower_width 96 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 --reduction 2 '
       '--fc_hw_dim 2_3_26 --expansion 1 --single_res --warmup 0.2 --lr_type cosine --strides 5 2 2 --conv_type conv --lr 0.0005 '
       '--norm none --act swish --outf custom_t --branch_type ERB --synthetic 12 --eval_freq 2 '
       '--custom_loss orn_amd.custom_losses:fusion_freq_ssim')


def test_train_cli_with_custom_loss(tmp_path, monkeypatch):
    from orn_amd import main_train
    monkeypatch.chdir(tmp_path)
    best = main_train.train(main_train.parse_args(CLI.split() + ['-b', '1']))
    assert list(best) == ['synthetic0']
    log = (tmp_path / 'result' / 'custom_t' / 'rank0.txt').read_text()
    psnr = [float(x) for x in re.findall(r'Epoch\[\d+/4\], lr:\S+ PSNR: ([0-9.]+)', log)]
    print(psnr)
    assert len(psnr) == 4
    assert psnr[-1] > psnr[0]
    assert (tmp_path / 'result' / 'custom_t' / 'model_latest.pth').exists()


def test_train_cli_custom_loss_refuses_a_batch(tmp_path, monkeypatch):
    from orn_amd import main_train
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match='-b'):
        main_train.train(main_train.parse_args(CLI.split() + ['-b', '2']))
    assert not (tmp_path / 'result' / 'custom_t' / 'rank0.txt').exists()
