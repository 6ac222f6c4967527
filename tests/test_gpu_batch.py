"""GPU tests of the batched optimiser step (-b B; include/orn.h N5, orn_engine_train_steps_batch): B frames per step, the per-frame
gradients summed on the device in frame order, one merge backward and one Adam launch per step.

Geometry unless stated: fc 2_3_26, strides 5 2 2, lower_width 96 -> 40 x 60: an fp32 first block (26 channels), a narrow block
and a fast block in the 16-bit modes, odd bias ranges (650 floats in the first block, 3 in the head), 5 frames."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FC, STRIDES = '2_3_26', [5, 2, 2]
N_FRAMES = 5
TOL = {'fp32': (5e-5, 1e-3, 2e-3), 'fp16': (3e-4, 0.01, 1e-2)}      # loss (relative), PSNR (dB), gradient (relative L2 per tensor)


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _generator(orn, bt, fc=FC, strides=STRIDES):
    torch.manual_seed(1)
    return orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=fc, expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=strides, sin_res=True,
                               lower_width=96, sigmoid=False, deploy=False, branch_type=bt)


_VIDEO = {}


def _video(hw, n=N_FRAMES):
    """Seeded frames and embeddings of one size, made once and never modified (tests that poison a frame do it on the engine's copy)."""
    if (hw, n) not in _VIDEO:
        from oracle import cpu_ref
        _VIDEO[(hw, n)] = (cpu_ref.synthetic_video(n, hw[0], hw[1], seed=5),
                           cpu_ref.positional_encoding(torch.tensor([k / n for k in range(n)]), 1.25, 40))
    return _VIDEO[(hw, n)]


def _engine(orn, bt, prec, loss_type='Fusion6', fc=FC, strides=STRIDES, n=N_FRAMES):
    eng = orn.engine.TrainEngine(_generator(orn, bt, fc, strides), loss_type=loss_type, beta=0.5, precision=prec)
    eng.set_video(*_video(tuple(eng.out_hw), n))
    return eng


def _state(eng):
    torch.cuda.synchronize()
    return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()


# ---------------------------------------------------------------- 1. one batched step against the oracle
_ORACLE = {}


def _oracle_batch(orn, bt, loss_type, fc, strides, hw, n, rows):
    """Loss, PSNR and every gradient of ONE step on the stacked batch `rows`: autograd over the oracle's forward on the stacked
    embeds, loss_fn on the stacked batch (utils.py:139-199), psnr_fn on the whole batch (utils.py:191).  Once per configuration."""
    key = (bt, loss_type, fc)
    if key not in _ORACLE:
        from oracle import cpu_ref
        frames, embeds = _video(hw, n)
        sd = _generator(orn, bt, fc, strides).state_dict()
        params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        out = cpu_ref.generator_forward(params, embeds[rows], fc, strides, bt)[0]
        target = frames[rows]
        if loss_type == 'Fusion10':        # utils.py:168 (cpu_ref.loss_fn stops at the SSIM-free ids): 0.7 L1 + 0.3 (1 - ms_ssim), batch means
            loss = 0.7 * torch.mean(torch.abs(out - target)) + 0.3 * (1 - cpu_ref.ms_ssim(out, target, data_range=1, size_average=True))
        else:
            loss = cpu_ref.loss_fn(out, target, loss_type)
        loss.backward()
        psnr = cpu_ref.psnr_fn([out], [target])[0, 0]
        _ORACLE[key] = dict(loss=loss.item(), psnr=psnr.item(), ref={k: p.grad for k, p in params.items() if p.grad is not None})
    return _ORACLE[key]


def _check_batch_vs_oracle(orn, bt, prec, loss_type, fc, strides, n, rows):
    eng = _engine(orn, bt, prec, loss_type, fc, strides, n)
    o = _oracle_batch(orn, bt, loss_type, fc, strides, tuple(eng.out_hw), n, rows)
    eng.set_schedule([(f, 1, 0.0) for f in rows])
    eng.run(1, batch=len(rows))
    torch.cuda.synchronize()
    st = eng.stats(1)[0].numpy()
    grads = {k: eng.grads[off:off + m].clone().cpu() for k, (off, m) in eng.layout.items()}
    ref = o['ref']
    tol_loss, tol_psnr, tol_g = TOL[prec]
    rel = sorted(((float((grads[k] - ref[k].flatten()).norm() / (ref[k].norm() + 1e-30)), k) for k in ref), reverse=True)
    print(f'{bt} {prec} {loss_type} B={len(rows)}: loss {st[0]:.7f} ref {o["loss"]:.7f}; psnr {st[4]:.4f} ref {o["psnr"]:.4f}; worst grads {rel[:3]}')
    assert abs(st[0] - o['loss']) <= tol_loss * abs(o['loss']), (st[0], o['loss'])
    assert abs(st[4] - o['psnr']) < tol_psnr, (st[4], o['psnr'])
    assert set(ref) == set(eng.layout)
    assert rel[0][0] < tol_g, rel[:8]
    assert st[5] == 0.0 and st[6] == rows[0] and st[7] == 1            # lr, the batch's first frame, Adam's step
    s = eng.scale_state()
    assert s['skipped'] == 0 and s['late_skipped'] == 0, s


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('bt', ['ERB', 'NeRV_vanilla'])
def test_one_batched_step_vs_oracle(orn, bt, prec):
    """lr 0, B = 3, frames [2, 0, 3] of 5: loss, PSNR and every gradient tensor of the arena against autograd on the stacked batch,
    with the tolerances of test_gpu_parity._check_full_step."""
    _check_batch_vs_oracle(orn, bt, prec, 'Fusion6', FC, STRIDES, N_FRAMES, [2, 0, 3])


def test_one_batched_step_vs_oracle_fusion10(orn):
    """The MS-SSIM loss (5 + 1 + 5 launches per frame) inside a batch of 2, at the 200 x 240 geometry of test_gpu_engine_loss_types."""
    _check_batch_vs_oracle(orn, 'ERB', 'fp16', 'Fusion10', '5_6_26', [5, 2, 2, 2], 3, [2, 0])


# ---------------------------------------------------------------- 2. the sum is the specified sum
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('bt', ['NeRV_vanilla', 'ERB'])
def test_batch_gradient_is_the_ordered_fp32_sum(orn, bt, prec):
    """G = ((g0 + g1) + g2) * float32(1/3), bit for bit, with g_i the arena after a single-frame step on frame i (lr 0, so the
    parameters stay put).  Vanilla: the whole arena.  ERB: the slots the backward writes directly (3x3 branch, head, stem); the
    other branches' gradients come from ONE merge backward of the summed dWf, which rounds differently from three."""
    eng = _engine(orn, bt, prec)
    rows = [2, 0, 3]
    g = []
    for f in rows:
        eng.set_schedule([(f, 1, 0.0)])
        eng.run(1, graph=False)
        torch.cuda.synchronize()
        g.append(eng.grads.clone())
    eng.set_schedule([(f, 1, 0.0) for f in rows])
    eng.run(1, batch=3)
    torch.cuda.synchronize()
    want = ((g[0] + g[1]) + g[2]) * torch.tensor(np.float32(1.0 / 3.0), device=g[0].device)
    assert want.dtype == torch.float32 and not torch.equal(want, g[0])
    if bt == 'NeRV_vanilla':
        assert torch.equal(eng.grads, want)
        return
    direct = [k for k in eng.layout if 'rbr_3x3_branch' in k or k.startswith('stem.') or k.startswith('head_layers.')]
    assert len(direct) == 2 * len(STRIDES) + 2 + 4
    for k in direct:
        off, n = eng.layout[k]
        assert torch.equal(eng.grads[off:off + n], want[off:off + n]), k
    # the merge backward ran (on the sum) and filled the rest.  It is linear in dWf, so it differs from the mean of three merge backwards
    # by rounding alone: fp32 sums, or in the 16-bit modes two half operands per product (2^-11 each) over two GEMM stages, ~2e-3 of
    # the tensor's scale at worst; 1e-2 of its largest element bounds that
    for k in set(eng.layout) - set(direct):
        off, n = eng.layout[k]
        assert torch.allclose(eng.grads[off:off + n], want[off:off + n], rtol=0, atol=1e-2 * float(want[off:off + n].abs().max())), k


# ---------------------------------------------------------------- 3. identical frames reduce to the single-frame step
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_identical_frames_reduce_to_the_single_frame_step(orn, prec):
    """A batch of B copies of one frame has that frame's gradient as its mean -- exactly: ((g + g) + g) + g = 4g in fp32 -- so three
    optimiser steps at B = 2 and B = 4 must leave the bits of the same three single-frame steps in the parameters, both Adam moments
    and ring columns 0-4.  Pins the MERGE_NONE frames, the single merge backward and the single Adam launch in one comparison."""
    lr = 5e-4
    single = [(1, 1, lr), (3, 2, lr), (0, 3, lr)]
    ref = _engine(orn, 'ERB', prec)
    ref.set_schedule(single)
    ref.run(3, graph=False)
    want, ring = _state(ref), ref.stats(3)

    def same(eng, what):
        got = _state(eng)
        for a, b, name in zip(got, want, ('params', 'adam_m', 'adam_v')):
            assert torch.equal(a, b), (what, name, float((a - b).abs().max()))
        st = eng.stats(3)
        assert torch.equal(st[:, :5], ring[:, :5]), (what, st[:, :5], ring[:, :5])
        assert torch.equal(st[:, 5:], ring[:, 5:]), what                 # lr, first frame, step
        assert eng.global_step == 3 and eng.applied_steps() == 3

    for B in (2, 4):
        eng = _engine(orn, 'ERB', prec)
        eng.set_schedule([e for e in single for _ in range(B)])
        eng.run(3, batch=B)
        same(eng, f'B={B}')
    eng = _engine(orn, 'ERB', prec)                                       # one call of 3 steps == calls of 1 + 2
    eng.set_schedule([e for e in single for _ in range(2)])
    eng.run(1, batch=2)
    eng.run(2, batch=2)
    same(eng, 'calls of 1 + 2')
    eng = _engine(orn, 'ERB', prec)                                       # the batched entry at batch = 1 == orn_engine_train_step
    eng.set_schedule(single)
    eng.run_batched(3, 1)
    same(eng, 'batch=1')
    assert not torch.equal(want[0], _state(_engine(orn, 'ERB', prec))[0])     # (the steps did move the parameters)


# ---------------------------------------------------------------- 4. guard
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_a_nan_frame_skips_the_whole_batch_once(orn, prec):
    """One NaN frame among three good ones in a batch of 4 (the recipe of test_a_nan_frame_poisons_nothing): the optimiser step is
    skipped as a whole -- parameters and moments bit-identical, skipped == 1, not 4 -- the next clean batch applies as Adam's step 1,
    and the scale has been halved once."""
    eng = _engine(orn, 'ERB', prec)
    eng.frames[2, 1, 3, 5] = float('nan')
    lr = 5e-4
    eng.set_schedule([(f, 1, lr) for f in (0, 2, 1, 3)] + [(f, 2, lr) for f in (0, 1, 3, 4)])
    before = _state(eng)
    s0 = eng.scale_state()
    eng.run(1, batch=4)
    after = _state(eng)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    s1 = eng.scale_state()
    assert s1['skipped'] == 1 and s1['flag'] == 1 and s1['scale'] == s0['scale'], s1      # the scale is constant within a step
    assert eng.applied_steps() == 0
    eng.run(1, batch=4)
    moved = _state(eng)
    s2 = eng.scale_state()
    assert s2['skipped'] == 1 and s2['backoffs'] == 1 and s2['flag'] == 0, s2
    assert s2['scale'] == max(s0['scale'] / 2, 1.0), (s0, s2)
    st = eng.stats(2)
    assert not torch.isfinite(st[0, 0]) and torch.isfinite(st[1, :5]).all()
    assert st[1, 7] == 1 and st[1, 6] == 0                               # Adam's count excludes the skipped step
    assert torch.isfinite(moved[0]).all() and not torch.equal(moved[0], before[0])
    assert torch.count_nonzero(moved[1]) > 0 and eng.applied_steps() == 1


# ---------------------------------------------------------------- 5. arguments
def test_bad_arguments_come_back_as_messages(orn):
    from orn_amd import _lib
    eng = _engine(orn, 'ERB', 'fp32')
    eng.set_schedule([(k % N_FRAMES, 1, 0.0) for k in range(8)])
    L = _lib.lib()

    def call(batch):
        return L.orn_engine_train_steps_batch(eng._h, _lib.ptr(eng.frames), _lib.ptr(eng.embeds), _lib.ptr(eng.sched), _lib.ptr(eng.cursor),
                                              _lib.ptr(eng.stats_ring), ctypes.c_int32(eng.n_slots), ctypes.c_int32(1), ctypes.c_int32(batch),
                                              ctypes.c_void_p(eng.stream.cuda_stream))
    assert call(2) == -1 and 'no batch workspace' in _lib.last_error()
    assert L.orn_engine_batch_ws_bytes(ctypes.byref(eng.desc), 0) == 0
    assert L.orn_engine_batch_ws_bytes(ctypes.byref(eng.desc), _lib.ORN_MAX_BATCH + 1) == 0
    eng.run(1, batch=2)                                                   # allocates a workspace for batches up to 2
    assert call(0) == -1 and 'batch=0' in _lib.last_error()
    assert call(3) == -1 and 'batch=3' in _lib.last_error()
    assert call(2) == 0
    with pytest.raises(orn.OrnError, match='no graph form'):
        eng.run(1, graph=True, batch=2)
    with pytest.raises(orn.OrnError, match='schedule entries'):
        eng.run(5, batch=2)                                               # 10 entries needed, 8 uploaded
    torch.cuda.synchronize()
    assert _lib.ORN_MAX_BATCH >= 16
