"""GPU tests of the pipelined form of the step (orn_engine_train_steps, include/orn.h): the last block's weight gradient, slab
reduction, merge backward, Adam update and next merge forward run on the engine's second stream, beside the boundary between this
step and the next (main_train.py:229-254 is still the unit of work).  It must change nothing but the clock: parameters, Adam moments
and the per-step statistics are compared BIT FOR BIT with the serial forms of the step (hipGraph replay, one call per step), whose
gradients the other test files pin to the CPU oracle."""
import pytest
import torch

from helpers import GEOS, pipelined_vs_oracle
from helpers import small_engine as _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _run(orn, prec, branch, geo, mode, steps, calls):
    eng = _engine(orn, prec, branch, geo)
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(steps * calls)])
    for _ in range(calls):
        eng.run(steps, graph=mode)
    torch.cuda.synchronize()
    return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.stats(steps * calls).clone()


@pytest.mark.parametrize('geo', sorted(GEOS))
@pytest.mark.parametrize('branch', ['ERB', 'NeRV_vanilla'])
@pytest.mark.parametrize('prec', ['fp16', 'bf16'])
def test_pipelined_steps_equal_serial_steps_bit_for_bit(orn, prec, branch, geo):
    """7 steps as two calls (4 + 3: the first step of a call merges every block itself, the later ones take the last block's
    merged kernel from the previous step's side branch; the end of a call joins the branch)."""
    ref = _run(orn, prec, branch, geo, True, 7, 1)            # hipGraph replay of the serial step
    pipe_a = _run(orn, prec, branch, geo, None, 7, 1)
    for a, b, what in zip(ref, pipe_a, ('params', 'adam_m', 'adam_v', 'stats')):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
    eng = _engine(orn, prec, branch, geo)
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(7)])
    eng.run(4)
    eng.run(3)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, ref[0]) and torch.equal(eng.adam_m, ref[1]) and torch.equal(eng.adam_v, ref[2])
    assert torch.isfinite(ref[0]).all() and not torch.equal(ref[1], torch.zeros_like(ref[1]))


@pytest.mark.parametrize('cfg', ['720p', '1080p'])
def test_pipelined_steps_equal_eager_steps_at_720p(orn, cfg):
    """BASELINE config 2 (720p, 9_16_26) and config 3's geometry (1080p, 9_16_48, a stride-3 block) at full size: 6 pipelined steps
    against 6 single-step calls, bit for bit."""
    import bench
    outs = []
    for mode in (False, None):
        eng = bench.make_engine(seed=7, precision='fp16', cfg=bench.CONFIGS[cfg], frames=6)
        eng.set_schedule([(k % 6, k + 1, 5e-4) for k in range(6)])
        eng.run(6, graph=mode)
        torch.cuda.synchronize()
        outs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.stats(6).clone()))
        del eng
    for a, b, what in zip(outs[0], outs[1], ('params', 'adam_m', 'adam_v', 'stats')):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))


def test_pipelined_epochs_equal_graph_replay_at_720p(orn):
    """A soak for the hand-offs between the streams (a missed dependency shows as a different bit sooner or later): 3 epochs of the
    132-frame bench video, shuffled schedule with the reference's LR ramp, as pipelined calls of one epoch each against the hipGraph
    replay of the serial step -- parameters, both moments and all 396 per-step records bit for bit -- and the pipelined run repeated
    (run-to-run identical)."""
    import bench
    outs = []
    for mode in (True, None, None):
        eng = bench.make_engine(seed=11, precision='fp16', cfg=bench.CONFIGS['720p'])
        eng.set_schedule(bench.schedule(396))
        for _ in range(3):
            eng.run(132, graph=mode)
        torch.cuda.synchronize()
        outs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.stats(396).clone()))
        assert eng.scale_state()['skipped'] == 0
        del eng
    for k in (1, 2):
        for a, b, what in zip(outs[0], outs[k], ('params', 'adam_m', 'adam_v', 'stats')):
            assert torch.equal(a, b), (k, what, float((a - b).abs().max()))


def test_a_skipped_step_is_skipped_on_both_streams(orn):
    """The guard under the pipeline: a step whose gradients overflow (scale forced to 2^40) must leave EVERY parameter and moment
    bit-identical -- the side branch's Adam launch (last block + head) follows the decision the main stream took -- and count once."""
    eng = _engine(orn, 'fp16', 'ERB', 'narrow_first')
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(40)])
    eng.run(3)
    torch.cuda.synchronize()
    assert eng.scale_state()['skipped'] == 0
    eng.set_grad_scale(2.0 ** 40)
    p0, m0, v0 = eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()
    eng.run(3)
    torch.cuda.synchronize()
    s = eng.scale_state()
    assert s['skipped'] == 3, s
    assert torch.equal(eng.params, p0) and torch.equal(eng.adam_m, m0) and torch.equal(eng.adam_v, v0)
    eng.run(30)                                                # every step advances: the scale halves until the gradients fit
    torch.cuda.synchronize()
    s = eng.scale_state()
    assert s['skipped'] < 33 and torch.isfinite(eng.params).all() and not torch.equal(eng.params, p0), s


def test_decode_after_pipelined_steps_uses_the_updated_last_block(orn):
    """The end of a call joins the side branch: a decode right behind it must see the last block's and the head's updated
    parameters (same image as after the same steps run serially)."""
    imgs = []
    for mode in (True, None):
        eng = _engine(orn, 'fp16', 'ERB', 'narrow_first')
        eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(5)])
        eng.run(5, graph=mode)
        imgs.append(eng.decode(eng.embeds[2]).clone())
        torch.cuda.synchronize()
    assert torch.equal(imgs[0], imgs[1])


# Pipelined steps against the CPU oracle, per precision: worst value measured on the MI355X over the 6 cases below (3 GEOS x 2 branch
# types), and the tolerance: <= 3x that, and no looser than the single-step ceilings of test_gpu_parity._check_full_step (loss 3e-4 /
# 2e-3 relative, PSNR 0.01 / 0.05 dB, gradient and m 1e-2 / 5e-2 relative L2, v twice that).
#   fp16 measured: loss 2.4e-5, PSNR 5.7e-5 dB, gradient 5.8e-3 (head bias of narrow_first, 3 elements), m 2.0e-3, v 1.4e-3,
#                  share of parameters off by > lr/2 1.7e-4
#   bf16 measured: loss 1.1e-4, PSNR 1.3e-3 dB, gradient 1.09e-2, m 9.6e-3, v 8.2e-3, share off 1.24e-3
ORACLE_TOL = {
    'fp16': dict(loss_rel=6e-5, psnr=1.5e-4, grad_rel=1e-2, m_rel=5e-3, v_rel=4e-3, off_share=4e-4),
    'bf16': dict(loss_rel=2.5e-4, psnr=3e-3, grad_rel=3e-2, m_rel=2.5e-2, v_rel=2e-2, off_share=3e-3),
}


def small_case_vs_oracle(orn, prec, branch, geo, lr=1e-3):
    """6 pipelined steps (a call of 4, then a call of 2) of a small model vs 6 steps of the CPU oracle: frames 3 0 4 1 2 3, lr falling
    from `lr` by 5 % a step.  Steps 2-4 run on the merged kernel the side branch built, step 5 crosses a call boundary."""
    g = GEOS[geo]
    eng = _engine(orn, prec, branch, geo)
    sd = {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}
    entries = [((3 + 2 * k) % 5, k + 1, lr * (1.0 - 0.05 * k)) for k in range(6)]
    out = pipelined_vs_oracle(eng, sd, eng.frames.cpu(), eng.embeds.cpu(), entries, (4, 2), g['fc'], g['strides'], branch)
    s = eng.scale_state()
    out['skips'] = s['skipped'] + s['late_skipped']
    return out


@pytest.mark.parametrize('geo', sorted(GEOS))
@pytest.mark.parametrize('branch', ['ERB', 'NeRV_vanilla'])
@pytest.mark.parametrize('prec', ['fp16', 'bf16'])
def test_pipelined_steps_vs_oracle(orn, prec, branch, geo):
    """Several pipelined steps at lr > 0 against the CPU oracle directly, so that a fault every launch form shares and that shows
    only once the parameters have moved (a stale merged kernel or half operand copy, an Adam that reads old moments) fails here:
    loss and PSNR of every step, the last step's gradients and both Adam moments per tensor (m is a running sum of the gradients:
    the sharp check), and the parameters in units of lr -- none may move further than Adam allows (2 lr a step), and only a small
    share may end more than lr/2 from the oracle's (Adam's first steps are ~lr sign(g): gradients near zero flip legitimately).
    Measured and tolerances: ORACLE_TOL.  With the parameter-side half copies of the merge backward (orn_merge_pack.h jobs 1/2/4/5)
    refreshed on the first step only, every ERB case fails here (gradient and m relative L2 0.82-0.92) while the bit-for-bit tests
    above, which compare launch forms with each other, all pass."""
    m = small_case_vs_oracle(orn, prec, branch, geo)
    tol = ORACLE_TOL[prec]
    assert m['skips'] == 0 and m['finite'], m
    assert m['oracle_moved_share'] > 0.5, m                    # the premise: the parameters do move, by several lr
    assert m['move_lr'] <= 2 * 6, m
    for key in ('loss_rel', 'psnr', 'grad_rel', 'm_rel', 'v_rel', 'off_share'):
        assert m[key] < tol[key], (key, m)


_BIASES = ('rbr_3x3_branch.bias', 'rbr_3x1_branch.bias', 'rbr_1x3_branch.bias')
_LAST_W = ('rbr_3x3_branch.weight', 'rbr_3x1_branch.weight', 'rbr_1x3_branch.weight', 'rbr_1x1_3x3_1x1_branch_1x1_2.weight')
_LATE_C = 3000.0          # the CPU oracle puts max |dWf| of the last block at 46 with it (> 4: its half copy overflows), every other block's < 1e-4


def _late_only_state(eng, on):
    """on=True: add _LATE_C to the three branch biases of the block below the last one (its SiLU output, the last block's input, becomes
    ~3 _LATE_C and nearly uniform) and divide the last block's merged kernel by _LATE_C (its output, the head's input and the image stay
    in range: tanh does not saturate, the last block's dy stays normal and the dy of the blocks below shrinks).  The last block's
    weight gradient sum(x dy) then leaves half range -- |dWf| > 4, a side-stream detector of the pipelined step -- while nothing on the
    caller's stream overflows.  on=False: the biases lose the constant again, the last block's weights come back (from the copy taken)."""
    nl = len(eng.model.layers)
    with torch.no_grad():
        for b in _BIASES:
            off, n = eng.layout[f'layers.{nl - 2}.{b}']
            eng.params[off:off + n] += _LATE_C if on else -_LATE_C
        for w in _LAST_W:
            off, n = eng.layout[f'layers.{nl - 1}.{w}']
            if on:
                eng._late_saved = getattr(eng, '_late_saved', {})
                eng._late_saved[w] = eng.params[off:off + n].clone()
                eng.params[off:off + n] /= _LATE_C
            else:
                eng.params[off:off + n] = eng._late_saved[w]


def test_late_only_overflow_is_counted_and_backs_the_scale_off(orn):
    """A step that only a detector of the pipelined step's side branch flags -- one that runs behind the caller's-stream Adam's skip
    decision: here the fp16 copy of the last block's merged-kernel gradient (|dWf| > 4, orn_merge_pack.h) -- is a LATE-ONLY skip:
    the lower blocks take the update, the last block and the head do not (include/orn.h).  It must be counted (late_skipped, not
    skipped: Adam's step numbers stay), reported in the flag until the scale has backed off for it, and back the scale off within
    two advances; the next clean call trains with no skip of either kind.  The premise is asserted: the loss is finite, the
    serial step of the same state skips (and counts) the whole step, and the pipelined one does update the lower blocks."""
    nl = len(GEOS['narrow_first']['strides'])
    # premise 1: the serial form skips the whole step
    ser = _engine(orn, 'fp16', 'ERB', 'narrow_first')
    _late_only_state(ser, True)
    ser.set_schedule([(k % 5, k + 1, 5e-4) for k in range(4)])
    p0 = ser.params.clone()
    ser.run(1, graph=False)
    torch.cuda.synchronize()
    s = ser.scale_state()
    assert s['skipped'] == 1 and torch.equal(ser.params, p0), s
    assert bool(torch.isfinite(ser.stats(1)[0]).all()), ser.stats(1)
    ser_late = s['late_skipped']                                # (the serial forms have no late detector)
    del ser
    # the pipelined step of the same state
    eng = _engine(orn, 'fp16', 'ERB', 'narrow_first')
    _late_only_state(eng, True)
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(4)])
    s0 = eng.scale_state()
    p0, m0, v0 = eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()
    eng.run(1)
    torch.cuda.synchronize()
    st = eng.stats(1)[0]
    assert bool(torch.isfinite(st).all()), st
    lo = min(off for k, (off, n) in eng.layout.items() if k.startswith(f'layers.{nl - 1}.') or k.startswith('head_layers.'))
    assert all(off >= lo for k, (off, n) in eng.layout.items() if k.startswith(f'layers.{nl - 1}.') or k.startswith('head_layers.'))
    for k in ('stem.0.weight', f'layers.{nl - 2}.rbr_3x3_branch.weight', f'layers.{nl - 2}.rbr_3x3_branch.bias'):
        off, n = eng.layout[k]
        assert not torch.equal(eng.params[off:off + n], p0[off:off + n]), k       # premise 2: the lower blocks took the step
    s1 = eng.scale_state()
    assert s1['skipped'] == 0 and s1['late_skipped'] == 1, s1
    for a, b, what in ((eng.params, p0, 'params'), (eng.adam_m, m0, 'adam_m'), (eng.adam_v, v0, 'adam_v')):
        assert torch.equal(a[lo:], b[lo:]), what            # the last block and the head: bit-unchanged
    assert torch.isfinite(eng.params).all()
    assert s1['flag'] == 1 and s1['scale'] == s0['scale'], s1      # pending: this call's only advance ran before the step
    assert eng.applied_steps() == 1                             # the lower blocks applied it: Adam's step count includes it
    # restore the state; the next call's first advance backs the scale off, and it trains cleanly
    _late_only_state(eng, False)
    p1 = eng.params.clone()
    eng.run(3)
    torch.cuda.synchronize()
    s2 = eng.scale_state()
    assert s2['scale'] == s0['scale'] / 2 and s2['backoffs'] == s0['backoffs'] + 1, s2
    assert s2['skipped'] == 0 and s2['late_skipped'] == 1 and s2['flag'] == 0, s2
    assert torch.isfinite(eng.params).all() and not torch.equal(eng.params[lo:], p1[lo:])
    assert ser_late == 0
    assert eng.stats(4)[1:, 7].tolist() == [2.0, 3.0, 4.0]          # Adam's step numbers did not lose the late-only skip
