"""GPU tests of the one-call evaluation (orn_engine_eval_frames, include/orn.h; decode_frames(msssim=True) on TrainEngine and
engine.Decoder; main_train.evaluate with --decoder engine): multi-frame decode plus a per-frame MS-SSIM column, computed on the
decoded fp32 planes by the batched kernels without leaving the device (main_eval.py:795-815, main_train.py:377-438,
utils.py:201-211).

Geometry: fc 5_6_26, strides 5 2 2 2, lower_width 96 -> 200 x 240, helpers.GEOS['narrow_first']'s layer pattern at the smallest
size above pytorch_msssim's 160.  The column must be bit-equal to ops.ms_ssim on the single-frame decode, within 2e-5 (the
tolerance of test_gpu_parity.test_msssim) of the fp64 oracle on the returned image, and must leave every other output of
decode_frames untouched."""
import types

import pytest
import torch

from helpers import small_engine

pytestmark = pytest.mark.gpu

GEO = dict(fc='5_6_26', strides=[5, 2, 2, 2], lower_width=96)
ROWS = [3, 0, 4, 0, 2]
COMBOS = [(p, b) for b in ('ERB', 'NeRV_vanilla') for p in ('fp16', 'bf16', 'fp32')]
IDS = ['-'.join(c) for c in COMBOS]


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine, main_train  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _generator(orn, branch):
    return orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=GEO['fc'], expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=GEO['strides'], sin_res=True,
                               lower_width=GEO['lower_width'], sigmoid=False, deploy=False, branch_type=branch)


def _engine(orn, prec, branch, n_frames=5, seed=1):
    """helpers.small_engine with this file's geometry."""
    from oracle import cpu_ref
    torch.manual_seed(seed)
    eng = orn.engine.TrainEngine(_generator(orn, branch), loss_type='Fusion6', beta=0.5, precision=prec)
    hw = eng.out_hw
    assert tuple(hw) == (200, 240)
    frames = cpu_ref.synthetic_video(n_frames, hw[0], hw[1], seed=5)
    embeds = cpu_ref.positional_encoding(torch.tensor([k / n_frames for k in range(n_frames)]), 1.25, 40)
    eng.set_video(frames, embeds)
    return eng


_CASES = {}


def _case(orn, prec, branch):
    """One engine per combination, 3 training steps, then everything the tests compare -- computed once, never modified."""
    key = (prec, branch)
    if key not in _CASES:
        eng = _engine(orn, prec, branch)
        eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(3)])
        eng.run(3)
        kw = dict(rows=ROWS, rgb8=True, stats=True)
        plain = eng.decode_frames(f32=True, **kw)
        out = eng.decode_frames(f32=True, msssim=True, chunk=2, **kw)
        again = eng.decode_frames(f32=True, msssim=True, chunk=2, **kw)
        in_ws = eng.decode_frames(f32=False, msssim=True, chunk=2, **kw)
        whole = eng.decode_frames(f32=True, msssim=True, chunk=5, **kw)
        single = torch.stack([orn.ops.ms_ssim(eng.decode(eng.embeds[r]), eng.frames[r:r + 1]) for r in ROWS])
        torch.cuda.synchronize()
        _CASES[key] = types.SimpleNamespace(eng=eng, plain=plain, out=out, again=again, in_ws=in_ws, whole=whole, single=single)
    return _CASES[key]


@pytest.mark.parametrize('prec,branch', COMBOS, ids=IDS)
def test_column_is_the_single_frame_value(orn, prec, branch):
    c = _case(orn, prec, branch)
    assert c.out['msssim'].shape == (len(ROWS),) and c.out['msssim'].dtype == torch.float32
    assert torch.equal(c.out['msssim'], c.single), (c.out['msssim'].tolist(), c.single.tolist())
    assert c.out['msssim'][1].item() == c.out['msssim'][3].item()           # row 0 twice
    assert bool(torch.isfinite(c.out['msssim']).all())


@pytest.mark.parametrize('prec,branch', COMBOS, ids=IDS)
def test_column_matches_oracle_on_the_returned_image(orn, prec, branch):
    from oracle import cpu_ref
    c = _case(orn, prec, branch)
    ref = cpu_ref.ms_ssim(c.out['img'].cpu().double(), c.eng.frames[ROWS].cpu().double(), size_average=False)
    err = (c.out['msssim'].cpu().double() - ref).abs()
    print(f'{prec}-{branch}: oracle {ref.tolist()} device {c.out["msssim"].tolist()} max |diff| {float(err.max()):.3e}')
    assert float(err.max()) <= 2e-5, (c.out['msssim'].tolist(), ref.tolist())


@pytest.mark.parametrize('prec,branch', COMBOS, ids=IDS)
def test_other_outputs_and_repeats_are_bit_identical(orn, prec, branch):
    c = _case(orn, prec, branch)
    assert 'msssim' not in c.plain
    for k in ('img', 'rgb8', 'stats'):
        assert torch.equal(c.out[k], c.plain[k]), k                         # what decode_frames writes without the column
        assert torch.equal(c.again[k], c.out[k]), k
    assert torch.equal(c.again['msssim'], c.out['msssim'])                  # a second call
    assert 'img' not in c.in_ws
    assert torch.equal(c.in_ws['msssim'], c.out['msssim'])                  # planes in the workspace instead of the caller's img
    assert torch.equal(c.in_ws['rgb8'], c.plain['rgb8']) and torch.equal(c.in_ws['stats'], c.plain['stats'])
    assert torch.equal(c.whole['msssim'], c.out['msssim'])                  # one chunk of 5 instead of 2, 2, 1


@pytest.mark.parametrize('prec,branch', COMBOS, ids=IDS)
def test_decoder_gives_the_same_column(orn, prec, branch):
    c = _case(orn, prec, branch)
    model = _generator(orn, branch)
    model.load_state_dict(c.eng.model.state_dict())
    dec = orn.engine.Decoder(model.cuda(), precision=prec)
    got = dec.decode_frames(rows=ROWS, embeds=c.eng.embeds, frames=c.eng.frames, rgb8=True, f32=True, stats=True, msssim=True, chunk=2)
    for k in ('msssim', 'img', 'rgb8', 'stats'):
        assert torch.equal(got[k], c.out[k]), k


@pytest.mark.parametrize('prec,branch', COMBOS, ids=IDS)
def test_main_train_evaluate_engine_vs_eager(orn, prec, branch):
    c = _case(orn, prec, branch)
    res = {}
    for decoder in ('eager', 'engine'):
        args = types.SimpleNamespace(decoder=decoder, test_gap=1)
        res[decoder] = orn.main_train.evaluate(c.eng.model, c.eng, args)
    (p0, _, m0), (p1, fps, m1) = res['eager'], res['engine']
    print(f'{prec}-{branch}: eager PSNR {p0:.6f} MS-SSIM {m0:.7f}; engine PSNR {p1:.6f} MS-SSIM {m1:.7f}')
    assert fps > 0
    assert abs(p1 - p0) <= 1e-4, (p0, p1)
    assert abs(m1 - m0) <= 1e-6, (m0, m1)
    # a validation split (frames / embeds of their own, every frame) and a gap on the resident video take the same path
    val = (c.eng.frames[1:4].contiguous(), c.eng.embeds[1:4].contiguous())
    args = types.SimpleNamespace(decoder='engine', test_gap=2)
    pv, _, mv = orn.main_train.evaluate(c.eng.model, c.eng, args, val)
    pg, _, mg = orn.main_train.evaluate(c.eng.model, c.eng, args)
    args.decoder = 'eager'
    pve, _, mve = orn.main_train.evaluate(c.eng.model, c.eng, args, val)
    pge, _, mge = orn.main_train.evaluate(c.eng.model, c.eng, args)
    assert abs(pv - pve) <= 1e-4 and abs(mv - mve) <= 1e-6 and abs(pg - pge) <= 1e-4 and abs(mg - mge) <= 1e-6


def test_small_image_gives_a_zero_column(orn):
    """80 x 120 (GEOS['narrow_first']): utils.msssim_fn's rule, H < 160 -> 0; the plain entry runs and nothing else changes."""
    eng = small_engine(orn, 'fp16', 'ERB', 'narrow_first')
    assert tuple(eng.out_hw) == (80, 120)
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(3)])
    eng.run(3)
    kw = dict(rows=ROWS, rgb8=True, f32=True, stats=True)
    plain = eng.decode_frames(**kw)
    out = eng.decode_frames(msssim=True, chunk=2, **kw)
    assert out['msssim'].shape == (len(ROWS),) and float(out['msssim'].abs().max()) == 0.0
    for k in ('img', 'rgb8', 'stats'):
        assert torch.equal(out[k], plain[k]), k
    only = eng.decode_frames(rows=ROWS, rgb8=False, f32=False, stats=False, msssim=True)
    assert list(only) == ['msssim'] and float(only['msssim'].abs().max()) == 0.0


def test_argument_errors(orn):
    c = _case(orn, 'fp16', 'ERB')
    eng, L, ptr = c.eng, orn._lib.lib(), orn._lib.ptr
    rows = torch.tensor(ROWS, dtype=torch.int32, device=eng.device)
    ms = torch.zeros(5, device=eng.device)
    need = L.orn_engine_eval_frames_ws_bytes(eng.desc, 1)
    assert 0 < need < L.orn_engine_eval_frames_ws_bytes(eng.desc, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=eng.device)
    st = orn._lib.stream()
    assert L.orn_engine_eval_frames(eng._h, ptr(eng.embeds), ptr(rows), 5, None, None, None, None, ptr(ms), ptr(ws), need, st) == -1
    assert 'needs targets' in orn._lib.last_error()
    assert L.orn_engine_eval_frames(eng._h, ptr(eng.embeds), ptr(rows), 5, ptr(eng.frames), None, None, None, ptr(ms), ptr(ws), need - 1, st) == -2
    # a workspace for one frame: five chunks, the same bits; nothing but the column asked for
    assert L.orn_engine_eval_frames(eng._h, ptr(eng.embeds), ptr(rows), 5, ptr(eng.frames), None, None, None, ptr(ms), ptr(ws), need, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(ms, c.out['msssim'])
