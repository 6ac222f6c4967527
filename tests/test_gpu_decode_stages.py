"""GPU tests of the per-stage decode (include/orn.h N9: orn_engine_eval_stages; TrainEngine.decode_stages, Decoder(stages=True),
main_eval --decode_stage, main_train's per-stage evaluation line).

Geometries: test_gpu_multires.py's -- fc 2_3_26, strides 5 2 2, lower_width 96: stages 10x15 (26 channels, an fp32 block in every
precision), 20x30 and 40x60 (96 channels, 16-bit blocks in the 16-bit modes) -- and, for MS-SSIM, fc 11_12_26, strides 5 2 2 2:
stages 55x60, 110x120 (no MS-SSIM below 160 rows), 220x240, 440x480.

Every stage must be the image the training step computed its loss on (the step's per-stage PSNR against the decode's, rtol 1e-5,
the rule of tests/test_gpu_decode.py; the kernel itself is held to the training forward's side head bit for bit by
tests/test_gpu_stage_out.py), the last stage must be decode_frames' bytes, and a stage must not depend on anything above it."""
import re
import types

import numpy as np
import pytest
import torch

import multires_fixture as mf

pytestmark = pytest.mark.gpu

FC, STRIDES = '2_3_26', [5, 2, 2]
FC_MS, STRIDES_MS = '11_12_26', [5, 2, 2, 2]
HWS = [(10, 15), (20, 30), (40, 60)]
N_FRAMES = 5
ROWS = [3, 0, 4, 0, 2]
PRECS = ('fp32', 'fp16', 'bf16')
KINDS = ('NeRV_vanilla', 'ERB')
COMBOS = [(p, b) for b in KINDS for p in PRECS]
IDS = ['-'.join(c) for c in COMBOS]
KEYS = ('rgb8', 'img', 'stats')


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine, checkpoint, main_train, main_eval  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _generator(bt, sin_res=False, fc=FC, strides=STRIDES):
    return mf.tiny_generator(bt, sin_res=sin_res, strides=strides, fc=fc, lower_width=96)


_VIDEO = {}


def _video(hw, n=N_FRAMES):
    if (hw, n) not in _VIDEO:
        from oracle import cpu_ref
        _VIDEO[(hw, n)] = (cpu_ref.synthetic_video(n, hw[0], hw[1], seed=5),
                           cpu_ref.positional_encoding(torch.tensor([k / n for k in range(n)]), 1.25, 40))
    return _VIDEO[(hw, n)]


def _engine(orn, gen, prec, n=N_FRAMES):
    eng = orn.engine.TrainEngine(gen, loss_type='L2', beta=0.5, precision=prec, lw=0.7)
    eng.set_video(*_video(tuple(eng.out_hw), n))
    return eng


def _torch_rgb8(img):
    return img.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)


def _stats64(img, rgb8, target):
    t = target.double()
    mf_ = (img.double() - t).pow(2).mean(dim=(1, 2, 3))
    mq = (rgb8.permute(0, 3, 1, 2).double() / 255 - t).pow(2).mean(dim=(1, 2, 3))
    return torch.stack([mf_, -10 * torch.log10(mf_), mq, -10 * torch.log10(mq)], dim=1)


def _same(a, b, keys=KEYS):
    return all(torch.equal(a[k], b[k]) for k in keys)


_CASES = {}


def _case(orn, prec, bt):
    """One engine per combination: a training step at lr 0 on frame 3, then everything the tests compare -- computed once, never
    modified."""
    if (prec, bt) not in _CASES:
        gen = _generator(bt)
        eng = _engine(orn, gen, prec)
        eng.set_schedule([(3, 1, 0.0)])
        eng.run(1, graph=False)
        torch.cuda.synchronize()
        step_psnr = eng.stage_stats(1)[0][:, 1].clone()
        allst = eng.decode_stages(rows=ROWS, f32=True)
        again = eng.decode_stages(rows=ROWS, f32=True)
        alone = {k: eng.decode_stages(stages=k, rows=ROWS, f32=True)[k] for k in range(3)}
        last = eng.decode_frames(rows=ROWS, f32=True)
        torch.cuda.synchronize()
        _CASES[(prec, bt)] = types.SimpleNamespace(gen=gen, eng=eng, step_psnr=step_psnr, all=allst, again=again, alone=alone, last=last)
    return _CASES[(prec, bt)]


@pytest.mark.parametrize('prec,bt', COMBOS, ids=IDS)
def test_every_stage_is_the_image_of_the_training_step(orn, prec, bt):
    """Shapes, bytes and statistics of every stage; the PSNR the step recorded for its frame (row 3 comes first) is the decode's."""
    c = _case(orn, prec, bt)
    assert sorted(c.all) == [0, 1, 2]
    targets = c.eng.stage_frames + [c.eng.frames]
    for s, (H, W) in enumerate(HWS):
        o = c.all[s]
        assert o['img'].shape == (len(ROWS), 3, H, W) and o['rgb8'].shape == (len(ROWS), H, W, 3) and o['stats'].shape == (len(ROWS), 4)
        assert o['rgb8'].dtype == torch.uint8 and torch.isfinite(o['img']).all() and float(o['img'].std()) > 0
        assert torch.equal(o['rgb8'], _torch_rgb8(o['img'])), s
        s64 = _stats64(o['img'], o['rgb8'], targets[s][ROWS])
        print(f'{prec} {bt} stage {s}: decode PSNR {o["stats"][0, 1].item():.6f}, the step\'s {c.step_psnr[s].item():.6f}')
        torch.testing.assert_close(o['stats'].double(), s64, rtol=1e-5, atol=0)
        torch.testing.assert_close(o['stats'][0, 1].cpu(), c.step_psnr[s], rtol=1e-5, atol=0)
        assert torch.equal(o['img'][1], o['img'][3]) and not torch.equal(o['img'][0], o['img'][1])     # rows 0 twice: no state leaks
    assert all(_same(c.all[s], c.again[s]) for s in range(3)), 'two calls differ'


@pytest.mark.parametrize('prec,bt', COMBOS, ids=IDS)
def test_the_last_stage_is_decode_frames(orn, prec, bt):
    c = _case(orn, prec, bt)
    assert _same(c.all[2], c.last) and _same(c.alone[2], c.last)


@pytest.mark.parametrize('prec,bt', COMBOS, ids=IDS)
def test_a_stage_does_not_depend_on_what_lies_above_it(orn, prec, bt):
    """Stage k alone is stage k beside all the others; and it keeps its bits, finite, once every parameter of the blocks above k, of
    the heads above k and of the last head is NaN -- those launches do not run."""
    c = _case(orn, prec, bt)
    for k in range(3):
        assert _same(c.alone[k], c.all[k]), k
    gen = _generator(bt)
    eng = _engine(orn, gen, prec)
    for k in (0, 1):
        with torch.no_grad():
            for name, (off, n) in eng.layout.items():
                parts = name.split('.')
                if parts[0] in ('layers', 'head_layers') and int(parts[1]) > k:
                    eng.params[off:off + n] = float('nan')
        got = eng.decode_stages(stages=k, rows=ROWS, f32=True)[k]
        assert torch.isfinite(got['img']).all() and torch.isfinite(got['stats']).all()
        assert _same(got, c.all[k]), k
        eng.params.copy_(c.eng.params)
    assert _same(eng.decode_stages(stages=2, rows=ROWS, f32=True)[2], c.all[2])


@pytest.mark.parametrize('bt', KINDS)
def test_fp32_stages_against_the_eager_module(orn, bt):
    """Every stage of the fp32 engine against the mirror's forward: rtol 1e-5 / atol 2e-6, the rule of
    test_gpu_multires.test_against_the_reference_fixture for images."""
    c = _case(orn, 'fp32', bt)
    with torch.no_grad():
        outs = c.gen(c.eng.embeds[ROWS])
    assert len(outs) == 3
    for s, o in enumerate(outs):
        err = float((c.all[s]['img'] - o).abs().max())
        print(f'fp32 {bt} stage {s}: max |engine - module| {err:.2e}')
        np.testing.assert_allclose(c.all[s]['img'].cpu().numpy(), o.cpu().numpy(), rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize('kind', mf.KINDS)
def test_fp32_stages_against_the_reference_fixture(orn, kind):
    """tests/golden/multires.npz: the reference's per-stage images and pooled targets, under test_against_the_reference_fixture's rule."""
    g = mf.load()
    tag = f'tiny_{kind}'
    gen = mf.tiny_generator(kind)
    gen.load_state_dict({k: torch.from_numpy(g[f'{tag}/sd/{k}']) for k in g[f'{tag}/keys']})
    embed, data = torch.from_numpy(g[f'{tag}/embed']), torch.from_numpy(g[f'{tag}/data'])
    for dec in (orn.engine.Decoder(gen, precision='fp32', stages=True),):
        tabs = dec.stage_targets(data)
        assert torch.equal(tabs[0].cpu(), torch.from_numpy(g[f'{tag}/target0'])) and torch.equal(tabs[1].cpu(), torch.from_numpy(g[f'{tag}/target1']))
        out = dec.decode_stages(embeds=embed, frames=data, f32=True)
        for i in range(2):
            np.testing.assert_allclose(out[i]['img'].cpu().numpy(), g[f'{tag}/img{i}'], rtol=1e-5, atol=2e-6)
            torch.testing.assert_close(out[i]['stats'].double(), _stats64(out[i]['img'], out[i]['rgb8'], tabs[i]), rtol=1e-5, atol=0)


@pytest.mark.parametrize('prec,bt', COMBOS, ids=IDS)
def test_decoder_from_a_checkpoint_gives_the_train_engines_bytes(orn, prec, bt, tmp_path):
    """Decoder(stages=True) on a model loaded from the train-mode state dict: every stage's bytes are the TrainEngine's.  The same
    engine is decode-only: the training entries refuse it."""
    from ctypes import c_int32
    c = _case(orn, prec, bt)
    path = tmp_path / 'm.pth'
    torch.save({'state_dict': {k: v.detach().cpu().clone() for k, v in c.gen.state_dict().items()}}, path)
    gen = _generator(bt)
    orn.checkpoint.load_into(gen, orn.checkpoint.load_state_dict_file(str(path)))
    dec = orn.engine.Decoder(gen.cuda(), precision=prec, stages=True)
    assert dec.desc.multi_res == 1
    tabs = c.eng.stage_frames + [c.eng.frames]
    got = dec.decode_stages(rows=ROWS, embeds=c.eng.embeds, frames=tabs, f32=True)
    for s in range(3):
        assert _same(got[s], c.all[s]), s
    assert _same(dec.decode_frames(rows=ROWS, embeds=c.eng.embeds, frames=c.eng.frames, f32=True), c.last)
    L, ptr = orn._lib.lib(), orn._lib.ptr
    sched = torch.zeros(1, 4, dtype=torch.int32, device='cuda')
    cursor = torch.zeros(1, dtype=torch.int32, device='cuda')
    ring = torch.zeros(4, 8, device='cuda')
    rc = L.orn_engine_train_step(dec._h, ptr(c.eng.frames), ptr(c.eng.embeds), ptr(sched), ptr(cursor), ptr(ring), c_int32(4), orn._lib.stream())
    assert rc != 0 and 'without grads' in orn._lib.last_error()
    rc = L.orn_engine_train_steps(dec._h, ptr(c.eng.frames), ptr(c.eng.embeds), ptr(sched), ptr(cursor), ptr(ring), c_int32(4), c_int32(1),
                                  orn._lib.stream())
    assert rc != 0 and 'without grads' in orn._lib.last_error()
    torch.cuda.synchronize()
    assert int(cursor) == 0


def test_refusals(orn):
    c = _case(orn, 'fp16', 'ERB')
    with pytest.raises(orn.OrnError, match='multi-resolution'):
        orn.engine.Decoder(_generator('ERB', sin_res=True), precision='fp16', stages=True)
    dec = orn.engine.Decoder(_generator('ERB'), precision='fp16')             # the default: the last stage alone
    assert dec.desc.multi_res == 0
    with pytest.raises(orn.OrnError, match='stage 1 is below the last.*multi_res = 0'):
        dec.decode_stages(stages=[1, 2], embeds=c.eng.embeds, stats=False)
    assert 'rgb8' in dec.decode_stages(stages=2, embeds=c.eng.embeds, stats=False)[2]
    with pytest.raises(orn.OrnError, match='no stage wanted'):
        c.eng.decode_stages(stages=1, rgb8=False, stats=False)
    with pytest.raises(orn.OrnError, match='target frames'):
        orn.engine.Decoder(_generator('ERB'), precision='fp16', stages=True).decode_stages(embeds=c.eng.embeds)
    with pytest.raises(orn.OrnError, match='row index out of range'):
        c.eng.decode_stages(rows=[N_FRAMES])
    with pytest.raises(orn.OrnError, match='distinct indices'):
        c.eng.decode_stages(stages=[3])
    # the C ABI itself: stats without targets, and msssim on a small stage
    L, ptr = orn._lib.lib(), orn._lib.ptr
    recs = (orn._lib.StageOut * orn._lib.ORN_MAX_LAYERS)()
    st = torch.full((1, 4), float('nan'), device='cuda')
    rows = torch.zeros(1, dtype=torch.int32, device='cuda')
    recs[1].stats = ptr(st)
    assert L.orn_engine_eval_stages(c.eng._h, ptr(c.eng.embeds), ptr(rows), 1, recs, None, 0, orn._lib.stream()) == -1
    assert 'stage 1: stats and msssim need targets' in orn._lib.last_error()
    recs[1].targets, recs[1].stats, recs[1].msssim = ptr(c.eng.stage_frames[1]), None, ptr(st)
    assert L.orn_engine_eval_stages(c.eng._h, ptr(c.eng.embeds), ptr(rows), 1, recs, None, 0, orn._lib.stream()) == -1
    assert 'must exceed 160' in orn._lib.last_error()
    torch.cuda.synchronize()
    assert torch.isnan(st).all()


def test_a_source_tensor_of_another_size_is_pooled_to_every_stage(orn):
    c = _case(orn, 'fp16', 'ERB')
    src, _ = _video((80, 120))
    tabs = c.eng.stage_targets(src)
    for s, hw in enumerate(HWS):
        assert torch.equal(tabs[s], orn.ops.ingest_frames(src.cuda(), hw)), s
    u8 = (src * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    tabs8 = c.eng.stage_targets(u8, [0, 2])
    assert sorted(tabs8) == [0, 2] and torch.equal(tabs8[0], orn.ops.ingest_frames(u8.cuda(), HWS[0]))
    out = c.eng.decode_stages(rows=ROWS, frames=src, f32=True)
    for s in range(3):
        assert torch.equal(out[s]['img'], c.all[s]['img'])
        torch.testing.assert_close(out[s]['stats'].double(), _stats64(out[s]['img'], out[s]['rgb8'], tabs[s][ROWS]), rtol=1e-5, atol=0)
    per = c.eng.decode_stages(stages=[0, 1], rows=ROWS, frames=[tabs[0], src], f32=True)      # one table per stage; the second is pooled
    assert _same(per[0], out[0]) and _same(per[1], out[1])


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_a_call_changes_no_state_and_no_later_step(orn, prec):
    """Parameters, gradients and Adam moments keep their bits over a call, and the training step behind it is the step without it."""
    entries = [(3, 1, 5e-4), (0, 2, 4e-4)]
    res = []
    for with_call in (False, True):
        eng = _engine(orn, _generator('ERB'), prec)
        eng.set_schedule(entries)
        eng.run(1, graph=False)
        if with_call:
            before = [t.clone() for t in (eng.params, eng.grads, eng.adam_m, eng.adam_v)]
            eng.decode_stages(rows=ROWS, f32=True)
            eng.decode_stages(stages=0, rows=[1])
            torch.cuda.synchronize()
            for a, b in zip(before, (eng.params, eng.grads, eng.adam_m, eng.adam_v)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        eng.run(1, graph=False)
        torch.cuda.synchronize()
        res.append([t.clone() for t in (eng.params, eng.grads, eng.adam_m, eng.adam_v, eng.stats_ring[:2], eng.stage_ring[:2])])
        assert eng.scale_state()['skipped'] == 0
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


_MS = {}


def _ms_case(orn, prec):
    if prec not in _MS:
        gen = _generator('ERB', fc=FC_MS, strides=STRIDES_MS)
        eng = _engine(orn, gen, prec, n=4)
        rows = [2, 0, 3, 1]
        out = {ch: eng.decode_stages(rows=rows, f32=True, msssim=True, chunk=ch) for ch in (1, 3)}
        noimg = eng.decode_stages(rows=rows, rgb8=False, stats=False, msssim=True, chunk=3)
        last = eng.decode_frames(rows=rows, f32=True, msssim=True)
        torch.cuda.synchronize()
        _MS[prec] = types.SimpleNamespace(eng=eng, rows=rows, out=out, noimg=noimg, last=last)
    return _MS[prec]


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_msssim_per_stage(orn, prec):
    """Two stages above 160 and two below: zeros below; above, ops.ms_ssim (orn_msssim_frames) of the returned image against the
    stage's target, bit for bit, whatever the chunk, with or without an img output; the last stage is decode_frames'."""
    c = _ms_case(orn, prec)
    targets = c.eng.stage_frames + [c.eng.frames]
    a, b = c.out[1], c.out[3]
    assert [tuple(a[s]['img'].shape[2:]) for s in range(4)] == [(55, 60), (110, 120), (220, 240), (440, 480)]
    for s in range(4):
        assert _same(a[s], b[s], KEYS + ('msssim',)), s
        assert a[s]['msssim'].shape == (4,)
        if s < 2:
            assert float(a[s]['msssim'].abs().max()) == 0.0
            continue
        want = torch.stack([orn.ops.ms_ssim(a[s]['img'][i:i + 1], targets[s][r:r + 1]).reshape(()) for i, r in enumerate(c.rows)])
        print(f'{prec} stage {s} MS-SSIM', a[s]['msssim'].tolist())
        assert torch.equal(a[s]['msssim'], want), (s, a[s]['msssim'], want)
        assert torch.equal(c.noimg[s]['msssim'], want) and sorted(c.noimg[s]) == ['msssim']
        assert 0.0 < float(want.min()) and float(want.max()) < 1.0
    assert _same(a[3], c.last, KEYS + ('msssim',))


CLI = ('-e 2 --lower_width 8 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 --reduction 2 '
       '--fc_hw_dim 3_4_8 --expansion 1 --loss L2 --warmup 0.2 --lr_type cosine --strides 2 2 2 --conv_type conv -b 1 --lw 0.5 '
       '--lr 0.0005 --norm none --act swish --outf stages_t --branch_type ERB --synthetic 6 --precision fp32 --eval_freq 1').split()


def test_cli_decodes_and_logs_every_stage(orn, tmp_path, monkeypatch, capsys):
    """The tiny synthetic geometry of test_gpu_multires (stages 6x8, 12x16, 24x32): main_train --decoder engine logs the per-stage line
    beside the usual ones; main_eval --decode_stage all prints one value per stage and returns the last stage's PSNR within 0.01 dB
    of the eager run (the bound of test_cli_trains_and_evaluates_without_single_res); --decode_stage 1 --dump_images writes stage 1's
    pictures."""
    from PIL import Image
    from orn_amd import main_eval, main_train
    monkeypatch.chdir(tmp_path)
    main_train.train(main_train.parse_args(CLI + ['--decoder', 'engine']))
    outf = tmp_path / 'result' / 'stages_t'
    log = (outf / 'rank0.txt').read_text()
    stage_lines = re.findall(r'Eval stages PSNR: \[([0-9.]+), ([0-9.]+), ([0-9.]+)\], MS-SSIM: \[([0-9.]+), ([0-9.]+), ([0-9.]+)\]', log)
    evals = re.findall(r'Eval best_PSNR at epoch\d+:\tcurrent: ([0-9.]+)', log)
    assert len(stage_lines) == 2 and len(evals) == 2, log
    assert all(abs(float(s[2]) - float(e)) < 0.011 for s, e in zip(stage_lines, evals))          # the triple stays the last stage's
    assert len(re.findall(r'PSNR: \[([0-9.]+), ([0-9.]+), ([0-9.]+)\], best: ([0-9.]+)', log)) == 2
    capsys.readouterr()
    p_eager = main_eval.main(CLI)
    p_all = main_eval.main(CLI + ['--decoder', 'engine', '--decode_stage', 'all'])
    text = capsys.readouterr().out
    m = re.findall(r'Eval stages PSNR: \[([0-9.]+), ([0-9.]+), ([0-9.]+)\], 8-bit PSNR: \[([0-9.]+), ([0-9.]+), ([0-9.]+)\], MS-SSIM: \[', text)
    assert len(m) == 1, text
    assert 5.0 < p_all < 60.0 and abs(p_eager - p_all) < 0.01, (p_eager, p_all)
    assert abs(float(m[0][2]) - p_all) < 0.006
    assert abs(float(m[0][2]) - float(evals[-1])) < 0.02                                           # what the training run's evaluation saw
    p_one = main_eval.main(CLI + ['--decoder', 'engine', '--decode_stage', '1', '--dump_images'])
    text = capsys.readouterr().out
    assert 'stage 1, 12x16' in text and abs(p_one - float(m[0][1])) < 0.006, text
    pngs = sorted((outf / 'visualize').glob('pred_*.png'))
    assert len(pngs) == 6 and all(Image.open(p).size == (16, 12) for p in pngs)
    assert main_eval.main(CLI + ['--decoder', 'engine']) == pytest.approx(p_all, abs=1e-9)          # without the flag: as before
