"""GPU tests of multi-frame decode (orn_engine_decode_frames, include/orn.h; TrainEngine.decode_frames, engine.Decoder): n frames
per call with the weight-only work of the forward done once, each frame ending on the device in 8-bit interleaved pixels, the
fp32 planar image and {mse, psnr} of both against the target frame (main_eval.py:795-815, main_train.py:377-438).

The float image must be what the single-frame decoder writes, bit for bit; the bytes what torch's three fp32 ops give; the
statistics what fp64 torch gives on the returned tensors (rtol 1e-5, the PSNR tolerance of tests/test_gpu_parity.py)."""
import ctypes
import os
import types

import pytest
import torch

from helpers import GEOS
from helpers import small_engine as _engine

pytestmark = pytest.mark.gpu

ROWS = [3, 0, 4, 0, 2]
COMBOS = [(p, b, g) for g in sorted(GEOS) for b in ('ERB', 'NeRV_vanilla') for p in ('fp16', 'bf16', 'fp32')]
IDS = ['-'.join(c) for c in COMBOS]


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine, checkpoint, main_train  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


_CASES = {}


def _case(orn, prec, branch, geo):
    """One engine per combination, 3 training steps, then everything the tests compare -- computed once, never modified."""
    key = (prec, branch, geo)
    if key not in _CASES:
        eng = _engine(orn, prec, branch, geo)
        eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(3)])
        eng.run(3)
        out = eng.decode_frames(rows=ROWS, f32=True)
        again = eng.decode_frames(rows=ROWS, f32=True)
        ref = torch.cat([eng.decode(eng.embeds[r]) for r in ROWS])
        torch.cuda.synchronize()
        _CASES[key] = types.SimpleNamespace(eng=eng, out=out, again=again, ref=ref)
    return _CASES[key]


def _torch_rgb8(img):
    return img.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)


def _stats64(img, rgb8, target):
    """[n,4] fp64: mse / psnr of the float image and of the bytes / 255 (utils.py:191)."""
    t = target.double()
    mf = (img.double() - t).pow(2).mean(dim=(1, 2, 3))
    mq = (rgb8.permute(0, 3, 1, 2).double() / 255 - t).pow(2).mean(dim=(1, 2, 3))
    return torch.stack([mf, -10 * torch.log10(mf), mq, -10 * torch.log10(mq)], dim=1)


@pytest.mark.parametrize('prec,branch,geo', COMBOS, ids=IDS)
def test_float_image_equals_single_frame_decode_bit_for_bit(orn, prec, branch, geo):
    """rows 3,0,4,0,2 after 3 training steps: frames 1.. reuse frame 0's merged kernels and operand copies, the output kernel
    shares the head's arithmetic; the repeated row 0 shows that no state leaks from frame to frame."""
    c = _case(orn, prec, branch, geo)
    assert c.out['img'].shape == c.ref.shape
    assert torch.isfinite(c.ref).all() and float(c.ref.std()) > 0
    assert torch.equal(c.out['img'], c.ref), float((c.out['img'] - c.ref).abs().max())
    assert torch.equal(c.out['img'][1], c.out['img'][3])
    assert not torch.equal(c.out['img'][0], c.out['img'][1])


@pytest.mark.parametrize('prec,branch,geo', COMBOS, ids=IDS)
def test_changed_parameters_are_seen_by_the_next_call(orn, prec, branch, geo):
    eng = _engine(orn, prec, branch, geo)
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(2)])
    first = eng.decode_frames(rows=ROWS, f32=True)['img'].clone()
    eng.run(2)
    second = eng.decode_frames(rows=ROWS, f32=True)['img']
    ref = torch.cat([eng.decode(eng.embeds[r]) for r in ROWS])
    assert torch.equal(second, ref), float((second - ref).abs().max())
    assert not torch.equal(second, first)


@pytest.mark.parametrize('prec,branch,geo', COMBOS, ids=IDS)
def test_rgb8_equals_torch_quantisation_exactly(orn, prec, branch, geo):
    c = _case(orn, prec, branch, geo)
    want = _torch_rgb8(c.out['img'])
    assert c.out['rgb8'].dtype == torch.uint8 and c.out['rgb8'].shape == want.shape and c.out['rgb8'].is_contiguous()
    assert torch.equal(c.out['rgb8'], want), int((c.out['rgb8'].int() - want.int()).abs().max())


def _hook(orn, img, target=None, want_img=False, misalign=0):
    """The planar output stage (the fp32 engine's) on a crafted image [3,H,W] -> (rgb8 [H,W,3], img copy or None, stats or None)."""
    L = orn._lib.lib()
    ptr = orn._lib.ptr
    _, H, W = img.shape
    buf = torch.full((H * W * 3 + 8,), 77, dtype=torch.uint8, device=img.device)
    rgb = buf[misalign:misalign + H * W * 3]
    copy = torch.empty_like(img) if want_img else None
    stats = torch.empty(4, device=img.device) if target is not None else None
    nb = L.orn_debug_decode_out_ws_bytes()
    ws = torch.zeros(nb // 4, device=img.device)
    rc = L.orn_debug_decode_out_f32(ptr(img), H, W, ptr(target), ctypes.c_void_p(rgb.data_ptr()), ptr(copy), ptr(stats), ptr(ws),
                                    ctypes.c_size_t(nb), orn._lib.stream())
    assert rc == 0, orn._lib.last_error()
    torch.cuda.synchronize()
    assert bool((buf[:misalign] == 77).all()) and bool((buf[misalign + H * W * 3:] == 77).all())     # nothing outside the image
    return rgb.view(H, W, 3), copy, stats


@pytest.mark.parametrize('misalign', [0, 1, 2, 3])
def test_quantisation_at_the_half_way_points(orn, misalign):
    """(k + 0.5)/255 for k = 0..255, their fp32 neighbours both ways, k/255, values below 0 and above 1: the inputs whose product
    with 255 sits on a rounding boundary of torch's two separately rounded ops (the kernel must not contract them).  7 x 51 pixels: 357 is no multiple of a wave's 64 pixels
    (ragged tail, byte stores) and, with the output shifted by 1..3 bytes, no run of bytes starts on a dword."""
    H, W = 7, 51
    k = torch.arange(256, dtype=torch.float64)
    mid = ((k + 0.5) / 255).float()
    one = torch.ones_like(mid)
    vals = torch.cat([mid, torch.nextafter(mid, one * 2), torch.nextafter(mid, -one),
                      (k / 255).float(), torch.tensor([-1.0, -1e-3, -0.0, 0.0, 1.0, 1.0 + 1e-6, 1.002, 2.0, 300.0, -300.0])])
    n = 3 * H * W
    assert n >= vals.numel()                                    # every crafted value is used
    img = vals.repeat((n + vals.numel() - 1) // vals.numel())[:n].view(3, H, W).cuda().contiguous()
    g = torch.Generator().manual_seed(3)
    target = torch.rand(3, H, W, generator=g).cuda()
    rgb, copy, stats = _hook(orn, img, target, want_img=True, misalign=misalign)
    want = _torch_rgb8(img[None])[0]
    assert len(torch.unique(want)) == 256                       # every byte value occurs
    assert torch.equal(rgb, want), int((rgb.int() - want.int()).abs().max())
    assert torch.equal(copy, img)
    s64 = _stats64(img[None], rgb[None], target[None])[0]
    print('hook stats', stats.tolist(), s64.tolist())
    torch.testing.assert_close(stats.double(), s64, rtol=1e-5, atol=0)


@pytest.mark.parametrize('prec,branch,geo', COMBOS, ids=IDS)
def test_stats_match_fp64_and_the_loss_kernel_and_repeat_bit_for_bit(orn, prec, branch, geo):
    c = _case(orn, prec, branch, geo)
    target = c.eng.frames[ROWS]
    s64 = _stats64(c.out['img'], c.out['rgb8'], target)
    print('stats', c.out['stats'].tolist(), s64.tolist())
    assert c.out['stats'].shape == (len(ROWS), 4)
    torch.testing.assert_close(c.out['stats'].double(), s64, rtol=1e-5, atol=0)
    for i, r in enumerate(ROWS):
        st, _ = orn.ops.loss_stats(c.out['img'][i:i + 1], c.eng.frames[r:r + 1], 'L2', want_grad=False)
        torch.testing.assert_close(c.out['stats'][i, 1], st[4], rtol=1e-5, atol=0)
    assert torch.equal(c.out['stats'], c.again['stats'])
    assert torch.equal(c.out['rgb8'], c.again['rgb8']) and torch.equal(c.out['img'], c.again['img'])


@pytest.mark.parametrize('prec,branch,geo', COMBOS, ids=IDS)
def test_output_selection(orn, prec, branch, geo):
    c = _case(orn, prec, branch, geo)
    a = c.eng.decode_frames(rows=ROWS, rgb8=True, f32=False, stats=False)
    assert set(a) == {'rgb8'} and torch.equal(a['rgb8'], c.out['rgb8'])
    b = c.eng.decode_frames(rows=ROWS, rgb8=False, f32=True, stats=False)
    assert set(b) == {'img'} and torch.equal(b['img'], c.out['img'])
    d = c.eng.decode_frames(rows=ROWS, rgb8=True, f32=False, stats=True)
    assert set(d) == {'rgb8', 'stats'} and torch.equal(d['rgb8'], c.out['rgb8']) and torch.equal(d['stats'], c.out['stats'])
    # the default: the whole resident video, bytes + stats
    e = c.eng.decode_frames()
    assert set(e) == {'rgb8', 'stats'} and e['rgb8'].shape[0] == c.eng.frames.shape[0]
    assert torch.equal(e['rgb8'][ROWS], c.out['rgb8']) and torch.equal(e['stats'][ROWS], c.out['stats'])


def test_argument_errors(orn):
    c = _case(orn, 'fp16', 'ERB', 'c96x2')
    eng, L, ptr = c.eng, orn._lib.lib(), orn._lib.ptr
    rows = torch.tensor(ROWS, dtype=torch.int32, device=eng.device)
    H, W = eng.out_hw
    rgb = torch.empty(len(ROWS), H, W, 3, dtype=torch.uint8, device=eng.device)
    stats = torch.empty(len(ROWS), 4, device=eng.device)
    st = orn._lib.stream()
    E_ARG = -1
    assert L.orn_engine_decode_frames(eng._h, ptr(eng.embeds), ptr(rows), 5, None, ptr(rgb), None, ptr(stats), st) == E_ARG
    assert 'targets' in orn._lib.last_error()
    assert L.orn_engine_decode_frames(eng._h, ptr(eng.embeds), ptr(rows), 5, ptr(eng.frames), None, None, None, st) == E_ARG
    assert 'no output' in orn._lib.last_error()
    assert L.orn_engine_decode_frames(eng._h, ptr(eng.embeds), ptr(rows), -1, ptr(eng.frames), ptr(rgb), None, None, st) == E_ARG
    assert 'n=-1' in orn._lib.last_error()
    assert L.orn_engine_decode_frames(eng._h, ptr(eng.embeds), ptr(rows), 0, None, ptr(rgb), None, None, st) == 0       # nothing to do
    with pytest.raises(orn._lib.OrnError):
        eng.decode_frames(rows=[0, 5])                   # 5 frames resident
    with pytest.raises(orn._lib.OrnError):
        eng.decode_frames(rows=[-1])


def _generator(orn, geo, branch):
    g = GEOS[geo]
    return orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=g['fc'], expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=g['strides'], sin_res=True,
                               lower_width=g['lower_width'], sigmoid=False, deploy=False, branch_type=branch)


def test_decoder_from_train_and_deploy_checkpoints(orn, tmp_path):
    """model_latest.pth and model_latest_deploy.pth of a small ERB fit, loaded into decode-only engines.  The train-mode Decoder
    merges the same parameters with the same kernels as the TrainEngine: bit-identical.  The deploy file holds the merged kernels
    as get_equivalent_kernel_bias computed them when the file was written; the fp32 engines show what that alone does to the
    image (nothing, where the module's merge is the engine's own bit-exact one), and the 16-bit Decoder, whose merge is fp32 too,
    must stay within twice that (max |difference| over all pixels of all frames)."""
    geo = 'narrow_first'
    eng = _engine(orn, 'fp16', 'ERB', geo)
    eng.set_schedule([(k % 5, k + 1, 5e-4) for k in range(5)])
    eng.run(5)
    torch.cuda.synchronize()
    args = types.SimpleNamespace(outf=str(tmp_path), branch_type='ERB', lr=5e-4, beta=0.5)
    orn.main_train.save_checkpoint(args, eng.model, eng, 0, 20.0)
    files = {'train': os.path.join(str(tmp_path), 'model_latest.pth'), 'deploy': os.path.join(str(tmp_path), 'model_latest_deploy.pth')}
    assert all(os.path.exists(f) for f in files.values())
    want = eng.decode_frames(f32=True)
    img = {}
    for kind, path in files.items():
        for prec in ('fp16', 'fp32'):
            model = _generator(orn, geo, 'ERB')
            loaded = orn.checkpoint.load_into(model, orn.checkpoint.load_state_dict_file(path))
            assert loaded == ('deploy' if kind == 'deploy' else 'ERB')
            dec = orn.engine.Decoder(model.cuda(), precision=prec)
            got = dec.decode_frames(embeds=eng.embeds, frames=eng.frames, f32=True)
            img[kind, prec] = got['img']
            if prec == 'fp16':
                one = dec.decode(eng.embeds[2])
                assert torch.equal(one[0], got['img'][2])
                assert torch.equal(got['rgb8'], _torch_rgb8(got['img']))
            if (kind, prec) == ('train', 'fp16'):
                for k in ('img', 'rgb8', 'stats'):
                    assert torch.equal(got[k], want[k]), k
            # a decode-only engine has no gradient or Adam arenas: the training entry points refuse it
            if (kind, prec) == ('deploy', 'fp16'):
                L, ptr = orn._lib.lib(), orn._lib.ptr
                sched = torch.zeros(1, 4, dtype=torch.int32, device=eng.device)
                cursor = torch.zeros(1, dtype=torch.int32, device=eng.device)
                ring = torch.zeros(4, 8, device=eng.device)
                rc = L.orn_engine_train_steps(dec._h, ptr(eng.frames), ptr(eng.embeds), ptr(sched), ptr(cursor), ptr(ring), 4, 1,
                                              orn._lib.stream())
                assert rc == -1 and 'without grads' in orn._lib.last_error()
    d32 = float((img['deploy', 'fp32'] - img['train', 'fp32']).abs().max())
    d16 = float((img['deploy', 'fp16'] - img['train', 'fp16']).abs().max())
    print(f'deploy vs train decode, max |diff|: fp32 engines {d32:.3e}, fp16 engines {d16:.3e}')
    assert d16 <= 2 * d32, (d16, d32)


def test_720p_frames_equal_single_frame_decode(orn):
    """The bench geometry at full size (720 x 1280, the two-work-group conv family, 8192 head blocks with a grid-stride loop)."""
    import bench
    eng = bench.make_engine(seed=7, precision='fp16', cfg=bench.CONFIGS['720p'], frames=6)
    eng.set_schedule([(k % 6, k + 1, 5e-4) for k in range(2)])
    eng.run(2)
    out = eng.decode_frames(f32=True)
    for k in range(6):
        ref = eng.decode(eng.embeds[k])
        assert torch.equal(out['img'][k], ref[0]), k
    assert torch.equal(out['rgb8'], _torch_rgb8(out['img']))
    s64 = _stats64(out['img'], out['rgb8'], eng.frames)
    torch.testing.assert_close(out['stats'].double(), s64, rtol=1e-5, atol=0)
