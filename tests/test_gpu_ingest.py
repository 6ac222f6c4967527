"""GPU tests of the frame ingest (include/orn.h K11; csrc/orn_ingest.hip): ToTensor + F.adaptive_avg_pool2d(data, (h, w)) on the
device, from uint8 HWC pixels (orn_frames_ingest_u8) and from fp32 planar frames (orn_frames_pool_f32).

The reference is torch's own CPU op on the ToTensor frames.  The kernel performs the same operations in the same order (fp32
row-major window sum from 0, then / kh, then / kw, both divisions correctly rounded; a byte is (float)b / 255.0f), so every
comparison is torch.equal: no tolerance."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the kernel's tiling (csrc/orn_ingest.hip): a work-group covers ING_TX x ING_TH output pixels of one frame and stages the source
# rows under them in passes of ING_STAGE_BYTES of LDS; when ING_TX columns' source span does not fit one pass, the tile narrows
ING_TX, ING_TH, ING_STAGE_BYTES = 128, 8, 32768

SHAPES = [
    ((27, 48), (18, 32)),        # ratio 1.5, overlapping windows of 1 to 2
    ((36, 64), (18, 32)),        # exact 2x
    ((30, 50), (18, 32)),        # windows up to 3, 150-byte rows
    ((54, 96), (18, 32)),        # 3x
    ((19, 33), (18, 32)),        # 99-byte rows, misaligned row starts
    ((18, 32), (18, 32)),        # identity: ToTensor for uint8, an exact copy for fp32
    ((12, 20), (18, 32)),        # upsampling
    ((36, 32), (18, 32)),        # one axis only
    # an output row spans two work-groups (161 > ING_TX, the second one 33 columns wide), two row tiles (12 > ING_TH, the second
    # one 4 rows high); a tile's 67 source rows of 1536 (uint8) / 3 x 2048 (fp32) bytes take 4 / 14 staging passes of 20 / 5
    # rows, and the 9-row windows straddle the pass boundaries
    ((100, 644), (12, 161)),
    # 90 source columns per output column: ING_TX columns' span (34.6 KB of bytes, 3 x 46 KB of floats) exceeds a pass, the tile
    # narrows to 64 (uint8) / 16 (fp32) columns; row windows of 2 to 3
    ((9, 2700), (4, 30)),
]
IDS = [f'{s[0]}x{s[1]}-{d[0]}x{d[1]}' for s, d in SHAPES]


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, model, utils, engine  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


_CASE = {}


def _case(src, dst, n=3):
    """(uint8 [n,H,W,3] with 0 and 255 present, its ToTensor frames [n,3,H,W], the pooled reference), all on the CPU; made once."""
    key = (src, dst, n)
    if key not in _CASE:
        g = torch.Generator().manual_seed(src[0] * 10007 + src[1] * 13 + dst[0])
        u8 = torch.randint(0, 256, (n, src[0], src[1], 3), generator=g, dtype=torch.uint8)
        u8[0, 0, 0, 0], u8[-1, -1, -1, -1], u8[0, 0, 1, 1], u8[-1, -1, 0, 2] = 0, 255, 255, 0
        tt = u8.permute(0, 3, 1, 2).float().div(255.0).contiguous()
        _CASE[key] = (u8, tt, F.adaptive_avg_pool2d(tt, dst))
    return _CASE[key]


@pytest.mark.parametrize('src,dst', SHAPES, ids=IDS)
def test_both_entries_equal_torch(orn, src, dst):
    u8, tt, want = _case(src, dst)
    got8 = orn.ops.ingest_frames(u8.cuda(), dst)
    assert got8.shape == want.shape and got8.dtype == torch.float32
    assert torch.equal(got8.cpu(), want), int((got8.cpu() != want).sum())
    got32 = orn.ops.ingest_frames(tt.cuda(), dst)
    assert torch.equal(got32.cpu(), want), int((got32.cpu() != want).sum())
    if src == dst:
        assert torch.equal(got8.cpu(), tt) and torch.equal(got32.cpu(), tt)
    # fp32 values that are not byte quotients
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, src[0], src[1], generator=g)
    gotx = orn.ops.ingest_frames(x.cuda(), dst)
    wantx = F.adaptive_avg_pool2d(x, dst)
    assert torch.equal(gotx.cpu(), wantx), int((gotx.cpu() != wantx).sum())


def test_1080p_to_720p(orn):
    src, dst = (1080, 1920), (720, 1280)
    u8, tt, want = _case(src, dst, n=2)
    got8 = orn.ops.ingest_frames(u8.cuda(), dst)
    assert torch.equal(got8.cpu(), want), int((got8.cpu() != want).sum())
    got32 = orn.ops.ingest_frames(tt.cuda(), dst)
    assert torch.equal(got32.cpu(), want), int((got32.cpu() != want).sum())


@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_chunks_and_neighbouring_memory(orn, kind):
    """chunk=1 equals chunk=None bit for bit, and the floats on both sides of dst keep their value (guard rows filled with a
    sentinel before the call); frame sizes whose byte count is odd, so the second and third frame start unaligned."""
    src, dst = (19, 33), (18, 32)
    u8, tt, want = _case(src, dst)
    x = (u8 if kind == 'u8' else tt).cuda()
    n, guard = x.shape[0], 4 * dst[1]
    whole = orn.ops.ingest_frames(x, dst)
    buf = torch.full((2 * guard + want.numel(),), -7.0, device='cuda')
    out = buf[guard:guard + want.numel()].view(n, 3, *dst)
    back = orn.ops.ingest_frames(x, dst, chunk=1, out=out)
    assert back.data_ptr() == out.data_ptr()
    assert torch.equal(out, whole) and torch.equal(out.cpu(), want)
    assert bool((buf[:guard] == -7.0).all()) and bool((buf[guard + want.numel():] == -7.0).all())
    two = orn.ops.ingest_frames(x, dst, chunk=2)
    assert torch.equal(two, whole)
    assert orn.ops.ingest_frames(x[:0], dst).shape == (0, 3) + dst
    for bad in (x.cpu(), x[0], x.double(), x.permute(0, 2, 3, 1) if kind == 'f32' else x.permute(0, 3, 1, 2)):
        with pytest.raises(orn._lib.OrnError):
            orn.ops.ingest_frames(bad, dst)


# ---- the engine: frames of another size are pooled in place of the OrnError ---------------------------------------------------
def _generator(orn, fc, strides, lower_width):
    torch.manual_seed(1)
    return orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=fc, expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=strides, sin_res=True,
                               lower_width=lower_width, sigmoid=False, deploy=False, branch_type='ERB')


TINY = dict(fc='3_4_8', strides=[2, 2, 2], lower_width=8)          # output 24 x 32
C96 = dict(fc='3_4_96', strides=[2, 2], lower_width=96)            # smoke()'s 16-bit geometry, output 12 x 16
_VIDEO = {}


def _video(big_hw, out_hw, n=4):
    """(source frames [n,3,H,W] at big_hw, torch's pool of them to out_hw, embeds); made once, never modified."""
    if (big_hw, out_hw) not in _VIDEO:
        from oracle import cpu_ref
        big = cpu_ref.synthetic_video(n, big_hw[0], big_hw[1], seed=5)
        embeds = cpu_ref.positional_encoding(torch.tensor([k / n for k in range(n)]), 1.25, 40)
        _VIDEO[(big_hw, out_hw)] = (big, F.adaptive_avg_pool2d(big, out_hw).contiguous(), embeds)
    return _VIDEO[(big_hw, out_hw)]


def _fit(orn, geo, prec, frames, embeds, steps, **run):
    eng = orn.engine.TrainEngine(_generator(orn, **geo), loss_type='Fusion6', beta=0.5, precision=prec)
    eng.set_video(frames, embeds)
    n, per = frames.shape[0], run.get('batch', 1)
    eng.set_schedule([(k % n, k // per + 1, 5e-4) for k in range(steps * per)])
    eng.run(steps, **run)
    torch.cuda.synchronize()
    return eng, eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.stats(steps).clone()


def test_set_video_pools_frames_of_another_size(orn):
    big, pooled, embeds = _video((36, 48), (24, 32))
    eng = orn.engine.TrainEngine(_generator(orn, **TINY), loss_type='Fusion6', beta=0.5)
    assert tuple(eng.out_hw) == (24, 32)
    eng.set_video(big, embeds)
    assert eng.frames.shape == (4, 3, 24, 32) and torch.equal(eng.frames.cpu(), pooled)
    # uint8 [N,H,W,3], as PIL decodes it
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (4, 36, 48, 3), generator=g, dtype=torch.uint8)
    eng.set_video(u8, embeds)
    assert torch.equal(eng.frames.cpu(), F.adaptive_avg_pool2d(u8.permute(0, 3, 1, 2).float().div(255.0), (24, 32)))
    eng.set_video(pooled, embeds)                                      # at size: as before
    assert torch.equal(eng.frames.cpu(), pooled)
    for bad in (big[0], big[:, :2], big.permute(0, 2, 3, 1), u8.permute(0, 3, 1, 2), u8[..., :2]):
        with pytest.raises(orn._lib.OrnError):
            eng.set_video(bad, embeds)
        with pytest.raises(orn._lib.OrnError):
            eng.decode_frames(frames=bad)


@pytest.mark.parametrize('form', ['graph', 'pipelined', 'batch2'])
def test_training_on_big_frames_equals_training_on_pooled_frames(orn, form):
    """Three hipGraph steps (fp32), three pipelined steps on smoke()'s 16-bit geometry, one -b 2 step: parameters, Adam moments
    and ring records bit-identical to the same engine fed torch's pooled frames."""
    geo, prec, big_hw, steps, run = {'graph': (TINY, 'fp32', (36, 48), 3, dict(graph=True)),
                                     'pipelined': (C96, 'fp16', (18, 24), 3, dict()),
                                     'batch2': (TINY, 'fp32', (36, 48), 1, dict(batch=2))}[form]
    out_hw = (24, 32) if geo is TINY else (12, 16)
    big, pooled, embeds = _video(big_hw, out_hw)
    a = _fit(orn, geo, prec, big, embeds, steps, **run)
    b = _fit(orn, geo, prec, pooled, embeds, steps, **run)
    assert tuple(a[0].out_hw) == out_hw and torch.equal(a[0].frames, b[0].frames)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(a[4]).all()) and a[4][:, 7].tolist() == [float(k + 1) for k in range(steps)]


def test_decode_frames_pools_its_targets(orn):
    big, pooled, embeds = _video((36, 48), (24, 32))
    eng = orn.engine.TrainEngine(_generator(orn, **TINY), loss_type='Fusion6', beta=0.5)
    eng.set_video(pooled, embeds)
    want = eng.decode_frames(frames=pooled, stats=True)
    got = eng.decode_frames(frames=big, stats=True)
    for k in ('rgb8', 'stats'):
        assert torch.equal(got[k], want[k]), k
    dec = orn.engine.Decoder(_generator(orn, **TINY).cuda(), precision='fp32')
    assert torch.equal(dec.decode_frames(embeds=embeds, frames=big)['stats'], dec.decode_frames(embeds=embeds, frames=pooled)['stats'])


# ---- the CLI: a PNG directory at 1.5x the model's output ------------------------------------------------------------------------
def test_png_directory_of_another_size_through_the_cli(tmp_path, monkeypatch, capsys):
    """60 x 90 PNGs under a 40 x 60 model (fc 2_3, strides 5 2 2): main_train pools them on the way in (the engine's resident
    frames are torch's pool of the files), runs two epochs, writes its checkpoints and reports a finite PSNR; main_eval
    --decoder engine then evaluates the fit against the pooled targets."""
    import math
    import numpy as np
    from PIL import Image
    import orn_amd
    from orn_amd import main_eval, main_train
    run = tmp_path / 'run'
    run.mkdir()
    d = tmp_path / 'data' / 'bigvid'
    d.mkdir(parents=True)
    rng = np.random.RandomState(3)
    imgs = []
    for k in range(5):
        a = rng.randint(0, 256, size=(60, 90, 3), dtype=np.uint8)
        Image.fromarray(a).save(d / f'{k:05d}.png')
        imgs.append(a)
    monkeypatch.chdir(run)
    flags = ('-e 2 --lower_width 96 --num_blocks 1 --dataset bigvid --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 '
             '--reduction 2 --fc_hw_dim 2_3_26 --expansion 1 --single_res --loss Fusion6 --warmup 0.2 --lr_type cosine --strides 5 2 2 '
             '--conv_type conv -b 1 --lr 0.0005 --norm none --act swish --outf big_t --branch_type ERB --eval_freq 1 --precision fp32').split()
    captured = {}
    orig = main_train.evaluate

    def spy(model, eng, args, val=None, gap=None):
        captured['frames'] = eng.frames.clone()
        return orig(model, eng, args, val, gap)
    monkeypatch.setattr(main_train, 'evaluate', spy)
    best = main_train.train(main_train.parse_args(flags))['bigvid']
    assert math.isfinite(best) and best > 5.0
    want = F.adaptive_avg_pool2d(torch.from_numpy(np.stack(imgs)).permute(0, 3, 1, 2).float().div(255.0), (40, 60))
    assert torch.equal(captured['frames'].cpu(), want)
    said = capsys.readouterr().out
    assert '60x90' in said and '40x60' in said and 'main_train.py:239' in said
    outf = run / 'result' / 'big_t'
    for f in ('model_latest.pth', 'model_latest_deploy.pth', 'model_train_best.pth', 'rank0.txt'):
        assert (outf / f).exists(), f
    psnr = main_eval.main(flags + ['--decoder', 'engine'])
    assert math.isfinite(psnr) and psnr > 5.0
