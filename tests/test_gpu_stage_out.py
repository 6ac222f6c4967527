"""The output kernel of a side stage (k_stage_out_nhwc, csrc/orn_decode_out.hip; orn_engine_eval_stages, include/orn.h N9) through the
hooks of include/orn_debug.h, IEEE half and bf16, both activations.

What it must give needs no tolerance of its own:
    img     the bits of orn_debug_side_head_fwd_* on the same stored inputs (pinned to fp64 by tests/test_gpu_side_head.py);
    rgb8    torch's three fp32 ops on the returned img, exactly;
    stats   fp64 torch on the returned tensors, rtol 1e-5 (the rule of tests/test_gpu_decode.py).
Two frames go back to back into one byte buffer, once more with the buffer shifted by one byte: at 5x7 (105 bytes) the second frame
starts off a 4-byte boundary either way, so the per-lane byte stores and the short last run are exercised beside the dword gather.
Every output sits between guard bands that must stay untouched."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16}
CHANNELS = (1, 3, 26, 32, 96, 128, 131, 160, 512)       # 26, 131: element-wise loads; 131, 160, 512: more than four groups per lane
IMAGES = ((1, 1), (4, 4), (5, 7), (10, 15), (46, 50))   # 4x4: exactly one 16-pixel run; 5x7: 35 pixels, a short last run
MAX_BLOCKS = 8192                                       # ORN_DECODE_MAX_BLOCKS (csrc/orn_internal.h)
BIG = (725, 724)                                        # 524900 pixels > 64 * MAX_BLOCKS: the stride loop (C = 8)
BAND = 64
KINDS = [(k, a) for k in DTYPES for a in (0, 1)]
KIND_IDS = [f'{k}-{"gelu" if a else "swish"}' for k, a in KINDS]


@pytest.fixture(scope='module')
def L():
    from orn_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, 'orn_debug_stage_out_f16_act'), 'liborn.so has no stage-out entry points'
    assert lib.orn_debug_decode_out_ws_bytes() == (2 * MAX_BLOCKS + 64) * 4
    return _lib


def make_inputs(C, H, W, kind, seed, frames=2):
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(3, C, generator=g) * 2 - 1) / math.sqrt(C)
    b = (torch.rand(3, generator=g) * 2 - 1) * 0.1
    z = (torch.randn(frames, H, W, C, generator=g) * 1.5).to(DTYPES[kind])
    target = torch.rand(frames, 3, H, W, generator=g)
    return z, w, b, target


def torch_rgb8(img):
    return img.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)


def stats64(img, rgb8, target):
    t = target.double()
    mf = (img.double() - t).pow(2).mean(dim=(1, 2, 3))
    mq = (rgb8.permute(0, 3, 1, 2).double() / 255 - t).pow(2).mean(dim=(1, 2, 3))
    return torch.stack([mf, -10 * torch.log10(mf), mq, -10 * torch.log10(mq)], dim=1)


def place_z(z, kind, misalign):
    """z on the device; misalign: two bytes past a 16-byte boundary (the element-wise form even where C % 8 == 0)."""
    if not misalign:
        zg = z.cuda().contiguous()
        assert zg.data_ptr() % 16 == 0
        return zg, zg
    buf = torch.zeros(z.numel() + 9, dtype=DTYPES[kind], device='cuda')
    zg = buf[9:].view(z.shape)
    zg.copy_(z)
    assert zg.data_ptr() % 16 == 2
    return zg, buf


def run(L, kind, act, z, w, b, target, sigmoid, offset=0, misalign=False, want=('rgb8', 'img', 'stats')):
    """Every frame of z [F,H,W,C] through the hook, outputs back to back inside guard bands.  Returns (rgb8 [F,H,W,3], img [F,3,H,W],
    stats [F,4]) -- None where not wanted -- after checking the bands and the ticket word."""
    lib = L.lib()
    hook = getattr(lib, f'orn_debug_stage_out_{kind}_act')
    F, H, W, C = z.shape
    HW = H * W
    zg, _keep = place_z(z, kind, misalign)
    wg, bg, tg = w.cuda().contiguous(), b.cuda().contiguous(), target.cuda().contiguous()
    rgb_buf = torch.full((BAND + offset + F * HW * 3 + BAND,), 0xA5, dtype=torch.uint8, device='cuda')
    img_buf = torch.full((BAND + F * 3 * HW + BAND,), float('nan'), device='cuda')
    st_buf = torch.full((BAND + F * 4 + BAND,), float('nan'), device='cuda')
    nb = lib.orn_debug_decode_out_ws_bytes()
    ws = torch.zeros(nb // 4, device='cuda')
    for k in range(F):
        p_rgb = ctypes.c_void_p(rgb_buf.data_ptr() + BAND + offset + k * HW * 3) if 'rgb8' in want else None
        p_img = ctypes.c_void_p(img_buf.data_ptr() + 4 * (BAND + k * 3 * HW)) if 'img' in want else None
        p_st = ctypes.c_void_p(st_buf.data_ptr() + 4 * (BAND + k * 4)) if 'stats' in want else None
        rc = hook(L.ptr(zg[k]), L.ptr(wg), L.ptr(bg), C, H, W, sigmoid, L.ptr(tg[k]) if 'stats' in want else None, p_rgb, p_img, p_st,
                  L.ptr(ws), ctypes.c_size_t(nb), L.stream(), act)
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
        assert int(ws.view(torch.int32)[2 * MAX_BLOCKS]) == 0, 'the ticket word is not back at zero'
    lo, hi = BAND + offset, BAND + offset + F * HW * 3
    assert bool((rgb_buf[:lo] == 0xA5).all()) and bool((rgb_buf[hi:] == 0xA5).all()), 'bytes outside the frames were written'
    assert bool(torch.isnan(img_buf[:BAND]).all()) and bool(torch.isnan(img_buf[BAND + F * 3 * HW:]).all())
    assert bool(torch.isnan(st_buf[:BAND]).all()) and bool(torch.isnan(st_buf[BAND + F * 4:]).all())
    rgb = rgb_buf[lo:hi].view(F, H, W, 3).clone() if 'rgb8' in want else None
    img = img_buf[BAND:BAND + F * 3 * HW].view(F, 3, H, W).clone() if 'img' in want else None
    st = st_buf[BAND:BAND + F * 4].view(F, 4).clone() if 'stats' in want else None
    if 'rgb8' not in want:
        assert bool((rgb_buf == 0xA5).all())
    if 'img' not in want:
        assert bool(torch.isnan(img_buf).all())
    return rgb, img, st


def side_head(L, kind, act, z, w, b, sigmoid, misalign=False):
    """orn_debug_side_head_fwd_* on the same stored inputs: [F,3,H,W]."""
    lib = L.lib()
    hook = getattr(lib, f'orn_debug_side_head_fwd_{kind}_act')
    F, H, W, C = z.shape
    zg, _keep = place_z(z, kind, misalign)
    wg, bg = w.cuda().contiguous(), b.cuda().contiguous()
    out = torch.empty(F, 3, H, W, device='cuda')
    for k in range(F):
        assert hook(L.ptr(zg[k]), L.ptr(wg), L.ptr(bg), C, H, W, sigmoid, L.ptr(out[k]), L.stream(), act) == 0, L.last_error()
    torch.cuda.synchronize()
    return out


def check(L, kind, act, C, H, W, sigmoid, seed, offsets=(0, 1)):
    z, w, b, target = make_inputs(C, H, W, kind, seed)
    ref = side_head(L, kind, act, z, w, b, sigmoid)
    assert torch.isfinite(ref).all()
    first = None
    for off in offsets:
        rgb, img, st = run(L, kind, act, z, w, b, target, sigmoid, offset=off)
        assert torch.equal(img, ref), f'img differs from the side head: max {float((img - ref).abs().max())}'
        want = torch_rgb8(img)
        assert torch.equal(rgb, want), int((rgb.int() - want.int()).abs().max())
        s64 = stats64(img, rgb, target.cuda())
        print(f'C={C} {H}x{W} sigmoid={sigmoid} offset={off} stats', st.tolist(), s64.tolist())
        torch.testing.assert_close(st.double(), s64, rtol=1e-5, atol=0)
        if first is None:
            first = (rgb, img, st)
        else:       # a second run, the byte buffer shifted: the same bits
            assert torch.equal(rgb, first[0]) and torch.equal(img, first[1]) and torch.equal(st, first[2])
    again = run(L, kind, act, z, w, b, target, sigmoid, offset=offsets[0])
    assert all(torch.equal(a, f) for a, f in zip(again, first)), 'two runs differ'


@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('kind,act', KINDS, ids=KIND_IDS)
def test_every_output_on_the_shape_grid(L, kind, act, C):
    for i, (H, W) in enumerate(IMAGES):
        for sigmoid in (0, 1):
            check(L, kind, act, C, H, W, sigmoid, seed=1000 * C + 10 * i + sigmoid)


@pytest.mark.parametrize('kind,act', KINDS, ids=KIND_IDS)
def test_stride_loop_beyond_the_grid_cap(L, kind, act):
    H, W = BIG
    assert H * W > 64 * MAX_BLOCKS
    check(L, kind, act, 8, H, W, 0, seed=77, offsets=(0,))


@pytest.mark.parametrize('kind,act', KINDS, ids=KIND_IDS)
def test_each_output_alone(L, kind, act):
    """Each output is optional: asked for alone it has the bits it has beside the others, and the others' buffers stay untouched."""
    z, w, b, target = make_inputs(26, 5, 7, kind, 5)
    rgb, img, st = run(L, kind, act, z, w, b, target, 0, offset=1)
    assert torch.equal(run(L, kind, act, z, w, b, target, 0, offset=1, want=('rgb8',))[0], rgb)
    assert torch.equal(run(L, kind, act, z, w, b, target, 0, want=('img',))[1], img)
    assert torch.equal(run(L, kind, act, z, w, b, target, 0, want=('stats',))[2], st)


@pytest.mark.parametrize('kind,act', KINDS, ids=KIND_IDS)
def test_vector_and_elementwise_forms_give_the_same_bits(L, kind, act):
    """C = 32: 16-byte loads on an aligned z, element-wise loads on the same values two bytes past a 16-byte boundary."""
    for (H, W) in ((5, 7), (10, 15), (46, 50)):
        z, w, b, target = make_inputs(32, H, W, kind, 11 + H)
        a = run(L, kind, act, z, w, b, target, 0)
        m = run(L, kind, act, z, w, b, target, 0, misalign=True)
        assert all(torch.equal(x, y) for x, y in zip(a, m))
        assert torch.equal(m[1], side_head(L, kind, act, z, w, b, 0, misalign=True))


def _act64(z, act):
    z = z.double()
    return 0.5 * z * torch.erfc(-z / math.sqrt(2.0)) if act else z * torch.sigmoid(z)


def crafted(kind, act, sigmoid, sweep=32):
    """Pre-activations whose head output sweeps, in steps of about one fp32 ulp of the output (at least 2^-25), across every boundary (k + 0.5) / 255,
    k = 3..252 -- the values whose product with 255 sits where torch's two separately rounded ops and a contracted fma part.
    C = 8 channels with weights 8, -8, 8/16, 8/16^2, ..: channel 1 holds a fixed value that cancels channel 0's offset, the others are
    the digits of a greedy expansion of the wanted pre-activation u over the activation values of the 16-bit grid in [0.5, 2].
    The device's own exp and the fp32 sums move each pixel by a few ulp: the sweep is wider than that."""
    dt = DTYPES[kind]
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(dt)
    grid = bits[torch.isfinite(bits.float()) & (bits.float() >= 0.5) & (bits.float() <= 2.0)]
    grid = grid[torch.argsort(grid.float())]
    A = _act64(grid, act)
    assert bool((A[1:] > A[:-1]).all())
    amin = A[0]
    D = A - amin                                                    # the digits a channel can add, ascending from 0
    wts = torch.tensor([8.0, -8.0] + [8.0 / 16 ** i for i in range(1, 7)], dtype=torch.float64)
    B0 = -5.8                                                       # u = B0 + 8 d_0 + sum_i w_i d_i
    bias = B0 - float(wts[2:].sum() * amin)
    k = torch.arange(3, 253, dtype=torch.float64)
    mid = ((k + 0.5) / 255).float().double()
    slope = mid * (1 - mid) if sigmoid else 2 * mid * (1 - mid)
    ustar = torch.log(mid / (1 - mid)) if sigmoid else torch.atanh(2 * mid - 1)
    ulp = torch.nextafter(mid.float(), torch.ones(1)).double() - mid
    # (tanh + 1) / 2 has the spacing of tanh's own values, 2^-25 near -1, however small the output is: no finer step is of use there
    ulp = torch.clamp(ulp, min=2.0 ** -25)
    j = torch.arange(-sweep, sweep + 1, dtype=torch.float64)
    u = (ustar[:, None] + j[None, :] * (ulp / slope)[:, None]).reshape(-1)
    r = u - B0
    assert bool((r > 0).all()) and bool((r < 8 * D[-1]).all())
    zs = []
    for c in (0, 2, 3, 4, 5, 6, 7):
        idx = (torch.searchsorted(D, (r / wts[c]).contiguous(), right=True) - 1).clamp(0, D.numel() - 1)
        r = r - wts[c] * D[idx]
        zs.append(grid[idx])
    fixed = grid[0].expand_as(zs[0])
    z = torch.stack([zs[0], fixed] + zs[1:], dim=1)                 # [pixels, 8]
    w = wts.float()[None, :].repeat(3, 1)
    b = torch.full((3,), bias, dtype=torch.float32)
    return z, w, b, mid.float(), j.numel()


@pytest.mark.parametrize('sigmoid', (0, 1))
@pytest.mark.parametrize('kind,act', KINDS, ids=KIND_IDS)
def test_quantisation_at_the_half_way_points(L, kind, act, sigmoid):
    z, w, b, mid, per = crafted(kind, act, sigmoid)
    n = z.shape[0]
    H, W = 125, n // 125
    assert H * W == n
    z = z.view(1, H, W, 8)
    target = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(2))
    ref = side_head(L, kind, act, z, w, b, sigmoid)
    for off in (0, 1, 2, 3):
        rgb, img, st = run(L, kind, act, z, w, b, target, sigmoid, offset=off)
        assert torch.equal(img, ref)
        want = torch_rgb8(img)
        assert torch.equal(rgb, want), int((rgb.int() - want.int()).abs().max())
        torch.testing.assert_close(st.double(), stats64(img, rgb, target.cuda()), rtol=1e-5, atol=0)
    # the crafted input does what it is for: each sweep crosses its boundary, and values sit on or right beside it
    v = img[0, 0].reshape(-1, per).cpu()
    m = mid[:, None]
    crossed = ((v < m).any(dim=1) & (v >= m).any(dim=1))
    one = torch.ones_like(m)
    near = ((v == m) | (v == torch.nextafter(m, one)) | (v == torch.nextafter(m, -one))).any(dim=1)
    print(f'{int(crossed.sum())} of {crossed.numel()} boundaries crossed, {int(near.sum())} with a value within one ulp, '
          f'{int((v == m).sum())} values exactly on one')
    assert bool(crossed.all())
    assert len(torch.unique(rgb)) >= 250


def test_bad_arguments_are_refused_with_nothing_written(L):
    from orn_amd._lib import last_error
    lib = L.lib()
    z, w, b, target = make_inputs(8, 5, 7, 'f16', 1, frames=1)
    zg, wg, bg, tg = z.cuda(), w.cuda(), b.cuda(), target.cuda()
    rgb = torch.full((5 * 7 * 3,), 0xA5, dtype=torch.uint8, device='cuda')
    img = torch.full((3, 5, 7), float('nan'), device='cuda')
    st = torch.full((4,), float('nan'), device='cuda')
    nb = lib.orn_debug_decode_out_ws_bytes()
    ws = torch.full((nb // 4,), float('nan'), device='cuda')
    for name in ('orn_debug_stage_out_f16', 'orn_debug_stage_out_bf16'):
        hook = getattr(lib, name)
        for C, tgt, stats in ((0, tg, st), (513, tg, st), (8, None, st)):
            rc = hook(L.ptr(zg), L.ptr(wg), L.ptr(bg), C, 5, 7, 0, L.ptr(tgt), L.ptr(rgb), L.ptr(img), L.ptr(stats), L.ptr(ws),
                      ctypes.c_size_t(nb), L.stream())
            assert rc == -1, (name, C, rc)                         # ORN_E_ARG
            assert last_error(), 'no error text'
        rc = hook(L.ptr(zg), L.ptr(wg), L.ptr(bg), 8, 5, 7, 0, None, None, None, None, None, ctypes.c_size_t(0), L.stream())
        assert rc == -1 and last_error()
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()) and bool(torch.isnan(img).all()) and bool(torch.isnan(st).all()) and bool(torch.isnan(ws).all())
