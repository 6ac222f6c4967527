"""GPU tests of the batched, sync-free MS-SSIM (orn_msssim_frames, include/orn.h; ops.ms_ssim_frames): one value per frame,
pytorch_msssim.ms_ssim(pred[k:k+1], target[k:k+1], data_range=1) as utils.py:201-211 calls it with batch 1.

Inputs follow test_gpu_parity.test_msssim: a blurred uniform target, pred = target + sigma_k * noise with sigma_k = 0.02 (k + 1),
clamped, so every frame has its own value (0.85 .. 0.99 on the oracle: no relu clamp involved).  Tolerance against the fp64
oracle: 2e-5 absolute, test_msssim's.  Everything else is bit equality."""
import ctypes
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, H, W): the smallest legal image (every level odd, a 1x1 map at the last level); H 180 -> 90 -> 45 -> 23 -> 12 (both
# paddings); mixed parities; a ragged last tile column at several levels
SHAPES = [(3, 161, 161), (4, 180, 240), (2, 176, 193), (3, 161, 417)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
E_ARG, E_WS = -1, -2


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import ops, utils  # noqa: F401
    orn_amd._lib.lib()
    return orn_amd


def _inputs(n, H, W):
    gen = torch.Generator().manual_seed(H + W)
    t = torch.rand(n, 3, H, W, generator=gen)
    t = torch.nn.functional.avg_pool2d(t, 5, 1, 2)                     # some structure so cs is not ~0
    sigma = 0.02 * torch.arange(1, n + 1, dtype=torch.float32).view(n, 1, 1, 1)
    p = (t + sigma * torch.randn(n, 3, H, W, generator=gen)).clamp(0, 1)
    return p, t


_CASES = {}


def _case(orn, shape):
    """Inputs, the fp64 oracle and the device result of one shape: computed once, never modified."""
    if shape not in _CASES:
        from oracle import cpu_ref
        p, t = _inputs(*shape)
        ref = cpu_ref.ms_ssim(p.double(), t.double(), size_average=False)
        pd, td = p.cuda(), t.cuda()
        out = orn.ops.ms_ssim_frames(pd, td)
        torch.cuda.synchronize()
        _CASES[shape] = types.SimpleNamespace(p=pd, t=td, ref=ref, out=out)
    return _CASES[shape]


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_matches_oracle_per_frame(orn, shape):
    c = _case(orn, shape)
    assert c.out.shape == (shape[0],) and c.ref.shape == (shape[0],)
    err = (c.out.cpu().double() - c.ref).abs()
    print(f'{shape}: oracle {c.ref.tolist()} device {c.out.tolist()} max |diff| {float(err.max()):.3e}')
    assert float(c.ref.min()) > 0.5 and len(set(c.ref.tolist())) == shape[0]       # every frame its own value, far from the clamp
    assert float(err.max()) <= 2e-5, (c.out.tolist(), c.ref.tolist())


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_bit_equal_to_single_frame_op(orn, shape):
    c = _case(orn, shape)
    single = torch.stack([orn.ops.ms_ssim(c.p[k:k + 1], c.t[k:k + 1]) for k in range(shape[0])])
    assert torch.equal(c.out, single), (c.out.tolist(), single.tolist())


# float32 bit patterns (tensor.view(torch.int32)) of ops.ms_ssim as commit 68b8921 computed them on an MI355X, when orn_msssim still
# had kernels of its own (k_ssim_cs_partial, k_avgpool2, k_msssim_finalize): printed by a script that called ops.ms_ssim on the
# inputs named below, before those kernels were removed.  Today both entry points run the same kernels; these are the old values.
# (a) every frame of _inputs(*shape) on its own (B = 1)
RECORDED_PER_FRAME = {
    (3, 161, 161): [1065145360, 1064602319, 1063822306],
    (4, 180, 240): [1065143038, 1064598536, 1063788901, 1062865015],
    (2, 176, 193): [1065152509, 1064587273],
    (3, 161, 417): [1065149782, 1064586291, 1063802435],
}
# (b) the whole batch of _inputs(*shape) in one call: the mean over 12 and 9 planes
RECORDED_BATCH = {(4, 180, 240): 1064098873, (3, 161, 417): 1064512836}
# (c) the B = 2, 161 x 177 input of test_gpu_parity.test_msssim: 6 planes
RECORDED_PARITY_2x161x177 = 1064252808


def _bits(x):
    return x.detach().reshape(-1).cpu().view(torch.int32).tolist()


def test_bits_are_the_recorded_ones(orn):
    assert set(RECORDED_PER_FRAME) == set(SHAPES)
    for shape in SHAPES:
        c = _case(orn, shape)
        single = torch.stack([orn.ops.ms_ssim(c.p[k:k + 1], c.t[k:k + 1]) for k in range(shape[0])])
        print(f'{shape}: frames {_bits(c.out)} single {_bits(single)} recorded {RECORDED_PER_FRAME[shape]}')
        assert _bits(c.out) == RECORDED_PER_FRAME[shape]
        assert _bits(single) == RECORDED_PER_FRAME[shape]
    for shape, want in RECORDED_BATCH.items():
        c = _case(orn, shape)
        got = _bits(orn.ops.ms_ssim(c.p, c.t))
        print(f'{shape}: batch {got} recorded {want}')
        assert got == [want]
    B, H, W = 2, 161, 177                                              # test_gpu_parity.test_msssim's construction
    gen = torch.Generator().manual_seed(H + W)
    t = torch.nn.functional.avg_pool2d(torch.rand(B, 3, H, W, generator=gen), 5, 1, 2)
    p = (t + 0.05 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    got = _bits(orn.ops.ms_ssim(p.cuda(), t.cuda()))
    print(f'parity input 2x161x177: {got} recorded {RECORDED_PARITY_2x161x177}')
    assert got == [RECORDED_PARITY_2x161x177]


def test_row_indirection(orn):
    c = _case(orn, SHAPES[0])                                          # 3 frames: a 3-frame target table
    rows = [2, 0, 2, 1]
    pred = c.p[rows].contiguous()
    via_rows = orn.ops.ms_ssim_frames(pred, c.t, rows=rows)
    direct = orn.ops.ms_ssim_frames(pred, c.t[rows].contiguous())
    on_device = orn.ops.ms_ssim_frames(pred, c.t, rows=torch.tensor(rows, dtype=torch.int64, device='cuda'))
    assert torch.equal(via_rows, direct) and torch.equal(on_device, direct)
    assert via_rows[0].item() == via_rows[2].item()
    assert torch.equal(via_rows, c.out[rows])
    with pytest.raises(orn._lib.OrnError, match='out of range'):
        orn.ops.ms_ssim_frames(pred, c.t, rows=[0, 1, 2, 3])


def _call(orn, p, t, rows, out, ws, ws_bytes):
    n, Ch, H, W = p.shape
    ptr = orn._lib.ptr
    return orn._lib.lib().orn_msssim_frames(ptr(p), ptr(t), ptr(rows), n, Ch, H, W, ptr(out), ptr(ws), ctypes.c_size_t(ws_bytes),
                                            orn._lib.stream())


def test_chunking_does_not_change_the_bits(orn):
    L = orn._lib.lib()
    n, H, W = 5, 161, 161
    p, t = (x.cuda() for x in _inputs(n, H, W))
    size = {f: L.orn_msssim_frames_ws_bytes(f, 3, H, W) for f in (1, 2, 5)}
    assert 0 < size[1] < size[2] < size[5]
    ws = torch.empty(size[5], dtype=torch.uint8, device='cuda')
    got = {}
    for f in (1, 2, 5):                                                # chunks of 1; 2, 2, 1; 5
        got[f] = torch.full((n,), -1.0, device='cuda')
        assert _call(orn, p, t, None, got[f], ws, size[f]) == 0, orn._lib.last_error()
    assert _call(orn, p, t, None, torch.empty(n, device='cuda'), ws, size[2] + size[1] // 2) == 0       # between two sizes: chunks of 2
    torch.cuda.synchronize()
    assert torch.equal(got[1], got[2]) and torch.equal(got[1], got[5]), got
    assert torch.equal(got[5], orn.ops.ms_ssim_frames(p, t))
    assert len(set(got[1].tolist())) == n and float(got[1].min()) > 0.5
    assert _call(orn, p, t, None, got[1], ws, size[1] - 1) == E_WS
    assert 'workspace too small' in orn._lib.last_error()


def test_captured_in_a_graph_and_replayed(orn):
    """No copy, no sync: the call records into a hipGraph and the replays follow inputs changed in place."""
    L = orn._lib.lib()
    c = _case(orn, SHAPES[2])
    n, _, H, W = c.p.shape
    second_p, second_t = c.t.flip(0).contiguous(), c.p.flip(0).contiguous()
    want = [c.out, orn.ops.ms_ssim_frames(second_p, second_t)]          # (the first call of the process is made eagerly: the taps)
    p, t = c.p.clone(), c.t.clone()
    out = torch.zeros(n, device='cuda')
    nbytes = L.orn_msssim_frames_ws_bytes(1, 3, H, W)                   # one frame per chunk: two chunks inside the graph
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        rc = _call(orn, p, t, None, out, ws, nbytes)
    assert rc == 0, orn._lib.last_error()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want[0]), (out.tolist(), want[0].tolist())
    p.copy_(second_p)
    t.copy_(second_t)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want[1]), (out.tolist(), want[1].tolist())
    assert not torch.equal(want[0], want[1])


def _call_single(orn, p, t, out, ws, ws_bytes):
    B, Ch, H, W = p.shape
    ptr = orn._lib.ptr
    return orn._lib.lib().orn_msssim(ptr(p), ptr(t), B, Ch, H, W, ptr(out), ptr(ws), ctypes.c_size_t(ws_bytes), orn._lib.stream())


def test_single_call_is_capturable(orn):
    """orn_msssim uploads nothing and does not synchronise: after one eager call it records into a hipGraph, and the replays
    follow inputs changed in place."""
    L = orn._lib.lib()
    c = _case(orn, SHAPES[0])                                          # 161 x 161: the smallest legal image
    first_p, first_t = c.p[0:1].contiguous(), c.t[0:1].contiguous()
    second_p, second_t = c.t[1:2].contiguous(), c.p[2:3].contiguous()
    want = [orn.ops.ms_ssim(first_p, first_t), orn.ops.ms_ssim(second_p, second_t)]     # eager (and the process's first call: the taps)
    p, t = first_p.clone(), first_t.clone()
    out = torch.zeros(1, device='cuda')
    nbytes = L.orn_msssim_ws_bytes(1, 3, 161, 161)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        rc = _call_single(orn, p, t, out, ws, nbytes)
    assert rc == 0, orn._lib.last_error()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[0]), (out.tolist(), want[0].item())
    p.copy_(second_p)
    t.copy_(second_t)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[1]), (out.tolist(), want[1].item())
    assert not torch.equal(want[0], want[1])


def test_single_call_workspace_size(orn):
    L = orn._lib.lib()
    c = _case(orn, SHAPES[0])
    p, t = c.p[0:1].contiguous(), c.t[0:1].contiguous()
    nbytes = L.orn_msssim_ws_bytes(1, 3, 161, 161)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    out = torch.zeros(1, device='cuda')
    assert _call_single(orn, p, t, out, ws, nbytes - 1) == E_WS
    assert 'workspace too small' in orn._lib.last_error()
    assert _call_single(orn, p, t, out, ws, nbytes) == 0, orn._lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out[0], c.out[0])


def test_argument_errors(orn):
    p = torch.zeros(1, 3, 160, 300, device='cuda')
    out, ws = torch.zeros(1, device='cuda'), torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    assert _call(orn, p, p, None, out, ws, ws.numel()) == E_ARG
    assert 'must exceed 160' in orn._lib.last_error()
    with pytest.raises(orn._lib.OrnError, match='must exceed 160'):
        orn.ops.ms_ssim_frames(p, p)
    q = torch.zeros(1, 3, 200, 240, device='cuda')
    assert _call(orn, q, q, None, None, ws, ws.numel()) == E_ARG and 'null pointer' in orn._lib.last_error()
    assert orn.ops.ms_ssim_frames(q[:0], q).shape == (0,)
