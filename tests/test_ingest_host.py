"""CPU tests of the frame ingest (include/orn.h K11): the two entries are exported and refuse bad arguments with text, and
FrameDir.load(out_hw=...) on the host is torch's own adaptive_avg_pool2d of the ToTensor frames."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    return orn_amd


def test_ingest_entries_are_exported_and_refuse_bad_arguments(orn):
    assert {'orn_frames_ingest_u8', 'orn_frames_pool_f32'} <= set(orn._lib.EXPORTS)
    L = orn._lib.lib()
    for fn, word in ((L.orn_frames_ingest_u8, 'ingest'), (L.orn_frames_pool_f32, 'pool')):
        assert fn(None, 1, 30, 50, None, 18, 32, None) == -1                     # null pointers
        assert word in orn._lib.last_error() and 'null' in orn._lib.last_error()
        for bad in ((1, 30, 50, 0, 32), (1, 30, 50, 18, 0), (1, 0, 50, 18, 32), (-1, 30, 50, 18, 32), (1, 30, 50, 18, 40000)):
            n, H, W, h, w = bad
            assert fn(None, n, H, W, None, h, w, None) == -1, bad
            assert word in orn._lib.last_error()
        assert fn(None, 0, 30, 50, None, 18, 32, None) == 0                      # n == 0: nothing to do
    assert L.orn_version() == 120


def _write(d, n, hw, seed=5):
    from PIL import Image
    d.mkdir()
    rng = np.random.RandomState(seed)
    imgs = []
    for k in range(n):
        a = rng.randint(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8)
        Image.fromarray(a).save(str(d / f'{k:04d}.png'))
        imgs.append(a)
    return imgs


def test_frame_dir_load_pools_on_the_host(orn, tmp_path):
    """load('cpu', out_hw=(18, 32)) of 30 x 50 PNGs is F.adaptive_avg_pool2d(load('cpu')[0], (18, 32)), exactly; times, indexing
    and the portrait transpose (before the pool) are those of the plain load."""
    from orn_amd import data
    imgs = _write(tmp_path / 'land', 5, (30, 50))
    fd = data.FrameDir(str(tmp_path / 'land'), (None,), 2)
    plain, t0 = fd.load('cpu')
    assert plain.shape == (2, 3, 30, 50)
    pooled, t1 = fd.load('cpu', out_hw=(18, 32))
    assert pooled.shape == (2, 3, 18, 32) and pooled.dtype == torch.float32 and pooled.is_contiguous()
    assert torch.equal(pooled, F.adaptive_avg_pool2d(plain, (18, 32)))
    assert torch.equal(t0, t1) and t1.tolist() == torch.tensor([0.0, 2.0 / 5]).tolist()
    same, _ = data.load_png_dir(str(tmp_path / 'land'), (None,), 2, 'cpu', out_hw=(30, 50))
    assert torch.equal(same, plain)
    # the uint8 HWC form the device path uploads: the file's pixels, untouched
    a, t = fd.item_hwc(1)
    assert a.dtype == np.uint8 and a.flags['C_CONTIGUOUS'] and np.array_equal(a, imgs[2]) and t == 2.0 / 5
    # portrait: transposed first, then pooled
    pimgs = _write(tmp_path / 'port', 2, (50, 30), seed=6)
    pp, _ = data.load_png_dir(str(tmp_path / 'port'), (None,), 1, 'cpu', out_hw=(18, 32))
    want = torch.from_numpy(np.stack(pimgs)).permute(0, 3, 2, 1).float().div(255.0)          # [n, 3, W, H]: landscape
    assert want.shape == (2, 3, 30, 50)
    assert torch.equal(pp, F.adaptive_avg_pool2d(want, (18, 32)))
    ph, _ = data.FrameDir(str(tmp_path / 'port')).item_hwc(0)
    assert ph.shape == (30, 50, 3) and np.array_equal(ph, pimgs[0].transpose(1, 0, 2))


def test_ingest_frames_refuses_host_tensors(orn):
    from orn_amd import ops
    with pytest.raises(orn._lib.OrnError):
        ops.ingest_frames(torch.zeros(1, 30, 50, 3, dtype=torch.uint8), (18, 32))
