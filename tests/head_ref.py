"""What the elementwise head tests share (test_gpu_side_head.py: the side heads; test_gpu_head16.py: the last stage's 16-bit head):
NaN guard bands around device outputs, SiLU and its derivative in the dtype of the argument, and the index map of the padded
un-shuffled gradient buffer."""
import numpy as np
import torch

BAND = 64           # guard elements on each side of every output


def banded(shape, dtype, fill=None):
    """(whole buffer, view of `shape` inside it): NaN guard bands of BAND elements around the view, which starts 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BAND,), float('nan'), dtype=dtype, device='cuda')
    view = buf[BAND:BAND + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def bands_intact(buf):
    return bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all())


def silu64(z):
    return z / (1 + torch.exp(-z))


def dsilu64(z):
    s = 1 / (1 + torch.exp(-z))
    return s * (1 + z * (1 - s))


def interior(t, C, H, W, s):
    """The padded un-shuffled buffer [H/s + 2, W/s + 2, C s^2] as [C,H,W] values of its interior (a copy)."""
    v = t[1:-1, 1:-1].reshape(H // s, W // s, s, s, C)              # [ph, pw, i, j, c]
    return v.permute(4, 0, 2, 1, 3).reshape(C, H, W)


def interior_pc(t, C, H, W, s):
    """The same interior pixel-major, [H W, C]: the layout of the channels-last pre-activation (a copy)."""
    v = t[1:-1, 1:-1].reshape(H // s, W // s, s, s, C)              # [ph, pw, i, j, c]
    return v.permute(0, 2, 1, 3, 4).reshape(H * W, C)


def bits(t):
    """The tensor's bit patterns, for an exact comparison that also tells -0 from 0 and NaN from NaN."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
