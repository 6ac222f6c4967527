"""Operands, float64 reference and the per-element check of the 16-bit weight gradient, shared by test_gpu_conv16_forms.py (the
per-op pair k_wgrad_nhwc_bf16 + k_wgrad_bf16_reduce) and test_gpu_wgrad16_batch.py (the engine's two batched launches): both run the
same work-group bodies, so they are held to the same reference and the same bound.

Reference: float64 on the CPU from the identical 16-bit-rounded operands; it does not use liborn.  Per element, never as a norm,
    |k - r| <= c * A,      A = the same sum on the absolute values of the operands (float64).
"""
import torch

FAST_C = 96                    # channels per pixel of every 16-bit channels-last buffer (ORN_FAST_C)
DT = {'bf16': torch.bfloat16, 'fp16': torch.float16}
SAMPLE_ABOVE = 50_000_000      # H * W * O above which wgrad_channels samples the output channels


def rand(shape, gen, chan_scale):
    """Seeded, not symmetric (a positive mean), a different scale per channel (last dim)."""
    return (torch.randn(shape, generator=gen, device='cuda') + 0.25) * chan_scale


def scales(n, gen, lo=-1.5, hi=1.5):
    return torch.exp2(torch.rand(n, generator=gen, device='cuda') * (hi - lo) + lo)


def oprime(O, s):
    """o' of every PyTorch output channel o: o' = (o % s^2) * Cn + o / s^2 (orn.h: o' = (i*s+j)*Cn + n, o = n*s^2 + i*s + j)."""
    o = torch.arange(O, device='cuda')
    return (o % (s * s)) * (O // (s * s)) + o // (s * s)


def padded(H, W, Cp, c_real, half, gen, slack=0, scale=None):
    """[H+2][W+2][Cp] zero-bordered, random in channels < c_real, zero above; `slack` NaN elements behind it."""
    n = (H + 2) * (W + 2) * Cp
    buf = torch.full((n + slack,), float('nan'), dtype=DT[half], device='cuda')
    x = buf[:n].view(H + 2, W + 2, Cp)
    x.zero_()
    sc = scale if scale is not None else scales(c_real, gen)
    x[1:H + 1, 1:W + 1, :c_real] = rand((H, W, c_real), gen, sc).to(DT[half])
    return buf, x


def wgrad_channels(H, W, O, s, seed):
    """PyTorch output channels to compare: all of them below ~50 M pixel-channel products, else the first 16 and last 16 o' (the
    ragged last 128-channel tile) and a seeded sample of 32 more (all C and taps of each)."""
    if H * W * O <= SAMPLE_ABOVE:
        return torch.arange(O)
    g = torch.Generator().manual_seed(seed)
    opsel = torch.cat([torch.arange(16), torch.arange(O - 16, O), torch.randperm(O - 32, generator=g)[:32] + 16])
    inv = torch.empty(O, dtype=torch.long)
    inv[oprime(O, s).cpu()] = torch.arange(O)
    return inv[opsel].sort().values


def wgrad_ref(xpad, dypad, H, W, C, O, s, sel):
    """float64 accumulation of dW and dbias from the padded 16-bit buffers (device tensors xpad [H+2][W+2][96], dypad [H+2][W+2][O] in
    o' order): r, A [len(sel)][C][9] for the PyTorch output channels sel, and rb, Ab [O] in PyTorch channel order."""
    op = oprime(O, s).cpu()
    ops = op[sel]
    r = torch.zeros(len(sel), C, 9, dtype=torch.float64)
    A = torch.zeros_like(r)
    rb = torch.zeros(O, dtype=torch.float64)
    Ab = torch.zeros_like(rb)
    step = max(1, 2_000_000 // (W * max(C, 96)))
    for h0 in range(0, H, step):
        h1 = min(H, h0 + step)
        dyf = dypad[1 + h0:1 + h1, 1:W + 1].double().cpu().reshape(-1, O)
        rb += dyf.sum(0)
        Ab += dyf.abs().sum(0)
        dy = dyf[:, ops]
        xs = xpad[h0:h1 + 2, :, :C].double().cpu()
        for tap in range(9):
            i, j = divmod(tap, 3)
            xt = xs[i:i + h1 - h0, j:j + W].reshape(-1, C)
            r[:, :, tap] += dy.T @ xt
            A[:, :, tap] += dy.abs().T @ xt.abs()
    return r, A, rb[op], Ab[op]


def check32(k, r, A, c, what, record=None):
    """fp32 output k against r: every element finite and |k - r| <= c * A.  record(ratio) sees the worst ratio |k - r| / A before
    the bound is asserted; it is returned too."""
    k = k.double()
    assert bool(torch.isfinite(k).all()), f'{what}: {int((~torch.isfinite(k)).sum())} non-finite outputs'
    d = (k - r).abs()
    ratio = float((d / A.clamp_min(1e-300)).max())
    if record is not None:
        record(ratio)
    bad = d > c * A
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements out of bound (worst ratio {ratio:.3e}, c {c:.3e}); '
                             f'first at flat index {i} (shape {tuple(bad.shape)}): kernel {float(k.flatten()[i])!r} reference '
                             f'{float(r.flatten()[i])!r}')
    return ratio
