"""Objectives for TrainEngine.step_with / run_with and `main_train --custom_loss MODULE:FUNCTION`: functions of
(pred, target), both [B,3,H,W] fp32 on the device, that return a scalar tensor and are differentiable in pred.

The three here carry the frequency term of the reference's two FFT objectives (utils.py:173-188), which the library
builds no kernel and no loss id for: torch.fft supplies that term and its gradient on the caller's stream, the
structural part stays on the library's loss kernels (ops.LossFn), and the engine does the rest of the step.  They are
names of their own: `loss_id`, `ops.loss_stats` and `utils.loss_fn` keep refusing 'Fusion13' / 'Fusion15'.
Any other module with functions of this signature serves the same way.
"""
import torch

from . import ops

# utils.py:179,187: 60 * (0.7 * L1 + 0.3 * (1 - s)) + frequency term; 0.7 / 0.3 with s = ssim is Fusion6, with s = ms_ssim Fusion10
PIXEL_WEIGHT = 60.0


def freq_l1(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean absolute difference between the 2-D spectra of pred and target over the last two dimensions, real and
    imaginary parts taken as separate numbers: mean(|Re F(p) - Re F(t)|, |Im F(p) - Im F(t)|) over 2*B*Ch*H*W values.
    (The reference takes this mean per batch element; at its batch size of 1 that is the same number.)"""
    fp = torch.view_as_real(torch.fft.fft2(pred, dim=(-2, -1)))
    ft = torch.view_as_real(torch.fft.fft2(target.detach(), dim=(-2, -1)))
    return (fp - ft).abs().mean()


def fusion_freq_ssim(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """60 * (0.7 * L1 + 0.3 * (1 - ssim)) + freq_l1: the first FFT objective of the reference's loss_fn."""
    return PIXEL_WEIGHT * ops.LossFn.apply(pred, target, 'Fusion6') + freq_l1(pred, target)


def fusion_freq_msssim(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """60 * (0.7 * L1 + 0.3 * (1 - ms_ssim)) + freq_l1: the second one (needs min(H, W) > 160, like every MS-SSIM loss)."""
    return PIXEL_WEIGHT * ops.LossFn.apply(pred, target, 'Fusion10') + freq_l1(pred, target)
