"""Host tests (no GPU) of the split step's surface: the --custom_loss spec parser of main_train, the binding of the two C entries,
and the shipped objectives' module."""
import re
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build, main_train, custom_losses  # noqa: F401
    _build.build()
    return orn_amd


def test_spec_parser(orn):
    mt = orn.main_train
    assert mt.parse_loss_spec('a.b:c') == ('a.b', 'c')
    assert mt.parse_loss_spec('orn_amd.custom_losses:fusion_freq_ssim') == ('orn_amd.custom_losses', 'fusion_freq_ssim')
    for bad in ('a.b', ':c', 'a.b:', '', 'a b:c', 'a:b:c'):
        with pytest.raises(ValueError):
            mt.parse_loss_spec(bad)
    fn = mt.load_custom_loss('orn_amd.custom_losses:fusion_freq_ssim')
    assert fn is orn.custom_losses.fusion_freq_ssim
    with pytest.raises(ValueError, match='no attribute'):
        mt.load_custom_loss('orn_amd.custom_losses:no_such_loss')
    with pytest.raises(ValueError, match='cannot import'):
        mt.load_custom_loss('orn_amd.no_such_module:f')
    with pytest.raises(ValueError, match='not callable'):
        mt.load_custom_loss('orn_amd.custom_losses:PIXEL_WEIGHT')


def test_cli_checks_the_flag_before_any_gpu_work(orn):
    """A bad spec and -b 2 raise ValueError from train() on a machine without a GPU: nothing of the device has been touched."""
    mt = orn.main_train
    with pytest.raises(ValueError, match='MODULE:FUNCTION'):
        mt.train(mt.parse_args(['--custom_loss', 'orn_amd.custom_losses']))
    with pytest.raises(ValueError, match='no attribute'):
        mt.train(mt.parse_args(['--custom_loss', 'orn_amd.custom_losses:nope']))
    with pytest.raises(ValueError, match='-b'):
        mt.train(mt.parse_args(['--custom_loss', 'orn_amd.custom_losses:freq_l1', '-b', '2']))
    assert mt.parse_args([]).custom_loss is None


def test_split_step_entries_are_declared_bound_and_exported(orn):
    hdr = open(os.path.join(ROOT, 'include', 'orn.h')).read()
    L = orn._lib.lib()
    for name in ('orn_engine_step_forward', 'orn_engine_step_backward'):
        assert re.search(r'ORN_API int %s\s*\(' % name, hdr)
        assert name in orn._lib.EXPORTS and hasattr(L, name)
    assert L.orn_version() == 120
    # argument errors come back as codes + text (no GPU needed)
    assert L.orn_engine_step_forward(None, None, None, None, None, 0, None, None) == -1
    assert 'step_forward' in orn._lib.last_error()
    assert L.orn_engine_step_backward(None, None, None, None, None, None, 0, None) == -1
    assert 'step_backward' in orn._lib.last_error()


def test_fft_objectives_are_new_names_not_loss_ids(orn):
    from orn_amd import _lib
    for name in ('Fusion13', 'Fusion15', 'fusion_freq_ssim', 'fusion_freq_msssim', 'freq_l1'):
        with pytest.raises(NotImplementedError):
            _lib.loss_id(name)
    for name in ('freq_l1', 'fusion_freq_ssim', 'fusion_freq_msssim'):
        assert callable(getattr(orn.custom_losses, name))


def test_freq_l1_on_cpu_matches_its_definition(orn):
    """freq_l1 is plain torch: on CPU tensors it equals the mean absolute difference of real and imaginary parts of fft2 in fp64."""
    import torch
    g = torch.Generator().manual_seed(3)
    p, t = torch.rand(2, 3, 10, 14, generator=g, dtype=torch.float64), torch.rand(2, 3, 10, 14, generator=g, dtype=torch.float64)
    d = torch.fft.fft2(p) - torch.fft.fft2(t)
    want = (d.real.abs().sum() + d.imag.abs().sum()) / (2 * d.numel())
    got = orn.custom_losses.freq_l1(p, t)
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
