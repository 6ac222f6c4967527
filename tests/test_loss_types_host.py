"""CPU tests of the loss table (include/orn.h ORN_LOSS_*, _lib.LOSS_TYPES, orn_loss_spec) and of the loss workspace sizes: every
loss of the reference's loss_fn (utils.py:139-189) but the two FFT ones resolves to the reference's weights, ids 0..2 keep their
workspace, and the MS-SSIM kinds refuse what pytorch_msssim refuses."""
import pytest


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    orn_amd._lib.lib()
    return orn_amd


# utils.py:142-172 as data: name -> (weight of mean|p-t|, weight of mse, weight of (1 - s), s)
REFERENCE = {
    'L2': (0.0, 1.0, 0.0, None), 'L1': (1.0, 0.0, 0.0, None), 'SSIM': (0.0, 0.0, 1.0, 'ssim'),
    'Fusion1': (0.0, 0.3, 0.7, 'ssim'), 'Fusion2': (0.3, 0.0, 0.7, 'ssim'), 'Fusion3': (0.0, 0.5, 0.5, 'ssim'),
    'Fusion4': (0.5, 0.0, 0.5, 'ssim'), 'Fusion5': (0.0, 0.7, 0.3, 'ssim'), 'Fusion6': (0.7, 0.0, 0.3, 'ssim'),
    'Fusion7': (0.3, 0.7, 0.0, None), 'Fusion8': (0.5, 0.5, 0.0, None), 'Fusion9': (0.9, 0.0, 0.1, 'ssim'),
    'Fusion10': (0.7, 0.0, 0.3, 'ms_ssim'), 'Fusion11': (0.9, 0.0, 0.1, 'ms_ssim'), 'Fusion12': (0.8, 0.0, 0.2, 'ms_ssim'),
}
SHAPES = [(1, 3, 45, 80), (2, 3, 30, 37), (1, 3, 161, 177), (2, 3, 163, 201), (1, 3, 720, 1280)]


def test_loss_names_cover_the_reference_but_the_fft_losses(orn):
    lt = orn._lib.LOSS_TYPES
    assert set(lt) == set(REFERENCE)
    assert sorted(lt.values()) == list(range(len(REFERENCE)))
    assert (lt['L2'], lt['L1'], lt['Fusion6']) == (0, 1, 2)          # ids 0, 1 and 2 keep their meaning
    for name in ('Fusion13', 'Fusion15', 'Fusion14', 'l2'):
        with pytest.raises(NotImplementedError) as ei:
            orn._lib.loss_id(name)
        assert 'Fusion10' in str(ei.value) and 'Fusion6' in str(ei.value)     # the text lists what is built


def test_weights_table_equals_the_reference(orn):
    import numpy as np
    kinds = {None: orn._lib.LOSS_KIND_NONE, 'ssim': orn._lib.LOSS_KIND_SSIM, 'ms_ssim': orn._lib.LOSS_KIND_MSSSIM}
    for name, (w1, w2, ws, s) in REFERENCE.items():
        w, kind = orn._lib.loss_spec(name)
        assert w == tuple(float(np.float32(x)) for x in (w1, w2, ws)), (name, w)
        assert kind == kinds[s], (name, kind)
    L = orn._lib.lib()
    assert L.orn_loss_spec(len(REFERENCE), None, None) < 0 and L.orn_loss_spec(-1, None, None) < 0


def test_ws_bytes_for_keeps_the_old_sizes(orn):
    L = orn._lib.lib()
    for B, Ch, H, W in SHAPES:
        old = L.orn_loss_ws_bytes(B, Ch, H, W)
        assert old > 0
        for t in (0, 1, 2):
            assert L.orn_loss_ws_bytes_for(t, B, Ch, H, W) == old
        # every kind but MS-SSIM uses the same tile partials
        for name, (_, _, _, s) in REFERENCE.items():
            if s != 'ms_ssim':
                assert L.orn_loss_ws_bytes_for(orn._lib.LOSS_TYPES[name], B, Ch, H, W) == old, name


def test_ws_bytes_for_unknown_id_is_zero(orn):
    L = orn._lib.lib()
    for t in (-1, len(REFERENCE), 99):
        assert L.orn_loss_ws_bytes_for(t, 1, 3, 200, 240) == 0


def test_ws_bytes_for_msssim_kinds(orn):
    L = orn._lib.lib()
    for name in ('Fusion10', 'Fusion11', 'Fusion12'):
        t = orn._lib.LOSS_TYPES[name]
        for H, W in ((160, 200), (200, 160), (45, 80), (160, 160)):
            assert L.orn_loss_ws_bytes_for(t, 1, 3, H, W) == 0, (name, H, W)
        for B, Ch, H, W in ((1, 3, 161, 177), (2, 3, 163, 201), (1, 3, 720, 1280)):
            n = L.orn_loss_ws_bytes_for(t, B, Ch, H, W)
            # at least: the tile partials, both pyramids' levels 1..4 (orn_msssim's workspace) and the four gradient planes
            assert n >= L.orn_loss_ws_bytes(B, Ch, H, W) + L.orn_msssim_ws_bytes(B, Ch, H, W) + B * Ch * ((H + 1) // 2) * ((W + 1) // 2) * 4
            assert n % 256 == 0
