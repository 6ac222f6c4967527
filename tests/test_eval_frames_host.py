"""CPU tests of the one-call evaluation's host side (include/orn.h: orn_msssim_frames, orn_engine_eval_frames): the argument
rules that need no GPU, and `--decoder` on the shared parser."""
import pytest


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    return orn_amd


def test_build_parser_has_decoder(orn):
    from orn_amd import main_train, main_eval
    assert main_train.build_parser().parse_args([]).decoder == 'eager'
    assert main_train.build_parser().parse_args(['--decoder', 'engine']).decoder == 'engine'
    assert main_eval.eval_parser().parse_args([]).decoder == 'eager'            # still there, once
    with pytest.raises(SystemExit):
        main_train.build_parser().parse_args(['--decoder', 'torch'])


def test_msssim_frames_workspace_and_argument_errors(orn):
    L = orn._lib.lib()
    assert L.orn_msssim_frames_ws_bytes(0, 3, 200, 240) == 0
    assert L.orn_msssim_frames_ws_bytes(1, 3, 160, 240) == 0                    # min(H, W) must exceed 160
    assert L.orn_msssim_frames_ws_bytes(1, 0, 200, 240) == 0
    one, two = L.orn_msssim_frames_ws_bytes(1, 3, 200, 240), L.orn_msssim_frames_ws_bytes(2, 3, 200, 240)
    assert two > one > 0
    assert L.orn_msssim_frames(None, None, None, 1, 3, 200, 240, None, None, 0, None) == -1
    assert 'msssim_frames' in orn._lib.last_error()
    assert L.orn_msssim_frames(None, None, None, 1, 3, 160, 300, None, None, 0, None) == -1
    assert 'must exceed 160' in orn._lib.last_error()
    assert L.orn_msssim_frames(None, None, None, 0, 3, 200, 240, None, None, 0, None) == 0      # nothing to do
    assert L.orn_engine_eval_frames_ws_bytes(None, 1) == 0
    assert L.orn_engine_eval_frames(None, None, None, 1, None, None, None, None, None, None, 0, None) == -1
    assert 'engine_decode_frames' in orn._lib.last_error()                     # msssim == NULL: the plain entry, its own text


def test_single_call_msssim_is_one_group_of_planes(orn):
    L = orn._lib.lib()
    for B, Ch, H, W in [(1, 3, 200, 240), (2, 3, 161, 177)]:
        assert L.orn_msssim_ws_bytes(B, Ch, H, W) == L.orn_msssim_frames_ws_bytes(1, B * Ch, H, W) > 0
    assert L.orn_msssim(None, None, 1, 3, 200, 240, None, None, 0, None) == -1
    assert 'msssim:' in orn._lib.last_error()
