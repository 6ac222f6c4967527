"""CPU tests of the per-stage decode's host side (include/orn.h N9: orn_engine_eval_stages; engine.Decoder(stages=True),
main_eval --decode_stage): what is declared where, the workspace size entry, the descriptor of a decode-only multi-resolution
engine, and the command line's refusals, none of which need a GPU."""
import os
import re
import sys
from ctypes import byref

import pytest

import multires_fixture as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('orn_engine_eval_stages_ws_bytes', 'orn_engine_eval_stages')
HOOKS = tuple(f'orn_debug_stage_out_{k}{a}' for k in ('bf16', 'f16') for a in ('', '_act'))


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    return orn_amd


def _desc(orn, gen, multi_res, precision=2):
    from orn_amd import engine
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    return engine.build_desc(gen, layout, total, 'L2', precision=precision, multi_res=multi_res)


def test_the_entries_and_hooks_are_declared_everywhere(orn):
    with open(os.path.join(ROOT, 'include', 'orn.h')) as f:
        h = f.read()
    with open(os.path.join(ROOT, 'include', 'orn_debug.h')) as f:
        dbg = f.read()
    L = orn._lib.lib()
    for name in ENTRIES:
        assert re.search(r'ORN_API \w+ ' + name + r'\(', h), name
        assert name in orn._lib.EXPORTS and name in orn._lib._SIGS
        assert hasattr(L, name)
    assert 'typedef struct orn_stage_out' in h and '#define ORN_VERSION 120' in h
    for name in HOOKS:
        assert re.search(r'ORN_API int ' + name + r'\(', dbg), name
        assert name in orn._lib._DEBUG_SIGS and hasattr(L, name)
    assert [f for f, _ in orn._lib.StageOut._fields_] == ['targets', 'rgb8', 'img', 'stats', 'msssim']
    assert [f for f, _ in orn._lib.EngineDesc._fields_][-2:] == ['act', 'reserved2_']


def test_workspace_size_entry(orn):
    """0 on bad arguments; otherwise it grows with the chunk and with the mask of stages that want an MS-SSIM column."""
    L = orn._lib.lib()
    gen = mf.tiny_generator('ERB', strides=[5, 2, 2, 2], fc='11_12_26', lower_width=96)     # 55x60, 110x120, 220x240, 440x480
    d = _desc(orn, gen, True)
    size = lambda mask, chunk: int(L.orn_engine_eval_stages_ws_bytes(byref(d), mask, chunk))
    assert L.orn_engine_eval_stages_ws_bytes(None, 0, 1) == 0
    assert size(0b1000, 0) == 0 and size(0b1000, -1) == 0
    assert size(0b0001, 1) == 0 and size(0b0010, 1) == 0          # 55x60 and 110x120: no MS-SSIM below 161
    assert size(0b10000, 1) == 0                                   # no such stage
    none, top, both = size(0, 1), size(0b1000, 1), size(0b1100, 1)
    assert 0 < none < top < both
    assert size(0b0100, 1) < both
    assert size(0b1000, 3) > top and size(0b1100, 3) > both
    # the one MS-SSIM workspace is shared: two stages cost less than the two alone
    assert both < top + size(0b0100, 1)
    single = _desc(orn, mf.tiny_generator('ERB', sin_res=True, strides=[5, 2, 2, 2], fc='11_12_26', lower_width=96), None)
    assert int(L.orn_engine_eval_stages_ws_bytes(byref(single), 0b1000, 2)) > 0          # sizes depend on the geometry alone
    assert L.orn_engine_eval_stages(None, None, None, 1, None, None, 0, None) == -1
    assert 'engine_eval_stages' in orn._lib.last_error()


def test_engine_workspace_sizes_are_unchanged(orn):
    """orn_engine_ws_bytes of every descriptor of the workspace fixture: all new memory is the caller's."""
    from orn_amd import _build  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import make_golden_engine_ws
    finally:
        sys.path.pop(0)
    diff = make_golden_engine_ws.check()
    assert not diff, '\n'.join(diff)


def test_descriptor_of_a_decode_only_multi_resolution_engine(orn):
    from orn_amd import engine
    L = orn._lib.lib()
    gen = mf.tiny_generator('ERB')                                  # 2_3_8, strides 2 2: stages 4x6, 8x12
    assert engine.is_multi_res(gen)
    d1, d0 = _desc(orn, gen, True), _desc(orn, gen, False)
    assert d1.multi_res == 1 and d0.multi_res == 0 and d1.n_layers == 2
    layout, _ = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    assert d1.side_head_w[0] == layout['head_layers.0.weight'][0] and d1.side_head_b[0] == layout['head_layers.0.bias'][0]
    assert d1.head_w == d0.head_w == layout['head_layers.1.weight'][0]
    w1, w0 = int(L.orn_engine_ws_bytes(byref(d1))), int(L.orn_engine_ws_bytes(byref(d0)))
    assert w1 > w0 > 0                                              # the side stages' images live behind the single-resolution carve
    import inspect
    sig = inspect.signature(engine.Decoder.__init__)
    assert sig.parameters['stages'].default is False
    assert 'decode_stages' in dir(engine.Decoder) and 'decode_stages' in dir(engine.TrainEngine)


def test_decode_stage_parses(orn):
    from orn_amd import main_eval
    p = main_eval.eval_parser()
    assert p.parse_args([]).decode_stage is None
    assert p.parse_args(['--decode_stage', 'all']).decode_stage == 'all'
    assert p.parse_args(['--decode_stage', '1']).decode_stage == '1'
    args = p.parse_args(['--decoder', 'engine', '--decode_stage', '2', '--strides', '5', '2', '2'])
    assert main_eval.check_decode_stage(args) == 2
    assert main_eval.check_decode_stage(p.parse_args(['--decoder', 'engine', '--decode_stage', 'all'])) == 'all'
    assert main_eval.check_decode_stage(p.parse_args(['--decoder', 'engine'])) is None
    for bad in ('3', '-1', 'top'):
        with pytest.raises(ValueError, match='decode_stage'):
            main_eval.check_decode_stage(p.parse_args(['--decoder', 'engine', '--decode_stage', bad, '--strides', '5', '2', '2']))


@pytest.mark.parametrize('extra,text', [(['--decoder', 'engine', '--single_res'], 'single_res'), (['--decoder', 'eager'], 'decoder engine'),
                                        ([], 'decoder engine')])
def test_decode_stage_is_refused_before_any_file_is_opened(orn, extra, text, tmp_path, monkeypatch):
    """--single_res and --decoder eager: ValueError from the arguments alone -- in an empty directory, where loading anything would
    be a FileNotFoundError instead."""
    from orn_amd import main_eval
    monkeypatch.chdir(tmp_path)
    argv = ['--outf', 'nothing_here', '--synthetic', '4', '--decode_stage', 'all'] + extra
    with pytest.raises(ValueError, match=text):
        main_eval.main(argv)
    assert not os.path.exists(tmp_path / 'result')
    with pytest.raises(FileNotFoundError):                          # a valid combination goes on to the checkpoint
        main_eval.main(['--outf', 'nothing_here', '--synthetic', '4', '--decode_stage', 'all', '--decoder', 'engine'])
