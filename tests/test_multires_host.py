"""Host side of the multi-resolution generator (model.py:597-625 without sin_res), no GPU: the module mirror against the reference
fixture, the engine descriptor, and what the command lines refuse."""
import numpy as np
import pytest
import torch

import multires_fixture as mf


@pytest.mark.parametrize('kind', mf.KINDS)
def test_generator_mirrors_the_reference(kind):
    """State-dict keys, their order, shapes and the seeded values of Generator(sin_res=False): a head per stage, registered and
    drawn right behind its block."""
    g = mf.load()
    tag = f'tiny_{kind}'
    gen = mf.tiny_generator(kind)
    sd = gen.state_dict()
    assert list(sd.keys()) == list(g[f'{tag}/keys'])
    assert [','.join(str(n) for n in v.shape) for v in sd.values()] == list(g[f'{tag}/shapes'])
    heads = [k for k in sd if k.startswith('head_layers.')]
    assert heads == ['head_layers.0.weight', 'head_layers.0.bias', 'head_layers.1.weight', 'head_layers.1.bias']
    for k, v in sd.items():
        r = g[f'{tag}/sd/{k}']
        assert np.array_equal(v.numpy().reshape(-1)[:8], r.reshape(-1)[:8]), k
        assert np.array_equal(v.numpy(), r), k


def test_single_res_generator_is_unchanged():
    """sin_res=True keeps one head, on the last stage, and the seeded values it had."""
    gen = mf.tiny_generator('ERB', sin_res=True)
    assert [k for k in gen.state_dict() if k.startswith('head_layers.')] == ['head_layers.1.weight', 'head_layers.1.bias']
    assert gen.head_layers[0] is None


def test_build_desc_fills_the_side_heads():
    from orn_amd import engine
    for sin_res in (False, True):
        gen = mf.tiny_generator('NeRV_vanilla', sin_res=sin_res, strides=[2, 2, 2])
        layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
        d = engine.build_desc(gen, layout, total, 'L2', lw=0.7)
        assert d.head_w == layout['head_layers.2.weight'][0] and d.head_b == layout['head_layers.2.bias'][0]
        if sin_res:     # the appended fields are all zero: exactly the engine of before
            assert d.multi_res == 0 and d.lw == 0.0
            assert all(d.side_head_w[i] == 0 and d.side_head_b[i] == 0 for i in range(8))
        else:
            assert d.multi_res == 1 and d.lw == np.float32(0.7)
            for i in range(2):
                assert d.side_head_w[i] == layout[f'head_layers.{i}.weight'][0]
                assert d.side_head_b[i] == layout[f'head_layers.{i}.bias'][0]


def test_desc_matches_the_header():
    """_lib.EngineDesc and orn_engine_desc agree in size: the library refuses a multi-resolution descriptor with a message that
    names its first bad field, and reads lw from where Python wrote it."""
    import ctypes
    from orn_amd import _lib, engine
    gen = mf.tiny_generator('NeRV_vanilla')
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    d = engine.build_desc(gen, layout, total, 'L2', lw=0.7)
    assert _lib.lib().orn_engine_ws_bytes(ctypes.byref(d)) > 0, _lib.last_error()
    s = engine.build_desc(mf.tiny_generator('NeRV_vanilla', sin_res=True), layout, total, 'L2')
    assert 0 < _lib.lib().orn_engine_ws_bytes(ctypes.byref(s)) < _lib.lib().orn_engine_ws_bytes(ctypes.byref(d))
    d.lw = float('nan')
    assert _lib.lib().orn_engine_ws_bytes(ctypes.byref(d)) == 0 and 'lw' in _lib.last_error()
    d.lw = 0.7
    d.side_head_w[0] = -1
    assert _lib.lib().orn_engine_ws_bytes(ctypes.byref(d)) == 0 and 'stage 0' in _lib.last_error()


def test_msssim_loss_names_the_stage_it_cannot_take():
    """An MS-SSIM loss needs min(H, W) > 160 at EVERY stage of a multi-resolution engine (the reference's ms_ssim asserts)."""
    import ctypes
    from orn_amd import _lib, engine
    gen = mf.tiny_generator('NeRV_vanilla', fc='21_21_8', strides=[4, 2])       # stages 84x84, 168x168
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    d = engine.build_desc(gen, layout, total, 'Fusion10', lw=1.0)
    assert _lib.lib().orn_engine_ws_bytes(ctypes.byref(d)) == 0
    assert 'stage 0' in _lib.last_error() and '84x84' in _lib.last_error()
    d.multi_res = 0
    assert _lib.lib().orn_engine_ws_bytes(ctypes.byref(d)) > 0


def test_custom_loss_needs_single_res():
    from orn_amd import main_train
    args = main_train.parse_args(['--custom_loss', 'orn_amd.custom_losses:fusion_freq_ssim', '--synthetic', '4'])
    assert not args.single_res
    with pytest.raises(ValueError, match='single_res'):
        main_train.custom_loss_of(args)
    args = main_train.parse_args(['--custom_loss', 'orn_amd.custom_losses:fusion_freq_ssim', '--synthetic', '4', '--single_res'])
    assert callable(main_train.custom_loss_of(args))


def test_finetune_needs_single_res():
    from orn_amd import main_eval
    with pytest.raises(ValueError, match='single_res'):
        main_eval.main(['--finetune', '--synthetic', '4'])
