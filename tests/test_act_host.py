"""--act gelu without a GPU: the mirror accepts it, the descriptor carries it behind every earlier field, the new entry points are
declared in all three places and refuse an unknown activation before they touch anything, the workspace does not depend on it, and
the default command line of main_train builds its generator."""
import ctypes
import os
import re
from ctypes import byref

import numpy as np
import pytest

import act_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWINS_ORN_H = ('orn_stem_fwd', 'orn_stem_bwd', 'orn_conv3x3_ps_silu_fwd', 'orn_conv3x3_ps_silu_bwd', 'orn_conv3x3_ps_silu_fwd_bf16',
               'orn_conv3x3_ps_silu_bwd_bf16', 'orn_conv3x3_ps_silu_fwd_f16', 'orn_conv3x3_ps_silu_bwd_f16')
TWINS_DEBUG = tuple(f'orn_debug_{n}' for n in (
    'conv_fwd_bf16', 'conv_fwd_f16', 'conv_dgrad_bf16', 'conv_dgrad_f16', 'head_fwd_bf16', 'head_fwd_f16', 'head_bwd_bf16', 'head_bwd_f16',
    'side_head_fwd_bf16', 'side_head_fwd_f16', 'side_head_bwd_bf16', 'side_head_bwd_f16', 'stage0_fwd', 'stage0_bwd', 'stem_bwd_slabs',
    'conv_fwd_f32', 'head_fwd_z', 'conv_bwd_f32_head'))


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build, _lib, engine, model, ops  # noqa: F401
    _build.build()
    _lib.lib()
    return orn_amd


def test_the_mirror_builds_with_gelu_and_names_what_is_built(orn):
    import torch
    g = act_fixture.load()
    for kind in act_fixture.KINDS:
        for sr in (1, 0):
            gelu = act_fixture.tiny_generator(kind, bool(sr), 'gelu')
            swish = act_fixture.tiny_generator(kind, bool(sr), 'swish')
            tag = f'tiny_{kind}_sr{sr}'
            sd = gelu.state_dict()
            assert list(sd.keys()) == list(swish.state_dict().keys()) == [str(k) for k in g[f'{tag}/keys']]
            assert [','.join(str(n) for n in v.shape) for v in sd.values()] == [str(s) for s in g[f'{tag}/shapes']]
            assert sum(p.numel() for p in gelu.parameters()) == int(g[f'{tag}/n_params'][0])
            for k in sd:        # the activation draws nothing: the seeded init is the reference's
                assert np.array_equal(sd[k].numpy(), g[f'{tag}/sd/{k}']), k
            assert isinstance(gelu.stem[1], torch.nn.GELU) and isinstance(gelu.stem[3], torch.nn.GELU)
            assert gelu.stem[1].approximate == 'none'
            assert isinstance(swish.stem[1], torch.nn.SiLU)
    assert [int(g[f'{t}/n_params'][0]) for t in act_fixture.TAGS] == [25179, 25206, 10459, 10486]
    for bad in ('relu', 'leaky', 'leaky01', 'relu6', 'softplus', 'hardswish'):
        with pytest.raises(NotImplementedError) as e:
            act_fixture.tiny_generator('ERB', True, bad)
        assert "'swish'" in str(e.value) and "'gelu'" in str(e.value) and repr(bad) in str(e.value)


def test_the_descriptor_carries_act_behind_every_earlier_field(orn):
    from orn_amd import _lib, engine
    D = _lib.EngineDesc
    names = [f[0] for f in D._fields_]
    assert names[-2:] == ['act', 'reserved2_'] and names[-3] == 'side_head_b'

    class Old(ctypes.Structure):
        _fields_ = D._fields_[:-2]
    for name in names[:-2]:
        assert getattr(D, name).offset == getattr(Old, name).offset, name
    assert D.act.offset == D.side_head_b.offset + 8 * _lib.ORN_MAX_LAYERS == ctypes.sizeof(Old)
    assert D.reserved2_.offset == D.act.offset + 4 and ctypes.sizeof(D) == ctypes.sizeof(Old) + 8
    assert (_lib.ACT_SWISH, _lib.ACT_GELU) == (0, 1) and orn.ops.ACTS == ('swish', 'gelu')
    for act, want in (('swish', 0), ('gelu', 1)):
        gen = act_fixture.tiny_generator('ERB', True, act)
        layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
        assert engine.build_desc(gen, layout, total, 'L1').act == want


def test_every_new_symbol_is_in_the_header_the_map_and_the_exports(orn):
    from orn_amd import _lib
    L = _lib.lib()
    orn_h = open(os.path.join(ROOT, 'include', 'orn.h')).read()
    dbg_h = open(os.path.join(ROOT, 'include', 'orn_debug.h')).read()
    assert re.search(r'#define ORN_ACT_SWISH 0\b', orn_h) and re.search(r'#define ORN_ACT_GELU 1\b', orn_h)
    assert re.search(r'#define ORN_VERSION 120\b', orn_h) and L.orn_version() == 120
    mp = open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'orn.map')).read()
    assert re.search(r'global:\s*orn_\*;', mp)          # the version script exports the orn_ prefix: every name below matches it
    for name in TWINS_ORN_H:
        twin = name + '_act'
        assert re.search(r'\b%s\s*\(' % twin, orn_h), twin
        assert twin in _lib.EXPORTS and hasattr(L, twin), twin
        assert _lib._SIGS[twin][1] == _lib._SIGS[name][1] + [ctypes.c_int], twin
    for name in TWINS_DEBUG + ('orn_debug_act_eval',):
        twin = name if name.endswith('act_eval') else name + '_act'
        assert re.search(r'\b%s\s*\(' % twin, dbg_h), twin
        assert twin in _lib._DEBUG_SIGS and hasattr(L, twin), twin


def test_an_unknown_activation_is_refused_before_anything_is_touched(orn):
    """Every twin with act = 7 and null pointers everywhere: ORN_E_ARG and a text that names the activation.  Nothing is launched."""
    from orn_amd import _lib
    L = _lib.lib()
    sigs = {n + '_act': _lib._SIGS[n + '_act'] for n in TWINS_ORN_H}
    sigs.update({n + '_act': _lib._DEBUG_SIGS[n + '_act'] for n in TWINS_DEBUG})
    for name, (_res, args) in sigs.items():
        vals = [None if a is ctypes.c_void_p or (isinstance(a, type) and issubclass(a, ctypes._Pointer)) else a(0) for a in args[:-1]]
        assert getattr(L, name)(*vals, 7) == -1, name
        assert 'unknown activation 7' in _lib.last_error(), (name, _lib.last_error())
    assert L.orn_debug_act_eval(7, 0, None, 0, None, None, None) == -1 and 'unknown activation 7' in _lib.last_error()
    gen = act_fixture.tiny_generator('ERB', True, 'gelu')
    from orn_amd import engine
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    d = engine.build_desc(gen, layout, total, 'L1')
    d.act = 7
    assert L.orn_engine_ws_bytes(byref(d)) == 0 and 'act = 7' in _lib.last_error()


@pytest.mark.parametrize('geo', ['720p', 'tiny'])
def test_the_workspace_does_not_depend_on_the_activation(orn, geo):
    import torch
    from orn_amd import _lib, engine
    L = _lib.lib()
    for kind in ('ERB', 'NeRV_vanilla', 'ECB'):
        for sin_res in (True, False):
            with torch.device('meta'):
                if geo == '720p':
                    gen = act_fixture.tiny_generator(kind, sin_res, 'swish', fc='9_16_26', lower_width=96, strides=(5, 2, 2, 2, 2))
                else:
                    gen = act_fixture.tiny_generator(kind, sin_res, 'swish')
            layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
            for precision in (0, 1, 2):
                d = engine.build_desc(gen, layout, total, 'Fusion6' if geo == '720p' else 'L1', 0.5, 0.999, 1e-8, precision)      # (6 x 8 stages take no SSIM)
                sizes = []
                for act in (0, 1):
                    d.act = act
                    sizes.append((L.orn_engine_ws_bytes(byref(d)), L.orn_engine_batch_ws_bytes(byref(d), 4),
                                  L.orn_engine_eval_frames_ws_bytes(byref(d), 8)))
                assert sizes[0] == sizes[1] and sizes[0][0] > 0, (kind, sin_res, precision, sizes)


def test_the_default_command_line_builds_its_generator(orn):
    """main_train.parse_args([]) names no activation: --act defaults to gelu, as in the reference, and the generator of that
    command line is built (NotImplementedError before --act gelu existed)."""
    import torch
    from orn_amd import main_train, model, utils
    args = main_train.parse_args([])
    assert args.act == 'gelu'
    pe = utils.PositionalEncoding(args.embed)
    with torch.device('meta'):
        gen = model.Generator(embed_length=pe.embed_length, stem_dim_num=args.stem_dim_num, fc_hw_dim=args.fc_hw_dim,
                              expansion=args.expansion, num_blocks=args.num_blocks, norm=args.norm, act=args.act, bias=True,
                              reduction=args.reduction, conv_type=args.conv_type, stride_list=args.strides, sin_res=args.single_res,
                              lower_width=args.lower_width, sigmoid=args.sigmoid, deploy=False, branch_type=args.branch_type)
    assert gen.act == 'gelu' and all(blk.act == 'gelu' for blk in gen.layers)
