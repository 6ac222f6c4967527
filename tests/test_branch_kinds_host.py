"""Host side of the ACB / RepVGG / ECB blocks (include/orn.h, N7): the model mirror against the reference fixture, the engine
descriptor, the C ABI's declarations and the checkpoint kinds.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import branch_fixture as bf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    return orn_amd


@pytest.mark.parametrize('kind', bf.KINDS)
def test_mirror_matches_reference_layout_and_init(orn, kind):
    """State-dict keys, shapes and the seeded initialisation (RNG order included) are the reference's."""
    g = bf.load()
    gen = bf.tiny_generator(orn, kind)
    sd = gen.state_dict()
    assert list(sd.keys()) == list(g[f'tiny_{kind}/keys'])
    for k, v in sd.items():
        r = g[f'tiny_{kind}/sd/{k}']
        assert tuple(v.shape) == r.shape, k
        assert np.array_equal(v.numpy(), r), k
    masks = [k for k, p in gen.named_parameters() if not p.requires_grad]
    assert masks == [k for k in sd if k.endswith('.mask')] and (len(masks) == 6) == (kind == 'ECB')
    # a gradient in the fixture for every trainable tensor, none for the masks
    assert {k for k, p in gen.named_parameters() if p.requires_grad} == {k[len(f'tiny_{kind}/grad/'):] for k in g if k.startswith(f'tiny_{kind}/grad/')}


def test_fixture_is_small_and_data_only():
    assert os.path.getsize(bf.PATH) < 300 * 1024
    z = np.load(bf.PATH, allow_pickle=False)            # no pickled objects: arrays only
    assert {'names', 'start', 'shapes', 'f32'} <= set(z.files)


@pytest.mark.parametrize('kind', bf.KINDS)
def test_build_desc_offsets(orn, kind):
    from orn_amd import _lib, engine
    gen = bf.tiny_generator(orn, kind)
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    d = engine.build_desc(gen, layout, total, 'Fusion6', 0.5)
    assert (d.n_layers, d.erb, d.branch_kind) == (2, 0, _lib.BRANCH_KINDS[kind])
    assert {'ACB': 2, 'RepVGG': 3, 'ECB': 4}[kind] == d.branch_kind
    for i in range(2):
        L, X = d.layer[i], d.branch[i]

        def off(name):
            return layout[f'layers.{i}.{name}'][0]
        assert (L.w3x3, L.b3x3) == (off('rbr_3x3_branch.weight'), off('rbr_3x3_branch.bias'))
        if kind == 'ACB':
            assert (L.w3x1, L.b3x1, L.w1x3, L.b1x3) == (off('rbr_3x1_branch.weight'), off('rbr_3x1_branch.bias'),
                                                        off('rbr_1x3_branch.weight'), off('rbr_1x3_branch.bias'))
            assert (L.w1, L.w2, L.w3, X.w1x1, X.sb[0].k0) == (-1, -1, -1, -1, -1)
        elif kind == 'RepVGG':
            assert (X.w1x1, X.b1x1) == (off('rbr_1x1_branch.weight'), off('rbr_1x1_branch.bias'))
            assert (L.w3x1, L.w1, X.sb[2].mask) == (-1, -1, -1)
        else:
            assert (L.w1, L.w2, L.w3) == (off('rbr_1x1_3x3_branch_1x1.weight'), off('rbr_1x1_3x3_branch_3x3.weight'), -1)
            assert (L.w3x1, X.w1x1) == (-1, -1)
            for t, seq in enumerate(('sbx', 'sby', 'lpl')):
                got = tuple(getattr(X.sb[t], f) for f in ('k0', 'b0', 'scale', 'bias', 'mask'))
                assert got == tuple(off(f'rbr_conv1x1_{seq}_branch.{f}') for f in ('k0', 'b0', 'scale', 'bias', 'mask'))
    assert _lib.lib().orn_engine_ws_bytes(d) > 0, _lib.last_error()
    # a missing tensor of the kind is refused with text, as ERB's are
    if kind == 'RepVGG':
        d.branch[1].w1x1 = -1
    elif kind == 'ECB':
        d.branch[1].sb[2].mask = -1
    else:
        d.layer[1].w1x3 = -1
    assert _lib.lib().orn_engine_ws_bytes(d) == 0 and f'missing {kind}' in _lib.last_error()


@pytest.mark.parametrize('kind', bf.KINDS)
def test_engine_accepts_720p_descriptor(orn, kind):
    from orn_amd import _lib, engine, model
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num='512_1', fc_hw_dim='9_16_26', expansion=1, num_blocks=1, norm='none',
                          act='swish', bias=True, reduction=2, conv_type='conv', stride_list=[5, 2, 2, 2, 2], sin_res=True,
                          lower_width=96, sigmoid=False, deploy=False, branch_type=kind)
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    van = None
    for prec in (0, 2):
        d = engine.build_desc(gen, layout, total, 'Fusion6', 0.5, precision=prec)
        n = _lib.lib().orn_engine_ws_bytes(d)
        assert n > 0, _lib.last_error()
        d.branch_kind = 0                               # the same arena as a single-conv engine: the merge's buffers come on top
        van = _lib.lib().orn_engine_ws_bytes(d)
        assert 0 < van < n
    # erb and a branch kind together are refused
    d = engine.build_desc(gen, layout, total)
    d.erb = 1
    assert _lib.lib().orn_engine_ws_bytes(d) == 0 and 'branch_kind' in _lib.last_error()
    d.erb, d.branch_kind = 0, 5
    assert _lib.lib().orn_engine_ws_bytes(d) == 0 and 'branch_kind' in _lib.last_error()


def test_zero_new_fields_are_todays_engine(orn):
    """A descriptor whose appended fields are zero describes the engine it described before they existed."""
    from orn_amd import _lib, engine
    for bt in ('ERB', 'NeRV_vanilla'):
        gen = bf.tiny_generator(orn, bt)
        layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
        d = engine.build_desc(gen, layout, total)
        assert d.branch_kind == 0 and d.reserved_ == 0
        assert all(getattr(d.branch[i], f) == 0 for i in range(_lib.ORN_MAX_LAYERS) for f in ('w1x1', 'b1x1'))
        assert _lib.lib().orn_engine_ws_bytes(d) > 0
    # the appended fields lie behind layer[]: no existing field moved
    assert _lib.EngineDesc.branch_kind.offset == _lib.EngineDesc.layer.offset + _lib.ORN_MAX_LAYERS * 96
    assert _lib.EngineDesc.layer.offset == 120 and _lib.EngineDesc.branch.offset == _lib.EngineDesc.branch_kind.offset + 8


def test_symbols_declared_and_mirrored(orn):
    from orn_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'orn.h')).read()
    for name in ('orn_branch_merge_fwd', 'orn_branch_merge_bwd_ws_bytes', 'orn_branch_merge_bwd'):
        assert re.search(r'ORN_API\s+\w+\s+' + name + r'\s*\(', hdr), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    for define, value in (('ORN_BRANCH_ACB', 2), ('ORN_BRANCH_REPVGG', 3), ('ORN_BRANCH_ECB', 4)):
        assert re.search(rf'#define\s+{define}\s+{value}\b', hdr), define
    assert re.search(r'#define\s+ORN_VERSION\s+120\b', hdr) and _lib.lib().orn_version() == 120
    assert 'branch_kind' in hdr and 'orn_branch_desc branch[ORN_MAX_LAYERS];' in hdr
    L = _lib.lib()
    # argument errors come back as codes + text (no GPU needed)
    assert L.orn_branch_merge_fwd(1, None, 4, 4, None, None, None) == -1 and 'kind 1' in _lib.last_error()
    assert L.orn_branch_merge_fwd(2, None, 4, 4, None, None, None) == -1
    assert L.orn_branch_merge_bwd_ws_bytes(7, 4, 4) == 0 and L.orn_branch_merge_bwd_ws_bytes(4, 0, 4) == 0
    # ECB: the slabs of dwA, ceil(O / 32) x 2C x C floats; the other kinds need nothing
    assert L.orn_branch_merge_bwd_ws_bytes(4, 96, 864) >= 27 * 2 * 96 * 96 * 4
    assert 0 < L.orn_branch_merge_bwd_ws_bytes(2, 96, 864) <= 256 and 0 < L.orn_branch_merge_bwd_ws_bytes(3, 96, 864) <= 256


def test_state_dict_kind_of_all_five_layouts(orn):
    from orn_amd import checkpoint
    for bt in ('NeRV_vanilla', 'ERB') + bf.KINDS:
        sd = bf.tiny_generator(orn, bt).state_dict()
        assert checkpoint.state_dict_kind(sd) == bt
    assert checkpoint.state_dict_kind(bf.tiny_generator(orn, 'ECB', deploy=True).state_dict()) == 'deploy'
    g = bf.load()
    for kind in bf.KINDS:                                # the reference's own key lists
        assert checkpoint.state_dict_kind({k: None for k in g[f'tiny_{kind}/keys']}) == kind


def test_deploy_structure_of_new_kinds(orn):
    """switch_to_deploy_structure (no GPU) leaves the deploy layout for every merged kind."""
    for kind in bf.KINDS:
        gen = bf.tiny_generator(orn, kind)
        for blk in gen.layers:
            blk.switch_to_deploy_structure()
        assert [k for k in gen.state_dict() if k.startswith('layers.')] == [f'layers.{i}.rbr_reparam.{p}' for i in range(2) for p in ('weight', 'bias')]


def test_dbb_still_raises(orn):
    from orn_amd import model
    with pytest.raises(NotImplementedError):
        model.NeRVBlock(ngf=4, new_ngf=4, stride=2, bias=True, norm='none', act='swish', deploy=False, conv_type='conv', branch_type='DBB')
    with pytest.raises(NotImplementedError):
        bf.tiny_generator(orn, 'DBB')
