"""Reader of tests/golden/act_gelu.npz (tools/make_golden_act.py, in the pack() layout of tools/make_golden_branches.py): the
reference's tiny generator with act='gelu', kinds ERB and NeRV_vanilla, each with one head (sr1) and with a head on every stage
(sr0).  Gives back name -> array, bit for bit."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'act_gelu.npz')
KINDS = ('ERB', 'NeRV_vanilla')
TAGS = tuple(f'tiny_{k}_sr{s}' for k in KINDS for s in (1, 0))
_cache = None


def load():
    global _cache
    if _cache is None:
        z = np.load(PATH, allow_pickle=False)
        out = {}
        f32 = np.ascontiguousarray(z['f32'].T).reshape(-1).view(np.float32)
        for i, (name, start, shape) in enumerate(zip(z['names'], z['start'], z['shapes'])):
            shape = tuple(int(n) for n in str(shape).split(',') if n)
            n = int(np.prod(shape)) if shape else 1
            out[str(name)] = z[f'x{i}'] if start < 0 else f32[start:start + n].reshape(shape)
        _cache = out
    return _cache


def tiny_generator(kind, sin_res=True, act='gelu', fc='3_4_8', lower_width=8, strides=(2, 2), seed=1):
    """The mirror of a fixture generator, seeded as the reference was (other arguments: the same recipe at another size)."""
    import torch
    from orn_amd import model
    torch.manual_seed(seed)
    return model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=fc, expansion=1, num_blocks=1, norm='none', act=act,
                           bias=True, reduction=2, conv_type='conv', stride_list=list(strides), sin_res=sin_res,
                           lower_width=lower_width, sigmoid=False, deploy=False, branch_type=kind)
