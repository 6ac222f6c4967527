"""Reader of tests/golden/branch_kinds.npz (tools/make_golden_branches.py::pack): the reference's ACB / RepVGG / ECB blocks on the
tiny generator.  The file stores every distinct fp32 array once, all of them as four byte planes; this gives back name -> array,
bit for bit."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'branch_kinds.npz')
KINDS = ('ACB', 'RepVGG', 'ECB')
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


def tiny_generator(orn, kind, deploy=False):
    """The mirror of the fixture's generator (test_tiny_generator_golden's, with another branch_type), seeded as the reference was."""
    import torch
    from orn_amd import model
    torch.manual_seed(1)
    return model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim='3_4_8', expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=[2, 2], sin_res=True,
                               lower_width=8, sigmoid=False, deploy=deploy, branch_type=kind)
