"""tests/golden/multires.npz (tools/make_golden_multires.py): the reference's multi-resolution generator (sin_res=False) on the tiny
geometry 2_3_8, strides [2, 2], lower_width 8, stem 32_1, seed 1, under loss = lw * loss_fn(out_0, t_0) + loss_fn(out_1, t_1)."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'multires.npz')
KINDS = ('NeRV_vanilla', 'ERB')
FC, STRIDES = '2_3_8', [2, 2]


def load():
    return np.load(PATH, allow_pickle=False)


def tiny_generator(kind, sin_res=False, strides=None, fc=FC, lower_width=8, sigmoid=False):
    """The mirror of the fixture's generator, seeded as the reference was."""
    import torch
    from orn_amd import model
    torch.manual_seed(1)
    return model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=fc, expansion=1, num_blocks=1, norm='none',
                           act='swish', bias=True, reduction=2, conv_type='conv', stride_list=list(strides or STRIDES),
                           sin_res=sin_res, lower_width=lower_width, sigmoid=sigmoid, deploy=False, branch_type=kind)
