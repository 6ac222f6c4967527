#!/usr/bin/env python3
"""Generate tests/golden/act_gelu.npz: the reference's tiny generator with act='gelu' (3_4_8, strides [2, 2], lower_width 8, stem
32_1, seed 1, embed 1.25_40 at t = 3/7, target from seed 77), kinds ERB and NeRV_vanilla, each with sin_res=True (one head) and
sin_res=False (a head on every stage).

Per generator (tag tiny_<kind>_sr<0|1>): state-dict keys and shapes, the full seeded state dict, every output image img<i> and its
target target<i> (adaptive_avg_pool2d of the one target to the image's size), the objective and every parameter gradient.
Objective: the L1 loss, or for the multi-resolution generators sum_i lw * L1_i + L1_last with lw = 1 (main_train.py:243).

Like tools/make_golden_branches.py this imports the reference at run time, runs only where the reference is present, writes data
only, and stores it in that file's pack() layout (tests/act_fixture.py reads it back)."""
import os
import sys

os.environ['MKL_CBWR'] = 'COMPATIBLE'           # as tools/make_golden.py: the one MKL branch that is the same on every x86 host

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_golden_branches import pack  # noqa: E402

KINDS = ('ERB', 'NeRV_vanilla')
LW = 1.0


def make_generator(ref_model, bt, sin_res):
    return ref_model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim='3_4_8', expansion=1, num_blocks=1, norm='none',
                               act='gelu', bias=True, reduction=2, conv_type='conv', stride_list=[2, 2], sin_res=sin_res,
                               lower_width=8, sigmoid=False, deploy=False, branch_type=bt)


def main():
    ref_model, ref_utils = make_golden._import_reference()
    _np = make_golden._np
    pe = ref_utils.PositionalEncoding('1.25_40')
    out = {'lw': np.array([LW], dtype=np.float64)}
    for bt in KINDS:
        for sin_res in (True, False):
            torch.manual_seed(1)
            gen = make_generator(ref_model, bt, sin_res)
            sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
            embed = pe(torch.tensor([3.0 / 7.0], dtype=torch.float32))
            target = torch.rand(1, 3, 12, 16, generator=torch.Generator().manual_seed(77))
            tag = f'tiny_{bt}_sr{int(sin_res)}'
            out[f'{tag}/embed'] = _np(embed)
            out[f'{tag}/keys'] = np.array(list(sd.keys()))
            out[f'{tag}/shapes'] = np.array([','.join(str(n) for n in v.shape) for v in sd.values()])
            out[f'{tag}/n_params'] = np.array([sum(p.numel() for p in gen.parameters())])
            for k, v in sd.items():
                out[f'{tag}/sd/{k}'] = _np(v)
            out_list = gen(embed)
            targets = [F.adaptive_avg_pool2d(target, o.shape[-2:]) for o in out_list]
            losses = [torch.mean(torch.abs(o - t)) for o, t in zip(out_list, targets)]
            loss = sum(LW * l_ for l_ in losses[:-1]) + losses[-1]
            loss.backward()
            out[f'{tag}/n_stages'] = np.array([len(out_list)])
            for i, (o, t) in enumerate(zip(out_list, targets)):
                out[f'{tag}/img{i}'] = _np(o)
                out[f'{tag}/target{i}'] = _np(t)
                out[f'{tag}/loss{i}'] = _np(losses[i])
            out[f'{tag}/loss'] = _np(loss)
            for k, p in gen.named_parameters():
                if p.grad is not None:
                    out[f'{tag}/grad/{k}'] = _np(p.grad)
    path = os.path.join(make_golden.OUT, 'act_gelu.npz')
    np.savez_compressed(path, **pack(out))
    print(f'{path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
