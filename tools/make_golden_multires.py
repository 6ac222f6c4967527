#!/usr/bin/env python3
"""Generate tests/golden/multires.npz: the reference's multi-resolution generator (model.py:597-625 with sin_res=False: a head on
every stage, forward returns one image per stage) under the objective of main_train.py:239-250,

    target_i = adaptive_avg_pool2d(data, out_i.shape[-2:])
    loss     = sum_{i < n-1} lw * loss_fn(out_i, target_i) + loss_fn(out_{n-1}, target_{n-1}),      lw = 0.7

on a tiny generator (fc_hw_dim 2_3_8, strides [2, 2], lower_width 8, stem 32_1, seed 1; stages 4x6 and 8x12), NeRV_vanilla and
ERB.  pytorch_msssim is not needed: loss_fn is taken as L2 (mse_loss) and as L1 (mean |.|), through plain torch.

Per branch type: state-dict keys, shapes and the full seeded state dict, embed, data, every stage's image and pooled target, and
per objective the loss sum and every parameter gradient.

Like tools/make_golden.py this imports the reference at run time, runs only where the reference is present, and writes data only."""
import os
import sys

os.environ['MKL_CBWR'] = 'COMPATIBLE'           # as tools/make_golden.py: the one MKL branch that is the same on every x86 host

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

LW = 0.7
KINDS = ('NeRV_vanilla', 'ERB')
OBJECTIVES = {'L2': lambda o, t: F.mse_loss(o, t), 'L1': lambda o, t: torch.mean(torch.abs(o - t))}


def make_generator(ref_model, bt):
    return ref_model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim='2_3_8', expansion=1, num_blocks=1, norm='none',
                               act='swish', bias=True, reduction=2, conv_type='conv', stride_list=[2, 2], sin_res=False,
                               lower_width=8, sigmoid=False, deploy=False, branch_type=bt)


def main():
    ref_model, ref_utils = make_golden._import_reference()
    _np = make_golden._np
    pe = ref_utils.PositionalEncoding('1.25_40')
    out = {'lw': np.array([LW], dtype=np.float64)}
    for bt in KINDS:
        torch.manual_seed(1)
        gen = make_generator(ref_model, bt)
        sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        embed = pe(torch.tensor([3.0 / 7.0], dtype=torch.float32))
        data = torch.rand(1, 3, 8, 12, generator=torch.Generator().manual_seed(77))
        tag = f'tiny_{bt}'
        out[f'{tag}/embed'] = _np(embed)
        out[f'{tag}/data'] = _np(data)
        out[f'{tag}/keys'] = np.array(list(sd.keys()))
        out[f'{tag}/shapes'] = np.array([','.join(str(n) for n in v.shape) for v in sd.values()])
        for k, v in sd.items():
            out[f'{tag}/sd/{k}'] = _np(v)
        for name, fn in OBJECTIVES.items():
            gen.zero_grad(set_to_none=True)
            out_list = gen(embed)
            targets = [F.adaptive_avg_pool2d(data, o.shape[-2:]) for o in out_list]
            # main_train.py:243
            losses = [fn(o, t) for o, t in zip(out_list, targets)]
            loss = sum(LW * l_ for l_ in losses[:-1]) + losses[-1]
            loss.backward()
            for i, (o, t) in enumerate(zip(out_list, targets)):
                out[f'{tag}/img{i}'] = _np(o)
                out[f'{tag}/target{i}'] = _np(t)
                out[f'{tag}/{name}/loss{i}'] = _np(losses[i])
            out[f'{tag}/n_stages'] = np.array([len(out_list)])
            out[f'{tag}/{name}/loss'] = _np(loss)
            for k, p in gen.named_parameters():
                out[f'{tag}/{name}/grad/{k}'] = _np(p.grad)
    path = os.path.join(make_golden.OUT, 'multires.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
