#!/usr/bin/env python3
"""Generate tests/golden/branch_kinds.npz: the reference's ACB / RepVGG / ECB blocks (model.py:345-393, 541-565) on the tiny
generator of tests/test_gpu_parity.py::test_tiny_generator_golden (3_4_8, strides [2, 2], lower_width 8, stem 32_1, seed 1).

Per kind: state-dict keys, the full seeded state dict, embed, target, the image of the reference's MULTI-BRANCH forward (separate
convolutions summed on the activations), its L1 loss and every parameter gradient.  `mask` (requires_grad=False) has no gradient
in the reference and none is stored.

Like tools/make_golden.py this imports the reference at run time, runs only where the reference is present, and writes data only."""
import os
import sys

os.environ['MKL_CBWR'] = 'COMPATIBLE'           # as tools/make_golden.py: the one MKL branch that is the same on every x86 host

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

KINDS = ('ACB', 'RepVGG', 'ECB')


def main():
    ref_model, ref_utils = make_golden._import_reference()
    _np = make_golden._np
    pe = ref_utils.PositionalEncoding('1.25_40')
    out = {}
    for bt in KINDS:
        torch.manual_seed(1)
        gen = make_golden.make_generator(ref_model, 80, '32_1', '3_4_8', [2, 2], 8, bt)
        sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        embed = pe(torch.tensor([3.0 / 7.0], dtype=torch.float32))
        target = torch.rand(1, 3, 12, 16, generator=torch.Generator().manual_seed(77))
        img = gen(embed)[0]
        loss = torch.mean(torch.abs(img - target))
        loss.backward()
        tag = f'tiny_{bt}'
        out[f'{tag}/embed'] = _np(embed)
        out[f'{tag}/target'] = _np(target)
        out[f'{tag}/img'] = _np(img)
        out[f'{tag}/loss_L1'] = _np(loss)
        out[f'{tag}/keys'] = np.array(list(sd.keys()))
        for k, v in sd.items():
            out[f'{tag}/sd/{k}'] = _np(v)
        for k, p in gen.named_parameters():
            if p.grad is not None:
                out[f'{tag}/grad/{k}'] = _np(p.grad)
    path = os.path.join(make_golden.OUT, 'branch_kinds.npz')
    np.savez_compressed(path, **pack(out))
    print(f'{path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


def pack(arrays):
    """name -> array as the file stores it (tests/branch_fixture.py reads it back, bit for bit).  Random fp32 values hardly
    deflate, and the three kinds share the seed, so the stem, the first 3x3 branch, embed and target are the same arrays three
    times over.  Lossless measures that keep the file small: every DISTINCT fp32 array is stored once, all of them in one array
    of four byte planes (`f32`, uint8 [4, N]: the sign / exponent planes deflate well, and one zip member has one header);
    `start[i]` is where `names[i]` begins in it (-1: not fp32, stored as the member `x<i>`)."""
    names, start, shapes, seen, parts, extra, n = [], [], [], {}, [], {}, 0
    for i, (name, a) in enumerate(arrays.items()):
        shapes.append(','.join(str(k) for k in np.shape(a)))            # (before ascontiguousarray, which makes a 0-d array 1-d)
        a = np.ascontiguousarray(a)
        names.append(name)
        if a.dtype != np.float32:
            extra[f'x{i}'] = a
            start.append(-1)
            continue
        key = a.tobytes()
        if key not in seen:
            seen[key] = n
            parts.append(a.reshape(-1).view(np.uint8).reshape(-1, 4).T)
            n += a.size
        start.append(seen[key])
    return dict(names=np.array(names), start=np.array(start, dtype=np.int64), shapes=np.array(shapes),
                f32=np.ascontiguousarray(np.concatenate(parts, axis=1)), **extra)


if __name__ == '__main__':
    main()
