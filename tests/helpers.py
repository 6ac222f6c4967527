"""Shared test helpers: seeded input generators that mirror tools/make_golden.py."""
import math

import torch

ERB_KEYS = (
    'rbr_3x3_branch.weight', 'rbr_3x3_branch.bias', 'rbr_3x1_branch.weight', 'rbr_3x1_branch.bias',
    'rbr_1x3_branch.weight', 'rbr_1x3_branch.bias', 'rbr_1x1_3x3_1x1_branch_1x1_1.weight',
    'rbr_1x1_3x3_1x1_branch_3x3.weight', 'rbr_1x1_3x3_1x1_branch_1x1_2.weight')


def _rand(gen, *shape, scale=1.0):
    return (torch.rand(*shape, generator=gen) * 2 - 1) * scale


def erb_inputs(C, O, seed):
    """Same seeded branch weights as tools/make_golden.py::erb_inputs."""
    g = torch.Generator().manual_seed(seed)
    return {
        'rbr_3x3_branch.weight': _rand(g, O, C, 3, 3, scale=1 / math.sqrt(9 * C)),
        'rbr_3x3_branch.bias': _rand(g, O, scale=1 / math.sqrt(9 * C)),
        'rbr_3x1_branch.weight': _rand(g, O, C, 3, 1, scale=1 / math.sqrt(3 * C)),
        'rbr_3x1_branch.bias': _rand(g, O, scale=1 / math.sqrt(3 * C)),
        'rbr_1x3_branch.weight': _rand(g, O, C, 1, 3, scale=1 / math.sqrt(3 * C)),
        'rbr_1x3_branch.bias': _rand(g, O, scale=1 / math.sqrt(3 * C)),
        'rbr_1x1_3x3_1x1_branch_1x1_1.weight': _rand(g, 2 * C, C, 1, 1, scale=1 / math.sqrt(C)),
        'rbr_1x1_3x3_1x1_branch_3x3.weight': _rand(g, O, 2 * C, 3, 3, scale=1 / math.sqrt(18 * C)),
        'rbr_1x1_3x3_1x1_branch_1x1_2.weight': _rand(g, O, O, 1, 1, scale=1 / math.sqrt(O)),
    }


GEOS = {
    # two blocks with 96 input channels: both on the 16-bit path, no fp32 block below them
    'c96x2': dict(fc='3_4_96', strides=[2, 2], lower_width=96),
    # the bench geometry in small: an fp32 first block (26 channels), a narrow block, two 96-channel blocks
    'narrow_first': dict(fc='2_3_26', strides=[5, 2, 2, 2], lower_width=96),
    # a stride-3 block in the middle (config 3's shape)
    'stride3': dict(fc='2_3_26', strides=[5, 3, 2], lower_width=96),
}


def small_engine(orn, prec, branch, geo, n_frames=5, seed=1):
    """A small engine of one of GEOS with its synthetic video set."""
    from oracle import cpu_ref
    g = GEOS[geo]
    torch.manual_seed(seed)
    gen = orn.model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=g['fc'], expansion=1, num_blocks=1, norm='none',
                              act='swish', bias=True, reduction=2, conv_type='conv', stride_list=g['strides'], sin_res=True,
                              lower_width=g['lower_width'], sigmoid=False, deploy=False, branch_type=branch)
    eng = orn.engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5, precision=prec)
    hw = eng.out_hw
    frames = cpu_ref.synthetic_video(n_frames, hw[0], hw[1], seed=5)
    embeds = cpu_ref.positional_encoding(torch.tensor([k / n_frames for k in range(n_frames)]), 1.25, 40)
    eng.set_video(frames, embeds)
    return eng


def pipelined_vs_oracle(eng, sd, frames, embeds, entries, calls, fc, strides, branch):
    """Run the schedule `entries` [(frame, step, lr)] on `eng` as pipelined calls (TrainEngine.run's default form) of `calls` steps
    each, and the same steps on the CPU oracle (cpu_ref.train_step in a loop, updating a copy of `sd` -- the engine's starting state
    dict -- and its Adam moments in place).  Checks the stats columns that must be exact (lr, frame, step) and returns the measured
    differences: worst relative loss error and PSNR error over the steps; worst per-tensor relative L2 of the last step's gradients
    and of both Adam moments at the end; how far the engine's parameters moved (max |p - p0| in units of the largest lr), the share
    of elements that end more than lr/2 from the oracle's, and the share of the oracle's elements that moved by more than lr/2."""
    import numpy as np
    from oracle import cpu_ref
    eng.set_schedule(entries)
    for n in calls:
        eng.run(n)
    torch.cuda.synchronize()
    st = eng.stats(len(entries)).numpy()
    p0 = {k: v.clone() for k, v in sd.items()}
    sd = {k: v.clone() for k, v in sd.items()}
    am = {k: torch.zeros_like(v) for k, v in sd.items()}
    av = {k: torch.zeros_like(v) for k, v in sd.items()}
    out = {'loss_rel': 0.0, 'psnr': 0.0}
    for i, (f, step, lr) in enumerate(entries):
        loss, psnr, grads = cpu_ref.train_step(sd, am, av, step, lr, embeds[f:f + 1], frames[f:f + 1], fc, strides, branch,
                                               'Fusion6', 0.5)
        assert st[i, 5] == np.float32(lr) and st[i, 6] == f and st[i, 7] == step, (i, st[i], (f, step, lr))
        out['loss_rel'] = max(out['loss_rel'], abs(float(st[i, 0]) - loss.item()) / abs(loss.item()))
        out['psnr'] = max(out['psnr'], abs(float(st[i, 4]) - psnr.item()))
    P, G, M, V = (t.cpu() for t in (eng.params, eng.grads, eng.adam_m, eng.adam_v))

    def worst(arena, ref):
        rel = [(float((arena[off:off + n] - ref[k].flatten()).norm() / (ref[k].norm() + 1e-30)), k)
               for k, (off, n) in eng.layout.items()]
        return max(rel)
    assert set(grads) == set(eng.layout)
    (out['grad_rel'], out['grad_key']), (out['m_rel'], out['m_key']) = worst(G, grads), worst(M, am)
    out['v_rel'], out['v_key'] = worst(V, av)
    lr = max(e[2] for e in entries)
    move = off = moved = total = 0
    for k, (o, n) in eng.layout.items():
        p = P[o:o + n]
        move = max(move, float((p - p0[k].flatten()).abs().max()) / lr)
        off += int(((p - sd[k].flatten()).abs() > lr / 2).sum())
        moved += int(((sd[k] - p0[k]).abs() > lr / 2).sum())
        total += n
    out.update(move_lr=move, off_share=off / total, oracle_moved_share=moved / total)
    out['finite'] = bool(torch.isfinite(P).all())
    return out
