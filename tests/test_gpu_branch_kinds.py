"""ACB / RepVGG / ECB blocks trained through the online merge (include/orn.h, N7), on the GPU:
  1. the merge op alone, forward and backward, against the tensor expression (exactly, where it is adds and copies) or its fp64
     form (ECB's products);
  2. the tiny generator of each kind against the reference's multi-branch forward and gradients (tests/golden/branch_kinds.npz);
  3. the engine of each kind against a NeRV_vanilla engine that is handed the merged kernel: bit for bit;
  4. three optimiser steps against torch autograd in fp64 on the multi-branch forward plus Adam;
  5. the CLIs.

Tolerance of the ECB products (1): max|k - r64| <= c * max(max|r32 - r64|, 2^-24 * max|r64|), r64 the formula in fp64, r32 the same
torch expression in fp32 on the CPU, c the next power of two above twice the worst ratio measured on an MI355X over the seven shapes
(at most 8).  The measured worst ratios are ECB_RATIO below (none above 4); the tests print each case's."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import branch_fixture as bf
import helpers

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 4), (5, 9), (8, 32), (26, 650), (96, 384), (96, 864)]
# worst max|k - r64| / max(max|r32 - r64|, 2^-24 max|r64|) over SHAPES on an MI355X -> c = next power of two above twice that
ECB_RATIO = {'wf': 1.130, 'dwA': 2.072, 'dwB': 1.105, 'dk0': 1.221, 'dscale': 1.794}
ECB_C = {'wf': 4, 'dwA': 8, 'dwB': 4, 'dk0': 4, 'dscale': 4}
GUARD = 64


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    return orn_amd


def cu(a):
    return torch.from_numpy(np.asarray(a)).cuda() if not isinstance(a, torch.Tensor) else a.cuda()


def bits_equal(a, b):
    """torch.equal on the bit patterns (NaN == NaN, -0 != 0): what 'bit for bit' means for gradients that may have overflowed."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the op alone ---------------------------------------------------------------------------------------------------------
_MASKS = {'sbx': [[1, 0, -1], [2, 0, -2], [1, 0, -1]], 'sby': [[1, 2, 1], [0, 0, 0], [-1, -2, -1]], 'lpl': [[0, 1, 0], [1, -4, 1], [0, 1, 0]]}
_INPUTS = {}


def branch_inputs(ops, kind, C, O):
    """Seeded CPU fp32 tensors of a block in ops.BRANCH_TENSORS order, plus g and dbf; made once per (kind, shape) and left unchanged."""
    key = (kind, C, O)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 * C + O)
        ts = []
        for name, shape in zip(ops.BRANCH_TENSORS[kind], ops.branch_shapes(kind, C, O)):
            leaf = name.split('.')[-1]
            if leaf == 'mask':
                ts.append(torch.tensor(_MASKS[name.split('.')[0]], dtype=torch.float32).expand(O, 1, 3, 3).contiguous())
            else:
                fan = max(1, int(np.prod(shape[1:])))
                ts.append(helpers._rand(gen, *shape, scale=1.0 if leaf in ('scale', 'bias', 'b0') else 1 / math.sqrt(fan)))
        _INPUTS[key] = (ts, helpers._rand(gen, O, C, 3, 3), helpers._rand(gen, O))
    return _INPUTS[key]


def merge_formula(kind, ts, dtype):
    """(Wf, bf) as the tensor expression of include/orn.h N7, in `dtype`, terms in the order written there."""
    ts = [t.to(dtype) for t in ts]
    w3x3, b3x3 = ts[0], ts[1]
    if kind == 'ACB':
        w3x1, b3x1, w1x3, b1x3 = ts[2:]
        return (w3x3 + F.pad(w1x3, (0, 0, 1, 1))) + F.pad(w3x1, (1, 1, 0, 0)), (b3x3 + b1x3) + b3x1
    if kind == 'RepVGG':
        return w3x3 + F.pad(ts[2], (1, 1, 1, 1)), b3x3 + ts[3]
    wA, wB = ts[2], ts[3]
    O, C = w3x3.shape[:2]
    T = torch.einsum('omk,mc->ock', wB.reshape(O, 2 * C, 9), wA.reshape(2 * C, C)).reshape(O, C, 3, 3)
    wf, bf = w3x3 + T, b3x3
    for t in range(3):
        k0, _, scale, bias, mask = ts[4 + 5 * t:9 + 5 * t]
        wf = wf + (scale * mask) * k0
        bf = bf + bias
    return wf, bf


def merge_backward_formula(kind, ts, g, dbf, dtype):
    """Gradients of BRANCH_TENSORS[kind] from g, dbf by the closed forms of include/orn.h N7, in `dtype`."""
    ts = [t.to(dtype) for t in ts]
    g, dbf = g.to(dtype), dbf.to(dtype)
    O, C = g.shape[:2]
    if kind == 'ACB':
        return [g, dbf, g[:, :, :, 1:2], dbf, g[:, :, 1:2, :], dbf]
    if kind == 'RepVGG':
        return [g, dbf, g[:, :, 1:2, 1:2], dbf]
    wA, wB = ts[2].reshape(2 * C, C), ts[3].reshape(O, 2 * C, 9)
    g9 = g.reshape(O, C, 9)
    out = [g, dbf, torch.einsum('omk,ock->mc', wB, g9).reshape(2 * C, C, 1, 1), torch.einsum('ock,mc->omk', g9, wA).reshape(O, 2 * C, 3, 3)]
    for t in range(3):
        k0, b0, scale, _, mask = ts[4 + 5 * t:9 + 5 * t]
        q = (mask.reshape(O, 1, 9) * g9).sum(-1)                       # [O, C]
        out += [(scale.reshape(O, 1) * q).reshape(O, C, 1, 1), torch.zeros_like(b0), (k0.reshape(O, C) * q).sum(1).reshape(O, 1, 1, 1), dbf,
                torch.zeros_like(mask)]
    return out


def guarded(shapes, device='cuda'):
    """One buffer holding NaN-seeded outputs of `shapes` between guard bands of a sentinel; returns (buffer, views)."""
    sizes = [int(np.prod(s)) for s in shapes]
    buf = torch.full((GUARD + sum(n + GUARD for n in sizes),), 12345.0, device=device)
    views, off = [], GUARD
    for s, n in zip(shapes, sizes):
        buf[off:off + n] = float('nan')
        views.append(buf[off:off + n].view(s))
        off += n + GUARD
    return buf, views


def check_guards(buf, shapes):
    off = 0
    for s in list(shapes) + [None]:
        assert bool((buf[off:off + GUARD] == 12345.0).all()), 'a guard band was written'
        if s is not None:
            off += GUARD + int(np.prod(s))
    assert not bool(torch.isnan(buf).any()), 'an output element was not written'


def ratio(k, r32, r64):
    k, r32 = k.double().cpu(), r32.double()
    den = max(float((r32 - r64).abs().max()), 2.0 ** -24 * float(r64.abs().max()))
    return float((k - r64).abs().max()) / den if den > 0 else float((k - r64).abs().max() > 0)


@pytest.mark.parametrize('C,O', SHAPES)
@pytest.mark.parametrize('kind', bf.KINDS)
def test_merge_forward(orn, kind, C, O):
    from orn_amd import ops
    ts, _, _ = branch_inputs(ops, kind, C, O)
    dev = [t.cuda() for t in ts]
    runs = []
    for _ in range(2):
        buf, (wf, bf_) = guarded([(O, C, 3, 3), (O,)])
        ops.branch_merge_fwd(kind, dev, out=(wf, bf_))
        torch.cuda.synchronize()
        check_guards(buf, [(O, C, 3, 3), (O,)])
        runs.append(buf)
    assert bits_equal(runs[0], runs[1])
    r_wf, r_bf = merge_formula(kind, ts, torch.float32)
    assert torch.equal(bf_.cpu(), r_bf)                               # adds only, in the order written
    if kind != 'ECB':
        assert torch.equal(wf.cpu(), r_wf)
        return
    r64 = merge_formula(kind, ts, torch.float64)[0]
    rt = ratio(wf, r_wf, r64)
    print(f'ECB forward C={C} O={O}: ratio wf {rt:.3f}')
    assert rt <= ECB_C['wf'], rt


@pytest.mark.parametrize('C,O', SHAPES)
@pytest.mark.parametrize('kind', bf.KINDS)
def test_merge_backward(orn, kind, C, O):
    from orn_amd import ops
    ts, g, dbf = branch_inputs(ops, kind, C, O)
    dev, gd, dbfd = [t.cuda() for t in ts], g.cuda(), dbf.cuda()
    shapes = ops.branch_shapes(kind, C, O)
    runs = []
    for _ in range(2):
        buf, grads = guarded(shapes)
        ops.branch_merge_bwd(kind, dev, gd, dbfd, grads=grads)
        torch.cuda.synchronize()
        check_guards(buf, shapes)
        runs.append(buf)
    assert bits_equal(runs[0], runs[1])
    r32 = merge_backward_formula(kind, ts, g, dbf, torch.float32)
    r64 = merge_backward_formula(kind, ts, g, dbf, torch.float64)
    for name, k, a, b in zip(ops.BRANCH_TENSORS[kind], grads, r32, r64):
        leaf = name.split('.')[-1]
        if kind == 'ECB' and leaf in ('wA', 'wB', 'k0', 'scale'):
            what = {'wA': 'dwA', 'wB': 'dwB', 'k0': 'dk0', 'scale': 'dscale'}[leaf]
            rt = ratio(k, a, b)
            print(f'ECB backward C={C} O={O}: ratio {what} ({name}) {rt:.3f}')
            assert rt <= ECB_C[what], (name, rt)
        elif leaf in ('b0', 'mask'):
            assert int(torch.count_nonzero(k.view(torch.int32))) == 0, name        # exactly +0, written
        else:
            assert torch.equal(k.cpu(), a.contiguous()), name                      # slices, copies, the bias fan-out
    # the engine's form: dWf / dbf already lie in the 3x3 branch's slots (grads[0] is g, grads[1] is dbf): nothing else changes
    g2, dbf2 = gd.clone(), dbfd.clone()
    buf, rest = guarded(shapes[2:])
    ops.branch_merge_bwd(kind, dev, g2, dbf2, grads=[g2, dbf2] + rest)
    torch.cuda.synchronize()
    check_guards(buf, shapes[2:])
    assert torch.equal(g2, gd) and torch.equal(dbf2, dbfd)
    for a, b in zip(rest, grads[2:]):
        assert bits_equal(a, b)


# ---- 2. against the reference fixture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', bf.KINDS)
def test_tiny_generator_against_reference(orn, kind):
    """Image, L1 loss and every gradient of the merged form against the reference's multi-branch fp32 forward and autograd, with
    test_tiny_generator_golden's tolerances.  (b0: the reference's gradients are rounding noise of 1e-13..2e-12, ours exactly 0.)"""
    from orn_amd import utils
    g = bf.load()
    tag = f'tiny_{kind}'
    gen = bf.tiny_generator(orn, kind).cuda()
    img = gen(cu(g[f'{tag}/embed']))[0]
    np.testing.assert_allclose(img.detach().cpu().numpy(), g[f'{tag}/img'], rtol=1e-5, atol=2e-6)

    class A:
        loss_type = 'L1'
    loss = utils.loss_fn(img, cu(g[f'{tag}/target']), A)
    assert abs(loss.item() - float(g[f'{tag}/loss_L1'])) < 1e-6
    loss.backward()
    worst = 0.0
    for k, p in gen.named_parameters():
        if not p.requires_grad:
            assert k.endswith('.mask') and p.grad is None
            continue
        r = g[f'{tag}/grad/{k}']
        atol = 2e-5 * max(np.abs(r).max(), 1e-6)
        worst = max(worst, float(np.max(np.abs(p.grad.cpu().numpy() - r) / (atol + 2e-4 * np.abs(r)))))
        np.testing.assert_allclose(p.grad.cpu().numpy(), r, rtol=2e-4, atol=atol, err_msg=k)
    print(f'{kind}: worst gradient error / tolerance {worst:.3f}')
    # deploy: one conv per block with the merged kernel gives the same image
    for layer in gen.layers:
        layer.switch_to_deploy()
    assert [k for k in gen.state_dict() if k.startswith('layers.')] == [f'layers.{i}.rbr_reparam.{p}' for i in range(2) for p in ('weight', 'bias')]
    with torch.no_grad():
        img_d = gen(cu(g[f'{tag}/embed']))[0]
    np.testing.assert_allclose(img_d.cpu().numpy(), g[f'{tag}/img'], rtol=1e-5, atol=2e-6)


# ---- 3. the engine is the vanilla engine on the merged kernel -------------------------------------------------------------------
TINY = dict(fc='3_4_8', strides=[2, 2], lower_width=8)
CONFIGS = [('fp32', 'tiny'), ('fp16', 'c96x2'), ('bf16', 'c96x2'), ('fp16', 'narrow_first'), ('bf16', 'narrow_first')]


def _generator(orn, geo, branch):
    from orn_amd import model
    g = TINY if geo == 'tiny' else helpers.GEOS[geo]
    torch.manual_seed(1)
    return model.Generator(embed_length=80, stem_dim_num='32_1', fc_hw_dim=g['fc'], expansion=1, num_blocks=1, norm='none', act='swish',
                           bias=True, reduction=2, conv_type='conv', stride_list=g['strides'], sin_res=True, lower_width=g['lower_width'],
                           sigmoid=False, deploy=False, branch_type=branch)


def _engine(orn, gen, prec, n_frames=5):
    from oracle import cpu_ref
    from orn_amd import engine
    eng = engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5, precision=prec)
    frames = cpu_ref.synthetic_video(n_frames, eng.out_hw[0], eng.out_hw[1], seed=5)
    embeds = cpu_ref.positional_encoding(torch.tensor([k / n_frames for k in range(n_frames)]), 1.25, 40)
    eng.set_video(frames, embeds)
    return eng


def _step(eng, form):
    entries = [(3, 1, 5e-4), (1, 1, 5e-4)] if form == 'batch2' else [(3, 1, 5e-4)]
    eng.set_schedule(entries)
    if form == 'batch2':
        eng.run(1, batch=2)
    else:
        eng.run(1, graph={'eager': False, 'graph': True}[form])
    torch.cuda.synchronize()


@pytest.mark.parametrize('form', ['eager', 'graph', 'batch2'])
@pytest.mark.parametrize('prec,geo', CONFIGS)
@pytest.mark.parametrize('kind', bf.KINDS)
def test_engine_is_vanilla_engine_on_merged_kernel(orn, kind, prec, geo, form):
    from orn_amd import ops
    gen = _generator(orn, geo, kind)
    eng = _engine(orn, gen, prec)
    nl = len(gen.layers)
    p0 = eng.params.clone()                                           # the parameters the step starts from
    rows = [0, 2, 4]
    bytes_k = eng.decode_frames(rows=rows, stats=False)['rgb8'].clone()
    fused = [eng.engine_fused_kernel(i) for i in range(nl)]           # what the decode's merge left in the workspace
    # the vanilla twin: same stem and head, every block's single conv = the merged kernel
    van = _generator(orn, geo, 'NeRV_vanilla')
    sd = {k: v.detach().clone() for k, v in gen.state_dict().items() if not k.startswith('layers.')}
    for i, (wf, bf_) in enumerate(fused):
        sd[f'layers.{i}.branch.weight'], sd[f'layers.{i}.branch.bias'] = wf, bf_
    van.load_state_dict(sd)
    veng = _engine(orn, van, prec)
    assert torch.equal(veng.decode_frames(rows=rows, stats=False)['rgb8'], bytes_k)
    _step(eng, form)
    for i, (wf, bf_) in enumerate(fused):                            # the step's merge saw the same parameters as the decode's
        wf2, bf2 = eng.engine_fused_kernel(i)
        assert torch.equal(wf2, wf) and torch.equal(bf2, bf_)
    _step(veng, form)
    assert bits_equal(eng.stats(1), veng.stats(1))
    assert eng.scale_state()['skipped'] == veng.scale_state()['skipped']

    def slot(e, name):
        off, n = e.layout[name]
        return e.grads[off:off + n]
    for name in [k for k in eng.layout if not k.startswith('layers.')]:
        assert bits_equal(slot(eng, name), slot(veng, name)), name    # stem and head gradients
    for i in range(nl):
        assert bits_equal(slot(eng, f'layers.{i}.rbr_3x3_branch.weight'), slot(veng, f'layers.{i}.branch.weight')), i
        assert bits_equal(slot(eng, f'layers.{i}.rbr_3x3_branch.bias'), slot(veng, f'layers.{i}.branch.bias')), i
    # the other branches' slots: the merge backward of the op on the engine's own dWf / dbf and the step's starting parameters
    for i, blk in enumerate(gen.layers):
        names = [k for k, _ in blk.named_parameters()]
        tensors = []
        for p in blk.branch_tensors():
            k = next(f'layers.{i}.{n}' for n, q in blk.named_parameters() if q is p)
            off, n = eng.layout[k]
            tensors.append((k, p0[off:off + n].view(p.shape)))
        assert len(tensors) == len(names)
        want = ops.branch_merge_bwd(kind, [t for _, t in tensors], slot(eng, tensors[0][0]).view(tensors[0][1].shape), slot(eng, tensors[1][0]))
        for (k, t), w in zip(tensors, want):
            assert bits_equal(slot(eng, k).view(t.shape), w), k


# ---- 4. three optimiser steps against fp64 autograd on the multi-branch forward ------------------------------------------------
def _seq_branch(x, k0, b0, scale, bias, mask):
    """model.py:272-284 in functional form: 1x1 conv, a border of b0 around it, then the depthwise scale * mask conv + bias."""
    y = F.conv2d(x, k0, b0)
    yp = b0.view(1, -1, 1, 1).expand(y.shape[0], -1, y.shape[2] + 2, y.shape[3] + 2).clone()
    yp[:, :, 1:-1, 1:-1] = y
    return F.conv2d(yp, scale * mask, bias, groups=k0.shape[0])


def multi_branch_forward(sd, embed, kind, strides, fc):
    """The reference's training forward of a generator of `kind` (separate convolutions summed on the activations, model.py:541-565),
    on a state dict of any dtype."""
    fh, fw, fd = fc
    x = F.silu(F.linear(F.silu(F.linear(embed, sd['stem.0.weight'], sd['stem.0.bias'])), sd['stem.2.weight'], sd['stem.2.bias']))
    x = x.view(x.shape[0], fd, fh, fw)
    for i, s in enumerate(strides):
        def P(n):
            return sd[f'layers.{i}.{n}']
        y = F.conv2d(x, P('rbr_3x3_branch.weight'), P('rbr_3x3_branch.bias'), padding=1)
        if kind == 'ACB':
            y = y + F.conv2d(x, P('rbr_3x1_branch.weight'), P('rbr_3x1_branch.bias'), padding=(1, 0))
            y = y + F.conv2d(x, P('rbr_1x3_branch.weight'), P('rbr_1x3_branch.bias'), padding=(0, 1))
        elif kind == 'RepVGG':
            y = y + F.conv2d(x, P('rbr_1x1_branch.weight'), P('rbr_1x1_branch.bias'))
        else:
            y = y + F.conv2d(F.conv2d(x, P('rbr_1x1_3x3_branch_1x1.weight')), P('rbr_1x1_3x3_branch_3x3.weight'), padding=1)
            for seq in ('sbx', 'sby', 'lpl'):
                y = y + _seq_branch(x, *[P(f'rbr_conv1x1_{seq}_branch.{f}') for f in ('k0', 'b0', 'scale', 'bias', 'mask')])
        x = F.silu(F.pixel_shuffle(y, s))
    n = len(strides) - 1
    out = F.conv2d(x, sd[f'head_layers.{n}.weight'], sd[f'head_layers.{n}.bias'])
    return (torch.tanh(out) + 1) * 0.5


@pytest.mark.parametrize('kind', bf.KINDS)
def test_three_steps_against_fp64_multi_branch(orn, kind):
    from oracle import cpu_ref
    from orn_amd import engine
    gen = _generator(orn, 'tiny', kind)
    sd0 = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    frames = cpu_ref.synthetic_video(5, 12, 16, seed=3)
    embeds = cpu_ref.positional_encoding(torch.tensor([k / 5.0 for k in range(5)], dtype=torch.float32), 1.25, 40)
    eng = engine.TrainEngine(gen, loss_type='Fusion6', beta=0.5)
    eng.set_video(frames, embeds)
    entries = [(3, 1, 5e-4), (0, 2, 4e-4), (4, 3, 3e-4)]
    eng.set_schedule(entries)
    eng.run(3, graph=False)
    torch.cuda.synchronize()
    st = eng.stats(3).numpy()
    sd = {k: v.double() for k, v in sd0.items()}
    am = {k: torch.zeros_like(v) for k, v in sd.items()}
    av = {k: torch.zeros_like(v) for k, v in sd.items()}
    for i, (f, step, lr) in enumerate(entries):
        params = {k: v.detach().clone().requires_grad_(not k.endswith('.mask')) for k, v in sd.items()}
        out = multi_branch_forward(params, embeds[f:f + 1].double(), kind, [2, 2], (3, 4, 8))
        loss = cpu_ref.loss_fn(out, frames[f:f + 1].double(), 'Fusion6')
        loss.backward()
        assert abs(st[i, 0] - loss.item()) < 5e-5, (i, st[i], loss.item())
        assert st[i, 6] == f and st[i, 7] == step
        with torch.no_grad():
            for k in sd:
                if params[k].grad is not None:
                    cpu_ref.adam_step(sd[k], params[k].grad, am[k], av[k], step, lr, 0.5)
    new = gen.state_dict()
    worst = 0.0
    for k in sd:
        diff = (new[k].cpu().double() - sd[k]).abs().max().item()
        worst = max(worst, diff)
        assert diff < 0.75 * 5e-4, (k, diff)
        if k.endswith('.mask') or k.endswith('.b0'):
            assert torch.equal(new[k].cpu(), sd0[k]), k               # never trained: bit-unchanged
    print(f'{kind}: worst parameter distance from the fp64 multi-branch reference after 3 steps: {worst / 5e-4:.3f} lr')


# ---- 5. the CLIs -------------------------------------------------------------------------------------------------------------
CLI = ('-e 2 --lower_width 8 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 --reduction 2 '
       '--fc_hw_dim 3_4_8 --expansion 1 --single_res --loss Fusion6 --warmup 0.2 --lr_type cosine --strides 2 2 --conv_type conv -b 1 '
       '--lr 0.0005 --norm none --act swish --outf ecb_t --branch_type ECB --synthetic 6 --precision fp32').split()


def test_cli_train_eval_ecb(orn, tmp_path, monkeypatch):
    from orn_amd import checkpoint, main_eval, main_train
    monkeypatch.chdir(tmp_path)
    main_train.train(main_train.parse_args(CLI))
    outf = tmp_path / 'result' / 'ecb_t'
    sd = checkpoint.load_state_dict_file(str(outf / 'model_latest.pth'))
    assert list(sd.keys()) == list(bf.load()['tiny_ECB/keys']) and checkpoint.state_dict_kind(sd) == 'ECB'
    dsd = checkpoint.load_state_dict_file(str(outf / 'model_latest_deploy.pth'))
    assert checkpoint.state_dict_kind(dsd) == 'deploy' and len(dsd) == 4 + 2 * 2 + 2
    assert 'Deploy Rep-Model Params' in (outf / 'rank0.txt').read_text()
    psnr_deploy = main_eval.main(CLI + ['--decoder', 'engine'])      # model_latest_deploy.pth is there: the deploy copy
    os.rename(outf / 'model_latest_deploy.pth', outf / 'kept_deploy.pth')
    psnr_train = main_eval.main(CLI + ['--decoder', 'engine'])       # the train form: loaded, merged, decoded
    assert psnr_train == psnr_deploy and 5.0 < psnr_train < 60.0
    with pytest.raises(ValueError, match='finetune'):
        main_eval.main(CLI + ['--prune_ratio', '0.4', '--finetune', '--finetune_epochs', '1'])
