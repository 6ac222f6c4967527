"""`python -m orn_amd.main_eval <flags>`: the evaluation path of the reference's main_eval.py:
load `model_latest(.pth|_deploy.pth)` -> global L1 prune (--prune_ratio) -> switch to deploy -> per-axis 8-bit
quantisation + Huffman size estimate (--quant_bit) -> decode every frame (PSNR, decoder FPS, bits per pixel).

`--decoder engine` decodes with the native engine at `--precision` (engine.Decoder: all frames in one
orn_engine_eval_frames call, PSNR of the float image and of the 8-bit pixels, the per-frame MS-SSIM and the `--dump_images`
bytes computed on the device); the default `eager` is the per-op fp32 module forward, frame by frame.

`--decode_stage all|K` (with `--decoder engine`, without `--single_res`): a multi-resolution fit is a scalable bitstream.  `all`
evaluates every stage in one call (engine.Decoder(stages=True).decode_stages, orn_engine_eval_stages) and prints one value per stage;
`K` decodes stage K alone -- the blocks above it and the last head do not run -- with PSNR, MS-SSIM where the size allows, FPS,
`--dump_images` and bpp at that stage's size.

`--finetune` (main_eval.py:213-545): load the TRAIN-mode checkpoint, prune the stem Linear weights and every conv
branch weight together (global L1), fine-tune `--finetune_epochs` on the native engine, then deploy/quantise/evaluate.
The reference's behaviour is kept, quirks included: Q1 -- with ERB the online merge reads `.weight`
directly, so torch's pruning hooks never fire and the branch conv weights stay frozen at their pruned-at-t0 values
(only stem weights under their mask, all biases and the head train); NeRV_vanilla convs train under their masks.
Q2 -- the LR comes from adjust_lr(epoch % total_epochs) with epoch continuing from the checkpoint (>= args.epochs),
i.e. the cosine evaluated past its end (0 at e = 300, 4e-5 x lr at 301, ...).  Q3 is `quantize_per_tensor`'s."""
import os
import time

import torch

from . import checkpoint, data as odata, eval_utils, model as omodel, ops, utils
from .main_train import build_parser


ERB_BRANCHES = ('rbr_3x3_branch', 'rbr_3x1_branch', 'rbr_1x3_branch', 'rbr_1x1_3x3_1x1_branch_1x1_1',
                'rbr_1x1_3x3_1x1_branch_3x3', 'rbr_1x1_3x3_1x1_branch_1x1_2')


def _prune_finetune(model, args, PE, ckpt_path, vid_index=0):
    """main_eval.py:213-531 on the native engine (see the module docstring for the reference quirks kept)."""
    from . import engine as oeng
    named = dict(model.named_parameters())
    prunable = {}
    for k in named:                                            # main_eval.py:296-302: stem Linear weights
        if k.startswith('stem.') and k.endswith('weight'):
            prunable[k] = named[k].detach()
    for i, blk in enumerate(model.layers):                     # main_eval.py:305-340 (ERB) / 244-264 (vanilla)
        names = ERB_BRANCHES if blk.branch_type == 'ERB' else ('branch',)
        for b in names:
            k = f'layers.{i}.{b}.weight'
            if k in named:
                prunable[k] = named[k].detach()
    originals = {k: v.clone() for k, v in prunable.items() if k.startswith('stem.')}     # weight_orig keeps them under the mask
    masks = eval_utils.global_l1_prune_masks(prunable, args.prune_ratio)
    zero = sum(int((m == 0).sum()) for m in masks.values())
    tot = sum(m.numel() for m in masks.values())
    print(f'global L1 prune of {len(masks)} tensors: {zero}/{tot} = {zero / tot:.3f} (asked {args.prune_ratio})')
    with torch.no_grad():
        for k, m in masks.items():
            named[k].mul_(m)
    eng = oeng.TrainEngine(model, loss_type=args.loss_type, beta=args.beta, precision=args.precision)
    gmask = {}
    for k, m in masks.items():                                 # Q1: ERB branch convs are frozen, the rest trains masked
        frozen = k.startswith('layers.') and args.branch_type == 'ERB'
        gmask[k] = torch.zeros_like(m) if frozen else m
    eng.set_grad_mask(gmask)
    hw = eng.out_hw
    from .main_train import load_frames
    frames, pos = load_frames(args, hw, eng.device, args.dataset, vid_index, args.frame_gap)
    n = frames.shape[0]
    eng.set_video(frames, PE(pos))
    try:
        start_epoch = int(torch.load(ckpt_path, map_location='cpu', weights_only=True).get('epoch', args.epochs))
    except Exception:
        start_epoch = args.epochs
    total = start_epoch + args.finetune_epochs
    g = torch.Generator()
    step = 0
    for epoch in range(start_epoch, total):
        g.manual_seed(args.manualSeed + epoch)
        order = torch.randperm(n, generator=g).tolist()
        entries = []
        for i, f in enumerate(order):
            step += 1                                          # fresh optimiser: main_eval.py:496 clears its state
            entries.append((f, step, utils.lr_value(epoch % total, i, n, args)))      # Q2
        eng.set_schedule(entries)
        eng.run(n)
        st = eng.stats(n)
        if (epoch - start_epoch) % max(1, args.finetune_epochs // 10) == 0 or epoch == total - 1:
            print(f'fine-tune epoch {epoch + 1}/{total} lr {float(st[-1, 5]):.2e} PSNR {float(st[:, 4].mean()):.2f}', flush=True)
    eng.set_grad_mask(None)
    torch.cuda.synchronize()
    # what stays pruned in the reference's state dict after the fine-tune: the stem Linear layers (weight_orig + weight_mask;
    # the ERB branch modules disappear in switch_to_deploy, a vanilla block keeps its pruned `branch`)
    keep = {k: m for k, m in masks.items() if k.startswith('stem.') or args.branch_type != 'ERB'}
    return keep, {k: v for k, v in originals.items() if k in keep}


def eval_parser():
    p = build_parser()
    p.add_argument('--finetune', action='store_true')
    p.add_argument('--finetune_epochs', type=int, default=100)
    p.add_argument('--cycles', type=int, default=1)
    p.add_argument('--video', default=None, help='which video of a multi-video training job (--dataset a,b,c or a multi-rank '
                                                  '--synthetic job: synthetic<k>) to evaluate; default: the first')
    p.add_argument('--decode_stage', default=None, metavar='all|K',
                   help='--decoder engine, multi-resolution fits: evaluate every stage in one call (all), or decode stage K alone '
                        '(0 = the smallest image; the blocks above K do not run)')
    return p


def check_decode_stage(args):
    """None (flag absent), 'all' or the stage index of --decode_stage; ValueError for a combination that has no such decode.  Reads
    nothing but args."""
    ds = getattr(args, 'decode_stage', None)
    if ds is None:
        return None
    if args.decoder != 'engine':
        raise ValueError(f'--decode_stage {ds} needs --decoder engine: the per-stage decode is the native engine\'s')
    if args.single_res:
        raise ValueError(f'--decode_stage {ds} with --single_res: a single-resolution generator has one stage, the output')
    if ds == 'all':
        return 'all'
    try:
        k = int(ds)
    except ValueError:
        raise ValueError(f'--decode_stage {ds!r}: expected all or a stage index') from None
    if not 0 <= k < len(args.strides):
        raise ValueError(f'--decode_stage {k}: the generator has stages 0..{len(args.strides) - 1} (--strides)')
    return k


def _stage_decode(model, args, embeds, tables, outf, n_param, bits, which):
    """--decode_stage: `tables` holds the target table of every stage decoded.  all: every stage in one call, the usual line for the last stage
    and one more with a value per stage; K: stage K alone, everything at its size."""
    from . import engine as oeng
    dec = oeng.Decoder(model, precision=args.precision, stages=True)
    hws = dec.stage_hw()
    sel = list(range(len(hws))) if which == 'all' else [which]
    n = embeds.shape[0]
    torch.cuda.synchronize()
    t0 = time.time()
    out = dec.decode_stages(stages=sel, embeds=embeds, frames=[tables[s] for s in sel], rgb8=True, f32=False, stats=True, msssim=True)
    torch.cuda.synchronize()
    fps = n / (time.time() - t0)
    show = sel[-1]                                          # the stage the Eval line, the images and the return value belong to
    st = out[show]['stats'].double().mean(0)
    psnr, psnr8 = float(st[1]), float(st[3])
    if args.dump_images:
        from PIL import Image
        visual_dir = os.path.join(outf, 'visualize')
        os.makedirs(visual_dir, exist_ok=True)
        print(f'Saving predictions to {visual_dir}')
        for k, arr in enumerate(out[show]['rgb8'].cpu().numpy()):
            Image.fromarray(arr).save(os.path.join(visual_dir, f'pred_{k}.png'))
    if which == 'all':
        cols = [out[s]['stats'].double().mean(0) for s in sel]
        print('Eval stages PSNR: [' + ', '.join(f'{float(c[1]):.2f}' for c in cols) + '], 8-bit PSNR: ['
              + ', '.join(f'{float(c[3]):.2f}' for c in cols) + '], MS-SSIM: [' + ', '.join(f'{float(out[s]["msssim"].mean()):.4f}' for s in sel) + ']')
    tag = 'all stages' if which == 'all' else f'stage {which}, {hws[which][0]}x{hws[which][1]}'
    msg = (f'Eval: PSNR {psnr:.2f} dB, 8-bit PSNR {psnr8:.2f} dB, MS-SSIM {float(out[show]["msssim"].mean()):.4f}, '
           f'decode {fps:.1f} FPS (engine, {args.precision}, {tag}), params {n_param / 1e6:.3f} M')
    if bits is not None:
        msg += f', bpp {bits / (n * hws[show][0] * hws[show][1]):.4f}'
    print(msg)
    return psnr


def _engine_decode(model, args, embeds, frames, outf, n_param, bits, hw):
    """--decoder engine: every frame through engine.Decoder in one call (main_eval.py:795-815)."""
    from . import engine as oeng
    n = frames.shape[0]
    dec = oeng.Decoder(model, precision=args.precision)
    torch.cuda.synchronize()
    t0 = time.time()
    out = dec.decode_frames(embeds=embeds, frames=frames, rgb8=True, f32=False, stats=True, msssim=True)
    torch.cuda.synchronize()
    fps = n / (time.time() - t0)
    st = out['stats'].double().mean(0)
    psnr, psnr8 = float(st[1]), float(st[3])
    if args.dump_images:
        from PIL import Image
        visual_dir = os.path.join(outf, 'visualize')
        os.makedirs(visual_dir, exist_ok=True)
        print(f'Saving predictions to {visual_dir}')
        for k, arr in enumerate(out['rgb8'].cpu().numpy()):
            Image.fromarray(arr).save(os.path.join(visual_dir, f'pred_{k}.png'))
    msssim = float(out['msssim'].mean())                             # per frame, from the same call (its launches are in the FPS above)
    msg = (f'Eval: PSNR {psnr:.2f} dB, 8-bit PSNR {psnr8:.2f} dB, MS-SSIM {msssim:.4f}, '
           f'decode {fps:.1f} FPS (engine, {args.precision}), params {n_param / 1e6:.3f} M')
    if bits is not None:
        msg += f', bpp {bits / (n * hw[0] * hw[1]):.4f}'
    print(msg)
    return psnr


def main(argv=None):
    args = eval_parser().parse_args(argv)
    decode_stage = check_decode_stage(args)
    if args.finetune and args.batchSize > 1:
        # the fine-tune's loop takes one frame per optimiser step; a -b it ignored would silently be another recipe
        raise ValueError(f'--finetune with -b/--batchSize {args.batchSize}: the prune fine-tune steps one frame at a time; use -b 1 '
                         '(batched steps are built for main_train only)')
    if args.finetune and not args.single_res:
        raise ValueError('--finetune needs --single_res: the prune fine-tune of a multi-resolution generator (a head on every stage) is '
                         'not built')
    args.warmup = int(args.warmup * args.epochs)          # main_eval.py:106 (as main_train.parse_args): warm-up in epochs
    outf = os.path.join('result', args.outf, f'{args.suffix}')
    # a job that fitted several videos wrote one sub-directory per video (main_train.video_outf)
    videos = [d for d in args.dataset.split(',') if d]
    vid_index = 0
    if args.synthetic and args.video:
        vid_index = int(args.video[len('synthetic'):])
        if os.path.isdir(os.path.join(outf, args.video)):
            outf = os.path.join(outf, args.video)
    elif len(videos) > 1:
        name = args.video or videos[0]
        if name not in videos:
            raise ValueError(f'--video {name} is not one of --dataset {videos}')
        vid_index = videos.index(name)
        args.dataset = name
        outf = os.path.join(outf, name)
    PE = utils.PositionalEncoding(args.embed)
    deploy_file = os.path.join(outf, 'model_latest_deploy.pth')
    train_file = os.path.join(outf, 'model_latest.pth')
    finetune = args.finetune and args.prune_ratio < 1
    from .main_train import MERGED_BRANCHES
    if args.finetune and args.branch_type in MERGED_BRANCHES and args.branch_type != 'ERB':
        # the reference's fine-tune prunes nothing of these blocks (main_eval.py:244-340 knows `branch` and ERB's attributes only)
        raise ValueError(f'--finetune with --branch_type {args.branch_type}: the prune fine-tune is built for NeRV_vanilla and ERB only')
    path = deploy_file if (args.branch_type in MERGED_BRANCHES and os.path.exists(deploy_file) and not finetune) else train_file
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    sd = checkpoint.load_state_dict_file(path)
    torch.manual_seed(args.manualSeed)
    model = omodel.Generator(embed_length=PE.embed_length, stem_dim_num=args.stem_dim_num, fc_hw_dim=args.fc_hw_dim,
                             expansion=args.expansion, num_blocks=args.num_blocks, norm=args.norm, act=args.act, bias=True,
                             reduction=args.reduction, conv_type=args.conv_type, stride_list=args.strides,
                             sin_res=args.single_res, lower_width=args.lower_width, sigmoid=args.sigmoid, deploy=False,
                             branch_type=args.branch_type)
    kind = checkpoint.load_into(model, sd)
    model = model.cuda()
    masks, originals = {}, None
    if finetune:
        masks, originals = _prune_finetune(model, args, PE, path, vid_index) if vid_index else _prune_finetune(model, args, PE, path)
    if kind != 'deploy':
        for blk in model.layers:
            blk.switch_to_deploy() if blk.branch_type in MERGED_BRANCHES else None
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    n_param = sum(v.numel() for v in sd.values())
    if args.prune_ratio < 1 and not finetune:
        # main_eval.py:551-650: global L1 over the stem Linear weights and the blocks' single convs (deploy-state
        # rbr_reparam for ERB, branch / rbr_reparam for NeRV_vanilla) -- not the head, not the biases
        prunable = {k: v for k, v in sd.items()
                    if k.endswith('.weight') and (k.startswith('stem.') or (k.startswith('layers.') and k.split('.')[2] in ('rbr_reparam', 'branch')))}
        masks = eval_utils.global_l1_prune_masks(prunable, args.prune_ratio)
        kept = sum(int(m.sum()) for m in masks.values())
        print(f'global L1 prune of {len(masks)} tensors: {1 - kept / sum(m.numel() for m in masks.values()):.3f} of the weights masked')
    # the state dict as the reference sees it from here on: pruned tensors as weight_orig + weight_mask (never removed)
    sd = eval_utils.pruned_state_dict(sd, masks, originals)
    bits = None
    if args.quant_bit != -1:
        sd, bits, count, _ = eval_utils.quantized_model_bits(sd, args.quant_bit, args.quant_axis)
        print(f'quantised to {args.quant_bit} bit: {bits / 8 / 1e6:.3f} MB entropy-coded over the {count} non-zero entries '
              f'({bits / max(count, 1):.2f} bits each; optimal prefix code, dahuffman parity unpinned)')
    model.load_state_dict(eval_utils.fold_pruned(sd))
    hw = [model.fc_h, model.fc_w]
    for s_ in args.strides:
        hw = [hw[0] * s_, hw[1] * s_]
    from .main_train import load_frames
    frames, pos = load_frames(args, hw, 'cuda', args.dataset, vid_index, args.test_gap)       # val_dataset: CustomDataSet(frame_gap=test_gap)
    n = frames.shape[0]
    embeds = PE(pos)
    if decode_stage is not None:
        # every stage's target is pooled from the source like the last stage's (main_train.py:420); synthetic frames ARE the source, at
        # the decoder's size
        from . import engine as oeng
        shws = oeng.stage_hw(model)
        tables = {}
        for s in (range(len(shws)) if decode_stage == 'all' else [decode_stage]):
            if tuple(shws[s]) == tuple(hw):
                tables[s] = frames
            elif args.synthetic:
                tables[s] = ops.ingest_frames(frames, tuple(shws[s]))
            else:
                tables[s] = load_frames(args, shws[s], 'cuda', args.dataset, vid_index, args.test_gap)[0]
        return _stage_decode(model, args, embeds, tables, outf, n_param, bits, decode_stage)
    if args.decoder == 'engine':
        return _engine_decode(model, args, embeds, frames, outf, n_param, bits, hw)
    psnrs = []
    torch.cuda.synchronize()
    t0 = time.time()
    dumped = []
    with torch.no_grad():
        for k in range(n):
            img = model(embeds[k:k + 1])[-1]                 # the last stage (main_eval.py:467-472: a multi-resolution model returns one image per stage)
            st, _ = ops.loss_stats(img, frames[k:k + 1], 'L2', want_grad=False)
            psnrs.append(st[4])
            if args.dump_images:                      # main_eval.py:795-803 (written after the timed loop)
                dumped.append(img[0].detach())
    torch.cuda.synchronize()
    fps = n / (time.time() - t0)
    psnr = float(torch.stack(psnrs).mean())
    if args.dump_images:
        from PIL import Image
        visual_dir = os.path.join(outf, 'visualize')
        os.makedirs(visual_dir, exist_ok=True)
        print(f'Saving predictions to {visual_dir}')
        for k, im in enumerate(dumped):              # torchvision.utils.save_image: x*255 + 0.5, clamp, uint8, HWC
            arr = im.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to('cpu', torch.uint8).numpy()
            Image.fromarray(arr).save(os.path.join(visual_dir, f'pred_{k}.png'))
    with torch.no_grad():                                            # untimed, as the FPS above is the decoder's
        ms = [utils.msssim_fn([model(embeds[k:k + 1])[-1]], [frames[k:k + 1]])[0, 0] for k in range(n)]
    msg = f'Eval: PSNR {psnr:.2f} dB, MS-SSIM {float(torch.stack(ms).mean()):.4f}, decode {fps:.1f} FPS, params {n_param / 1e6:.3f} M'
    if bits is not None:
        msg += f', bpp {bits / (n * hw[0] * hw[1]):.4f}'
    print(msg)
    return psnr


if __name__ == '__main__':
    main()
