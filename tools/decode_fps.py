"""Decode throughput of the engine at the bench geometry (720p, 132 frames), fp16 and fp32, one process:

  a  a loop of single-frame orn_engine_decode calls (fp32 image per call; all there was before orn_engine_decode_frames)
  b  decode_frames -> RGB8 + stats (one call for all frames)
  c  decode_frames -> fp32 images only
  d  a + what main_eval does per frame with torch ops today: the L2 loss kernel for the PSNR and mul/add/clamp/uint8/permute
     for the pixels (kept on the device: the host copy of --dump_images is not counted)
  e  the engine evaluation before orn_engine_eval_frames: decode_frames -> stats, then per frame a single-frame decode and
     utils.msssim_fn (one MS-SSIM call per frame)
  f  the one-call evaluation: decode_frames -> stats + per-frame MS-SSIM (orn_engine_eval_frames)

Every variant is warmed up, then timed REPEATS times, the variants alternating inside a repeat; a timing is a host clock around
PASSES passes over the video that end in a device synchronise.  Prints one JSON document (every repeat, frames/s).

    python tools/decode_fps.py [--out profiles/decode_fps.json] [--only b]      # --only: one variant, for a profiler run
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 132
REPEATS = 5
PASSES = {'fp16': 4, 'fp32': 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default=None, choices=['a', 'b', 'c', 'd', 'e', 'f'])
    ap.add_argument('--precisions', default='fp16,fp32')
    ap.add_argument('--frames', type=int, default=FRAMES)
    args = ap.parse_args()
    import torch
    import bench
    from orn_amd import ops, utils
    if not torch.cuda.is_available():
        raise SystemExit('decode_fps: needs a GPU (there is no CPU path and no CPU number)')
    res = {'geometry': bench.CONFIGS['720p']['name'], 'frames': args.frames, 'repeats': REPEATS, 'unit': 'frames/s',
           'device': torch.cuda.get_device_name(0), 'variants': {
               'a': 'loop of orn_engine_decode', 'b': 'decode_frames rgb8 + stats', 'c': 'decode_frames f32 only',
               'd': 'loop of orn_engine_decode + torch quantise + L2 loss kernel per frame',
               'e': 'decode_frames stats + per-frame orn_engine_decode + msssim_fn', 'f': 'decode_frames stats + msssim, one call'},
           'results': {}}
    for prec in args.precisions.split(','):
        eng = bench.make_engine(seed=1234, precision=prec, cfg=bench.CONFIGS['720p'], frames=args.frames)
        n = args.frames
        keep = {}

        def va():
            for k in range(n):
                keep['a'] = eng.decode(eng.embeds[k])

        def vb():
            keep['b'] = eng.decode_frames(rgb8=True, f32=False, stats=True)

        def vc():
            keep['c'] = eng.decode_frames(rgb8=False, f32=True, stats=False)

        def vd():
            for k in range(n):
                img = eng.decode(eng.embeds[k])
                st, _ = ops.loss_stats(img, eng.frames[k:k + 1], 'L2', want_grad=False)
                keep['d'] = (st, img[0].mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8))

        def ve():
            st = eng.decode_frames(rgb8=False, f32=False, stats=True)['stats']
            ms = [utils.msssim_fn([eng.decode(eng.embeds[k])], [eng.frames[k:k + 1]])[0, 0] for k in range(n)]
            keep['e'] = (st, torch.stack(ms))

        def vf():
            keep['f'] = eng.decode_frames(rgb8=False, f32=False, stats=True, msssim=True)

        variants = {'a': va, 'b': vb, 'c': vc, 'd': vd, 'e': ve, 'f': vf}
        if args.only:
            variants = {args.only: variants[args.only]}
        for f in variants.values():                     # warm-up: every shape the timed window uses
            f()
        torch.cuda.synchronize()
        passes = PASSES.get(prec, 1)
        out = {v: [] for v in variants}
        for _ in range(REPEATS):
            for v, f in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _p in range(passes):
                    f()
                torch.cuda.synchronize()
                out[v].append(round(n * passes / (time.perf_counter() - t0), 1))
        res['results'][prec] = {'passes': passes, 'fps': out, 'median': {v: sorted(x)[len(x) // 2] for v, x in out.items()}}
        if 'b' in keep:
            res['results'][prec]['mean_psnr_db'] = round(float(keep['b']['stats'][:, 1].double().mean()), 4)
        if 'e' in keep and 'f' in keep:
            res['results'][prec]['f_over_e'] = [round(f / e, 3) for e, f in zip(out['e'], out['f'])]
            res['results'][prec]['msssim_e_equals_f'] = bool(torch.equal(keep['e'][1], keep['f']['msssim']))
            res['results'][prec]['mean_msssim'] = round(float(keep['f']['msssim'].double().mean()), 6)
        del eng, keep
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
