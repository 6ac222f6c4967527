"""What the split step (orn_engine_step_forward / orn_engine_step_backward; TrainEngine.run_with) costs at the bench geometry
(720p ERB, 132 frames, fp16).  Five ways to run the same number of optimiser steps:

  a  built-in Fusion6, run(graph=False): one orn_engine_train_step call per step -- the serial step the seam is cut from
  b  built-in Fusion6, run(): the pipelined form (bench.py's)
  c  the seam fed by ops.loss_stats(pred, target, 'Fusion6'): the same loss kernel, called from Python between the two halves
  d  run_with(mean |pred - target|): an objective made of torch ops and autograd
  e  run_with(custom_losses.fusion_freq_ssim): torch.fft + the library's Fusion6 kernel through ops.LossFn

One fresh process per variant and repeat, the variants taking turns (a b c d e, a b c d e, ...): a drift of the box falls on all of
them alike.  Each process runs one warm-up epoch (132 steps) of its variant and is then timed over STEPS steps; a timing is a host
clock around the run, which ends in a device synchronise.  The medians over the repeats and the differences c - a, e - a (what the
seam itself costs; what a torch-composed FFT objective costs on top) are written out.  There is no threshold on them.

    python tools/custom_loss_fps.py [--out profiles/custom_loss_fps.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

STEPS = 264
REPEATS = 3
VARIANTS = {'a': 'built-in Fusion6, run(graph=False)', 'b': 'built-in Fusion6, run() (pipelined)',
            'c': 'seam + ops.loss_stats(Fusion6)', 'd': 'run_with(torch L1)', 'e': 'run_with(fusion_freq_ssim)'}


def runner(eng, variant):
    """n -> enqueue n steps of the variant on eng"""
    from orn_amd import custom_losses, ops
    if variant == 'a':
        return lambda n: eng.run(n, graph=False)
    if variant == 'b':
        return eng.run
    if variant == 'c':
        def seam(n):
            for _ in range(n):
                pred = eng.forward_step()
                f = eng.open_frame
                stats, g = ops.loss_stats(pred, eng.frames[f:f + 1], 'Fusion6', want_grad=True)
                eng.backward_step(g, stats[0])
        return seam
    if variant == 'd':
        return lambda n: eng.run_with(lambda p, t: (p - t).abs().mean(), n)
    return lambda n: eng.run_with(custom_losses.fusion_freq_ssim, n)


def measure(variant, precision):
    """The child's work: one engine, one warm-up epoch, one timed run."""
    import torch
    import bench
    import loss_fps
    if not torch.cuda.is_available():
        raise SystemExit('custom_loss_fps: needs a GPU (there is no CPU path and no CPU number)')
    n = bench.CFG['frames']
    eng = loss_fps.make_engine(bench, 'Fusion6', precision)
    run = runner(eng, variant)
    eng.set_schedule(bench.schedule(n))
    run(n)
    torch.cuda.synchronize()
    eng.set_schedule(bench.schedule(STEPS, start_step=n))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(STEPS)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = eng.stats(STEPS)
    sc = eng.scale_state()
    return {'ms_per_step': round(1e3 * dt / STEPS, 4), 'mean_psnr_db': round(float(st[:, 4].double().mean()), 3),
            'finite': bool(torch.isfinite(st).all()), 'steps_skipped': sc['skipped'] + sc['late_skipped'],
            'device': torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--variants', default=','.join(VARIANTS))
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--child', default=None, help='(internal) measure this one variant in this process and print its record')
    args = ap.parse_args()
    if args.child:
        print('CUSTOM_LOSS_FPS ' + json.dumps(measure(args.child, args.precision)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    names = [v for v in args.variants.split(',') if v]
    res = {'geometry': bench.CONFIGS['720p']['name'], 'precision': args.precision, 'warmup_steps': bench.CFG['frames'], 'steps': STEPS,
           'repeats': REPEATS, 'processes': 'one per variant and repeat, variants alternating',
           'results': {v: {'what': VARIANTS[v], 'ms_per_step': [], 'mean_psnr_db': [], 'steps_skipped': []} for v in names}}
    for rep in range(REPEATS):
        for v in names:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', v, '--precision', args.precision],
                               capture_output=True, text=True, cwd=ROOT, timeout=300)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('CUSTOM_LOSS_FPS ')]
            if r.returncode != 0 or not lines:
                raise SystemExit(f'custom_loss_fps: variant {v} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
            rec = json.loads(lines[-1][len('CUSTOM_LOSS_FPS '):])
            res['device'] = rec.pop('device')
            if not rec.pop('finite'):
                raise SystemExit(f'custom_loss_fps: variant {v}: non-finite stats')
            for k, val in rec.items():
                res['results'][v][k].append(val)
            print(f'repeat {rep} variant {v}: {rec}', file=sys.stderr, flush=True)
    for v, r in res['results'].items():
        ms = sorted(r['ms_per_step'])
        r['median_ms_per_step'] = ms[len(ms) // 2]
        r['median_frames_per_s'] = round(1e3 / ms[len(ms) // 2], 1)
    med = {v: r['median_ms_per_step'] for v, r in res['results'].items()}
    if 'a' in med:
        res['ms_over_a'] = {v: round(med[v] - med['a'], 4) for v in med if v != 'a'}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
