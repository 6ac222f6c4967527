"""Per-frame training throughput of the batched optimiser step (-b B; include/orn.h N5) against the single-frame forms, at the
bench geometry (720p ERB, 132 frames, fp16, Fusion6):

  pipelined_b1   TrainEngine.run(n)                the pipelined single-frame step (bench.py's headline form)
  graph_b1       TrainEngine.run(n, graph=True)    hipGraph replay of the serial single-frame step
  batched_b1/2/4/8   TrainEngine.run_batched(n, B) the batched form: serial launches, one merge forward / merge backward / Adam per B frames

One fresh process per configuration and repeat (several engines in one process slow each other), the configurations
alternating inside each of REPEATS rounds so that drift of the box hits all alike.  A process runs one warm-up epoch (132 frames)
and then times FRAMES frames (FRAMES / B optimiser steps): a host clock around one run call that ends in a device synchronise.
Writes frames/s and ms per frame of every repeat and their medians.  Nothing is gated on it: it records where the batched form lands.

    python tools/batch_fps.py [--out profiles/batch_fps.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 264
REPEATS = 3
CONFIGS = ['pipelined_b1', 'graph_b1', 'batched_b1', 'batched_b2', 'batched_b4', 'batched_b8']


def entries(bench, n_frames, B, first_step):
    """bench.schedule's frame order, B frames per optimiser step: a batch carries the step number and the lr of its first frame."""
    sched = bench.schedule(n_frames)
    return [(f, first_step + k // B, sched[k - k % B][2]) for k, (f, _, _) in enumerate(sched)]


def measure(config):
    """The child's work: one engine, one warm-up epoch, FRAMES timed frames."""
    import torch
    import bench
    from loss_fps import make_engine
    if not torch.cuda.is_available():
        raise SystemExit('batch_fps: needs a GPU (there is no CPU path and no CPU number)')
    form, B = config.split('_b')
    B = int(B)
    n = bench.CFG['frames']
    eng = make_engine(bench, 'Fusion6', 'fp16')

    def run(n_frames, first_step):
        eng.set_schedule(entries(bench, n_frames, B, first_step))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if form == 'batched':
            eng.run_batched(n_frames // B, B)
        else:
            eng.run(n_frames, graph=True if form == 'graph' else None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    run(n // B * B, 1)                                       # warm-up epoch (drop_last)
    secs = run(FRAMES, n // B + 1)
    st = eng.stats(FRAMES // B)
    sc = eng.scale_state()
    return {'ms_per_frame': round(1e3 * secs / FRAMES, 4), 'frames_per_s': round(FRAMES / secs, 1),
            'ms_per_optimiser_step': round(1e3 * secs * B / FRAMES, 4), 'mean_psnr_db': round(float(st[:, 4].double().mean()), 3),
            'finite': bool(torch.isfinite(st).all()), 'steps_skipped': sc['skipped'] + sc['late_skipped'],
            'device': torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_fps.json'))
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--child', default=None, help='(internal) measure this one configuration in this process and print its record')
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        print('BATCH_FPS ' + json.dumps(measure(args.child)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    configs = args.configs.split(',')
    res = {'geometry': bench.CONFIGS['720p']['name'], 'precision': 'fp16', 'loss': 'Fusion6', 'warmup_frames': bench.CFG['frames'],
           'timed_frames': FRAMES, 'repeats': REPEATS, 'processes': 'one per configuration and repeat, configurations alternating',
           'results': {c: {'ms_per_frame': [], 'frames_per_s': []} for c in configs}}
    for _ in range(REPEATS):
        for c in configs:
            # a child that fails or overruns its limit ends the measurement: nothing more is started on the GPU behind it
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', c], capture_output=True, text=True, cwd=ROOT, timeout=180)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('BATCH_FPS ')]
            if r.returncode != 0 or not lines:
                raise SystemExit(f'batch_fps: {c} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
            rec = json.loads(lines[-1][len('BATCH_FPS '):])
            res['device'] = rec.pop('device')
            print(f'{c}: {rec["ms_per_frame"]} ms/frame', file=sys.stderr, flush=True)
            out = res['results'][c]
            out['ms_per_frame'].append(rec['ms_per_frame'])
            out['frames_per_s'].append(rec['frames_per_s'])
            out.update({k: rec[k] for k in ('mean_psnr_db', 'finite', 'steps_skipped')})
    for c, out in res['results'].items():
        ms = sorted(out['ms_per_frame'])
        out['median_ms_per_frame'] = ms[len(ms) // 2]
        out['median_frames_per_s'] = round(1e3 / ms[len(ms) // 2], 1)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
