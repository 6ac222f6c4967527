"""Training throughput of the engine at the bench geometry (720p ERB, 132 frames, fp16, the pipelined step) by loss type:

  Fusion6   the bench's loss: one loss launch (k_fusion6 with the target-statistics cache)
  Fusion1   an SSIM-family loss: the same launch with the L2 pixel term
  Fusion10  an MS-SSIM loss: 5 forward level launches + 1 coefficient launch + 5 backward level launches in the step

One fresh process per loss, one after the other (as bench.py measures: the engine's two streams are the first the process creates;
a second engine in the same process shares hardware queues with the first and its pipelined step slows down by 0.2 ms).  Each
process runs one warm-up epoch (132 steps) and is then timed REPEATS times over STEPS steps; a timing is a host clock around one
TrainEngine.run call that ends in a device synchronise.  Prints one JSON document (every repeat, ms/step and frames/s).  There is no
threshold on it: it records what the extra launches cost.

    python tools/loss_fps.py [--out profiles/loss_types_fps.json] [--losses Fusion6,Fusion1,Fusion10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 264
REPEATS = 3
LOSSES = 'Fusion6,Fusion1,Fusion10'


def make_engine(bench, loss_type, precision):
    """bench.make_engine (720p, seed 1234) with another loss type."""
    import torch
    from orn_amd import engine, model, ops
    from orn_amd.data import synthetic_video
    cfg, C = bench.CONFIGS['720p'], bench.CFG
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num=C['stem_dim_num'], fc_hw_dim=cfg['fc_hw_dim'], expansion=C['expansion'],
                          num_blocks=1, norm='none', act='swish', bias=True, reduction=C['reduction'], conv_type='conv',
                          stride_list=cfg['strides'], sin_res=True, lower_width=C['lower_width'], sigmoid=False, deploy=False,
                          branch_type='ERB')
    eng = engine.TrainEngine(gen, loss_type=loss_type, beta=C['beta'], precision=precision)
    n = C['frames']
    frames = synthetic_video(n, cfg['hw'][0], cfg['hw'][1], seed=1234, device=eng.device)
    pos = torch.tensor([float(k) / n for k in range(n)], dtype=torch.float32)
    eng.set_video(frames, ops.pe_forward(pos.to(eng.device), 1.25, 40))
    return eng


def measure(loss_type, precision):
    """The child's work: one engine, warm-up epoch, REPEATS timed runs."""
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('loss_fps: needs a GPU (there is no CPU path and no CPU number)')
    n = bench.CFG['frames']
    eng = make_engine(bench, loss_type, precision)
    eng.set_schedule(bench.schedule(n))                     # one warm-up epoch
    eng.run(n)
    torch.cuda.synchronize()
    done, secs = n, []
    for _ in range(REPEATS):
        eng.set_schedule(bench.schedule(STEPS, start_step=done))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(STEPS)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        done += STEPS
    st = eng.stats(STEPS)
    sc = eng.scale_state()
    ms = sorted(1e3 * t / STEPS for t in secs)
    return {'ms_per_step': [round(1e3 * t / STEPS, 4) for t in secs], 'median_ms_per_step': round(ms[len(ms) // 2], 4),
            'median_frames_per_s': round(1e3 / ms[len(ms) // 2], 1), 'last_run_mean_psnr_db': round(float(st[:, 4].double().mean()), 3),
            'last_run_mean_struct': round(float(st[:, 3].double().mean()), 5), 'finite': bool(torch.isfinite(st).all()),
            'steps_skipped': sc['skipped'] + sc['late_skipped'], 'device': torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--losses', default=LOSSES)
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--child', default=None, help='(internal) measure this one loss in this process and print its record')
    args = ap.parse_args()
    if args.child:
        print('LOSS_FPS ' + json.dumps(measure(args.child, args.precision)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    res = {'geometry': bench.CONFIGS['720p']['name'], 'precision': args.precision, 'form': 'TrainEngine.run (pipelined step)',
           'warmup_steps': bench.CFG['frames'], 'steps': STEPS, 'repeats': REPEATS, 'processes': 'one per loss, sequential', 'results': {}}
    for lt in args.losses.split(','):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', lt, '--precision', args.precision],
                           capture_output=True, text=True, cwd=ROOT)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('LOSS_FPS ')]
        if r.returncode != 0 or not lines:
            raise SystemExit(f'loss_fps: {lt} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        res['results'][lt] = json.loads(lines[-1][len('LOSS_FPS '):])
        res['device'] = res['results'][lt].pop('device')
    base = res['results'].get('Fusion6')
    if base:
        for lt, r in res['results'].items():
            r['ms_over_fusion6'] = round(r['median_ms_per_step'] - base['median_ms_per_step'], 4)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
