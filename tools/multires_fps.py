"""Step time of the engine at the bench geometry (720p, 132 frames, ERB, fp16, Fusion6) with a head and a loss at every stage
(Generator(sin_res=False), lw = 1) beside the single-resolution step: what four side heads, four more Fusion6 launches and their
finalizes, and the first block kept apart from the second cost.

Both rows are hipGraph replays of the SERIAL step (TrainEngine.run(graph=True)); a multi-resolution engine has no pipelined form.  The
procedure of tools/branch_fps.py: one fresh process per row, one after the other; each runs one warm-up epoch (132 steps) and is then
timed REPEATS times over STEPS steps, a timing being a host clock around one TrainEngine.run call that ends in a device
synchronise.  No target-statistics cache is set for either row (target_cache=False): the side stages' tables would otherwise be
filtered once per video and the rows would differ in more than the heads.  Prints one JSON document; there is no threshold on it.

    python tools/multires_fps.py [--out profiles/multires_fps.json]
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
ROWS = ('single_res', 'multi_res')


def make_engine(bench, multi, precision):
    """bench.make_engine (720p, ERB, seed 1234) with or without a head on every stage."""
    import torch
    from orn_amd import engine, model, ops
    from orn_amd.data import synthetic_video
    cfg, C = bench.CONFIGS['720p'], bench.CFG
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num=C['stem_dim_num'], fc_hw_dim=cfg['fc_hw_dim'], expansion=C['expansion'],
                          num_blocks=1, norm='none', act='swish', bias=True, reduction=C['reduction'], conv_type='conv',
                          stride_list=cfg['strides'], sin_res=not multi, lower_width=C['lower_width'], sigmoid=False, deploy=False,
                          branch_type='ERB')
    eng = engine.TrainEngine(gen, loss_type='Fusion6', beta=C['beta'], precision=precision, target_cache=False, lw=1.0)
    n = C['frames']
    frames = synthetic_video(n, cfg['hw'][0], cfg['hw'][1], seed=1234, device=eng.device)
    pos = torch.tensor([float(k) / n for k in range(n)], dtype=torch.float32)
    eng.set_video(frames, ops.pe_forward(pos.to(eng.device), 1.25, 40))
    return eng


def measure(row, precision):
    """The child's work: one engine, warm-up epoch, REPEATS timed runs."""
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('multires_fps: needs a GPU (there is no CPU path and no CPU number)')
    n = bench.CFG['frames']
    eng = make_engine(bench, row == 'multi_res', precision)
    eng.set_schedule(bench.schedule(n))                     # one warm-up epoch
    eng.run(n, graph=True)
    torch.cuda.synchronize()
    done, secs = n, []
    for _ in range(REPEATS):
        eng.set_schedule(bench.schedule(STEPS, start_step=done))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(STEPS, graph=True)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        done += STEPS
    st = eng.stats(STEPS)
    sc = eng.scale_state()
    ms = sorted(1e3 * t / STEPS for t in secs)
    rec = {'ms_per_step': [round(1e3 * t / STEPS, 4) for t in secs], 'median_ms_per_step': round(ms[len(ms) // 2], 4),
           'median_frames_per_s': round(1e3 / ms[len(ms) // 2], 1),
           'params_M': round(sum(p.numel() for p in eng.model.parameters()) / 1e6, 3),
           'last_run_mean_psnr_db': round(float(st[:, 4].double().mean()), 3), 'finite': bool(torch.isfinite(st).all()),
           'steps_skipped': sc['skipped'] + sc['late_skipped'], 'device': torch.cuda.get_device_name(0)}
    if eng.multi_res:
        rec['stages'] = [list(hw) for hw in eng.stage_hw()]
        rec['last_run_mean_psnr_db_per_stage'] = [round(float(v), 3) for v in eng.stage_stats(STEPS)[:, :, 1].double().mean(dim=0)]
        # per side stage: head forward, loss, loss finalize, head backward, its dW / db finish; and one record launch per step
        rec['launches_per_side_stage'], rec['launches_per_step_added'] = 5, 5 * (len(rec['stages']) - 1) + 1
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--child', default=None, help='(internal) ROW -- measure this one in this process and print its record')
    args = ap.parse_args()
    if args.child:
        print('MULTIRES_FPS ' + json.dumps(measure(args.child, args.precision)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    res = {'geometry': bench.CONFIGS['720p']['name'], 'precision': args.precision, 'loss': 'Fusion6', 'block': 'ERB', 'lw': 1.0,
           'step_form': 'hipGraph replay of the serial step', 'target_stats_cache': False, 'warmup_steps': bench.CFG['frames'],
           'steps': STEPS, 'repeats': REPEATS, 'processes': 'one per row, sequential',
           'not_measured': 'the split of the added time by kernel (no profiler run); the pipelined single-resolution step '
                           '(TrainEngine.run(), bench.py) is not a row here: a multi-resolution engine has no such form',
           'results': {}}
    for row in ROWS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', row, '--precision', args.precision],
                           capture_output=True, text=True, cwd=ROOT, timeout=240)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('MULTIRES_FPS ')]
        if r.returncode != 0 or not lines:          # (a child that failed may have faulted the device: nothing more is started)
            raise SystemExit(f'multires_fps: {row} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        rec = json.loads(lines[-1][len('MULTIRES_FPS '):])
        res['device'] = rec.pop('device')
        res['results'][row] = rec
    res['multi_over_single_ms'] = round(res['results']['multi_res']['median_ms_per_step'] - res['results']['single_res']['median_ms_per_step'], 4)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
