"""Step time of the engine at the bench geometry (720p, 132 frames, fp16, Fusion6) by block kind: what the online merge of the paper's
comparison blocks costs beside the single conv of NeRV_vanilla and beside ERB.

  NeRV_vanilla  one 3x3 conv per block, no merge
  ACB, RepVGG   the merge is elementwise: one forward launch, one backward launch (orn_merge_lin.hip)
  ECB           the same launches with the 1x1 -> 3x3 product and its two gradients inside, and a small second backward launch
  ERB           the grouped-GEMM merge of orn_merge.hip / orn_merge_h16.hip

Two forms per kind:
  graph   hipGraph replay of the SERIAL step (TrainEngine.run(graph=True)): the same launches in the same order for every kind
  run     TrainEngine.run(): plain stream launches, PIPELINED over the engine's second stream where the engine can (NeRV_vanilla and
          ERB in a 16-bit mode), serial otherwise (ACB, RepVGG, ECB have no pipelined form)

The procedure of tools/loss_fps.py: one fresh process per (kind, form), one after the other (an engine's streams are the first the
process creates); each runs one warm-up epoch (132 steps) and is then timed REPEATS times over STEPS steps, a timing being a host clock
around one TrainEngine.run call that ends in a device synchronise.  Prints one JSON document (every repeat, ms/step, frames/s).  There
is no threshold on it.

    python tools/branch_fps.py [--out profiles/branch_kinds_fps.json] [--kinds NeRV_vanilla,ACB,RepVGG,ECB,ERB]
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
KINDS = 'NeRV_vanilla,ACB,RepVGG,ECB,ERB'
FORMS = ('graph', 'run')


def make_engine(bench, kind, precision):
    """bench.make_engine (720p, seed 1234) with another block kind."""
    import torch
    from orn_amd import engine, model, ops
    from orn_amd.data import synthetic_video
    cfg, C = bench.CONFIGS['720p'], bench.CFG
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num=C['stem_dim_num'], fc_hw_dim=cfg['fc_hw_dim'], expansion=C['expansion'],
                          num_blocks=1, norm='none', act='swish', bias=True, reduction=C['reduction'], conv_type='conv',
                          stride_list=cfg['strides'], sin_res=True, lower_width=C['lower_width'], sigmoid=False, deploy=False,
                          branch_type=kind)
    eng = engine.TrainEngine(gen, loss_type='Fusion6', beta=C['beta'], precision=precision)
    n = C['frames']
    frames = synthetic_video(n, cfg['hw'][0], cfg['hw'][1], seed=1234, device=eng.device)
    pos = torch.tensor([float(k) / n for k in range(n)], dtype=torch.float32)
    eng.set_video(frames, ops.pe_forward(pos.to(eng.device), 1.25, 40))
    return eng


def measure(kind, form, precision):
    """The child's work: one engine, warm-up epoch, REPEATS timed runs."""
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('branch_fps: needs a GPU (there is no CPU path and no CPU number)')
    graph = {'graph': True, 'run': None}[form]
    n = bench.CFG['frames']
    eng = make_engine(bench, kind, precision)
    eng.set_schedule(bench.schedule(n))                     # one warm-up epoch
    eng.run(n, graph=graph)
    torch.cuda.synchronize()
    done, secs = n, []
    for _ in range(REPEATS):
        eng.set_schedule(bench.schedule(STEPS, start_step=done))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(STEPS, graph=graph)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        done += STEPS
    st = eng.stats(STEPS)
    sc = eng.scale_state()
    ms = sorted(1e3 * t / STEPS for t in secs)
    pipelined = form == 'run' and precision != 'fp32' and kind in ('NeRV_vanilla', 'ERB')
    return {'step_form': 'pipelined' if pipelined else 'serial', 'ms_per_step': [round(1e3 * t / STEPS, 4) for t in secs],
            'median_ms_per_step': round(ms[len(ms) // 2], 4), 'median_frames_per_s': round(1e3 / ms[len(ms) // 2], 1),
            'params_M': round(sum(p.numel() for p in eng.model.parameters()) / 1e6, 3),
            'last_run_mean_psnr_db': round(float(st[:, 4].double().mean()), 3), 'finite': bool(torch.isfinite(st).all()),
            'steps_skipped': sc['skipped'] + sc['late_skipped'], 'device': torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--kinds', default=KINDS)
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--child', default=None, help='(internal) KIND:FORM -- measure this one in this process and print its record')
    args = ap.parse_args()
    if args.child:
        kind, form = args.child.split(':')
        print('BRANCH_FPS ' + json.dumps(measure(kind, form, args.precision)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    res = {'geometry': bench.CONFIGS['720p']['name'], 'precision': args.precision, 'loss': 'Fusion6', 'warmup_steps': bench.CFG['frames'],
           'steps': STEPS, 'repeats': REPEATS, 'processes': 'one per (kind, form), sequential', 'results': {}}
    for kind in args.kinds.split(','):
        res['results'][kind] = {}
        for form in FORMS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', f'{kind}:{form}', '--precision', args.precision],
                               capture_output=True, text=True, cwd=ROOT, timeout=240)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('BRANCH_FPS ')]
            if r.returncode != 0 or not lines:          # (a child that failed may have faulted the device: nothing more is started)
                raise SystemExit(f'branch_fps: {kind} {form} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
            rec = json.loads(lines[-1][len('BRANCH_FPS '):])
            res['device'] = rec.pop('device')
            res['results'][kind][form] = rec
    van = res['results'].get('NeRV_vanilla', {}).get('graph')
    if van:
        for kind, forms in res['results'].items():
            forms['graph']['ms_over_vanilla_serial'] = round(forms['graph']['median_ms_per_step'] - van['median_ms_per_step'], 4)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
