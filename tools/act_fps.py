"""Step time of the engine at the bench geometry (720p, 132 frames, ERB, fp16, Fusion6) by block activation (--act): what the GELU
epilogues (erfc per activation element in the forward convs' activation copy, in the dgrad epilogues and in the head) cost beside swish.

Two forms per activation:
  graph   hipGraph replay of the SERIAL step (TrainEngine.run(graph=True))
  run     TrainEngine.run(): plain stream launches, pipelined over the engine's second stream

The procedure of tools/branch_fps.py: one fresh process per (activation, form), one after the other; each runs one warm-up epoch (132
steps) and is then timed REPEATS times over STEPS steps, a timing being a host clock around one TrainEngine.run call that ends in a
device synchronise.  Prints one JSON document (every repeat, ms/step, frames/s).  There is no threshold on it.

    python tools/act_fps.py [--out profiles/act_fps.json] [--acts swish,gelu]
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
ACTS = 'swish,gelu'
FORMS = ('graph', 'run')


def make_engine(bench, act, precision):
    """bench.make_engine (720p, ERB, seed 1234) with the given activation."""
    import torch
    from orn_amd import engine, model, ops
    from orn_amd.data import synthetic_video
    cfg, C = bench.CONFIGS['720p'], bench.CFG
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num=C['stem_dim_num'], fc_hw_dim=cfg['fc_hw_dim'], expansion=C['expansion'],
                          num_blocks=1, norm='none', act=act, bias=True, reduction=C['reduction'], conv_type='conv',
                          stride_list=cfg['strides'], sin_res=True, lower_width=C['lower_width'], sigmoid=False, deploy=False,
                          branch_type='ERB')
    eng = engine.TrainEngine(gen, loss_type='Fusion6', beta=C['beta'], precision=precision)
    n = C['frames']
    frames = synthetic_video(n, cfg['hw'][0], cfg['hw'][1], seed=1234, device=eng.device)
    pos = torch.tensor([float(k) / n for k in range(n)], dtype=torch.float32)
    eng.set_video(frames, ops.pe_forward(pos.to(eng.device), 1.25, 40))
    return eng


def measure(act, form, precision):
    """The child's work: one engine, warm-up epoch, REPEATS timed runs."""
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('act_fps: needs a GPU (there is no CPU path and no CPU number)')
    graph = {'graph': True, 'run': None}[form]
    n = bench.CFG['frames']
    eng = make_engine(bench, act, precision)
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
    pipelined = form == 'run' and precision != 'fp32'
    return {'step_form': 'pipelined' if pipelined else 'serial', 'ms_per_step': [round(1e3 * t / STEPS, 4) for t in secs],
            'median_ms_per_step': round(ms[len(ms) // 2], 4), 'median_frames_per_s': round(1e3 / ms[len(ms) // 2], 1),
            'params_M': round(sum(p.numel() for p in eng.model.parameters()) / 1e6, 3),
            'last_run_mean_psnr_db': round(float(st[:, 4].double().mean()), 3), 'finite': bool(torch.isfinite(st).all()),
            'steps_skipped': sc['skipped'] + sc['late_skipped'], 'device': torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--acts', default=ACTS)
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--child', default=None, help='(internal) ACT:FORM -- measure this one in this process and print its record')
    args = ap.parse_args()
    if args.child:
        act, form = args.child.split(':')
        print('ACT_FPS ' + json.dumps(measure(act, form, args.precision)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    res = {'geometry': bench.CONFIGS['720p']['name'], 'precision': args.precision, 'branch_type': 'ERB', 'loss': 'Fusion6', 'warmup_steps': bench.CFG['frames'],
           'steps': STEPS, 'repeats': REPEATS, 'processes': 'one per (act, form), sequential', 'results': {}}
    for act in args.acts.split(','):
        res['results'][act] = {}
        for form in FORMS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', f'{act}:{form}', '--precision', args.precision],
                               capture_output=True, text=True, cwd=ROOT, timeout=240)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('ACT_FPS ')]
            if r.returncode != 0 or not lines:          # (a child that failed may have faulted the device: nothing more is started)
                raise SystemExit(f'act_fps: {act} {form} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
            rec = json.loads(lines[-1][len('ACT_FPS '):])
            res['device'] = rec.pop('device')
            res['results'][act][form] = rec
    sw = res['results'].get('swish')
    if sw:
        for act, forms in res['results'].items():
            for form in FORMS:
                forms[form]['ms_over_swish'] = round(forms[form]['median_ms_per_step'] - sw[form]['median_ms_per_step'], 4)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
