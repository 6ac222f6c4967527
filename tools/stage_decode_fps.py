"""Decode rate of every stage of a multi-resolution fit at the bench geometry (720p, 132 frames, ERB, fc 9_16_26, strides 5 2 2 2 2:
stages 45x80, 90x160, 180x320, 360x640, 720x1280), fp16 and fp32: what a preview decode that stops at stage k costs beside the full
decode, and what evaluating every stage in one call costs beside the frame-by-frame eager evaluation.

Rows, per precision:
    last_default        Decoder(model).decode_frames                  the last stage on the default (single-resolution) decoder
    last_stages         Decoder(model, stages=True).decode_frames     the same on the decoder that knows every stage's head
    stage_0 .. stage_4  Decoder(stages=True).decode_stages(stages=k)  stage k alone: the blocks above k and the last head do not run
    all_eval            decode_stages of all stages, stats + MS-SSIM  main_train's / main_eval's per-stage evaluation
    eager_all_eval      (fp32 only) the module forward frame by frame, psnr_fn and msssim_fn over its output list, as
                        main_train.py:378-438 evaluates
The decode rows write bytes and PSNR (rgb8 + stats), decode_frames' defaults.  One fresh process per row, one after the other, each
under its own time limit; one warm-up call, then the median of REPEATS calls, a timing being a host clock around one call that
ends in a device synchronise.  `launches`: kernel and memset launches of one timed call, counted from the entry points' code (the
merge and operand-copy launches of frame 0 are listed apart: `launches_frame0_extra`).  Prints one JSON document; there is no
threshold on it.

    python tools/stage_decode_fps.py [--out profiles/stage_decode_fps.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
N_STAGES = 5
STAGE_ROWS = (45, 90, 180, 360, 720)
ROWS = ('last_default', 'last_stages') + tuple(f'stage_{k}' for k in range(N_STAGES)) + ('all_eval', 'eager_all_eval')
CHILD_TIMEOUT = {'eager_all_eval': 420}


def make_model(bench):
    """bench.make_engine's generator (720p, ERB, seed 1) with a head on every stage, and its synthetic video."""
    import torch
    from orn_amd import model, ops
    from orn_amd.data import synthetic_video
    cfg, C = bench.CONFIGS['720p'], bench.CFG
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num=C['stem_dim_num'], fc_hw_dim=cfg['fc_hw_dim'], expansion=C['expansion'],
                          num_blocks=1, norm='none', act='swish', bias=True, reduction=C['reduction'], conv_type='conv',
                          stride_list=cfg['strides'], sin_res=False, lower_width=C['lower_width'], sigmoid=False, deploy=False,
                          branch_type='ERB').cuda()
    n = C['frames']
    frames = synthetic_video(n, cfg['hw'][0], cfg['hw'][1], seed=1234, device='cuda')
    pos = torch.tensor([float(k) / n for k in range(n)], dtype=torch.float32)
    return gen, frames, ops.pe_forward(pos.cuda(), 1.25, 40)


def launches(row, precision, n, chunk=8):
    """(launches of one call, how many of them are frame 0's alone), read off orn_engine_forward.hip for this geometry.  Per frame:
    the stem's two linear launches; one conv launch per block up to the top stage -- a 16-bit multi-resolution engine runs its first
    block (26 channels) in fp32 and converts its output to channels-last, one more launch once a second block runs; the default
    16-bit decoder runs its first two blocks as one launch; one output launch per wanted 16-bit stage, two (head, planar output) per
    wanted stage of an fp32 block.  Per call: one memset for the ticket; six MS-SSIM launches per chunk of 8 frames and per stage more
    than 160 rows high.  Frame 0 merges: a W2 transpose and two grouped merge launches that carry the stem's linear layers, one
    launch more than the two linear launches they replace."""
    if row == 'eager_all_eval':
        return None, None
    half = precision != 'fp32'
    multi = row != 'last_default'
    top = N_STAGES - 1 if row in ('last_default', 'last_stages', 'all_eval') else int(row.split('_')[1])
    convs = top + 1
    if half and multi and top >= 1:
        convs += 1
    if half and not multi:
        convs -= 1
    wanted = range(N_STAGES) if row == 'all_eval' else [top]
    outs = sum(1 if (half and s >= 1) else 2 for s in wanted)
    total = 1 + n * (2 + convs + outs) + 1
    if row == 'all_eval':
        total += 6 * sum(1 for h in STAGE_ROWS if h > 160) * ((n + chunk - 1) // chunk)
    return total, 1


def measure(row, precision):
    import torch
    import bench
    from orn_amd import engine, utils
    if not torch.cuda.is_available():
        raise SystemExit('stage_decode_fps: needs a GPU (there is no CPU path and no CPU number)')
    gen, frames, embeds = make_model(bench)
    n = frames.shape[0]
    rec = {}
    if row == 'eager_all_eval':
        hws = engine.stage_hw(gen)
        targets = [frames if tuple(hw) == tuple(frames.shape[2:]) else torch.nn.functional.adaptive_avg_pool2d(frames, hw) for hw in hws]

        def call():
            ps, ms = [], []
            with torch.no_grad():
                for k in range(n):
                    outs = gen(embeds[k:k + 1])
                    tg = [t[k:k + 1] for t in targets]
                    ps.append(utils.psnr_fn(outs, tg))
                    ms.append(utils.msssim_fn(outs, tg))
            return torch.cat(ps).mean(0)
    else:
        dec = engine.Decoder(gen, precision=precision, stages=row != 'last_default')
        tabs = dec.stage_targets(frames)
        rec['stages'] = [list(hw) for hw in dec.stage_hw()]
        if row.startswith('last_'):
            def call():
                return dec.decode_frames(embeds=embeds, frames=frames)['stats'][:, 1].mean()
        elif row == 'all_eval':
            def call():
                out = dec.decode_stages(embeds=embeds, frames=[tabs[s] for s in range(N_STAGES)], rgb8=False, stats=True, msssim=True)
                return torch.stack([out[s]['stats'][:, 1].mean() for s in range(N_STAGES)])
        else:
            k = int(row.split('_')[1])

            def call():
                return dec.decode_stages(stages=k, embeds=embeds, frames=[tabs[k]])[k]['stats'][:, 1].mean()
    call()                                                  # warm-up
    torch.cuda.synchronize()
    secs = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val = call()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    ms = sorted(1e3 * t for t in secs)
    total, extra = launches(row, precision, n)
    if row.startswith('stage_') and k < N_STAGES - 1:
        # (untimed) block k's conv fills no next-block buffer when the forward stops there, and the conv launcher may then pick another
        # kernel form: are the bytes those of stage k decoded beside the last stage?
        alone = dec.decode_stages(stages=k, embeds=embeds, frames=[tabs[k]])[k]
        beside = dec.decode_stages(stages=[k, N_STAGES - 1], embeds=embeds, frames=[tabs[k], tabs[N_STAGES - 1]])[k]
        rec['bytes_equal_beside_last_stage'] = bool(torch.equal(alone['rgb8'], beside['rgb8']))
        rec['max_byte_difference_beside_last_stage'] = int((alone['rgb8'].int() - beside['rgb8'].int()).abs().max())
    rec.update({'ms_per_call': [round(1e3 * t, 3) for t in secs], 'median_ms_per_call': round(ms[len(ms) // 2], 3),
                'median_frames_per_s': round(n / (ms[len(ms) // 2] * 1e-3), 1), 'frames': n,
                'mean_psnr_db': [round(float(v), 3) for v in val.reshape(-1)], 'launches': total, 'launches_frame0_extra': extra,
                'device': torch.cuda.get_device_name(0)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--precisions', default='fp16,fp32')
    ap.add_argument('--child', default=None, help='(internal) ROW -- measure this one in this process and print its record')
    ap.add_argument('--precision', default='fp16', help='(internal) the child\'s precision')
    args = ap.parse_args()
    if args.child:
        print('STAGE_DECODE_FPS ' + json.dumps(measure(args.child, args.precision)), flush=True)
        return
    import subprocess
    import bench                                            # (imports no torch: this process never opens the GPU)
    res = {'geometry': bench.CONFIGS['720p']['name'] + ', a head on every stage (sin_res=False)', 'block': 'ERB (train-mode model: merged for frame 0 of '
           'every call)', 'frames': bench.CFG['frames'], 'outputs': 'rgb8 + stats (decode rows); stats + MS-SSIM (evaluation rows)',
           'warmup_calls': 1, 'repeats': REPEATS, 'processes': 'one per row, sequential, each under its own time limit',
           'not_measured': 'the split of a call by kernel (no profiler run); launch counts are read off the code, not traced', 'results': {}}
    for prec in args.precisions.split(','):
        res['results'][prec] = {}
        for row in ROWS:
            if row == 'eager_all_eval' and prec != 'fp32':
                continue                                    # the module forward is fp32 whatever the engine's precision
            cmd = ['timeout', '-k', '10', str(CHILD_TIMEOUT.get(row, 180)), sys.executable, os.path.abspath(__file__), '--child', row,
                   '--precision', prec]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('STAGE_DECODE_FPS ')]
            if r.returncode != 0 or not lines:      # (a child that failed may have faulted the device: nothing more is started)
                raise SystemExit(f'stage_decode_fps: {prec} {row} failed (rc={r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
            rec = json.loads(lines[-1][len('STAGE_DECODE_FPS '):])
            res['device'] = rec.pop('device')
            res['results'][prec][row] = rec
            print(f'{prec} {row}: {rec["median_ms_per_call"]} ms per call, {rec["median_frames_per_s"]} frames/s', file=sys.stderr, flush=True)
        rows = res['results'][prec]
        full = rows['last_stages']['median_ms_per_call']
        res['results'][prec]['ratio_to_full_decode'] = {f'stage_{k}': round(rows[f'stage_{k}']['median_ms_per_call'] / full, 4)
                                                        for k in range(N_STAGES)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
