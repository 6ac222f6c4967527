"""Time of bringing a video's frames onto the device as the engine's fp32 [n,3,h,w] target table: 132 frames held as uint8 HWC
arrays in host memory (what PIL hands over; the PNG decode is not counted), 720p target, one process:

  a  the path before orn_frames_ingest_u8: ToTensor per frame on the host (uint8 -> fp32, / 255), stack, one fp32 upload
  b  uint8 upload in chunks of CHUNK frames + orn_frames_ingest_u8 at identity size (FrameDir.load's device path)
  c  the same from 1080p sources pooled to 720p (adaptive_avg_pool2d, windows of 2 x 2)

Every variant is warmed up, then timed REPEATS times, the variants alternating inside a repeat; a timing is a host clock around
one load that ends in a device synchronise.  The kernel alone (sources resident, all frames in one launch) is timed with device
events around LAUNCHES back-to-back launches; its bytes are those the algorithm needs, from the shapes: every source byte once,
every output float once (365 MB / 821 MB in, 1.46 GB out: far beyond the Infinity Cache).  Prints one JSON document.

    python tools/ingest_time.py [--out profiles/ingest.json]
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
LAUNCHES = 10
CHUNK = 16
TARGET = (720, 1280)
SOURCES = {'b': (720, 1280), 'c': (1080, 1920)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, default=FRAMES)
    args = ap.parse_args()
    import numpy as np
    import torch
    import orn_amd  # noqa: F401
    from orn_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('ingest_time: needs a GPU (there is no CPU path and no CPU number)')
    n, (h, w) = args.frames, TARGET
    rng = np.random.RandomState(1234)
    host = {v: [rng.randint(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8) for _ in range(n)] for v, hw in SOURCES.items()}
    keep = {}

    def va():
        frames = torch.stack([torch.from_numpy(a).permute(2, 0, 1).float().div(255.0) for a in host['b']]).contiguous()
        keep['a'] = frames.to('cuda')

    def chunked(v):
        out = torch.empty(n, 3, h, w, device='cuda')
        for k0 in range(0, n, CHUNK):
            u8 = torch.from_numpy(np.stack(host[v][k0:k0 + CHUNK])).to('cuda')
            ops.ingest_frames(u8, TARGET, out=out[k0:k0 + u8.shape[0]])
        keep[v] = out

    variants = {'a': va, 'b': lambda: chunked('b'), 'c': lambda: chunked('c')}
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    same = bool(torch.equal(keep['a'], keep['b']))
    secs = {v: [] for v in variants}
    for _ in range(REPEATS):
        for v, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            secs[v].append(round(time.perf_counter() - t0, 4))
    keep.clear()
    torch.cuda.empty_cache()

    kernel = {}
    out = torch.empty(n, 3, h, w, device='cuda')
    for v, hw in SOURCES.items():
        u8 = torch.from_numpy(np.stack(host[v])).to('cuda')
        nbytes = u8.numel() + out.numel() * 4
        ops.ingest_frames(u8, TARGET, out=out)                         # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _k in range(LAUNCHES):
                ops.ingest_frames(u8, TARGET, out=out)
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1) / LAUNCHES, 4))
        med = sorted(ms)[len(ms) // 2]
        kernel[v] = {'source': list(hw), 'bytes_read': u8.numel(), 'bytes_written': out.numel() * 4, 'ms_per_launch': ms,
                     'median_ms': med, 'gb_per_s': round(nbytes / (med * 1e-3) / 1e9, 1)}
        del u8
    med = {v: sorted(x)[len(x) // 2] for v, x in secs.items()}
    res = {'frames': n, 'target': list(TARGET), 'chunk': CHUNK, 'repeats': REPEATS, 'device': torch.cuda.get_device_name(0),
           'variants': {'a': 'host ToTensor + stack + one fp32 upload (720p sources)',
                        'b': 'uint8 upload in chunks + orn_frames_ingest_u8, 720p sources (identity size)',
                        'c': 'uint8 upload in chunks + orn_frames_ingest_u8, 1080p sources pooled to 720p'},
           'load_seconds': secs, 'load_median_seconds': med, 'a_over_b': round(med['a'] / med['b'], 2),
           'b_equals_a_bit_for_bit': same,
           'kernel_alone': {'launches_per_timing': LAUNCHES, 'what': 'orn_frames_ingest_u8, all frames resident, one launch', **kernel}}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
