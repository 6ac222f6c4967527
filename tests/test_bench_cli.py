"""bench.py's own options: a plain run prints the headline line only, --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), capture_output=True, text=True,
                         timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS='1'))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_stub_run_is_the_headline_leg_only(tmp_path):
    """--steps sets the timed steps, ms_per_step is the time of one of them, and the legs of --full stay out of a plain run."""
    d = _bench('--cpu-stub', '--steps', '5', '--warmup', '2', '--dump-outputs', str(tmp_path / 'out'))
    assert d['steps'] == 5 and d['warmup'] == 2 and d['n_gpus'] == 1
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in d, k
    assert abs(d['ms_per_step'] - 1e3 / d['value']) < 1e-9 * d['ms_per_step']
    assert not {'roofline', 'sustained', 'cfg3_1080p', 'fp32', 'cpu_baseline'} & set(d)
    stats = np.load(tmp_path / 'out' / 'last_step_stats.npy')
    assert stats.dtype == np.float32 and stats.shape == (8,)


@pytest.mark.gpu
def test_dump_outputs_of_a_plain_gpu_run(tmp_path):
    """The arrays the timed path hands back after its last step: the whole parameter arena (each tensor padded to 256 B), a fixed
    sample of both Adam moments, the stats row the JSON line's witnesses come from -- float32, finite, 64 MB at most."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from orn_amd import engine, model
    out = tmp_path / 'out'
    d = _bench('--steps', '3', '--warmup', '1', '--burn-in', '0', '--dump-outputs', str(out))
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and 'roofline' not in d
    a = {n: np.load(out / f'{n}.npy') for n in ('params', 'adam_m_sample', 'adam_v_sample', 'last_step_stats')}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    torch.manual_seed(1)
    gen = model.Generator(embed_length=80, stem_dim_num='512_1', fc_hw_dim='9_16_26', expansion=1, num_blocks=1, norm='none',
                          act='swish', bias=True, reduction=2, conv_type='conv', stride_list=[5, 2, 2, 2, 2], sin_res=True,
                          lower_width=96, sigmoid=False, deploy=False, branch_type='ERB')
    layout, total = engine.arena_layout([(k, tuple(p.shape)) for k, p in gen.named_parameters()])
    assert a['params'].shape == (total,) and sum(n for _, n in layout.values()) == 7576025
    assert a['adam_m_sample'].shape == a['adam_v_sample'].shape == (bench.DUMP_SAMPLE,)
    assert (a['adam_v_sample'] >= 0).all() and (a['adam_v_sample'] > 0).any()
    assert sum(os.path.getsize(out / f'{n}.npy') for n in a) <= 64 << 20
    st = a['last_step_stats']
    assert st[0] == np.float32(d['config']['last_timed_step_loss'])
    assert int(st[7]) == d['config']['last_timed_step_adam_count']
