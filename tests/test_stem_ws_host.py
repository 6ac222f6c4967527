"""Host checks of the stem backward's workspace size (no GPU): orn_stem_bwd_ws_bytes is exported, covers what the kernels write
for every (B, Hd, Nout) -- at B == 1 one row of Hd partial sums per 16 outputs, more than the 256 rows of the batched form from
Nout = 4097 on -- and ops.StemFn sizes its workspace from it (tests/test_gpu_stage0.py runs the kernels against a guarded
workspace of exactly that size)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def orn():
    import orn_amd
    from orn_amd import _build
    _build.build()
    return orn_amd


def test_stem_bwd_ws_bytes_is_exported(orn):
    assert 'orn_stem_bwd_ws_bytes' in orn._lib.EXPORTS
    assert hasattr(orn._lib.lib(), 'orn_stem_bwd_ws_bytes')
    assert 'orn_stem_bwd_ws_bytes' in open(os.path.join(ROOT, 'include', 'orn.h')).read()


def test_stem_bwd_ws_bytes_covers_every_row_the_kernels_write(orn):
    L = orn._lib.lib()
    for B in (1, 2, 3, 16):
        for Hd in (1, 8, 32, 300, 512):
            for Nout in (1, 15, 16, 17, 3744, 4096, 4097, 4112, 6912, 65536):
                rows = max(256, -(-Nout // 16))
                need = 4 * (B * Nout + 2 * B * Hd + rows * B * Hd)
                got = L.orn_stem_bwd_ws_bytes(B, Hd, Nout)
                assert got >= need and got % 4 == 0, (B, Hd, Nout, got, need)
    assert L.orn_stem_bwd_ws_bytes(0, 8, 16) == 0 and L.orn_stem_bwd_ws_bytes(1, 0, 16) == 0 and L.orn_stem_bwd_ws_bytes(1, 8, -1) == 0


def test_stem_fn_sizes_its_workspace_from_the_library(orn):
    src = open(os.path.join(os.path.dirname(orn._lib.__file__), 'ops.py')).read()
    assert '256 * B * Hd' not in src
    assert 'orn_stem_bwd_ws_bytes' in src
