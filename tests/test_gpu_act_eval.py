"""The activation functions themselves (csrc/orn_act.h), as the kernels call them: orn_debug_act_eval for swish and gelu, the fast
pair (16-bit kernels) and the exact pair (fp32 path), against fp64 on the CPU -- gelu in its erfc form, 0.5 z erfc(-z / sqrt 2).

Inputs: every finite fp16 bit pattern; every finite bf16 bit pattern with |z| <= 2^7; 2^16 seeded fp32 values in [-12, 12].
Figure, per function: the worst |k - r| / (2^-24 (1 + |z|)).  Bound: 3x the worst value measured on the MI355X (the project's
standing rule), per function in BOUND below with the measured value beside it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SWISH, GELU = 0, 1
# (act, exact) -> (bound on f, bound on df) = 3 x the measured worst, which stands beside it
MEASURED = {
    (SWISH, 0): (2.0231, 1.5578),
    (SWISH, 1): (2.0231, 1.5979),
    (GELU, 0): (1.1395, 1.9552),      # the fast pair is the exact pair
    (GELU, 1): (1.1395, 1.9552),
}
BOUND = {k: (3 * f, 3 * d) for k, (f, d) in MEASURED.items()}


def _inputs():
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.float16).float()
    b = bits.view(torch.bfloat16).float()
    g = torch.Generator().manual_seed(2024)
    return {'fp16': h[torch.isfinite(h)], 'bf16': b[torch.isfinite(b) & (b.abs() <= 128.0)],
            'fp32': (torch.rand(65536, generator=g) * 24.0 - 12.0)}


def _ref(act, z):
    z = z.double()
    if act == SWISH:
        s = torch.sigmoid(z)
        # exp(-z) overflows fp64 sigmoid to exactly 0 below -745: the product is then -0, which is the limit
        return z * s, s * (1.0 + z * (1.0 - s))
    e = torch.special.erfc(-z / math.sqrt(2.0))
    return 0.5 * z * e, 0.5 * e + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _ulp16(r, kind):
    """spacing of the 16-bit format at |r| (subnormal spacing below the smallest normal)"""
    mant, emin = (10, -14) if kind == 'fp16' else (7, -126)
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


@pytest.fixture(scope='module')
def table():
    """{(act, exact, sweep): (z, f, df)} from the device, one launch each; the references are formed once per activation."""
    from orn_amd import _lib
    L = _lib.lib()
    out = {}
    for name, z in _inputs().items():
        zc = z.cuda().contiguous()
        for act in (SWISH, GELU):
            for exact in (0, 1):
                f, df = torch.empty_like(zc), torch.empty_like(zc)
                _lib.check(L.orn_debug_act_eval(act, exact, _lib.ptr(zc), zc.numel(), _lib.ptr(f), _lib.ptr(df), _lib.stream()), 'orn_debug_act_eval')
                torch.cuda.synchronize()
                out[(act, exact, name)] = (z, f.cpu(), df.cpu())
    return out


@pytest.mark.parametrize('exact', [0, 1])
@pytest.mark.parametrize('act', [SWISH, GELU])
def test_against_fp64(table, act, exact):
    worst_f = worst_d = 0.0
    for name in ('fp16', 'bf16', 'fp32'):
        z, f, df = table[(act, exact, name)]
        rf, rd = _ref(act, z)
        assert torch.isfinite(f).all() and torch.isfinite(df).all(), name          # no NaN, no Inf anywhere
        scale = 2.0 ** -24 * (1.0 + z.double().abs())
        ef, ed = ((f.double() - rf).abs() / scale).max().item(), ((df.double() - rd).abs() / scale).max().item()
        print(f'act {act} exact {exact} {name}: worst f {ef:.3f}, df {ed:.3f}  [2^-24 (1 + |z|)]')
        worst_f, worst_d = max(worst_f, ef), max(worst_d, ed)
        if name != 'fp32' and act == GELU:      # what a 16-bit kernel stores: within half an ulp16 of the reference before its own rounding
            # (swish is not held to it: its helpers, unchanged, flush results below 2^-126 -- z < -87 -- to zero; measured 245 bf16 ulps there)
            half = ((f.double() - rf).abs() / _ulp16(rf, name)).max().item()
            print(f'act {act} exact {exact} {name}: worst f error {half:.4f} ulp16(r)')
            assert half <= 0.5, (name, half)
        # structure: the tail towards -inf ends in a zero of either sign, the derivative stays inside its range
        tail = z <= -128.0
        assert (f[tail] == 0).all(), name
        assert df.min().item() >= -0.13 and df.max().item() <= 1.13, (name, df.min().item(), df.max().item())
    print(f'act {act} exact {exact}: worst f {worst_f:.3f} (bound {BOUND[(act, exact)][0]:.2f}), df {worst_d:.3f} (bound {BOUND[(act, exact)][1]:.2f})')
    assert worst_f <= BOUND[(act, exact)][0], worst_f
    assert worst_d <= BOUND[(act, exact)][1], worst_d


def test_swish_is_the_swish_of_before(table):
    """OrnAct<swish> forwards to orn_silu / orn_silu_grad (_exact): gelu and swish differ, and the exact swish is torch's to fp32
    rounding (the helpers themselves are unchanged; the serial == pipelined and engine == engine tests pin the kernels)."""
    z, f, _ = table[(SWISH, 1, 'fp32')]
    assert torch.allclose(f, torch.nn.functional.silu(z), rtol=3e-7, atol=1e-7)
    zg, fg, _ = table[(GELU, 1, 'fp32')]
    assert torch.allclose(fg, torch.nn.functional.gelu(zg.double()).float(), rtol=1e-6, atol=1e-7)
    assert not torch.allclose(f, fg, atol=1e-2)
