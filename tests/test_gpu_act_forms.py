"""Every kernel form that evaluates the activation, elementwise against fp64 with act = GELU.

The rules are those of test_gpu_conv16_forms.py, test_gpu_conv32_forms.py, test_gpu_head16.py, test_gpu_side_head.py and
test_gpu_stage0.py, unchanged, and so is their code: this module runs THEIR case runners and checks -- the fp64 reference from the
identical rounded operands, ulp16(r) + c A for 16-bit outputs and c A for fp32 outputs, the guards, rings and NaN-seeded slack -- with
three things replaced for the duration of a test (apply_gelu):
  - the library handle: every entry that has an `_act` twin is called through the twin with ORN_ACT_GELU;
  - the reference's activation: gelu(z) = 0.5 z erfc(-z / sqrt 2) and its derivative, in the dtype they are given;
  - the constants: c (and n, the fp32 ulps of the forward epilogue) per form and build, from the tables below.
Differences from those files, as the activation demands: the gain on apad is 1.13 (|gelu'| <= 1.129) where it is 1.1 for swish; the
allowance for the fp32 evaluation of act'(z) keeps its form e (1 + |z|) |dx| with e = 3 x 1.9552 x 2^-24, three times what
tests/test_gpu_act_eval.py measured for gelu's df (swish: 2^-20, and in test_gpu_stage0.py 2^-20 times the sigmoid).

Constants.  conv16, conv32, stage 0: 3x the worst ratio measured with GELU on an MI355X over the cases of this module (those files'
rule: at most 3x), the measured value beside each.  Forms of those modules that evaluate no activation and are not run here have no
entry.  head16 and side heads: the next power of two at least twice the worst ratio measured at constant 1, those files' rule.
Where GELU reads above what swish measured, the entry says so.  One figure stands out and is GELU's, not a kernel's: the fp32 forward
epilogue measured in fp32 ulps of a = gelu(z) reads 165 (8-row tiles, s = 2) where swish reads 2.4 -- deep in the negative tail a is
tiny and erfc's argument rounding, relative 2 x^2 2^-24 at x = z / sqrt 2, is all of it; the absolute error there stays what the sweep
of test_gpu_act_eval.py found, 1.14 x 2^-24 (1 + |z|).
Each case prints its ratios before it asserts, and the last test prints the worst per form.
Cases: the smallest shapes that still reach each form (the product shapes stay with the swish modules)."""
import math

import pytest
import torch

import conv32_cases as K
import test_gpu_conv16_forms as c16
import test_gpu_conv32_forms as c32
import test_gpu_head16 as h16
import test_gpu_side_head as sh
import test_gpu_stage0 as s0

pytestmark = pytest.mark.gpu

GELU = 1
E_DF = 3 * 1.9552 * 2.0 ** -24          # allowance per unit of (1 + |z|) |dx| for the evaluation of gelu'(z)
GAIN_APAD = 1.13

# ---- c per form and build: 3x the worst measured with GELU (MI355X, this module's cases) ---------------------------------------
C16_TOL = {                                                    # measured bf16 / fp16
    'fwd':          {'bf16': 1.4e-7, 'fp16': 2.9e-7},          # 4.58e-8 / 9.45e-8
    'fwd2':         {'bf16': 1.7e-7, 'fp16': 2.3e-7},          # 5.58e-8 / 7.44e-8
    'dgrad2':       {'bf16': 1.1e-7, 'fp16': 2.4e-7},          # 3.59e-8 / 7.78e-8 (fp16: above swish's 3.57e-8, below its c of 1.0e-7)
    'dgrad_split':  {'bf16': 1.8e-8, 'fp16': 2.1e-8},          # 5.75e-9 / 6.89e-9
}
C32_TOL = {
    'fwd_small_s2':      2.7e-7,     # 8.99e-8
    'fwd_small_gen':     2.2e-7,     # 7.30e-8
    'fwd_8row_s2':       1.9e-6,     # 6.15e-7
    'fwd_8row_gen':      8.6e-7,     # 2.83e-7
    'dgrad_small':       5.5e-7,     # 1.81e-7
    'dgrad_small_split': 4.7e-7,     # 1.55e-7
    'dgrad_8row_split':  1.0e-6,     # 3.31e-7
    'dgrad_8row_tail':   1.1e-6,     # 3.66e-7
    'dgrad_8row_plain':  1.6e-6,     # 5.05e-7 (above swish's 3.89e-7, below its c of 1.1e-6)
    'wgrad1':            3.9e-7,     # 1.29e-7
    'wgrad2':            5.4e-7,     # 1.80e-7
    'dbias':             1.3e-7,     # 4.22e-8
    'head_dx':           7.5e-7,     # 2.50e-7
    'head_dwf':          4.5e-7,     # 1.49e-7 (above swish's 1.20e-7 and its c of 3.6e-7)
    'head_dbf':          1.7e-7,     # 5.45e-8 (above swish's 5.31e-8 and its c of 1.5e-7)
    'head_dw':           1.2e-7,     # 3.71e-8
    'head_db':           8.1e-8,     # 2.69e-8
    'head_chain':        1.6e-7,     # 5.17e-8
    'headz':             0.0,        # 0: all of the difference lies inside the n ulps below (2.22 of 4.0)
}
# n (fp32 ulps of a) of the GELU epilogue per forward form, same rule (docstring: the tail of gelu); headz: fixed beforehand, as there
N32_TOL = {
    'fwd_small_s2':      28.0,       # 9.14
    'fwd_small_gen':     4.3,        # 1.43
    'fwd_8row_s2':       494.0,      # 164.6
    'fwd_8row_gen':      138.0,      # 45.9
    'headz':             c32.N_TOL['headz'],     # 4.0, not measured there either; GELU reads 2.22
}
S0_TOL = {
    'fwd z':          1.2e-6,   # 3.97e-7
    'fwd xpad bf16':  3.7e-7,   # 1.22e-7
    'fwd xpad fp16':  4.2e-7,   # 1.39e-7
    'bwd dbf':        2.2e-7,   # 7.10e-8
    'bwd dwf':        1.1e-6,   # 3.62e-7
    'bwd slabs':      1.5e-7,   # 4.75e-8
    'bwd dx':         1.9e-7,   # 6.18e-8
    'stem db1':       1.6e-7,   # 5.15e-8 (above swish's 4.78e-8 and its c of 1.4e-7)
    'stem dw1':       1.6e-7,   # 5.19e-8 (above swish's 4.82e-8 and its c of 1.4e-7)
    'stem db0':       3.2e-9,   # 1.04e-9
    'stem dw0':       3.2e-9,   # 1.05e-9
}
# worst at constant 1 over this module's cases -> the next power of two at least twice it
HEAD16 = {'C_FWD': 2,           # 0.616 (f16, sigmoid, C = 32, 20x30)
          'C_DY': 0.25,         # 0.109 (bf16, sigmoid, C = 96, 20x30); every other case is below 0: the 16-bit rounding covers it
          'C_DW': 4}            # 1.926 (bf16, sigmoid, C = 32, 20x30)
SIDE = {'C_FWD': 1,             # 0.443 (bf16, sigmoid, C = 96)
        'C_BWD': 1,             # no case above 0: the rounding terms u16 |r| + d16 cover all of it; 1 is the rule's own unit
        'C_DW': 8}              # 2.244 (bf16, sigmoid, C = 96)


def gelu64(z):
    return 0.5 * z * torch.special.erfc(-z / math.sqrt(2.0))


def dgelu64(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


class GeluLib:
    """The library with every entry that has an `_act` twin routed through the twin at ORN_ACT_GELU."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        twin = getattr(self._lib, name + '_act', None) if name.startswith('orn_') else None
        if twin is None:
            return getattr(self._lib, name)
        return lambda *args: twin(*args, GELU)


class GeluModule:
    """orn_amd._lib as test_gpu_head16.py / test_gpu_side_head.py take it, handing out the GELU library."""

    def __init__(self, mod):
        self._mod, self._proxy = mod, GeluLib(mod.lib())

    def lib(self):
        return self._proxy

    def __getattr__(self, name):
        return getattr(self._mod, name)


@pytest.fixture(scope='module')
def lib():
    import orn_amd
    real = orn_amd._lib.lib()
    for name in ('orn_debug_conv_fwd_f16_act', 'orn_debug_stage0_bwd_act', 'orn_debug_conv_bwd_f32_head_act', 'orn_debug_act_eval'):
        assert hasattr(real, name), name
    torch.set_num_threads(16)
    return GeluLib(real)


@pytest.fixture(scope='module')
def libmod():
    from orn_amd import _lib
    return GeluModule(_lib)


def apply_gelu(monkeypatch):
    """The five modules' references and constants switched to GELU (undone by the monkeypatch)."""
    for m in (c16, c32, s0):
        monkeypatch.setattr(m, '_silu', gelu64)
        monkeypatch.setattr(m, '_silu_grad', dgelu64)
    for m in (h16, sh):
        monkeypatch.setattr(m, 'silu64', gelu64)
        monkeypatch.setattr(m, 'dsilu64', dgelu64)
    monkeypatch.setattr(c16, 'C_TOL', C16_TOL)
    check16 = c16._check16

    def check16_gelu(k, r, A, half, form, what, gain=1.0, extra=0.0):
        if gain != 1.0:                                  # the apad epilogue: |act'| bounds what the error of the fp32 z turns into
            assert gain == 1.1
            gain = GAIN_APAD
        if isinstance(extra, torch.Tensor):              # _run_dgrad's allowance, 2^-20 (1 + |z|) |dx| there
            extra = extra * (E_DF / 2.0 ** -20)
        return check16(k, r, A, half, form, what, gain=gain, extra=extra)
    monkeypatch.setattr(c16, '_check16', check16_gelu)
    monkeypatch.setattr(c32, 'C_TOL', C32_TOL)
    monkeypatch.setattr(c32, 'N_TOL', N32_TOL)
    monkeypatch.setattr(s0, 'C_TOL', S0_TOL)
    monkeypatch.setattr(s0, '_silu_grad_allow', lambda z: E_DF * (1 + z.abs()))
    for k, v in HEAD16.items():
        monkeypatch.setattr(h16, k, v)
    for k, v in SIDE.items():
        monkeypatch.setattr(sh, k, v)


@pytest.fixture()
def gelu(monkeypatch):
    apply_gelu(monkeypatch)


# ---- 16-bit conv forward with apad -------------------------------------------------------------------------------------------
FWD16 = [
    # H, W, O, s, c_real, form
    (13, 37, 384, 2, 32, 'fwd'),         # narrow form
    (13, 37, 384, 2, 33, 'fwd'),         # full form
    (5, 7, 384, 2, 96, 'fwd'),           # an image smaller than one tile
    (17, 33, 864, 3, 96, 'fwd'),         # a ragged N tile with s = 3
    (23, 95, 96, 1, 96, 'fwd'),          # s = 1
    (153, 639, 384, 2, 96, 'fwd2'),      # 400 tiles: k_conv2_nhwc<1>
]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('H,W,O,s,c_real,form', FWD16)
def test_conv16_fwd_apad(lib, gelu, half, H, W, O, s, c_real, form):
    c16._run_fwd(lib, half, H, W, O, s, c_real, True, form, seed=H * 7919 + W * 31 + O + s + c_real + 2)


# ---- 16-bit dgrad, fused mode -------------------------------------------------------------------------------------------------
DGRAD16 = [
    # H, W, O, sp, form
    (6, 6, 864, 3, 'dgrad_split'), (9, 33, 1152, 3, 'dgrad_split'), (16, 62, 384, 1, 'dgrad_split'),      # split + k_dgrad_finish
    (122, 226, 384, 2, 'dgrad2'), (129, 255, 864, 3, 'dgrad2'),                                           # k_conv2_nhwc<0>
]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('H,W,O,sp,form', DGRAD16)
def test_conv16_dgrad_fused(lib, gelu, half, H, W, O, sp, form):
    c16._run_dgrad(lib, half, H, W, O, sp, 'fused', 96, form, seed=H * 7919 + W * 31 + O + sp + 96)


def test_conv16_dgrad_fp16_overflow_is_inf(lib, gelu):
    """Exactly the elements whose reference leaves the half range come out +-inf (split + k_dgrad_finish with GELU)."""
    c16.test_conv16_dgrad_fp16_overflow_is_inf(lib, 16, 64, 'dgrad_split')


# ---- the last stage's 16-bit head and the side heads ---------------------------------------------------------------------------
HEAD_SHAPES = ((2, 2, 2), (20, 30, 2))          # the smallest, and the first with a ragged last work-group
SIDE_SHAPES = ((2, 2, 2), (5, 5, 5))
WORST_HEADS = {}


@pytest.mark.parametrize('C', (32, 96))
@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_head16(libmod, gelu, kind, C):
    worst = h16.Worst(('forward',))
    for n, (H, W, s) in enumerate(HEAD_SHAPES):
        z, w, b, _ = h16.make_inputs(kind, C, H, W, 4000 + 16 * n + C // 32, special=(H, W, s) == h16.SPECIAL_AT)
        u, mag = h16.fwd_ref(z, w, b)
        for sigmoid in (False, True):
            out = h16.run_fwd(libmod, kind, z.cuda(), w.cuda(), b.cuda(), C, H, W, sigmoid)
            worst.add((h16.fwd_ratio(out, u, mag, sigmoid),), (C, H, W, 'sigmoid' if sigmoid else 'tanh'))
    back = h16.backward_cases(libmod, kind, C, HEAD_SHAPES, 2000)
    print(f'\nRATIO head16 gelu {kind} C={C}: {worst}; {back}')
    WORST_HEADS[('head16', kind)] = [max(a, b) for a, b in zip(WORST_HEADS.get(('head16', kind), [0, 0, 0]), worst.v + back.v)]
    assert worst.v[0] <= HEAD16['C_FWD'], (worst.v[0], worst.at[0])
    assert back.v[0] <= HEAD16['C_DY'], (back.v[0], back.at[0])
    assert back.v[1] <= HEAD16['C_DW'], (back.v[1], back.at[1])


@pytest.mark.parametrize('sigmoid', [False, True], ids=['tanh', 'sigmoid'])
@pytest.mark.parametrize('C', (32, 96))
@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_side_head(libmod, gelu, kind, C, sigmoid):
    worst = [0.0, 0.0, 0.0]
    for n, (H, W, s) in enumerate(SIDE_SHAPES):
        r = sh.run_case(libmod, C, H, W, s, kind, sigmoid, seed=1000 + n + C)[:3]
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f'\nRATIO side head gelu {kind} C={C} {"sigmoid" if sigmoid else "tanh"}: forward {worst[0]:.3f}, accumulate {worst[1]:.3f}, '
          f'dW/db {worst[2]:.3f}')
    WORST_HEADS[('side', kind)] = [max(a, b) for a, b in zip(WORST_HEADS.get(('side', kind), [0, 0, 0]), worst)]
    assert worst[0] <= SIDE['C_FWD'] and worst[1] <= SIDE['C_BWD'] and worst[2] <= SIDE['C_DW'], worst


# ---- stage 0 and the stem's slab backward ------------------------------------------------------------------------------------------
S0_CASES = [s0.CASES[i] for i in (0, 2, 6, 12)]      # one wave; ragged C16 / Cn; W % 4 != 0; the 720p shape
STEM_CASES = [(15, 8, 80, 1), (2065, 300, 130, 65)]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', S0_CASES, ids=s0._case_id)
def test_stage0_fwd(lib, gelu, case, half):
    s0.test_stage0_fwd(lib, case, half)


@pytest.mark.parametrize('case', S0_CASES, ids=s0._case_id)
def test_stage0_bwd(lib, gelu, case):
    s0.test_stage0_bwd(lib, case)


@pytest.mark.parametrize('Nout,Hd,E,nslab', STEM_CASES)
def test_stem_bwd_slabs(lib, gelu, Nout, Hd, E, nslab):
    s0.test_stem_bwd_slabs(lib, Nout, Hd, E, nslab)


# ---- the fp32 path -----------------------------------------------------------------------------------------------------------------
FWD32 = [K.FWD_CASES[i] for i in (0, 2, 5, 7)]       # small s = 2 (pair stores), small s = 3, 8-row s = 2, 8-row s = 3
BWD32 = [K.BWD_CASES[i] for i in (0, 2, 4, 8, 9, 14)]   # dgrad small / small split (s = 3) / 8-row split / tail / plain; wgrad 1 and 2


@pytest.mark.parametrize('shape,want,what', FWD32, ids=c32._ids(FWD32))
def test_conv32_fwd(lib, gelu, shape, want, what):
    c32.test_conv32_fwd_form(lib, shape, want, what)


@pytest.mark.parametrize('shape,want,what', BWD32, ids=c32._ids(BWD32))
def test_conv32_bwd(lib, gelu, shape, want, what):
    c32.test_conv32_bwd_form(lib, shape, want, what)


@pytest.mark.parametrize('sigmoid', [0, 1], ids=['tanh', 'sigmoid'])
def test_conv32_head_fwd_on_z(lib, gelu, sigmoid):
    shape, what = K.HEADZ_CASES[0]
    c32.test_conv32_head_fwd_on_z(lib, shape, what, sigmoid)


@pytest.mark.parametrize('sigmoid', [0, 1], ids=['tanh', 'sigmoid'])
@pytest.mark.parametrize('Cn', (3, 24))
def test_conv32_fused_head_bwd(lib, gelu, Cn, sigmoid):
    hw, blocks, what = K.HEAD_HW[0]
    c32.test_conv32_fused_head_bwd(lib, Cn, hw, blocks, what, sigmoid)


def test_zz_worst_ratios(lib):
    """Prints what this run measured per form, and checks that the cases above reached every form they name."""
    for name, table in (('conv16', c16.WORST), ('conv32', c32.WORST), ('stage0', s0.WORST), ('heads', WORST_HEADS)):
        for k in sorted(table, key=str):
            v = table[k]
            print(f'WORST {name} {k}: ' + (', '.join(f'{x:.3f}' for x in v) if isinstance(v, list) else f'{v:.3e}'))
    assert ('fwd2', 'fp16') in c16.WORST and ('dgrad2', 'bf16') in c16.WORST and 'head_dx' in c32.WORST and 'stem dw0' in s0.WORST
