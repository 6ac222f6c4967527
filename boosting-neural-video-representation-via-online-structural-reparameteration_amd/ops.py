"""torch.autograd glue over the C ABI of liborn.so (include/orn.h).

Every function here takes CUDA (HIP) fp32 tensors, launches hand-written gfx950 kernels on the
current torch stream and returns torch tensors.  Nothing falls back to PyTorch math: a CPU tensor
or a missing library raises OrnError.
"""
import math
from ctypes import c_double, c_float, c_int, c_size_t

import torch

from . import _lib
from ._lib import check, lib, ptr, stream


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.OrnError('liborn ops need tensors on the GPU (there is no CPU path)')
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ---- A1 ------------------------------------------------------------------------------------
def pe_forward(pos: torch.Tensor, lbase: float, levels: int) -> torch.Tensor:
    """utils.py:121-129 on the device.  pos [B] -> [B, 2*levels]."""
    pos = _f32c(pos)
    pw = torch.tensor([lbase ** i for i in range(levels)], dtype=torch.float64).to(torch.float32).to(pos.device)
    out = torch.empty(pos.shape[0], 2 * levels, dtype=torch.float32, device=pos.device)
    check(lib().orn_pe_fwd(ptr(pos), c_int(pos.shape[0]), ptr(pw), c_int(levels), ptr(out), stream()), 'orn_pe_fwd')
    return out


# ---- A2 ------------------------------------------------------------------------------------
# --act (model.py:24-45): what is built, by name -> ORN_ACT_* of include/orn.h
ACTS = ('swish', 'gelu')


def act_id(act) -> int:
    """ORN_ACT_* of an --act name (or of an id already); NotImplementedError, naming what is built, for anything else."""
    if isinstance(act, int) and 0 <= act < len(ACTS):
        return act
    if act not in ACTS:
        raise NotImplementedError(f'act={act!r} is outside the MI355X hot path (built: {ACTS}); see SURVEY.md section 8 for the scope')
    return ACTS.index(act)


class StemFn(torch.autograd.Function):
    """act(W1 act(W0 e + b0) + b1) (model.py:186-188); act: an --act name of ACTS (default swish)."""

    @staticmethod
    def forward(ctx, embed, w0, b0, w1, b1, act='swish'):
        ctx.act = act_id(act)
        embed, w0, b0, w1, b1 = map(_f32c, (embed, w0, b0, w1, b1))
        B, E = embed.shape
        Hd, Nout = w0.shape[0], w1.shape[0]
        dev = embed.device
        pre1 = torch.empty(B, Hd, device=dev)
        h1 = torch.empty(B, Hd, device=dev)
        pre2 = torch.empty(B, Nout, device=dev)
        h2 = torch.empty(B, Nout, device=dev)
        check(lib().orn_stem_fwd_act(ptr(embed), ptr(w0), ptr(b0), ptr(w1), ptr(b1), B, E, Hd, Nout,
                                     ptr(pre1), ptr(h1), ptr(pre2), ptr(h2), stream(), ctx.act), 'orn_stem_fwd_act')
        ctx.save_for_backward(embed, w1, pre1, h1, pre2)
        ctx.dims = (B, E, Hd, Nout)
        return h2

    @staticmethod
    def backward(ctx, dh2):
        embed, w1, pre1, h1, pre2 = ctx.saved_tensors
        B, E, Hd, Nout = ctx.dims
        dev = embed.device
        dh2 = _f32c(dh2)
        dw0 = torch.empty(Hd, E, device=dev)
        db0 = torch.empty(Hd, device=dev)
        dw1 = torch.empty(Nout, Hd, device=dev)
        db1 = torch.empty(Nout, device=dev)
        ws = _ws(lib().orn_stem_bwd_ws_bytes(B, Hd, Nout), dev)
        check(lib().orn_stem_bwd_act(ptr(embed), ptr(w1), ptr(pre1), ptr(h1), ptr(pre2), ptr(dh2), B, E, Hd, Nout,
                                     ptr(dw0), ptr(db0), ptr(dw1), ptr(db1), ptr(ws), stream(), ctx.act), 'orn_stem_bwd_act')
        return None, dw0, db0, dw1, db1, None


# ---- A3 ------------------------------------------------------------------------------------
class ErbMergeFn(torch.autograd.Function):
    """get_equivalent_kernel_bias (model.py:450-516): 9 branch tensors -> (Wf, bf)."""

    @staticmethod
    def forward(ctx, w3x3, b3x3, w3x1, b3x1, w1x3, b1x3, w1, w2, w3):
        ts = list(map(_f32c, (w3x3, b3x3, w3x1, b3x1, w1x3, b1x3, w1, w2, w3)))
        O, C = ts[0].shape[0], ts[0].shape[1]
        dev = ts[0].device
        T = torch.empty(O, C, 3, 3, device=dev)
        wf = torch.empty(O, C, 3, 3, device=dev)
        bf = torch.empty(O, device=dev)
        check(lib().orn_erb_merge_fwd(*[ptr(t) for t in ts], C, O, ptr(T), ptr(wf), ptr(bf), stream()),
              'orn_erb_merge_fwd')
        ctx.save_for_backward(ts[6], ts[7], ts[8], T)
        ctx.dims = (C, O)
        return wf, bf

    @staticmethod
    def backward(ctx, g, dbf):
        w1, w2, w3, T = ctx.saved_tensors
        C, O = ctx.dims
        dev = w1.device
        g = _f32c(g) if g is not None else torch.zeros(O, C, 3, 3, device=dev)
        dbf = _f32c(dbf) if dbf is not None else torch.zeros(O, device=dev)
        d3x3 = torch.empty(O, C, 3, 3, device=dev)
        db3x3 = torch.empty(O, device=dev)
        d3x1 = torch.empty(O, C, 3, 1, device=dev)
        db3x1 = torch.empty(O, device=dev)
        d1x3 = torch.empty(O, C, 1, 3, device=dev)
        db1x3 = torch.empty(O, device=dev)
        dw1 = torch.empty(2 * C, C, 1, 1, device=dev)
        dw2 = torch.empty(O, 2 * C, 3, 3, device=dev)
        dw3 = torch.empty(O, O, 1, 1, device=dev)
        nb = lib().orn_erb_merge_bwd_ws_bytes(C, O)
        ws = _ws(nb, dev)
        check(lib().orn_erb_merge_bwd(ptr(g), ptr(dbf), ptr(w1), ptr(w2), ptr(w3), ptr(T), C, O, ptr(d3x3), ptr(db3x3),
                                      ptr(d3x1), ptr(db3x1), ptr(d1x3), ptr(db1x3), ptr(dw1), ptr(dw2), ptr(dw3),
                                      ptr(ws), c_size_t(ws.numel()), stream()), 'orn_erb_merge_bwd')
        return d3x3, db3x3, d3x1, db3x1, d1x3, db1x3, dw1, dw2, dw3


# ---- N7 ------------------------------------------------------------------------------------
# Tensor order of a block of each kind, as BranchMergeFn / branch_merge_fwd / branch_merge_bwd take and return them: the fields
# of orn_branch_ptrs (include/orn.h), ECB's three 1x1 -> mask branches in the order sbx, sby, lpl.
BRANCH_TENSORS = {
    'ACB': ('w3x3', 'b3x3', 'w3x1', 'b3x1', 'w1x3', 'b1x3'),
    'RepVGG': ('w3x3', 'b3x3', 'w1x1', 'b1x1'),
    'ECB': ('w3x3', 'b3x3', 'wA', 'wB') + tuple(f'{t}.{f}' for t in _lib.ECB_SEQ for f in _lib.SEQ_FIELDS),
}


def branch_shapes(kind: str, C: int, O: int):
    """Shapes of BRANCH_TENSORS[kind] for a block C -> O (model.py:345-393)."""
    sh = {'w3x3': (O, C, 3, 3), 'b3x3': (O,), 'w3x1': (O, C, 3, 1), 'b3x1': (O,), 'w1x3': (O, C, 1, 3), 'b1x3': (O,),
          'w1x1': (O, C, 1, 1), 'b1x1': (O,), 'wA': (2 * C, C, 1, 1), 'wB': (O, 2 * C, 3, 3),
          'k0': (O, C, 1, 1), 'b0': (O,), 'scale': (O, 1, 1, 1), 'bias': (O,), 'mask': (O, 1, 3, 3)}
    return [sh[n.split('.')[-1]] for n in BRANCH_TENSORS[kind]]


def _branch_ptrs(kind: str, tensors) -> '_lib.BranchPtrs':
    names = BRANCH_TENSORS[kind]
    if len(tensors) != len(names):
        raise _lib.OrnError(f'{kind}: {len(tensors)} tensors for {names}')
    p = _lib.BranchPtrs()
    for n, t in zip(names, tensors):
        if '.' in n:
            seq, f = n.split('.')
            setattr(p.sb[_lib.ECB_SEQ.index(seq)], f, t.data_ptr())
        else:
            setattr(p, n, t.data_ptr())
    return p


def branch_merge_fwd(kind: str, tensors, out=None):
    """(Wf [O,C,3,3], bf [O]) of an ACB / RepVGG / ECB block (orn_branch_merge_fwd).  tensors: BRANCH_TENSORS[kind], fp32 on the
    GPU.  out: (wf, bf) to fill in place of new tensors."""
    ts = [_f32c(t) for t in tensors]
    O, C = ts[0].shape[0], ts[0].shape[1]
    wf, bf = out if out is not None else (torch.empty(O, C, 3, 3, device=ts[0].device), torch.empty(O, device=ts[0].device))
    p = _branch_ptrs(kind, ts)
    check(lib().orn_branch_merge_fwd(_lib.BRANCH_KINDS[kind], p, C, O, ptr(wf), ptr(bf), stream()), 'orn_branch_merge_fwd')
    return wf, bf


def branch_merge_bwd(kind: str, tensors, g, dbf, grads=None):
    """Gradients of BRANCH_TENSORS[kind] from g = dL/dWf and dbf = dL/dbf (orn_branch_merge_bwd), in that order; ECB's b0 and mask
    get zeros.  grads: preallocated outputs (grads[0] may be g and grads[1] dbf: no copy then)."""
    ts = [_f32c(t) for t in tensors]
    g, dbf = _f32c(g), _f32c(dbf)
    O, C = ts[0].shape[0], ts[0].shape[1]
    if grads is None:
        grads = [torch.empty_like(t) for t in ts]
    nb = lib().orn_branch_merge_bwd_ws_bytes(_lib.BRANCH_KINDS[kind], C, O)
    ws = _ws(nb, g.device)
    p, d = _branch_ptrs(kind, ts), _branch_ptrs(kind, grads)
    check(lib().orn_branch_merge_bwd(_lib.BRANCH_KINDS[kind], p, ptr(g), ptr(dbf), C, O, d, ptr(ws), c_size_t(ws.numel()), stream()),
          'orn_branch_merge_bwd')
    return grads


class BranchMergeFn(torch.autograd.Function):
    """get_equivalent_kernel_bias of an ACB / RepVGG / ECB block: BranchMergeFn.apply(kind, *BRANCH_TENSORS[kind]) -> (Wf, bf).
    The reference has no merge for these kinds (its switch_to_deploy knows ERB's attributes only); include/orn.h, N7, defines it."""

    @staticmethod
    def forward(ctx, kind, *tensors):
        ts = [_f32c(t) for t in tensors]
        ctx.kind = kind
        ctx.save_for_backward(*ts)
        return branch_merge_fwd(kind, ts)

    @staticmethod
    def backward(ctx, g, dbf):
        ts = ctx.saved_tensors
        O, C = ts[0].shape[0], ts[0].shape[1]
        g = g if g is not None else torch.zeros(O, C, 3, 3, device=ts[0].device)
        dbf = dbf if dbf is not None else torch.zeros(O, device=ts[0].device)
        return (None, *branch_merge_bwd(ctx.kind, ts, g, dbf))


# ---- A4 ------------------------------------------------------------------------------------
class ConvPsSiluFn(torch.autograd.Function):
    """conv3x3(pad 1) + bias -> PixelShuffle(s) -> act (model.py:539,567); act: an --act name of ACTS (default swish)."""

    @staticmethod
    def forward(ctx, x, wf, bf, s, act='swish'):
        ctx.act = act_id(act)
        x, wf, bf = _f32c(x), _f32c(wf), _f32c(bf)
        B, C, H, W = x.shape
        O = wf.shape[0]
        if wf.shape[1] != C or tuple(wf.shape[2:]) != (3, 3) or O % (s * s):
            raise _lib.OrnError(f'conv3x3_ps_silu: bad shapes x={tuple(x.shape)} w={tuple(wf.shape)} s={s}')
        dev = x.device
        need_grad = any(ctx.needs_input_grad[:3])
        a = torch.empty(B, O // (s * s), H * s, W * s, device=dev)
        z = torch.empty_like(a) if need_grad else None
        check(lib().orn_conv3x3_ps_silu_fwd_act(ptr(x), ptr(wf), ptr(bf), B, C, O, H, W, s, ptr(z), ptr(a), stream(), ctx.act),
              'orn_conv3x3_ps_silu_fwd_act')
        if need_grad:
            ctx.save_for_backward(x, wf, z)
        ctx.dims = (B, C, O, H, W, s)
        return a

    @staticmethod
    def backward(ctx, da):
        x, wf, z = ctx.saved_tensors
        B, C, O, H, W, s = ctx.dims
        dev = x.device
        da = _f32c(da)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dwf = torch.empty_like(wf)
        dbf = torch.empty(O, device=dev)
        nb = lib().orn_conv3x3_ps_silu_bwd_ws_bytes(B, C, O, H, W)
        ws = _ws(nb, dev)
        check(lib().orn_conv3x3_ps_silu_bwd_act(ptr(x), ptr(wf), ptr(z), ptr(da), B, C, O, H, W, s, ptr(dx), ptr(dwf),
                                                ptr(dbf), ptr(ws), c_size_t(ws.numel()), stream(), ctx.act),
              'orn_conv3x3_ps_silu_bwd_act')
        return dx, dwf, dbf, None, None


# ---- A5 ------------------------------------------------------------------------------------
class HeadFn(torch.autograd.Function):
    """1x1 conv -> (tanh+1)/2 or sigmoid (model.py:621-622)."""

    @staticmethod
    def forward(ctx, a, w, b, sigmoid):
        a, w, b = _f32c(a), _f32c(w), _f32c(b)
        B, C, H, W = a.shape
        out = torch.empty(B, 3, H, W, device=a.device)
        check(lib().orn_head_fwd(ptr(a), ptr(w), ptr(b), B, C, H, W, int(bool(sigmoid)), ptr(out), stream()), 'orn_head_fwd')
        ctx.save_for_backward(a, w, out)
        ctx.sigmoid = int(bool(sigmoid))
        return out

    @staticmethod
    def backward(ctx, dout):
        a, w, out = ctx.saved_tensors
        B, C, H, W = a.shape
        dev = a.device
        dout = _f32c(dout)
        da = torch.empty_like(a)
        dw = torch.empty_like(w)
        db = torch.empty(3, device=dev)
        nb = lib().orn_head_bwd_ws_bytes(B, C, H, W)
        ws = _ws(nb, dev)
        check(lib().orn_head_bwd(ptr(a), ptr(w), ptr(out), ptr(dout), B, C, H, W, ctx.sigmoid, ptr(da), ptr(dw), ptr(db),
                                 ptr(ws), c_size_t(ws.numel()), stream()), 'orn_head_bwd')
        return da, dw, db, None


# ---- side heads of the multi-resolution generator (orn_side_head.hip, include/orn_debug.h) -------
_H16 = {torch.bfloat16: 'bf16', torch.float16: 'f16'}


def _side_fn(name: str):
    fn = getattr(lib(), name, None)
    if fn is None:
        raise _lib.OrnError(f'{name} is not in this build of liborn.so')
    return fn


def side_head_fwd(x, w, b, sigmoid: bool = False) -> torch.Tensor:
    """The head of one stage, model.py:621-622, -> out [3,H,W] fp32.  x: the block's stored output in the layout the engine keeps it
    in -- bf16 / fp16 [H,W,C] channels-last PRE-activation (the head forms SiLU itself), or fp32 [C,H,W] activation."""
    w, b = _f32c(w).reshape(3, -1), _f32c(b)
    (C, H, W) = x.shape if x.dtype == torch.float32 else (x.shape[2], x.shape[0], x.shape[1])
    out = torch.empty(3, H, W, device=x.device)
    name = f'orn_debug_side_head_fwd_{_H16.get(x.dtype, "f32")}'
    check(_side_fn(name)(ptr(x), ptr(w), ptr(b), C, H, W, int(bool(sigmoid)), ptr(out), stream()), name)
    return out


def side_head_bwd_(x, w, out, dout, grad, sigmoid: bool = False, lw: float = 1.0, sp: int = 1, gs: float = 1.0):
    """The accumulating backward of a side head: ADDS this head's term to `grad`, in place, and returns (dW [3,C], db [3]).
    du = dout * lw * act'(out).  16-bit x [H,W,C] (pre-activation z): grad is the block's padded un-shuffled gradient buffer
    [H/sp + 2, W/sp + 2, C sp^2] of x's dtype, carrying the scale gs; every interior element becomes
    round(fp32(grad) + gs * (W^T du) * SiLU'(z)), the ring stays as it is; dW, db come back un-scaled.  fp32 x [C,H,W] (activation):
    grad [C,H,W] += W^T du (sp, gs unused)."""
    w, out, dout = _f32c(w).reshape(3, -1), _f32c(out), _f32c(dout)
    f32 = x.dtype == torch.float32
    (C, H, W) = x.shape if f32 else (x.shape[2], x.shape[0], x.shape[1])
    want = (C, H, W) if f32 else (H // sp + 2, W // sp + 2, C * sp * sp)
    if grad.dtype != x.dtype or tuple(grad.shape) != want or not grad.is_contiguous():
        raise _lib.OrnError(f'side_head_bwd_: grad {grad.dtype} {tuple(grad.shape)} vs contiguous {x.dtype} {want}')
    dw = torch.empty(3, C, device=x.device)
    db = torch.empty(3, device=x.device)
    ws = _ws(_side_fn('orn_debug_side_head_bwd_ws_bytes')(C, H, W), x.device)
    if f32:
        check(_side_fn('orn_debug_side_head_bwd_f32')(ptr(x), ptr(w), ptr(out), ptr(dout), C, H, W, int(bool(sigmoid)), c_float(lw),
                                                      ptr(grad), ptr(dw), ptr(db), ptr(ws), c_size_t(ws.numel()), stream()),
              'orn_debug_side_head_bwd_f32')
    else:
        name = f'orn_debug_side_head_bwd_{_H16[x.dtype]}'
        check(_side_fn(name)(ptr(x), ptr(w), ptr(out), ptr(dout), C, H, W, int(bool(sigmoid)), sp, c_float(lw), c_float(gs),
                             ptr(grad), ptr(dw), ptr(db), ptr(ws), c_size_t(ws.numel()), stream()), name)
    return dw, db


# ---- A7 / A10 ------------------------------------------------------------------------------
def loss_stats(pred, target, loss_type: str = 'Fusion6', want_grad: bool = True, loss_scale: float = 1.0):
    """-> (stats[8] device tensor, dpred or None).  stats = [loss, L1, MSE, SSIM (MS-SSIM for Fusion10-12), PSNR, 0, 0, 0].
    loss_type: any name of _lib.LOSS_TYPES; the MS-SSIM losses need min(H, W) > 160."""
    lt = _lib.loss_id(loss_type)
    pred, target = _f32c(pred), _f32c(target)
    if pred.shape != target.shape or pred.dim() != 4:
        raise _lib.OrnError(f'loss: shapes {tuple(pred.shape)} vs {tuple(target.shape)}')
    B, Ch, H, W = pred.shape
    dev = pred.device
    stats = torch.empty(8, device=dev)
    dpred = torch.empty_like(pred) if want_grad else None
    nb = lib().orn_loss_ws_bytes_for(lt, B, Ch, H, W)      # 0 for a shape the loss does not take: the call below says why
    ws = _ws(nb, dev)
    check(lib().orn_loss_fwd_bwd(ptr(pred), ptr(target), B, Ch, H, W, lt, c_float(loss_scale),
                                 ptr(stats), ptr(dpred), ptr(ws), c_size_t(ws.numel()), stream()), 'orn_loss_fwd_bwd')
    return stats, dpred


class LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, loss_type):
        stats, dpred = loss_stats(pred, target.detach(), loss_type, want_grad=True)
        ctx.save_for_backward(dpred)
        return stats[0].clone()

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None


# ---- A9 ------------------------------------------------------------------------------------
def adam_step_(p, g, m, v, lr: float, step: int, beta1: float = 0.5, beta2: float = 0.999, eps: float = 1e-8):
    """In-place Adam over flat fp32 arenas (main_train.py:196,250)."""
    for t in (p, g, m, v):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise _lib.OrnError('adam_step_: arenas must be contiguous CUDA fp32 tensors')
    n = p.numel()
    check(lib().orn_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), c_size_t(n), c_double(lr), c_double(beta1), c_double(beta2),
                              c_double(eps), c_int(step), stream()), 'orn_adam_step')


# ---- N3 ------------------------------------------------------------------------------------
def ms_ssim(pred, target) -> torch.Tensor:
    """pytorch_msssim.ms_ssim(pred, target, data_range=1, size_average=True) as utils.py:205 calls it."""
    pred, target = _f32c(pred.detach()), _f32c(target.detach())
    B, Ch, H, W = pred.shape
    out = torch.empty(1, device=pred.device)
    nb = lib().orn_msssim_ws_bytes(B, Ch, H, W)
    ws = _ws(nb, pred.device)
    check(lib().orn_msssim(ptr(pred), ptr(target), B, Ch, H, W, ptr(out), ptr(ws), c_size_t(ws.numel()), stream()), 'orn_msssim')
    return out[0]


def ms_ssim_frames(pred, target, rows=None, chunk=None) -> torch.Tensor:
    """One MS-SSIM value per frame, enqueued without a host sync (orn_msssim_frames): out[k] = ms_ssim(pred[k:k+1], target[rows[k]])
    as utils.py:201-211 calls it with batch 1, bit-identical to `ms_ssim` on that pair.  pred [n,Ch,H,W]; target [*,Ch,H,W];
    rows: indices into target (sequence or tensor; default: frame k against target[k]).  A sequence or host tensor is range-checked
    here; a device tensor is taken as it is (checking it would synchronise).  chunk: frames per group of six launches (default
    min(n, 8); the values do not depend on it)."""
    pred, target = _f32c(pred.detach()), _f32c(target.detach())
    n, Ch, H, W = pred.shape
    if target.dim() != 4 or tuple(target.shape[1:]) != (Ch, H, W):
        raise _lib.OrnError(f'ms_ssim_frames: target {tuple(target.shape)} vs pred {tuple(pred.shape)}')
    if rows is None:
        if target.shape[0] < n:
            raise _lib.OrnError(f'ms_ssim_frames: {n} frames against {target.shape[0]} targets')
    else:
        rows = torch.as_tensor(rows)
        if rows.numel() != n:
            raise _lib.OrnError(f'ms_ssim_frames: {rows.numel()} rows for {n} frames')
        if not rows.is_cuda and n and (int(rows.min()) < 0 or int(rows.max()) >= target.shape[0]):
            raise _lib.OrnError(f'ms_ssim_frames: row index out of range [0, {target.shape[0]})')
        rows = rows.to(pred.device, torch.int32).reshape(-1).contiguous()
    out = torch.empty(n, device=pred.device)
    if n == 0:
        return out
    ws = _ws(lib().orn_msssim_frames_ws_bytes(max(1, min(n, chunk or 8)), Ch, H, W), pred.device)
    check(lib().orn_msssim_frames(ptr(pred), ptr(target), ptr(rows), n, Ch, H, W, ptr(out), ptr(ws), c_size_t(ws.numel()), stream()),
          'orn_msssim_frames')
    return out


# ---- K11 -----------------------------------------------------------------------------------
def ingest_frames(src, out_hw, chunk=None, out=None) -> torch.Tensor:
    """ToTensor + F.adaptive_avg_pool2d(data, out_hw) as main_train.py:200,239 form a target, on the device, bit-identical to ATen's
    CPU result.  src: uint8 [n,H,W,3] as PIL decodes it (orn_frames_ingest_u8) or fp32 [n,3,H,W] (orn_frames_pool_f32), on the GPU.
    Returns fp32 [n,3,h,w]; out_hw == (H, W) gives exactly ToTensor / an exact copy.  chunk: frames per launch (default: all; the
    values do not depend on it).  out: an fp32 [n,3,h,w] tensor (or slice of one along n) to fill in place of a new one -- a caller
    that uploads a long video piece by piece ingests each piece into its slice, so the source is never resident as a whole."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise _lib.OrnError('ingest_frames: liborn ops need tensors on the GPU (there is no CPU path)')
    h, w = int(out_hw[0]), int(out_hw[1])
    if src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3:
        (n, H, W), fn, what = src.shape[:3], lib().orn_frames_ingest_u8, 'orn_frames_ingest_u8'
    elif src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 3:
        n, (H, W), fn, what = src.shape[0], src.shape[2:], lib().orn_frames_pool_f32, 'orn_frames_pool_f32'
    else:
        raise _lib.OrnError(f'ingest_frames: {src.dtype} {tuple(src.shape)} is neither uint8 [n,H,W,3] nor float32 [n,3,H,W]')
    src = src.contiguous()
    if out is None:
        out = torch.empty(n, 3, h, w, device=src.device)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (n, 3, h, w) or out.device != src.device or not out.is_contiguous()):
        raise _lib.OrnError(f'ingest_frames: out {out.dtype} {tuple(out.shape)} vs contiguous float32 {(n, 3, h, w)} on {src.device}')
    step = n if chunk is None else max(1, int(chunk))
    for k in range(0, n, max(step, 1)):
        m = min(step, n - k)
        check(fn(ptr(src[k:k + m]), m, H, W, ptr(out[k:k + m]), h, w, stream()), what)
    return out
