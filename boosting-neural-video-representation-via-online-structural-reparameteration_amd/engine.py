"""TrainEngine: the reference's per-frame training step (main_train.py:229-254) driven through
`orn_engine_*` (include/orn.h).

PyTorch is the allocator only: the module's parameters are re-homed as views into one flat fp32
arena (so `state_dict()`, checkpoints and the eager autograd path keep working on the same
memory), gradients and Adam state get arenas of the same shape, the video is resident in HBM, and
every step reads its frame index / LR / step count from a device-side schedule, so whole epochs are
enqueued without a host sync -- as plain stream launches pipelined over the engine's second stream
(`run()`'s default, orn_engine_train_steps) or as hipGraph replays of the serial step (`graph=True`).
A loss the library does not build trains through the split step (`step_with` / `run_with`): the engine's
forward, a torch function of its output on the caller's stream, the engine's backward and Adam.
"""
import contextlib
import ctypes
from ctypes import byref, c_int32, c_size_t, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import EngineDesc, OrnError, check, lib

_ALIGN = 64          # floats (256 B): every tensor starts on a 256-byte boundary inside the arena
_ERB_FIELDS = {
    'rbr_3x3_branch.weight': 'w3x3', 'rbr_3x3_branch.bias': 'b3x3',
    'rbr_3x1_branch.weight': 'w3x1', 'rbr_3x1_branch.bias': 'b3x1',
    'rbr_1x3_branch.weight': 'w1x3', 'rbr_1x3_branch.bias': 'b1x3',
    'rbr_1x1_3x3_1x1_branch_1x1_1.weight': 'w1', 'rbr_1x1_3x3_1x1_branch_3x3.weight': 'w2',
    'rbr_1x1_3x3_1x1_branch_1x1_2.weight': 'w3',
}
# ACB / RepVGG / ECB (orn_engine_desc.branch_kind): fields of orn_layer_desc where it has one (ACB's as ERB's; ECB's wA / wB in
# w1 / w2), else of orn_branch_desc ('x.' prefix)
_BRANCH_FIELDS = {
    'ACB': {k: f for k, f in _ERB_FIELDS.items() if f in ('w3x3', 'b3x3', 'w3x1', 'b3x1', 'w1x3', 'b1x3')},
    'RepVGG': {'rbr_3x3_branch.weight': 'w3x3', 'rbr_3x3_branch.bias': 'b3x3', 'rbr_1x1_branch.weight': 'x.w1x1', 'rbr_1x1_branch.bias': 'x.b1x1'},
    'ECB': {'rbr_3x3_branch.weight': 'w3x3', 'rbr_3x3_branch.bias': 'b3x3',
            'rbr_1x1_3x3_branch_1x1.weight': 'w1', 'rbr_1x1_3x3_branch_3x3.weight': 'w2',
            **{f'rbr_conv1x1_{seq}_branch.{f}': f'x.sb.{t}.{f}' for t, seq in enumerate(_lib.ECB_SEQ) for f in _lib.SEQ_FIELDS}},
}
_SINGLE_FIELDS = {'branch.weight': 'w3x3', 'branch.bias': 'b3x3', 'rbr_reparam.weight': 'w3x3', 'rbr_reparam.bias': 'b3x3'}


def arena_layout(named_shapes: Sequence[Tuple[str, Tuple[int, ...]]]):
    """name -> (offset, numel) with every tensor aligned to 256 B; returns (layout, total_floats)."""
    off = 0
    out = {}
    for name, shape in named_shapes:
        n = int(np.prod(shape)) if len(shape) else 1
        out[name] = (off, n)
        off += (n + _ALIGN - 1) // _ALIGN * _ALIGN
    return out, off


def stage_hw(model) -> List[Tuple[int, int]]:
    """Image size of every stage of `model`; the last is the decoder's output."""
    H, W, out = model.fc_h, model.fc_w, []
    for blk in model.layers:
        H, W = H * blk.stride, W * blk.stride
        out.append((H, W))
    return out


def is_multi_res(model) -> bool:
    """A head on every stage (Generator(sin_res=False), model.py:597-625), not on the last alone."""
    return len(model.head_layers) > 1 and all(h is not None for h in model.head_layers)


def build_desc(model, layout, total, loss_type='Fusion6', beta1=0.5, beta2=0.999, eps=1e-8, precision=0, lw=1.0,
               multi_res=None) -> EngineDesc:
    """Describe `model` (our Generator mirror) to the native engine.  A multi-resolution model (is_multi_res) gives a multi-resolution
    engine with the side stages' weight lw (--lw); multi_res=False describes its last stage alone (decode-only engines)."""
    d = EngineDesc()
    n_layers = len(model.layers)
    if n_layers > _lib.ORN_MAX_LAYERS:
        raise OrnError(f'{n_layers} layers > ORN_MAX_LAYERS')
    blk0 = model.layers[0]
    erb = (not blk0.deploy) and blk0.branch_type == 'ERB'
    kind = None if blk0.deploy else _lib.BRANCH_KINDS.get(blk0.branch_type)
    d.n_layers, d.erb, d.branch_kind = n_layers, int(erb), kind or 0
    d.embed_len, d.stem_dim = model.stem[0].in_features, model.stem[0].out_features
    d.fc_h, d.fc_w, d.fc_dim = model.fc_h, model.fc_w, model.fc_dim
    d.sigmoid = int(bool(model.sigmoid))
    d.act = ops.act_id(getattr(model, 'act', 'swish'))      # --act: the stem's and every block's activation (ORN_ACT_*)
    d.loss_type = _lib.loss_id(loss_type)
    d.precision = precision
    d.beta1, d.beta2, d.eps = beta1, beta2, eps
    d.stem_w0, d.stem_b0 = layout['stem.0.weight'][0], layout['stem.0.bias'][0]
    d.stem_w1, d.stem_b1 = layout['stem.2.weight'][0], layout['stem.2.bias'][0]
    d.head_w, d.head_b = layout[f'head_layers.{n_layers - 1}.weight'][0], layout[f'head_layers.{n_layers - 1}.bias'][0]
    d.n_params = total
    if is_multi_res(model) if multi_res is None else multi_res:
        d.multi_res, d.lw = 1, lw
        for i in range(n_layers - 1):
            d.side_head_w[i], d.side_head_b[i] = layout[f'head_layers.{i}.weight'][0], layout[f'head_layers.{i}.bias'][0]
    in_hw = [(model.fc_h, model.fc_w)] + stage_hw(model)      # a block's input: the stage below it
    for i, blk in enumerate(model.layers):
        L = d.layer[i]
        L.C, L.O, L.s, (L.H, L.W) = blk.ngf, blk.out_channels, blk.stride, in_hw[i]
        for f in ('w3x3', 'b3x3', 'w3x1', 'b3x1', 'w1x3', 'b1x3', 'w1', 'w2', 'w3'):
            setattr(L, f, -1)
        X = d.branch[i]
        if kind:                                            # (another kind's descriptor leaves these zero and unread)
            X.w1x1 = X.b1x1 = -1
            for t in range(3):
                for f in _lib.SEQ_FIELDS:
                    setattr(X.sb[t], f, -1)
        fields = _ERB_FIELDS if erb else _BRANCH_FIELDS[blk0.branch_type] if kind else _SINGLE_FIELDS
        for key, f in fields.items():
            name = f'layers.{i}.{key}'
            if name not in layout:
                continue
            if f.startswith('x.sb.'):
                setattr(X.sb[int(f.split('.')[2])], f.split('.')[3], layout[name][0])
            elif f.startswith('x.'):
                setattr(X, f[2:], layout[name][0])
            else:
                setattr(L, f, layout[name][0])
    return d


def make_schedule(entries: Sequence[Tuple[int, int, float]]) -> np.ndarray:
    """[(frame, step, lr)] -> int32 [n,4] array with the orn_step_sched memory layout."""
    arr = np.zeros((len(entries), 4), dtype=np.int32)
    for i, (frame, step, lr) in enumerate(entries):
        arr[i, 0] = frame
        arr[i, 1] = step
        arr[i, 2] = np.float32(lr).view(np.int32)
    return arr


class _Decoding:
    """Construction and the forward-only entry points of an engine handle (`_h`, `device`, `out_hw`, `desc`; `frames` / `embeds`
    when a video is resident): shared by TrainEngine and the decode-only Decoder."""
    frames = None
    embeds = None

    def _rehome(self, model, device, grads: bool):
        """The module's parameters become views into one flat arena, `params` (so the module and the engine share the memory), and
        with `grads` their .grad views into a second one."""
        if not torch.cuda.is_available():
            raise OrnError(f'{type(self).__name__} needs a GPU: there is no CPU path')
        self.device = torch.device(device or f'cuda:{torch.cuda.current_device()}')
        self.model = model
        self.layout, self.n_params = arena_layout([(k, tuple(p.shape)) for k, p in model.named_parameters()])
        self.params = torch.zeros(self.n_params, device=self.device)
        if grads:
            self.grads = torch.zeros(self.n_params, device=self.device)
        with torch.no_grad():
            for k, p in model.named_parameters():
                off, n = self.layout[k]
                view = self.params[off:off + n].view(p.shape)
                view.copy_(p.detach().to(self.device))
                p.data = view
                if grads:
                    p.grad = self.grads[off:off + n].view(p.shape)

    def _create(self, precision: str, train: bool, *desc_args, **desc_kw):
        """The engine of build_desc(model, ..): its zeroed workspace and, for training, the Adam arenas beside `grads`."""
        self.precision = {'fp32': 0, 'bf16': 1, 'fp16': 2}[precision]
        self.desc = build_desc(self.model, self.layout, self.n_params, *desc_args, precision=self.precision, **desc_kw)
        nbytes = lib().orn_engine_ws_bytes(byref(self.desc))
        if nbytes == 0:
            raise OrnError('orn_engine_ws_bytes: ' + _lib.last_error())
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        if train:
            self.adam_m, self.adam_v = (torch.zeros(self.n_params, device=self.device) for _ in range(2))
        arenas = (self.grads, self.adam_m, self.adam_v) if train else (None, None, None)
        self._h = c_void_p()
        check(lib().orn_engine_create(byref(self.desc), _lib.ptr(self.params), *(_lib.ptr(t) for t in arenas), _lib.ptr(self.ws),
                                      c_size_t(nbytes), byref(self._h)), 'orn_engine_create')
        self.out_hw = self.stage_hw()[-1]

    def stage_hw(self) -> List[Tuple[int, int]]:
        """Image size of every stage, the last included."""
        return stage_hw(self.model)

    def decode(self, embed: torch.Tensor) -> torch.Tensor:
        """Forward only: embed [E] or [1,E] -> image [1,3,H,W]."""
        embed = embed.to(self.device, torch.float32).contiguous().view(-1)
        img = torch.empty(1, 3, *self.out_hw, device=self.device)
        check(lib().orn_engine_decode(self._h, _lib.ptr(embed), _lib.ptr(img), _lib.stream()), 'orn_engine_decode')
        return img

    def decode_frames(self, rows=None, embeds=None, frames=None, rgb8=True, f32=False, stats=True, msssim=False, chunk=None) -> dict:
        """Decode many frames in one call (orn_engine_decode_frames; main_eval.py:795-815, main_train.py:377-438): the weight-only
        work of the forward runs once, and each frame ends on the device in what is asked for.
        rows: indices (sequence or tensor) into `embeds` [*,E] and `frames` [*,3,H,W]; both default to the resident video
        (set_video) and rows to all of it.  Returns device tensors, enqueued on the current stream without a host sync:
          'rgb8'  uint8 [n,H,W,3], torchvision.utils.save_image's bytes;  'img' float [n,3,H,W] (f32=True);
          'stats' float [n,4]: mse, PSNR of the float image, mse, PSNR of the bytes / 255, against frames[rows] (stats=True; needs frames);
          'msssim' float [n] (msssim=True; needs frames): MS-SSIM of each frame against frames[rows] as utils.py:201-211 computes it per
            frame, in the same call (orn_engine_eval_frames), bit-identical to ops.ms_ssim on the decoded frame; zeros when the image
            is less than 160 high (utils.msssim_fn's rule).  chunk: frames per group of MS-SSIM launches, which sizes the workspace
            (default min(n, 8); the values do not depend on it)."""
        embeds = self.embeds if embeds is None else embeds.to(self.device, torch.float32).contiguous()
        frames = self.frames if frames is None else self._target_frames(frames, 'decode_frames: ')
        if embeds is None:
            raise OrnError('decode_frames: no embeds given and no video resident (set_video)')
        if embeds.dim() != 2 or embeds.shape[1] != self.desc.embed_len:
            raise OrnError(f'decode_frames: embeds {tuple(embeds.shape)} vs (*, {self.desc.embed_len})')
        if (stats or msssim) and frames is None:
            raise OrnError('decode_frames: stats and msssim need target frames (frames=, or set_video)')
        if rows is None:
            rows = torch.arange(embeds.shape[0], dtype=torch.int32)
        rows = torch.as_tensor(rows).to(torch.int32).reshape(-1)
        n = int(rows.numel())
        limit = embeds.shape[0] if not (stats or msssim) else min(embeds.shape[0], frames.shape[0])
        if n and (int(rows.min()) < 0 or int(rows.max()) >= limit):        # the device would read out of bounds
            raise OrnError(f'decode_frames: row index out of range [0, {limit})')
        rows = rows.to(self.device).contiguous()
        H, W = self.out_hw
        out = {}
        if rgb8:
            out['rgb8'] = torch.empty(n, H, W, 3, dtype=torch.uint8, device=self.device)
        if f32:
            out['img'] = torch.empty(n, 3, H, W, device=self.device)
        if stats:
            out['stats'] = torch.empty(n, 4, device=self.device)
        if msssim and H < 160:                              # utils.msssim_fn (utils.py:201-211): no MS-SSIM below 160 rows
            out['msssim'] = torch.zeros(n, device=self.device)
            msssim = False
        if msssim and n:
            out['msssim'] = torch.empty(n, device=self.device)
            ws = self._eval_ws(max(1, min(n, chunk or 8)))
            check(lib().orn_engine_eval_frames(self._h, _lib.ptr(embeds), _lib.ptr(rows), c_int32(n), _lib.ptr(frames),
                                               _lib.ptr(out.get('rgb8')), _lib.ptr(out.get('img')), _lib.ptr(out.get('stats')),
                                               _lib.ptr(out['msssim']), _lib.ptr(ws), c_size_t(ws.numel()), _lib.stream()),
                  'orn_engine_eval_frames')
        elif msssim:
            out['msssim'] = torch.empty(0, device=self.device)
        elif rgb8 or f32 or stats or 'msssim' not in out:     # (a zero column alone needs no decode; no output at all is the library's error)
            check(lib().orn_engine_decode_frames(self._h, _lib.ptr(embeds), _lib.ptr(rows), c_int32(n), _lib.ptr(frames) if stats else None,
                                                 _lib.ptr(out.get('rgb8')), _lib.ptr(out.get('img')), _lib.ptr(out.get('stats')),
                                                 _lib.stream()), 'orn_engine_decode_frames')
        self._decode_keep = (embeds, frames, rows)          # alive until the stream has drained
        return out

    def _target_frames(self, frames: torch.Tensor, what: str = '', hw=None) -> torch.Tensor:
        """Target frames as the engine reads them: fp32 [N,3,h,w] on the device at `hw` (default: the decoder's output size).  fp32
        [N,3,H,W] or uint8 [N,H,W,3] (as PIL decodes it) of another size are pooled there as the reference pools every target,
        F.adaptive_avg_pool2d(data, output.shape[-2:]) (main_train.py:239,420; main_eval.py:467,807), by ops.ingest_frames."""
        hw = tuple(self.out_hw if hw is None else hw)
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise OrnError(f'{what}frames must be a [N,3,H,W] tensor (or uint8 [N,H,W,3]), got {tuple(getattr(frames, "shape", ()))}')
        if frames.dtype == torch.uint8:
            if frames.shape[3] != 3:
                raise OrnError(f'{what}uint8 frames {tuple(frames.shape)} are not [N,H,W,3]')
            return ops.ingest_frames(frames.to(self.device), hw)
        if frames.shape[1] != 3:
            raise OrnError(f'{what}frames {tuple(frames.shape)} are not [N,3,H,W]')
        frames = frames.to(self.device, torch.float32).contiguous()
        if tuple(frames.shape[2:]) != hw:
            frames = ops.ingest_frames(frames, hw)
        return frames

    def stage_targets(self, frames=None, stages: Optional[Sequence[int]] = None) -> dict:
        """{stage: target table fp32 [N,3,H_i,W_i]} as decode_stages reads them.  frames: a list with one table per stage of `stages`
        (any table not at its stage's size is pooled there), or ONE tensor, pooled to every stage from itself as the reference pools
        every stage's target from the source (main_train.py:420); None: the resident tables (TrainEngine.set_video), where there are any."""
        hws = self.stage_hw()
        stages = list(range(len(hws))) if stages is None else list(stages)
        out = {}
        if frames is None:
            resident = list(getattr(self, 'stage_frames', None) or []) + [self.frames]
            for s in stages:
                if len(resident) == len(hws) and resident[s] is not None:
                    out[s] = resident[s]
                elif s == len(hws) - 1 and self.frames is not None:
                    out[s] = self.frames
            return out
        if isinstance(frames, (list, tuple)):
            if len(frames) != len(stages):
                raise OrnError(f'decode_stages: {len(frames)} frame tables for {len(stages)} stages (one per requested stage, or one tensor)')
            return {s: self._target_frames(t, f'decode_stages: stage {s}: ', hws[s]) for s, t in zip(stages, frames)}
        return {s: self._target_frames(frames, 'decode_stages: ', hws[s]) for s in stages}

    def decode_stages(self, stages=None, rows=None, embeds=None, frames=None, rgb8=True, f32=False, stats=True, msssim=False,
                      chunk=None) -> dict:
        """decode_frames for any stage of a multi-resolution fit (orn_engine_eval_stages; main_train.py:378-438): one forward per frame
        up to the highest stage asked for -- the blocks above it and the last head do not run -- and one output launch per stage.
        stages: an int, a sequence, or None for all.  frames: as stage_targets (one table per requested stage, or one tensor pooled to
        every stage; default: the resident tables).  Returns {stage: dict} with decode_frames' keys at that stage's size: 'rgb8'
        [n,H_i,W_i,3], 'img' [n,3,H_i,W_i], 'stats' [n,4], 'msssim' [n] (zeros for a stage less than 160 high, utils.msssim_fn's rule).
        The last stage's entries are the bytes decode_frames gives.  Needs a multi-resolution engine (a TrainEngine of such a model,
        or Decoder(stages=True)) for any stage below the last.  No host sync."""
        hws = self.stage_hw()
        nl = len(hws)
        sel = list(range(nl)) if stages is None else [stages] if isinstance(stages, int) else [int(s) for s in stages]
        if not sel or len(set(sel)) != len(sel) or min(sel) < 0 or max(sel) >= nl:
            raise OrnError(f'decode_stages: stages {sel} must be distinct indices in [0, {nl})')
        embeds = self.embeds if embeds is None else embeds.to(self.device, torch.float32).contiguous()
        if embeds is None:
            raise OrnError('decode_stages: no embeds given and no video resident (set_video)')
        if embeds.dim() != 2 or embeds.shape[1] != self.desc.embed_len:
            raise OrnError(f'decode_stages: embeds {tuple(embeds.shape)} vs (*, {self.desc.embed_len})')
        need = stats or msssim
        targets = self.stage_targets(frames, sel) if need else {}
        if need and any(s not in targets for s in sel):
            raise OrnError(f'decode_stages: stats and msssim need target frames of stages {[s for s in sel if s not in targets]} '
                           '(frames=, or set_video on a multi-resolution TrainEngine)')
        if rows is None:
            rows = torch.arange(embeds.shape[0], dtype=torch.int32)
        rows = torch.as_tensor(rows).to(torch.int32).reshape(-1)
        n = int(rows.numel())
        limit = min([embeds.shape[0]] + [t.shape[0] for t in targets.values()])
        if n and (int(rows.min()) < 0 or int(rows.max()) >= limit):        # the device would read out of bounds
            raise OrnError(f'decode_stages: row index out of range [0, {limit})')
        rows = rows.to(self.device).contiguous()
        recs = (_lib.StageOut * _lib.ORN_MAX_LAYERS)()
        result, mask, wanted, zero_col = {}, 0, False, False
        for s in sel:
            H, W = hws[s]
            out = result[s] = {}
            if rgb8:
                out['rgb8'] = torch.empty(n, H, W, 3, dtype=torch.uint8, device=self.device)
            if f32:
                out['img'] = torch.empty(n, 3, H, W, device=self.device)
            if stats:
                out['stats'] = torch.empty(n, 4, device=self.device)
            ms = None
            if msssim and H < 160:                          # utils.msssim_fn (utils.py:201-211): no MS-SSIM below 160 rows
                out['msssim'] = torch.zeros(n, device=self.device)
                zero_col = True
            elif msssim:
                ms = out['msssim'] = torch.empty(n, device=self.device)
                mask |= 1 << s
            r = recs[s]
            r.rgb8, r.img, r.stats, r.msssim = (_lib.ptr(t) for t in (out.get('rgb8'), out.get('img'), out.get('stats'), ms))
            if stats or ms is not None:
                r.targets = _lib.ptr(targets[s])
            wanted = wanted or rgb8 or f32 or stats or ms is not None
        ws = None
        if mask and n:
            c = max(1, min(n, chunk or 8))
            nbytes = lib().orn_engine_eval_stages_ws_bytes(byref(self.desc), mask, c)
            if nbytes == 0:
                raise OrnError(f'decode_stages: MS-SSIM needs images larger than 160 x 160 (stages {[hws[s] for s in sel]})')
            ws = getattr(self, '_stages_ws_buf', None)
            if ws is None or ws.numel() < nbytes:
                ws = self._stages_ws_buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if wanted or not zero_col:      # (zero columns alone need no decode; no output at all is the library's error)
            check(lib().orn_engine_eval_stages(self._h, _lib.ptr(embeds), _lib.ptr(rows), c_int32(n), recs, _lib.ptr(ws),
                                               c_size_t(ws.numel() if ws is not None else 0), _lib.stream()), 'orn_engine_eval_stages')
        self._decode_keep = (embeds, targets, rows)         # alive until the stream has drained
        return result

    def _eval_ws(self, chunk: int) -> torch.Tensor:
        """The workspace of orn_engine_eval_frames for `chunk` frames, cached on the object (kept alive; it only grows)."""
        nbytes = lib().orn_engine_eval_frames_ws_bytes(byref(self.desc), chunk)
        if nbytes == 0:
            raise OrnError(f'decode_frames: MS-SSIM needs an image larger than 160 x 160 (decoder output {tuple(self.out_hw)})')
        ws = getattr(self, '_eval_ws_buf', None)
        if ws is None or ws.numel() < nbytes:
            ws = self._eval_ws_buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            try:
                lib().orn_engine_destroy(h)
                self._h = c_void_p()
            except Exception:          # interpreter shutdown: module globals may already be gone
                pass


class Decoder(_Decoding):
    """Decode-only engine for a fitted model (loaded from a train-mode or a `_deploy` checkpoint, checkpoint.load_into): the
    parameter arena and the workspace, no gradient or Adam arenas -- the training entry points refuse such an engine.
    precision: 'fp16' | 'bf16' run the blocks on 16-bit MFMA as the training engine does (the arithmetic a fit at that
    precision was evaluated with); 'fp32' is the reference's.  stages=True (multi-resolution models only): the engine also knows the
    heads of the stages below the last, for decode_stages."""

    def __init__(self, model, precision: str = 'fp16', device: Optional[torch.device] = None, stages: bool = False):
        if stages and not is_multi_res(model):
            raise OrnError('Decoder(stages=True) needs a multi-resolution model (a head on every stage; Generator(sin_res=False))')
        self._rehome(model, device, grads=False)
        # (by default a multi-resolution model decodes its last stage: the single-resolution engine on the tensors the two share;
        # stages=True describes every stage's head, so that decode_stages reaches the stages below the last)
        self._create(precision, False, 'L2', multi_res=bool(stages))


class TrainEngine(_Decoding):
    """Native training engine for one video (one process / one GPU per video)."""

    def __init__(self, model, loss_type: str = 'Fusion6', beta: float = 0.5, precision: str = 'fp32',
                 device: Optional[torch.device] = None, n_slots: int = 4096, target_cache: bool = True, lw: float = 1.0):
        self._rehome(model, device, grads=True)                # parameters now live in the arena, their grads in the grad arena
        dev = self.device
        # a model with a head on every stage (Generator(sin_res=False)) trains them all: sum_{i < n-1} lw * loss_i + loss_{n-1}
        self._create(precision, True, loss_type, beta, lw=lw)
        self.multi_res = bool(self.desc.multi_res)
        self.target_cache = bool(target_cache) and _lib.loss_spec(loss_type)[1] == _lib.LOSS_KIND_SSIM
        self.tstats = None
        self.n_slots = n_slots
        self.stats_ring = torch.zeros(n_slots, 8, device=dev)
        self.stage_ring = None
        self.stage_frames, self.stage_tstats = [], []
        if self.multi_res:                                 # {loss_i, psnr_i} of every stage, beside each step's record
            self.stage_ring = torch.zeros(n_slots, self.desc.n_layers, 2, device=dev)
            check(lib().orn_engine_set_stage_stats(self._h, _lib.ptr(self.stage_ring), c_int32(n_slots)), 'orn_engine_set_stage_stats')
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sched = None
        self.frames = None
        self.embeds = None
        self._sched_host = None                            # host copy of the uploaded schedule and of the device cursor: which
        self._cursor_host = 0                              # frame the next step takes is known without a sync (step_with)
        self._sched_len = 0
        self._batch_max = 0                                # frames the batch workspace takes (run_batched; 0: none yet)
        self.open_frame = None
        self.global_step = 0
        self.skipped_carry = 0                             # steps skipped by engines this one replaced (main_train fall-back)
        # HIP graphs cannot be captured on the legacy default stream: the engine runs on its own
        # stream, ordered against the caller's current stream on entry and exit.
        self.stream = torch.cuda.Stream(device=dev)

    @contextlib.contextmanager
    def _on_stream(self):
        """Orders the engine's stream behind the caller's current one, yields its handle, then orders the caller's behind it."""
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        yield c_void_p(self.stream.cuda_stream)
        cur.wait_stream(self.stream)

    def _step_args(self):
        """What every stepping entry takes first: the handle, the resident video, the schedule with its cursor, the stats ring."""
        if self.frames is None or self.sched is None:
            raise OrnError('set_video() and set_schedule() first')
        return [self._h, _lib.ptr(self.frames), _lib.ptr(self.embeds), _lib.ptr(self.sched), _lib.ptr(self.cursor),
                _lib.ptr(self.stats_ring), c_int32(self.n_slots)]

    # ---- data ---------------------------------------------------------------------------------
    def set_video(self, frames: torch.Tensor, embeds: torch.Tensor, stage_frames: Optional[Sequence[torch.Tensor]] = None):
        """frames [N,3,H,W] fp32 in [0,1] (resident in HBM), embeds [N,E] (PE of k/N).  Frames of another size than the decoder's
        output, or uint8 [N,H,W,3], are pooled to it once, on the device (_target_frames): the target-statistics cache, the
        schedule, every step form and the evaluation see the pooled table only.
        A multi-resolution engine also needs every lower stage's target, adaptive_avg_pool2d of the SOURCE frames to that stage's size
        (main_train.py:239): pooled here from `frames` as given, or taken from stage_frames (one fp32 [N,3,H_i,W_i] table per stage
        below the last) when the caller has pooled a source it does not keep resident (a frame directory read piece by piece)."""
        source = frames
        frames = self._target_frames(frames)
        if embeds.shape != (frames.shape[0], self.desc.embed_len):
            raise OrnError(f'embeds {tuple(embeds.shape)} vs ({frames.shape[0]}, {self.desc.embed_len})')
        self.frames = frames
        self.embeds = embeds.to(self.device, torch.float32).contiguous()
        # SSIM kinds (SSIM, Fusion1-6, Fusion9: the maps are the same): the target side of the SSIM statistics, once per video (two valid-map planes per image plane: 2.9 GB for
        # 132 frames of 720p, 29 GB for 600 of 1080p, of 288 GB); the step then filters three maps instead of five.
        # Skipped when it does not fit beside the video with room to spare.
        self.tstats = None
        check(lib().orn_engine_set_target_stats(self._h, None), 'orn_engine_set_target_stats')
        if self.target_cache:
            n, _, H, W = self.frames.shape
            nbytes = lib().orn_loss_target_stats_bytes(n, 3, H, W)
            free, _ = torch.cuda.mem_get_info(self.device)
            if 0 < nbytes < free // 2:
                self.tstats = torch.empty(nbytes // 4, device=self.device)
                cur = torch.cuda.current_stream()
                check(lib().orn_loss_target_stats(_lib.ptr(self.frames), n, 3, H, W, _lib.ptr(self.tstats), c_void_p(cur.cuda_stream)),
                      'orn_loss_target_stats')
                check(lib().orn_engine_set_target_stats(self._h, _lib.ptr(self.tstats)), 'orn_engine_set_target_stats')
        if self.multi_res:
            self._set_stage_tables(source, stage_frames)

    def _set_stage_tables(self, source: torch.Tensor, given=None):
        """The target table of every stage below the last: F.adaptive_avg_pool2d(data, out_i.shape[-2:]) of main_train.py:239, pooled
        from the SOURCE pixels (not from the last stage's table) by ops.ingest_frames, as the last stage's table is; and, for the
        SSIM kinds, the target side of its SSIM statistics."""
        src = source.to(self.device)
        src = src.contiguous() if src.dtype == torch.uint8 else src.to(torch.float32).contiguous()
        self.stage_frames, self.stage_tstats = [], []
        cur = c_void_p(torch.cuda.current_stream().cuda_stream)
        for i, (h, w) in enumerate(self.stage_hw()[:-1]):
            if given is not None:
                tab = given[i].to(self.device, torch.float32).contiguous()
                if tuple(tab.shape) != (self.frames.shape[0], 3, h, w):
                    raise OrnError(f'set_video: stage_frames[{i}] {tuple(tab.shape)} vs {(self.frames.shape[0], 3, h, w)}')
            else:
                tab = ops.ingest_frames(src, (h, w))
            self.stage_frames.append(tab)
            check(lib().orn_engine_set_stage_targets(self._h, i, _lib.ptr(tab)), 'orn_engine_set_stage_targets')
            ts = None
            nbytes = lib().orn_loss_target_stats_bytes(tab.shape[0], 3, h, w) if self.target_cache else 0
            if 0 < nbytes < torch.cuda.mem_get_info(self.device)[0] // 2:
                ts = torch.empty(nbytes // 4, device=self.device)
                check(lib().orn_loss_target_stats(_lib.ptr(tab), tab.shape[0], 3, h, w, _lib.ptr(ts), cur), 'orn_loss_target_stats')
            self.stage_tstats.append(ts)
            check(lib().orn_engine_set_stage_target_stats(self._h, i, _lib.ptr(ts)), 'orn_engine_set_stage_target_stats')

    def set_schedule(self, entries: Sequence[Tuple[int, int, float]]):
        """Upload the next run's per-step (frame, global step, lr) entries and rewind the cursor."""
        arr = make_schedule(entries)
        if self.frames is not None and len(entries) and (arr[:, 0].min() < 0 or arr[:, 0].max() >= self.frames.shape[0]):
            raise OrnError('schedule frame index out of range')
        if self.sched is None or self.sched.shape[0] < arr.shape[0]:
            self.sched = torch.zeros(max(arr.shape[0], 1), 4, dtype=torch.int32, device=self.device)
        self.sched[:arr.shape[0]].copy_(torch.from_numpy(arr), non_blocking=False)
        self.cursor.zero_()
        self._sched_len = arr.shape[0]
        self._sched_host, self._cursor_host = arr, 0

    # ---- stepping -----------------------------------------------------------------------------
    def run(self, n_steps: int, graph=None, batch: int = 1):
        """Enqueue `n_steps` optimiser steps consuming the uploaded schedule (no host sync).
        batch > 1 (-b B, main_train.py:205-254): every optimiser step takes `batch` consecutive schedule entries -- the caller
        uploads n_steps * batch of them -- and applies the mean of their frames' gradients (orn_engine_train_steps_batch: serial
        form, no graph form); `global_step` and applied_steps() count optimiser steps.
        graph=None (default): orn_engine_train_steps -- plain stream launches, pipelined over the engine's second stream where the
        engine can (16-bit modes; include/orn.h); graph=True: hipGraph replay of the serial step; graph=False: one
        orn_engine_train_step call per step.  All three give bit-identical results, except for a step that only the pipelined form's
        late overflow checks flag (a late-only skip: the serial forms skip the whole step, the pipelined form all but the lower
        blocks' update; counted in scale_state()['late_skipped'], include/orn.h)."""
        if batch != 1:
            if graph:
                raise OrnError('run: the batched step has no graph form (graph=True with batch > 1)')
            return self.run_batched(n_steps, batch)
        args = self._step_args()
        with self._on_stream() as st:
            if graph is None:
                check(lib().orn_engine_train_steps(*args, c_int32(n_steps), st), 'orn_engine_train_steps')
            elif graph:
                check(lib().orn_engine_train_steps_graph(*args, c_int32(n_steps), st), 'orn_engine_train_steps_graph')
            else:
                for _ in range(n_steps):
                    check(lib().orn_engine_train_step(*args, st), 'orn_engine_train_step')
        self.global_step += n_steps
        self._cursor_host += n_steps

    def run_batched(self, n_steps: int, batch: int):
        """`n_steps` optimiser steps of `batch` frames each through orn_engine_train_steps_batch (what run() calls for batch > 1;
        batch = 1 gives the bits of the single-frame step).  The batch workspace is allocated on first use and grows with `batch`."""
        args = self._step_args()
        if not 1 <= batch <= _lib.ORN_MAX_BATCH:
            raise OrnError(f'run: batch={batch} outside [1, {_lib.ORN_MAX_BATCH}]')
        if n_steps * batch > self._sched_len:
            raise OrnError(f'run: {n_steps} steps of {batch} frames need {n_steps * batch} schedule entries, {self._sched_len} uploaded')
        if self._batch_max < batch:
            nbytes = lib().orn_engine_batch_ws_bytes(byref(self.desc), batch)
            if nbytes == 0:
                raise OrnError('orn_engine_batch_ws_bytes: ' + _lib.last_error())
            torch.cuda.synchronize()                            # (steps in flight may still use the workspace this one replaces)
            self._batch_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            check(lib().orn_engine_set_batch_ws(self._h, _lib.ptr(self._batch_ws), c_size_t(nbytes), batch), 'orn_engine_set_batch_ws')
            self._batch_max = batch
        with self._on_stream() as st:
            check(lib().orn_engine_train_steps_batch(*args, c_int32(n_steps), c_int32(batch), st), 'orn_engine_train_steps_batch')
        self.global_step += n_steps
        self._cursor_host += n_steps * batch

    # ---- the split step: a caller-supplied loss (orn_engine_step_forward / orn_engine_step_backward) --------------------------
    def forward_step(self) -> torch.Tensor:
        """First half of one optimiser step: the schedule advance and the training forward, enqueued without a host sync.
        Returns the engine's output as a [1,3,H,W] fp32 VIEW into its workspace (no copy), ordered before the caller's current
        stream.  The step is now open: until backward_step() every other stepping or decoding call of this engine raises OrnError.
        `open_frame` holds the index of the step's frame (its target is frames[open_frame]), from the host copy of the schedule."""
        if self.multi_res:
            raise OrnError('forward_step: a multi-resolution engine has no split step (a caller-supplied objective takes one image; '
                           'build the model with sin_res=True)')
        *args, _ring, n_slots = self._step_args()
        if self._cursor_host >= self._sched_len:
            raise OrnError(f'forward_step: the uploaded schedule ({self._sched_len} entries) is used up')
        pred = c_void_p()
        with self._on_stream() as st:
            check(lib().orn_engine_step_forward(*args, n_slots, byref(pred), st), 'orn_engine_step_forward')
        self.open_frame = int(self._sched_host[self._cursor_host, 0])
        self._cursor_host += 1
        H, W = self.out_hw
        off = pred.value - self.ws.data_ptr()                   # the pointer lies inside the engine's workspace tensor
        assert 0 <= off and off + 12 * H * W <= self.ws.numel(), 'image pointer outside the workspace'
        return self.ws[off:off + 12 * H * W].view(torch.float32).view(1, 3, H, W)

    def backward_step(self, dpred: Optional[torch.Tensor], loss: Optional[torch.Tensor] = None):
        """Second half: the backward from dpred = dLoss/dpred of the UNSCALED loss ([1,3,H,W] or [3,H,W], fp32, contiguous, on the
        engine's device; read in place), merge backward and Adam, enqueued without a host sync.  loss: optional one-element device
        tensor, the step's stats[0].  A NaN / inf in either skips the step (scale_state()['skipped']).  dpred=None abandons the
        open step: nothing is applied and it counts as skipped."""
        H, W = self.out_hw
        if dpred is not None:
            if not isinstance(dpred, torch.Tensor) or not dpred.is_cuda or dpred.device != self.device:
                raise OrnError(f'backward_step: dpred must be a tensor on {self.device}')
            if dpred.dtype != torch.float32 or tuple(dpred.shape) not in ((1, 3, H, W), (3, H, W)):
                raise OrnError(f'backward_step: dpred {dpred.dtype} {tuple(dpred.shape)} vs float32 (1, 3, {H}, {W})')
            if not dpred.is_contiguous():
                raise OrnError('backward_step: dpred must be contiguous')
        if loss is not None:
            if not isinstance(loss, torch.Tensor) or not loss.is_cuda or loss.device != self.device or loss.numel() != 1:
                raise OrnError(f'backward_step: loss must be a one-element tensor on {self.device}')
            loss = loss.detach().to(torch.float32).reshape(1)
        with self._on_stream() as st:
            check(lib().orn_engine_step_backward(self._h, _lib.ptr(self.frames), _lib.ptr(self.embeds), _lib.ptr(dpred), _lib.ptr(loss),
                                                 _lib.ptr(self.stats_ring), c_int32(self.n_slots), st), 'orn_engine_step_backward')
        for t in (dpred, loss):                                 # allocated on the caller's stream, read on the engine's
            if t is not None:
                t.record_stream(self.stream)
        self._seam_keep = (dpred, loss)
        self.global_step += 1

    def step_with(self, fn) -> torch.Tensor:
        """One optimiser step on the objective fn(pred, target) -> scalar tensor: pred is the engine's output [1,3,H,W] (a leaf that
        requires grad, sharing the engine's memory), target the step's frame [1,3,H,W]; fn is built from torch ops (and ops.LossFn)
        on the current stream.  Its gradient comes from torch.autograd.grad; forward, backward, merge backward, Adam, the
        non-finite guard and the loss scale stay on the engine.  No host sync.  If fn raises, the step is abandoned (counted as
        skipped) and the exception propagates.  Returns the detached loss."""
        pred = self.forward_step().detach().requires_grad_(True)
        target = self.frames[self.open_frame:self.open_frame + 1]
        try:
            with torch.enable_grad():
                loss = fn(pred, target)
                if not isinstance(loss, torch.Tensor) or loss.numel() != 1:
                    raise OrnError('step_with: fn(pred, target) must return a one-element tensor')
                (g,) = torch.autograd.grad(loss.reshape(()), pred)
        except BaseException:
            self.backward_step(None)
            raise
        loss = loss.detach()
        self.backward_step(g.contiguous(), loss)
        return loss

    def run_with(self, fn, n_steps: int):
        """`n_steps` optimiser steps of step_with(fn), consuming the uploaded schedule like run() (single frame per step; no
        batched, pipelined or graph form)."""
        for _ in range(n_steps):
            self.step_with(fn)

    def set_grad_mask(self, masks=None):
        """0/1 gradient masks per parameter name ({name: tensor like the parameter}; missing names = 1); None removes
        the mask.  Used by the prune fine-tune (main_eval.py:213-531)."""
        if masks is None:
            self._gmask = None
            check(lib().orn_engine_set_grad_mask(self._h, None), 'orn_engine_set_grad_mask')
            return
        gm = torch.ones(self.n_params, device=self.device)
        for k, m in masks.items():
            off, n = self.layout[k]
            gm[off:off + n] = m.to(self.device, torch.float32).reshape(-1)
        self._gmask = gm                                    # keep alive: the engine holds the raw pointer
        check(lib().orn_engine_set_grad_mask(self._h, _lib.ptr(gm)), 'orn_engine_set_grad_mask')

    def profile_step(self):
        """One eager optimiser step with HIP events around the conv launches, on the engine's stream.  Returns a dict of
        host lists / floats in ms: 'fwd'[i] forward conv of layer i, 'dgrad'[i] dgrad launch of layer i (fp32 mode: the
        layer's whole backward call), 'wgrad' the batched wgrad launch of the 16-bit layers, 'wgrad_reduce' its split-K
        reduction.  Consumes one schedule entry; synchronises."""
        args = self._step_args()
        n = self.desc.n_layers
        ms = (ctypes.c_float * (2 * n + 2))()
        with self._on_stream() as st:
            check(lib().orn_engine_profile_step(*args, ms, st), 'orn_engine_profile_step')
        self.global_step += 1
        self._cursor_host += 1
        v = [float(x) for x in ms]
        return {'fwd': v[:n], 'dgrad': v[n:2 * n], 'wgrad': v[2 * n], 'wgrad_reduce': v[2 * n + 1]}

    def applied_steps(self) -> int:
        """Optimiser steps that changed the parameters so far: enqueued steps minus the ones the non-finite guard skipped, in this
        engine (device counter) and in engines it replaced (`skipped_carry`, set by main_train's precision fall-back).  This is
        torch.optim.Adam's 'step' of a checkpoint (include/orn.h).  A late-only skip of the pipelined form does not come off: the lower
        blocks applied that step.  Synchronises."""
        return int(self.global_step - self.skipped_carry - self.scale_state()['skipped'])

    def scale_state(self) -> dict:
        """Dynamic loss scale / non-finite guard of the engine (device state; synchronises): scale, ceiling, flag, steps
        skipped so far, clean steps since the last change, halvings, late-only skips of the pipelined form so far (the last block's
        and the head's update skipped, the lower blocks' applied; include/orn.h)."""
        out = (ctypes.c_float * 8)()
        check(lib().orn_engine_scale_state(self._h, out), 'orn_engine_scale_state')
        return {'scale': float(out[0]), 'ceiling': float(out[2]), 'flag': int(out[3]), 'skipped': int(out[4]),
                'good': int(out[5]), 'backoffs': int(out[6]), 'late_skipped': int(out[7])}

    def set_grad_scale(self, scale: float, ceiling: float = 0.0):
        """Override the live gradient scale of the 16-bit modes (and its ceiling if > 0)."""
        check(lib().orn_engine_set_grad_scale(self._h, ctypes.c_float(scale), ctypes.c_float(ceiling)), 'orn_engine_set_grad_scale')

    def stats(self, n: int) -> torch.Tensor:
        """[n,8] host tensor of the last run's first n steps: loss, L1, MSE, SSIM, PSNR, lr, frame, step."""
        return self.stats_ring[:n].cpu()

    def stage_stats(self, n: int) -> torch.Tensor:
        """[n, n_stages, 2] host tensor of the last run's first n steps (multi-resolution engine): the un-weighted loss and the PSNR of
        every stage, the last stage in the last row.  After a batched run: the frames of the last optimiser step, in batch order."""
        if self.stage_ring is None:
            raise OrnError('stage_stats: not a multi-resolution engine')
        return self.stage_ring[:n].cpu()

    def engine_fused_kernel(self, layer: int):
        """(Wf, bf) of block `layer` exactly as the ENGINE's last merge left them in its workspace (copies; ERB, ACB, RepVGG, ECB)."""
        wf, bf = c_void_p(), c_void_p()
        check(lib().orn_engine_fused_kernel(self._h, layer, byref(wf), byref(bf)), 'orn_engine_fused_kernel')
        shape = tuple(dict(self.model.named_parameters())[f'layers.{layer}.rbr_3x3_branch.weight'].shape)
        n = shape[0] * shape[1] * 9
        torch.cuda.synchronize()
        base = self.ws.data_ptr()

        def view(ptr, cnt):                       # the pointers lie inside the engine's workspace tensor
            off = ptr - base
            assert 0 <= off and off + 4 * cnt <= self.ws.numel(), 'fused kernel pointer outside the workspace'
            return self.ws[off:off + 4 * cnt].view(torch.float32).clone()
        return view(wf.value, n).view(shape), view(bf.value, shape[0])

    def fused_kernel(self, layer: int):
        """(Wf, bf) of block `layer` as produced by the last merge (model.py:450-478), as tensors."""
        blk = self.model.layers[layer]
        if self.desc.erb or self.desc.branch_kind:
            with torch.no_grad():
                return blk.get_equivalent_kernel_bias()
        conv = blk.rbr_reparam if blk.deploy else blk.branch
        return conv.weight, conv.bias
