"""The reference's Python call surface for the hot path, backed by the HIP engine.

Mirrors, name for name and argument for argument, what src/deepCam/train_hdf5_ddp.py calls in its step loop:

  architecture/deeplab_xception.py:398-465   DeepLabv3_plus(n_input, n_classes, os, pretrained, rank) / .forward
  utils/losses.py:28-52                      fp_loss(logit, target, weight, fpw_1, fpw_2)
  utils/utils.py:32-60                       compute_score(prediction, gt, num_classes, device_id)
  train_hdf5_ddp.py:213-218                  optim.Adam / optim.AdamW / apex FusedLAMB  -> Adam, AdamW, LAMB below
  utils/parsing_helpers.py:27-37             get_lr_schedule(start_lr, scheduler_arg, optimizer, last_step)
  train_hdf5_ddp.py:251-253                  GradualWarmupScheduler(optimizer, multiplier, total_epoch, after_scheduler)

so ``outputs = net.forward(inputs); loss = fp_loss(...); optimizer.zero_grad(); loss.backward(); optimizer.step()``
runs unmodified.  ``TrainStep`` is the same sequence without the autograd round trip (what bench.py and train.py use).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from collections import OrderedDict
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from . import ops as _ops
from .engine import Engine

CLASS_FREQ = (0.986267818390377, 0.0004578708870701058, 0.01327431072255291)   # train_hdf5_ddp.py:206


def class_weights(loss_pow: float = -0.125) -> List[float]:
    return [f ** loss_pow for f in CLASS_FREQ]


# ------------------------------------------------------------------------------------------------------------------
# loss / metric
# ------------------------------------------------------------------------------------------------------------------
_cw_cache: Dict[tuple, torch.Tensor] = {}
_dlogits_for: Dict[int, torch.Tensor] = {}      # logits.data_ptr() -> engine-owned gradient buffer (zero-copy hand-over)


def _cw_tensor(weight: Sequence[float], device) -> torch.Tensor:
    key = (tuple(float(w) for w in weight), str(device))
    t = _cw_cache.get(key)
    if t is None:
        # losses.py:35 goes list -> numpy float64 -> float32
        t = torch.from_numpy(np.array(weight)).float().to(device)
        _cw_cache[key] = t
    return t


def wce_fused(logit: torch.Tensor, target: torch.Tensor, weight: Sequence[float], dlogits: Optional[torch.Tensor] = None,
              pred: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
              loss_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass over the logits: returns the fp64 loss SUM tensor [1]; optionally fills dlogits / pred / counts."""
    if logit.dim() != 4 or logit.size(1) != 3:
        raise L.DeepcamHipError("fp_loss: logits must be [B,3,H,W]")
    if logit.dtype != torch.float32 or not logit.is_contiguous():
        logit = logit.float().contiguous()
    B, _, H, W = logit.shape
    t = target.squeeze(1) if target.dim() == 4 else target
    if t.dtype not in (torch.uint8, torch.int32, torch.int64):
        t = t.long()
    if not t.is_contiguous():
        t = t.contiguous()
    if tuple(t.shape) != (B, H, W):
        raise L.DeepcamHipError(f"fp_loss: target shape {tuple(t.shape)} does not match logits {tuple(logit.shape)}")
    if loss_sum is None:
        loss_sum = torch.zeros(1, dtype=torch.float64, device=logit.device)
    _ops.OPS.wce_fused(logit, t, _cw_tensor(weight, logit.device), 1.0 / float(B * H * W), loss_sum, dlogits, pred, counts)
    return loss_sum


class _FpLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, target, weight):
        dl = _dlogits_for.get(logit.data_ptr())
        if dl is None or dl.shape != logit.shape:
            dl = torch.empty_like(logit, dtype=torch.float32)
        s = wce_fused(logit.detach(), target, weight, dlogits=dl)
        ctx.dl = dl
        n = logit.numel() // logit.size(1)
        return (s / n).to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, go):
        dl = ctx.dl
        dl.mul_(go)          # the kernel already produced d(mean)/d(logit); autograd's incoming scalar is usually 1
        return dl, None, None


def fp_loss(logit, target, weight, fpw_1=0, fpw_2=0):
    """mean over B*H*W of w[y]*CE(logit, y).  fpw_1 / fpw_2 are accepted and ignored exactly like the reference, whose
    false-positive masks are identically zero (losses.py:41,46)."""
    return _FpLoss.apply(logit, target, weight)


def iou_from_counts(counts) -> float:
    c = [int(v) for v in counts]
    ious = []
    for j in range(3):
        union = c[j] + c[3 + j] + c[6 + j]
        ious.append(np.float32(1.0) if union == 0 else np.float32(c[j]) / np.float32(union))   # utils.py:55-58
    return float(np.float32(ious[0] + ious[1] + ious[2]) / np.float32(3.0))


def compute_score(prediction, gt, num_classes=3, device_id=None, type="iou", weights=None):
    if num_classes != 3:
        raise L.DeepcamHipError("compute_score: the fused kernel is built for the 3 DeepCAM classes")
    pred = prediction if prediction.dtype == torch.int64 else prediction.long()
    pred = pred.contiguous()
    g = gt if gt.dtype in (torch.uint8, torch.int32, torch.int64) else gt.long()
    g = g.contiguous()
    counts = torch.zeros(9, dtype=torch.int64, device=pred.device)
    _ops.OPS.confusion_counts(pred, g, counts)
    return torch.tensor(iou_from_counts(counts.cpu().tolist()), dtype=torch.float32, device=pred.device)


# ------------------------------------------------------------------------------------------------------------------
# model
# ------------------------------------------------------------------------------------------------------------------
class _NetFn(torch.autograd.Function):
    """Train mode: the primary engines (batch statistics).  Eval mode with autograd on: the frozen-BatchNorm engines (running statistics in
    forward and backward), so that ``net.eval(); loss.backward()`` differentiates what the eval forward computed."""

    @staticmethod
    def forward(ctx, x, anchor, module):
        frozen = not module.training
        eng = module.engine_for(x, frozen=frozen)
        ctx.eng, ctx.module, ctx.frozen = eng, module, frozen
        ctx.x_meta = (tuple(x.shape), x.dtype, x.device)
        out = _ops.OPS.net_forward(x, _ops.engine_handle(eng), module.training)
        if len(_dlogits_for) > 64:               # engines come and go with input shapes: drop entries of freed buffers
            _dlogits_for.clear()
        _dlogits_for[out.data_ptr()] = eng.dlogits
        return out

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.eng
        if ctx.frozen and ctx.module._ddp_reducer is not None:
            raise NotImplementedError("backward through the model in eval mode (frozen BatchNorm) is not supported under DistributedDataParallel: "
                                      "the gradient reducer is wired to the train-mode engines; call net.train(), or run the eval-mode backward "
                                      "on the unwrapped module of one process")
        # torch semantics: a backward() that arrives without an optimizer.zero_grad() / step() since the previous one ACCUMULATES into p.grad.
        # The engine's backward program writes every parameter's gradient exactly once (it overwrites), so the gradients of the earlier
        # backward calls are set aside first and added back behind this one -- a 226 MB copy and add on the micro-batch path only; the
        # reference's loop (zero_grad before every backward, train_hdf5_ddp.py:358-364) never takes it.
        stash = None
        if eng.grads_live[0]:
            if getattr(ctx.module, "_grad_stash", None) is None:      # (one per module: its engines share the arena)
                ctx.module._grad_stash = torch.empty_like(eng.grads)
            stash = ctx.module._grad_stash
            stash.copy_(eng.grads)
        eng.grads_live[0] = True
        _ops.OPS.net_backward(dlogits, _ops.engine_handle(eng))
        red = ctx.module._ddp_reducer
        if red is not None:
            # under dist.DistributedDataParallel: wait for the bucketed all-reduces launched during backward, re-arm the
            # buckets and leave the AVERAGED gradient in the arena (train_hdf5_ddp.py:227,363).  A reducer that a fused TrainStep
            # has taken over averages inside the optimizer kernel: finish(average=True) refuses (the gradients would otherwise be
            # scaled twice, or -- had the reference been dropped -- the buckets launched by this backward would never be waited for)
            red.finish(average=True)
        dx = None
        if ctx.needs_input_grad[0]:
            # dL/dx: the stem's data gradient over the stem output's gradient this backward has just left (Engine.input_grad); the parameter
            # gradients above do not depend on it
            shape, dtype, device = ctx.x_meta
            if shape != (eng.B, eng.n_input, eng.H, eng.W):
                raise L.DeepcamHipError(f"input gradient: the input must be the NCHW batch {(eng.B, eng.n_input, eng.H, eng.W)}, got {shape}")
            dx = eng.input_grad()
            if dx.dtype != dtype or dx.device != device:
                dx = dx.to(device=device, dtype=dtype)
        if stash is not None:
            eng.grads.add_(stash)
        ctx.module._attach_grads()
        return dx, None, None


class DeepLabv3_plus(torch.nn.Module):
    """Drop-in for architecture.deeplab_xception.DeepLabv3_plus (os=16, DeconvUpsampler).  Parameters are views of the
    engine's flat fp32 arena with the reference's names, so ``state_dict()`` interchanges with reference checkpoints."""

    def __init__(self, n_input=3, n_classes=21, os=16, pretrained=False, normalizer=None, _print=True, rank=0,
                 dtype=torch.bfloat16, seed=None):
        super().__init__()
        if os != 16:
            raise NotImplementedError                       # deeplab_xception.py:140-141,415-416 (train uses os=16)
        if pretrained:
            raise NotImplementedError("pretrained weights need a download (train_hdf5_ddp.py:199 passes False)")
        if _print and rank == 0:
            print("Constructing DeepLabv3+ model...")
            print("Number of output channels: {}".format(n_classes))
            print("Output stride: {}".format(os))
            print("Number of Input Channels: {}".format(n_input))
        self.n_input, self.n_classes, self.act_dtype = n_input, n_classes, dtype
        self._seed = seed
        self._engines: Dict[tuple, Engine] = {}
        self._frozen_engines: Dict[tuple, Engine] = {}      # eval mode with autograd on (frozen BatchNorm), built on first use
        self._primary: Optional[Engine] = None
        self._anchor = None
        self._ddp_reducer = None      # set by dist.DistributedDataParallel
        self._init_seed_state = torch.random.get_rng_state() if seed is None else None

    # -- engines are shape-specialised and built lazily; all of them share one parameter store
    def engine_for(self, x: torch.Tensor = None, shape: tuple = None, frozen: bool = False) -> Engine:
        shp = tuple(x.shape) if x is not None else tuple(shape)
        B, Cin, H, W = shp
        key = (B, H, W)
        if frozen:
            # the frozen-BatchNorm engine of this shape: shares the parameter, gradient and buffer arenas with the primary engine; it is not
            # handed to a gradient reducer (an eval-mode backward under DistributedDataParallel raises in _NetFn.backward)
            feng = self._frozen_engines.get(key)
            if feng is None:
                if self._primary is None:
                    self.engine_for(shape=shp)
                feng = Engine(B, H, W, self.act_dtype, n_input=self.n_input, n_classes=self.n_classes, share_from=self._primary,
                              frozen_bn=True)
                self._frozen_engines[key] = feng
            return feng
        eng = self._engines.get(key)
        if eng is None:
            if self._primary is None:
                if self._seed is None and self._init_seed_state is not None:
                    # reproduce "torch.manual_seed(333); DeepLabv3_plus(...)": draw the weights from the RNG state
                    # that was current when the module was constructed
                    keep = torch.random.get_rng_state()
                    torch.random.set_rng_state(self._init_seed_state)
                    eng = Engine(B, H, W, self.act_dtype, n_input=self.n_input, n_classes=self.n_classes, seed=None)
                    torch.random.set_rng_state(keep)
                else:
                    eng = Engine(B, H, W, self.act_dtype, n_input=self.n_input, n_classes=self.n_classes, seed=self._seed)
                self._primary = eng
                self._register_arena(eng)
            else:
                eng = Engine(B, H, W, self.act_dtype, n_input=self.n_input, n_classes=self.n_classes, share_from=self._primary)
            self._engines[key] = eng
            if self._ddp_reducer is not None:
                self._ddp_reducer.hook(eng)       # every engine that shares the arena reports its gradients to the reducer
        return eng

    def materialize(self, batch: int, height: int, width: int) -> Engine:
        """Build the engine for a given input shape ahead of the first forward (so that .parameters() exists)."""
        return self.engine_for(shape=(batch, self.n_input, height, width))

    def _register_arena(self, eng: Engine) -> None:
        for name in eng.layout.state_keys:
            mod, _, leaf = name.rpartition(".")
            if name in eng.layout.params:
                t = torch.nn.Parameter(eng.param_view(name), requires_grad=True)
                self._flat_register(name, t, is_param=True)
            else:
                self._flat_register(name, eng.buffer_view(name), is_param=False)
        self._anchor = torch.zeros(1, device=eng.device, requires_grad=True)

    def _flat_register(self, name: str, t: torch.Tensor, is_param: bool) -> None:
        # nn.Module wants dotted names to be a module tree: build empty container modules along the path
        parts = name.split(".")
        m = self
        for p in parts[:-1]:
            if p not in m._modules:
                m.add_module(p, torch.nn.Module())
            m = m._modules[p]
        if is_param:
            m.register_parameter(parts[-1], t)
        else:
            m.register_buffer(parts[-1], t)

    def _attach_grads(self) -> None:
        eng = self._primary
        for name, p in self.named_parameters():
            p.grad = eng.grad_view(name)

    def parameters(self, recurse: bool = True):
        if self._primary is None:
            raise L.DeepcamHipError("call net.materialize(batch, H, W) (or run one forward) before asking for parameters: "
                                    "the HIP engine is specialised to the input shape")
        return super().parameters(recurse)

    def to(self, *args, **kwargs):
        # parameters live in HIP memory from the start; .to(device) of the reference is a no-op here
        return self

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if input.dim() != 4 or input.size(1) != self.n_input:
            raise RuntimeError(f"expected input [B,{self.n_input},H,W], got {tuple(input.shape)}")
        if torch.is_grad_enabled() and self.training:
            self.engine_for(input)
            return _NetFn.apply(input, self._anchor, self)
        eng = self.engine_for(input)
        if torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in self.parameters())):
            # eval mode with autograd on (saliency, fine-tuning with frozen statistics): BatchNorm on its running statistics, differentiated
            # as the affine map it then is -- the frozen-BatchNorm engine.  Under no_grad / inference_mode the plain eval forward below runs
            return _NetFn.apply(input, self._anchor, self)
        return _ops.OPS.net_forward(input, _ops.engine_handle(eng), self.training)

    def load_state_dict(self, state_dict, strict: bool = True):
        if self._primary is None:
            raise L.DeepcamHipError("materialize the model before load_state_dict")
        sd = OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state_dict.items())
        r = super().load_state_dict(sd, strict=strict)
        self._primary.mark_weights_changed()
        return r

    @property
    def engine(self) -> Engine:
        return self._primary


# ------------------------------------------------------------------------------------------------------------------
# optimizers over the flat arena
# ------------------------------------------------------------------------------------------------------------------
class ArenaOptimizer:
    """torch.optim.Optimizer surface (param_groups, state_dict, load_state_dict, zero_grad, step) for the fused
    multi-tensor kernels.  state_dict() uses torch.optim.Adam's layout so checkpoints interchange with the reference."""

    kind = L.DC_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, engine: Engine = None):
        params = list(params)
        if engine is None:
            raise L.DeepcamHipError("ArenaOptimizer needs the model's engine (use make_optimizer(net, ...))")
        self.engine = engine
        lay = engine.layout
        if len(params) != len(lay.params):
            raise L.DeepcamHipError("the optimizer must own all model parameters (one arena, one launch)")
        self.param_groups = [dict(params=params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                  maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)]
        dev = engine.device
        self.m = torch.zeros(lay.n_params, dtype=torch.float32, device=dev)
        self.v = torch.zeros(lay.n_params, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.max_grad_norm = max_grad_norm
        self.grad_scale = 1.0
        self.grad_arena: Optional[torch.Tensor] = None     # use_gradients(): read the gradient from here instead of engine.grads
        # learning rate (float32) and step count (int32) side by side: ONE 8-byte host-to-device copy per step
        self._scal_host = torch.zeros(2, dtype=torch.int32).pin_memory()
        self._lr_host = self._scal_host[:1].view(torch.float32)
        self._step_host = self._scal_host[1:]
        self._scalars_copied = None
        self._scal_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        self.lr_dev = self._scal_dev[:1].view(torch.float32)
        self.step_dev = self._scal_dev[1:]
        self._offsets = torch.tensor(lay.offsets(), dtype=torch.int64, device=dev)
        # the LAMB workspace holds an n-element update direction (226 MB): only LAMB allocates it
        self._lamb_ws = (torch.zeros(L.load().dc_lamb_workspace_words(len(lay.params), lay.n_params), dtype=torch.float32, device=dev)
                         if self.kind == L.DC_LAMB else None)
        self.state = {}

    def zero_grad(self, set_to_none: bool = True):
        # every backward overwrites the whole gradient arena (each parameter exactly once): nothing to clear.  What this call does is end the
        # accumulation window: a backward() behind it starts from its own gradients, one that arrives WITHOUT it adds to the previous ones
        # (_NetFn.backward)
        self.engine.grads_live[0] = False
        return None

    def use_gradients(self, arena: Optional[torch.Tensor]) -> None:
        """Point the update at another fp32 arena of the gradient arena's size and layout (the accumulation arena of a virtual-rank step,
        Engine.grad_acc); None: the engine's own gradient arena again.  Not part of state_dict(): it names a buffer, not optimizer state."""
        if arena is not None and (arena.numel() != self.engine.grads.numel() or arena.dtype != torch.float32
                                  or arena.device != self.engine.grads.device):
            raise L.DeepcamHipError("use_gradients: the arena must be an fp32 tensor of the gradient arena's size on its device")
        self.grad_arena = arena

    def sync_scalars(self) -> None:
        """Push lr / step count to the device scalars the kernels read (keeps a captured hipGraph in step).
        The copies are asynchronous and the host enqueues steps ahead of the GPU, so the pinned source words must not be
        rewritten before the copy that reads them has run: wait for the previous copy's event first.  (Without the wait the
        device could pick up the step count of a LATER step -- wrong bias corrections, different from run to run.)  The host
        can still run one whole step ahead."""
        if self._scalars_copied is not None:
            self._scalars_copied.synchronize()
        self._lr_host[0] = float(self.param_groups[0]["lr"])
        self._step_host[0] = self.step_count
        self._scal_dev.copy_(self._scal_host, non_blocking=True)
        self._scalars_copied = torch.cuda.current_stream().record_event()

    def launch(self) -> None:
        """optimizer.step() through the dispatcher: torch.ops.deepcam.optimizer_step."""
        _ops.OPS.optimizer_step(_ops.optimizer_handle(self))

    def _launch_kernels(self) -> None:
        g = self.param_groups[0]
        eng = self.engine
        n = eng.layout.n_params
        b1, b2 = g["betas"]
        grads = eng.grads if self.grad_arena is None else self.grad_arena
        if self.kind == L.DC_LAMB:
            L.call("dc_lamb_step", len(eng.layout.params), L.dptr(self._offsets), n, L.dptr(eng.params), L.dptr(grads),
                   L.dptr(self.m), L.dptr(self.v), L.dptr(self.lr_dev), b1, b2, g["eps"], g["weight_decay"], L.dptr(self.step_dev),
                   self.max_grad_norm, self.grad_scale, L.dptr(self._lamb_ws), L.stream_ptr())
        else:
            L.call("dc_adam_step", self.kind, n, L.dptr(eng.params), L.dptr(grads), L.dptr(self.m), L.dptr(self.v),
                   L.dptr(self.lr_dev), b1, b2, g["eps"], g["weight_decay"], L.dptr(self.step_dev), self.grad_scale, L.stream_ptr())
        eng.mark_weights_changed()

    def step(self, closure=None):
        self.step_count += 1
        self.sync_scalars()
        self.launch()
        self.engine.grads_live[0] = False

    # -- torch.optim.Adam-compatible serialisation
    def state_dict(self):
        lay = self.engine.layout
        state = {}
        for i, p in enumerate(lay.params.values()):
            n = math.prod(p.shape)
            state[i] = {"step": torch.tensor(float(self.step_count)),
                        "exp_avg": self.m[p.offset:p.offset + n].view(p.shape).clone(),
                        "exp_avg_sq": self.v[p.offset:p.offset + n].view(p.shape).clone()}
        if self.step_count == 0:
            state = {}
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(lay.params)))
        return {"state": state, "param_groups": [g]}

    def load_state_dict(self, sd):
        lay = self.engine.layout
        g = sd["param_groups"][0]
        for k, v in g.items():
            if k != "params":
                self.param_groups[0][k] = v
        st = sd.get("state", {})
        self.step_count = 0
        # a parameter without an entry has no state (a step-0 checkpoint has none at all): its moments start from zero, as in torch.optim,
        # whatever this optimizer held before
        self.m.zero_()
        self.v.zero_()
        for i, p in enumerate(lay.params.values()):
            s = st.get(i, st.get(str(i)))
            if s is None:
                continue
            n = math.prod(p.shape)
            self.m[p.offset:p.offset + n].copy_(s["exp_avg"].reshape(-1).to(self.m.device, torch.float32))
            self.v[p.offset:p.offset + n].copy_(s["exp_avg_sq"].reshape(-1).to(self.v.device, torch.float32))
            # torch.optim keeps 'step' per parameter; apex FusedLAMB keeps it in the param group
            self.step_count = int(float(s["step"])) if "step" in s else int(g.get("step", 0))


class Adam(ArenaOptimizer):
    kind = L.DC_ADAM


class AdamW(ArenaOptimizer):
    kind = L.DC_ADAMW


class LAMB(ArenaOptimizer):
    """apex.optimizers.FusedLAMB stand-in (train_hdf5_ddp.py:218).  Parity with apex is UNPINNED (apex is not vendored by
    the reference nor installable here); the definition is DESIGN.md's: global grad-norm clip at max_grad_norm, Adam
    moments with bias correction, decoupled weight decay inside the update, per-tensor trust ratio ||w||/||u||."""
    kind = L.DC_LAMB


def make_optimizer(name: str, net: DeepLabv3_plus, lr: float, eps: float, weight_decay: float) -> ArenaOptimizer:
    cls = {"Adam": Adam, "AdamW": AdamW, "LAMB": LAMB}.get(name)
    if cls is None:
        raise NotImplementedError("Error, optimizer {} not supported".format(name))          # train_hdf5_ddp.py:220
    return cls(net.parameters(), lr=lr, eps=eps, weight_decay=weight_decay, engine=net.engine)


# ------------------------------------------------------------------------------------------------------------------
# LR schedules
# ------------------------------------------------------------------------------------------------------------------
class MultiStepSchedule:
    """MultiStepLR exactly as the reference drives it: recursive (multiplies the optimizer's CURRENT lr by gamma when its
    counter lands on a milestone) and already stepped once by its constructor; see oracle/optim.py for the derivation."""

    def __init__(self, optimizer, milestones: Sequence[int], gamma: float, last_epoch: int = -1):
        self.optimizer, self.milestones, self.gamma = optimizer, list(milestones), gamma
        self.last_epoch = last_epoch
        self._last_lr = [g["lr"] for g in optimizer.param_groups]
        self.step()

    def get_last_lr(self):
        return self._last_lr

    def step(self):
        self.last_epoch += 1
        n = self.milestones.count(self.last_epoch)
        for g in self.optimizer.param_groups:
            if n:
                g["lr"] = g["lr"] * self.gamma ** n
        self._last_lr = [g["lr"] for g in self.optimizer.param_groups]


def get_lr_schedule(start_lr, scheduler_arg, optimizer, last_step=-1):
    optimizer.param_groups[0]["initial_lr"] = start_lr                     # parsing_helpers.py:29
    if scheduler_arg["type"] == "multistep":
        milestones = [int(x) for x in scheduler_arg["milestones"].split()]
        gamma = float(scheduler_arg["decay_rate"])
        return MultiStepSchedule(optimizer, milestones, gamma, last_epoch=last_step)
    raise ValueError("Error, scheduler type {} not supported.".format(scheduler_arg["type"]))


class GradualWarmupScheduler:
    """PARITY UNPINNED stand-in for ildoonet/pytorch-gradual-warmup-lr (train_hdf5_ddp.py:251-253): linear ramp of the lr
    from base to base*multiplier over total_epoch steps -- or, for multiplier == 1.0 (the reference's default
    --lr_warmup_factor), from 0 to base as that package's get_lr does -- then hands over to after_scheduler (whose lr is
    scaled by multiplier at the hand-over)."""

    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        if multiplier < 1.0:
            raise ValueError("multiplier should be greater thant or equal to 1.")
        self.optimizer, self.multiplier, self.total_epoch, self.after = optimizer, multiplier, total_epoch, after_scheduler
        self.base_lrs = [g.get("initial_lr", g["lr"]) for g in optimizer.param_groups]
        self.last_epoch = 0
        self.finished = False
        self._apply()

    def _apply(self):
        if self.last_epoch > self.total_epoch:
            if not self.finished:
                for g, b in zip(self.optimizer.param_groups, self.base_lrs):
                    g["lr"] = b * self.multiplier
                self.finished = True
            return
        for g, b in zip(self.optimizer.param_groups, self.base_lrs):
            if self.multiplier == 1.0:
                g["lr"] = b * (float(self.last_epoch) / self.total_epoch)
            else:
                g["lr"] = b * ((self.multiplier - 1.0) * self.last_epoch / self.total_epoch + 1.0)

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def step(self):
        self.last_epoch += 1
        if self.finished and self.after is not None:
            self.after.step()
        else:
            self._apply()


# ------------------------------------------------------------------------------------------------------------------
# fused train step (no autograd round trip)
# ------------------------------------------------------------------------------------------------------------------
class TrainStep:
    """inputs -> forward -> weighted CE (+argmax, IoU counts) -> backward -> [gradient hook] -> optimizer, as one flat
    launch sequence on the current stream.  Equivalent to train_hdf5_ddp.py:348-364.

    virtual_ranks=K > 1: one call is the step of K data-parallel ranks (train_hdf5_ddp.py:227,345-364) on this device.  It takes K * batch
    samples; micro-batch v (samples v * batch ... (v + 1) * batch - 1) is what rank v would have seen: forward with its own BatchNorm batch
    statistics, its own mean loss (gradient scale 1 / (batch * H * W)), backward.  As the gradient buckets of a micro-batch become ready they
    are summed into a second arena (dc_grad_accumulate through dist.GradReducer.accumulate_into: ascending v, ((g0 + g1) + g2) ... in fp32),
    and ONE optimizer update reads that arena with grad_scale 1 / K (1 / (K * world) with a reducer attached, whose collective then runs
    once per K micro-batches, during the last one's backward).  The BatchNorm running buffers and num_batches_tracked are virtual rank 0's
    after the step, as a checkpoint written by rank 0 holds them.  loss() and iou() are the means over the ranks (rank_losses(), rank_ious()
    give every rank's own).  K = 1 is the plain step, launch for launch, and allocates nothing more."""

    def __init__(self, net: DeepLabv3_plus, optimizer: ArenaOptimizer, weight: Sequence[float], batch: int, height: int,
                 width: int, with_metrics: bool = False, virtual_ranks: int = 1):
        self.net, self.opt = net, optimizer
        self.K = int(virtual_ranks)
        if self.K < 1:
            raise L.DeepcamHipError(f"TrainStep: virtual_ranks must be at least 1, got {virtual_ranks}")
        self.eng = net.engine_for(shape=(batch, net.n_input, height, width))
        self.weight = list(weight)
        dev = self.eng.device
        # loss sum (one double) and the nine confusion counts behind it in ONE 80-byte buffer: one memset per step clears both
        # (K virtual ranks: one such slot per micro-batch, still one memset, so that every rank's own loss and IoU can be read back)
        self._acc = torch.zeros(10 * self.K, dtype=torch.int64, device=dev)
        self.loss_sum = self._acc[:1].view(torch.float64)
        self.with_metrics = with_metrics
        self.pred = torch.empty((self.K * batch, height, width), dtype=torch.int64, device=dev) if with_metrics else None
        self.counts = self._acc[1:] if with_metrics else None
        self.npix = batch * height * width          # of ONE micro-batch: the loss gradient is a rank's own mean
        self.after_backward = None      # set by attach_reducer
        self._own_reducer = False
        if self.K > 1:
            # the bucket plan and the hand-off on the reducer's stream are dist.GradReducer's; at world size 1 it has nothing to send
            from .dist import GradReducer
            acc = self.eng.enable_grad_accumulation()
            self._reducer = GradReducer(self.eng, 1)
            self._reducer.accumulate_into(acc)
            self._own_reducer = True
            self.opt.use_gradients(acc)
            self.opt.grad_scale = 1.0 / self.K
        self._eng_handle = _ops.engine_handle(self.eng)
        # loss inside the classifier's kernel (bf16 engine; fp32: the separate dc_wce_fused pass over stored logits);
        # store_logits: also write the fp32 NCHW logits (nobody reads them in the fused step)
        self.fuse_head_loss = net.act_dtype == torch.bfloat16
        self.store_logits = False

    def attach_reducer(self, reducer) -> None:
        """Data parallelism for the fused step: the reducer's buckets are all-reduced (SUM) while backward runs, the step
        waits for them before the optimizer and the 1/world averaging rides in the optimizer kernel (no extra pass)."""
        self.after_backward = reducer.finish
        self._reducer = reducer
        self._own_reducer = False
        self.opt.grad_scale = 1.0 / (self.K * reducer.world)
        # one averaging mechanism per module: the autograd path (DistributedDataParallel -> finish(average=True)) is switched off
        reducer.averaging_in_optimizer = True
        reducer.hook(self.eng)
        if self.K > 1:
            # the buckets of every micro-batch are summed into the accumulation arena; the last micro-batch's go on to the collective from there
            reducer.accumulate_into(self.eng.grad_acc)
            self.eng.on_grad_ready = reducer.ready       # (in place of the world-1 reducer this step was built with)
        # (net._ddp_reducer stays set: a loss.backward() through the wrapped module after this point reaches finish(average=True), which
        # raises on a reducer whose averaging lives in the optimizer, instead of silently leaving launched buckets un-waited)

    def launch(self, x: torch.Tensor, labels: torch.Tensor) -> None:
        L.call("dc_memset_async", L.dptr(self._acc), 0, 80 * self.K if self.counts is not None or self.K > 1 else 8, L.stream_ptr())
        if self.K == 1:
            self._micro_batch(x, labels, self.pred, self.loss_sum, self.counts)
            if self.after_backward is not None:
                self.after_backward()
        else:
            eng, B, red = self.eng, self.eng.B, self._reducer
            if x.size(0) != self.K * B or labels.size(0) != self.K * B:
                raise L.DeepcamHipError(f"TrainStep: {self.K} virtual ranks of batch {B} take {self.K * B} samples, got {x.size(0)} "
                                        f"(labels: {labels.size(0)})")
            for v in range(self.K):
                red.acc_first, red.acc_send = v == 0, v == self.K - 1
                slot = self._acc[10 * v:10 * v + 10]
                self._micro_batch(x[v * B:(v + 1) * B], labels[v * B:(v + 1) * B], None if self.pred is None else self.pred[v * B:(v + 1) * B],
                                  slot[:1].view(torch.float64), slot[1:] if self.with_metrics else None)
                if v == 0:
                    eng._copy_buffers(aside=True)       # virtual rank 0's running statistics (a train-mode forward never reads them)
                red.finish()                            # re-arms the buckets; behind the last micro-batch: the wait for the collectives
            eng._copy_buffers(aside=False)
        self.opt.launch()

    def _micro_batch(self, x: torch.Tensor, labels: torch.Tensor, pred: Optional[torch.Tensor], loss_sum: torch.Tensor,
                     counts: Optional[torch.Tensor]) -> None:
        """forward, loss and backward of one (micro-)batch; its loss sum and IoU counts go to the slot it is given"""
        eng = self.eng
        if self.fuse_head_loss:
            # the loss pass rides inside the classifier's forward kernel (dc_head_fwd_loss): the logits are neither stored nor re-read
            t = labels.squeeze(1) if labels.dim() == 4 else labels
            if t.dtype not in (torch.uint8, torch.int32, torch.int64):
                t = t.long()
            if not t.is_contiguous():
                t = t.contiguous()
            if tuple(t.shape) != (eng.B, eng.H, eng.W):
                raise L.DeepcamHipError(f"TrainStep: target shape {tuple(t.shape)} does not match the engine {(eng.B, eng.H, eng.W)}")
            eng.loss_args = {"labels": t, "weight": _cw_tensor(self.weight, eng.device), "grad_scale": 1.0 / float(self.npix),
                             "loss_sum": loss_sum, "pred": pred, "counts": counts, "store_logits": self.store_logits}
            try:
                _ops.OPS.net_forward(x, self._eng_handle, True)
            finally:
                eng.loss_args = None
        else:
            logits = _ops.OPS.net_forward(x, self._eng_handle, True)
            wce_fused(logits, labels, self.weight, dlogits=eng.dlogits, pred=pred, counts=counts, loss_sum=loss_sum)
        _ops.OPS.net_backward(eng.dlogits, self._eng_handle)

    def enable_graph(self) -> None:
        """Capture the whole step (about 1000 launches) into one hipGraph; later calls copy the batch into static
        buffers and replay.  Single-process only: the RCCL hand-off of the gradient reducer stays eager."""
        if self.after_backward is not None or (self.eng.on_grad_ready is not None and not self._own_reducer):
            raise L.DeepcamHipError("hipGraph capture is for the single-GPU step (the all-reduce path launches eagerly)")
        eng = self.eng
        self._static_batch()
        if eng.packed_version != eng.version[0]:
            eng.pack_weights()
        # weights change every step: repacking is part of the captured sequence
        eng.packed_version = -1
        self._graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.launch(self._gx, self._gy)              # warm-up on the side stream (lazy attribute setup, allocator)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eng.packed_version = -1
        with torch.cuda.graph(self._graph):
            self.launch(self._gx, self._gy)
        # the warm-up applied one optimizer update with whatever was in the static buffers (the capture pass records, it executes nothing):
        # callers enable the graph before training starts (bench) or accept one extra step on stale data
        self.graphed = True

    def _static_batch(self) -> None:
        """the buffers a captured or recorded step reads its batch from: K * batch samples, micro-batch v a view of them"""
        eng = self.eng
        self._gx = eng.x_static if self.K == 1 else torch.zeros((self.K * eng.B, eng.n_input, eng.H, eng.W), dtype=torch.float32,
                                                                device=eng.device)
        self._gy = torch.zeros((self.K * eng.B, eng.H, eng.W), dtype=torch.int64, device=eng.device)

    def enable_program(self) -> None:
        """Record the whole step as a C-side launch list (lib.Program, dc_program_*: every library call of one step with its arguments,
        stream fences included) and replay it with ONE call per step: later calls copy the batch into static buffers, push the
        optimizer's scalars and run the list -- no Python between two launches.  The recording pass is a real step on whatever the
        static buffers hold, as with enable_graph.  With a gradient reducer attached the step can be recorded when the reducer's collective
        is the library's own (GradReducer(collective="library"): dc_grad_allreduce_enqueue / _wait and the stream fences are C calls and
        land in the list); torch.distributed's collectives are Python objects and cannot."""
        red = getattr(self, "_reducer", None)
        if self.K > 1 and not self._own_reducer:
            raise L.DeepcamHipError(f"enable_program(): a step of {self.K} virtual ranks with a gradient reducer attached runs eagerly only "
                                    "(record it without a reducer, or attach the reducer to a plain step)")
        if ((self.after_backward is not None or self.eng.on_grad_ready is not None) and not self._own_reducer
                and getattr(red, "collective", None) != "library"):
            raise L.DeepcamHipError("the recorded launch list needs the library's own collective (GradReducer(collective='library')): "
                                    "torch.distributed's all-reduce hooks run in Python")
        eng = self.eng
        self._static_batch()
        eng.packed_version = -1           # weights change every step: repacking is part of the recorded sequence
        self.opt.step_count += 1
        self.opt.sync_scalars()
        self.launch(self._gx, self._gy)   # warm-up (lazy attribute setup); a real step, like the recording pass below
        torch.cuda.synchronize()
        eng.packed_version = -1
        self.opt.step_count += 1
        self.opt.sync_scalars()
        self._program = L.Program()
        self._program_stream = L.stream_ptr().value      # the recorded launches carry THIS stream; replay must run under the same one
        with self._program.recording():
            self.launch(self._gx, self._gy)
        eng.packed_version = -1
        self.programmed = True

    def __call__(self, x: torch.Tensor, labels: torch.Tensor) -> None:
        self.opt.step_count += 1
        self.opt.sync_scalars()
        if getattr(self, "programmed", False):
            # the batch copy and the optimizer's scalar hand-over above are enqueued on the CURRENT stream, the recorded launches on the stream
            # of the recording pass: under another current stream the step would read a stale or half-copied batch
            if L.stream_ptr().value != self._program_stream:
                raise L.DeepcamHipError("TrainStep: the recorded launch list was recorded under another stream; call the step under that stream "
                                        "or record again (enable_program)")
            self._gx.copy_(x, non_blocking=True)
            self._gy.copy_(labels.squeeze(1) if labels.dim() == 4 else labels, non_blocking=True)
            try:
                self._program.run()
            except L.DeepcamHipError:
                # a list that failed half way may have forked the weight-gradient stream without joining it: close the fork before raising
                if self.eng.use_side_stream:
                    L.call("dc_stream_fence", C.c_void_p(self.eng.side.cuda_stream), L.stream_ptr())
                raise
            self.eng.version[0] += 1
            return
        if getattr(self, "graphed", False):
            self._gx.copy_(x, non_blocking=True)
            self._gy.copy_(labels, non_blocking=True)
            self._graph.replay()
            self.eng.version[0] += 1
            return
        self.launch(x, labels)

    def rank_losses(self) -> List[float]:
        """the mean loss of every virtual rank's micro-batch of the last step (one device-to-host read)"""
        acc = self._acc.cpu()
        return [float(acc[10 * v:10 * v + 1].view(torch.float64).item()) / self.npix for v in range(self.K)]

    def rank_ious(self) -> List[float]:
        acc = self._acc.cpu().tolist()
        return [iou_from_counts(acc[10 * v + 1:10 * v + 10]) for v in range(self.K)]

    def loss(self) -> float:
        """K = 1: the batch's mean loss; K virtual ranks: the mean of the ranks' losses (what train_hdf5_ddp.py:400-410 logs), which is
        the loss sum over K * batch * H * W"""
        if self.K == 1:
            return float(self.loss_sum.item()) / self.npix
        return sum(self.rank_losses()) / self.K

    def iou(self) -> float:
        if self.K == 1:
            return iou_from_counts(self.counts.cpu().tolist())
        return sum(self.rank_ious()) / self.K


# ------------------------------------------------------------------------------------------------------------------
# batched validation step
# ------------------------------------------------------------------------------------------------------------------
class ValStep:
    """The reference's validation pass (train_hdf5_ddp.py:423-512: net.eval(), forward, fp_loss, compute_score at batch 1, mean over the
    samples) on batches: eval forward on a forward-only engine (Engine(forward_only=True): the net's weights and running statistics, pooled
    activations), per-sample loss sums and IoU counts behind the classifier (dc_head_fwd_score; fp32: dc_head_fwd + dc_wce_score) and their
    reduction to the three running sums (count, sum of per-sample losses, sum of per-sample IoUs) on the device (dc_val_accumulate).
    Nothing here synchronises; result() is the one device-to-host read."""

    def __init__(self, net: DeepLabv3_plus, weight: Sequence[float], batch: int, height: int, width: int):
        if net.engine is None:
            raise L.DeepcamHipError("ValStep: materialize the model first (its parameters live in the primary engine's arena)")
        self.net, self.B, self.H, self.W = net, batch, height, width
        self.eng = Engine(batch, height, width, net.act_dtype, n_input=net.n_input, n_classes=net.n_classes, share_from=net.engine,
                          forward_only=True)
        dev = self.eng.device
        # per-sample loss sums (B doubles) and counts (B x 9 int64) in ONE buffer: one memset per call clears both
        self._score = torch.zeros(10 * batch, dtype=torch.int64, device=dev)
        self.loss_sum = self._score[:batch].view(torch.float64)
        self.counts = self._score[batch:].view(batch, 9)
        self.acc = torch.zeros(3, dtype=torch.float64, device=dev)            # count, sum of losses, sum of IoUs
        self._per = torch.zeros((batch, 2), dtype=torch.float64, device=dev)
        self._weight = _cw_tensor(weight, dev)
        self._last_valid = 0
        self.store_logits = False       # bf16: also write the fp32 NCHW logits (the score needs them in registers only)
        self._eng_handle = _ops.engine_handle(self.eng)

    def __call__(self, x: torch.Tensor, labels: torch.Tensor, n_valid: Optional[int] = None) -> None:
        """x: the NCHW fp32 batch or the input pipeline's NHWC batch (Engine.forward); the samples from n_valid on are padding: they are
        computed by the network's body, but neither scored nor counted."""
        eng, B = self.eng, self.B
        nv = B if n_valid is None else int(n_valid)
        if not 0 < nv <= B:
            raise L.DeepcamHipError(f"ValStep: n_valid must lie in [1, {B}], got {n_valid}")
        t = labels.squeeze(1) if labels.dim() == 4 else labels
        if t.dtype not in (torch.uint8, torch.int32, torch.int64):
            t = t.long()
        if not t.is_contiguous():
            t = t.contiguous()
        if tuple(t.shape) != (B, self.H, self.W) or t.device != eng.device:
            raise L.DeepcamHipError(f"ValStep: labels must be {(B, self.H, self.W)} on {eng.device}, got {tuple(t.shape)} on {t.device}")
        L.call("dc_memset_async", L.dptr(self._score), 0, 80 * B, L.stream_ptr())
        eng.score_args = {"labels": t, "weight": self._weight, "n_valid": nv, "loss_sum": self.loss_sum, "counts": self.counts,
                          "store_logits": self.store_logits}
        try:
            _ops.OPS.net_forward(x, self._eng_handle, False)
        finally:
            eng.score_args = None
        L.call("dc_val_accumulate", B, nv, self.H * self.W, L.dptr(self.loss_sum), L.dptr(self.counts), L.dptr(self.acc), L.dptr(self._per),
               L.stream_ptr())
        self._last_valid = nv

    def reset(self) -> None:
        L.call("dc_memset_async", L.dptr(self.acc), 0, 24, L.stream_ptr())

    def result(self) -> tuple:
        """(count, sum of per-sample losses, sum of per-sample IoUs) since reset(): one device-to-host read."""
        c, ls, iou = self.acc.cpu().tolist()
        return c, ls, iou

    def per_sample(self) -> List[tuple]:
        """(loss, IoU) of every valid sample of the last call."""
        return [tuple(r) for r in self._per[:self._last_valid].cpu().tolist()]

    def close(self) -> None:
        self.eng.close()


# ------------------------------------------------------------------------------------------------------------------
# inference on unlabelled data
# ------------------------------------------------------------------------------------------------------------------
def predict_from_logits(logits: torch.Tensor, confidence: bool = False, n_valid: Optional[int] = None):
    """(mask uint8 [B,H,W], confidence fp32 [B,H,W] or None, class_counts int64 [B,3]) of fp32 NCHW logits [B,3,H,W] (dc_logits_predict):
    the first-max class of torch.max(logits, 1)[1] (train_hdf5_ddp.py:458) as one byte, its softmax probability, the pixels per class and
    sample.  Samples from n_valid on are not read; their rows of the outputs are zero."""
    if logits.dim() != 4 or logits.size(1) != 3 or not logits.is_cuda:
        raise L.DeepcamHipError(f"predict_from_logits: logits must be a device tensor [B, 3, H, W], got {tuple(logits.shape)} on {logits.device}")
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        logits = logits.float().contiguous()
    B, _, H, W = logits.shape
    nv = B if n_valid is None else int(n_valid)
    mask = torch.zeros((B, H, W), dtype=torch.uint8, device=logits.device)
    conf = torch.zeros((B, H, W), dtype=torch.float32, device=logits.device) if confidence else None
    counts = torch.zeros((B, 3), dtype=torch.int64, device=logits.device)
    L.call("dc_logits_predict", B, nv, H, W, L.dptr(logits), L.dptr(mask), L.dptr(conf), L.dptr(counts), L.stream_ptr())
    return mask, conf, counts


EVENT_FIELDS = ("root", "class", "pixels", "area", "sum_row", "sum_cx", "sum_sx", "row_min", "row_max", "seam")
EVENT_SCALE = 1 << 20


def event_weight_tables(height: int, width: int):
    """(wy [H], cx [W], sx [W]) int32 numpy arrays: cos(lat_r), cos(lon_c), sin(lon_c) times 2^20, rounded to nearest (ties to even), with
    lat = linspace(-90, 90, H) and lon = linspace(-180, 180, W) degrees, evaluated in float64.  Integer weights make every sum of the
    catalogue exact and independent of the order in which pixels arrive."""
    lat = np.deg2rad(np.linspace(-90.0, 90.0, height))
    lon = np.deg2rad(np.linspace(-180.0, 180.0, width))
    q = lambda v: np.rint(v * EVENT_SCALE).astype(np.int32)  # noqa: E731
    return q(np.cos(lat)), q(np.cos(lon)), q(np.sin(lon))


def _filled_rows(table: torch.Tensor, fill):
    """Per valid sample only the filled rows of a device table [B, cap, ...]: a list of numpy arrays table[b, :fill[b]], b < len(fill) (at
    least one sample).  One copy to the host, cut at the fullest sample's rows."""
    host = table[:len(fill), :max(max(fill), 1)].cpu().numpy()
    return [host[b, :fill[b]].copy() for b in range(len(fill))]


class EventCatalog:
    """Connected components of class masks on the device (dc_mask_components + dc_component_stats, csrc/components.hip): what a user of a
    tropical-cyclone / atmospheric-river detector works with -- how many events a snapshot holds, where they are and how large.
    Classes 1 and 2 are foreground; a component is a maximal set of pixels of one class under 4- or 8-connectivity, with periodic columns
    when wrap is set (the fields are global longitude bands).  The object owns the label map (int32, 0 = background, else 1 + the smallest
    r * W + c of the component), the workspace, the weight tables, the table (int64 [B, cap, 10], EVENT_FIELDS) and the counts (int32
    [B, 3]: all, class 1, class 2 -- not capped).  A call launches on the current stream and does not synchronise; events() reads back."""

    def __init__(self, batch: int, height: int, width: int, connectivity: int = 8, wrap: bool = True, cap: int = 4096, device=None):
        if connectivity not in (4, 8):
            raise L.DeepcamHipError(f"EventCatalog: connectivity must be 4 or 8, got {connectivity}")
        if batch < 1 or height < 1 or width < 1 or cap < 1:
            raise L.DeepcamHipError("EventCatalog: batch, height, width and cap must be positive")
        self.B, self.H, self.W, self.connectivity, self.wrap, self.cap = batch, height, width, connectivity, bool(wrap), cap
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.tables = event_weight_tables(height, width)
        self._wy, self._cx, self._sx = (torch.from_numpy(t).to(dev) for t in self.tables)
        self._labels = torch.zeros((batch, height, width), dtype=torch.int32, device=dev)
        self._table = torch.zeros((batch, cap, len(EVENT_FIELDS)), dtype=torch.int64, device=dev)
        self._ncomp = torch.zeros((batch, 3), dtype=torch.int32, device=dev)
        self._ws = torch.empty(max(L.load().dc_mask_components_workspace(batch, height, width), 256), dtype=torch.uint8, device=dev)
        self._last_valid = 0

    def __call__(self, mask: torch.Tensor, n_valid: Optional[int] = None) -> "EventCatalog":
        """mask: device uint8 [B, H, W].  Samples from n_valid on are padding: not read, their labels and counts stay as they were."""
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (self.B, self.H, self.W) or not mask.is_cuda or not mask.is_contiguous():
            raise L.DeepcamHipError(f"EventCatalog: mask must be a contiguous device uint8 tensor [{self.B}, {self.H}, {self.W}], got "
                                    f"{mask.dtype} {tuple(mask.shape)} on {mask.device}")
        nv = self.B if n_valid is None else int(n_valid)
        st = L.stream_ptr()
        L.call("dc_mask_components", self.B, nv, self.H, self.W, L.dptr(mask), self.connectivity, int(self.wrap), L.dptr(self._labels),
               L.dptr(self._ws), st)
        L.call("dc_component_stats", self.B, nv, self.H, self.W, L.dptr(mask), L.dptr(self._labels), L.dptr(self._wy), L.dptr(self._cx),
               L.dptr(self._sx), self.cap, L.dptr(self._table), L.dptr(self._ncomp), L.dptr(self._ws), st)
        self._last_valid = nv
        return self

    @property
    def labels(self) -> torch.Tensor:
        """int32 [n_valid, H, W] of the last call (a view)"""
        return self._labels[:self._last_valid]

    @property
    def table(self) -> torch.Tensor:
        """int64 [n_valid, cap, 10] of the last call (a view): the raw rows, zero beyond min(count, cap)"""
        return self._table[:self._last_valid]

    def counts(self) -> torch.Tensor:
        """int32 [n_valid, 3] of the last call (a view): components of any class, of class 1, of class 2"""
        return self._ncomp[:self._last_valid]

    @property
    def rank_map(self) -> torch.Tensor:
        """int32 [n_valid, H, W] of the last call (a view of the workspace's first segment, valid until the next call): at every root pixel
        (labels == r * W + c + 1) the row index of that component, undefined elsewhere.  What dc_component_overlap reads."""
        n = self.B * self.H * self.W
        return self._ws[:4 * n].view(torch.int32).view(self.B, self.H, self.W)[:self._last_valid]

    def rows(self):
        """(counts, rows) on the host: the counts first, then only the rows that are filled -- one list entry per valid sample, each an
        int64 numpy array [min(total, cap), 10]."""
        nv = self._last_valid
        if nv == 0:
            return [], []
        ncomp = self._ncomp[:nv].cpu().numpy()
        return ncomp, _filled_rows(self._table, [min(int(t), self.cap) for t in ncomp[:, 0]])

    def _fill(self, nv: int):
        """The rows the table holds for each of the first nv samples: min(total, cap) (EventFields and EventShape cut their tables by it)"""
        return [min(int(t), self.cap) for t in self._ncomp[:nv, 0].cpu().tolist()]

    def events(self, min_pixels: int = 0):
        """Per valid sample of the last call a list of dicts (decode), components below min_pixels left out on the host."""
        _, rows = self.rows()
        return [self.decode(r, self.H, self.W, min_pixels=min_pixels) for r in rows]

    @staticmethod
    def decode(rows, height: int, width: int, min_pixels: int = 0):
        """Raw rows [n, 10] (EVENT_FIELDS) -> dicts: class, pixels, area_fraction (area / sum_r W * wy[r]: the share of the sphere), lat (the
        mean row through linspace(-90, 90, H)), lon (atan2(sum sx, sum cx) in degrees: the circular mean, right across the seam), row_min,
        row_max, crosses_seam, root."""
        wy = event_weight_tables(height, width)[0]
        whole = float(width) * float(wy.astype("int64").sum())
        out = []
        for r in rows:
            root, cls, n, area, sr, scx, ssx, rmin, rmax, seam = (int(v) for v in r)
            if n < max(min_pixels, 1):
                continue
            lat = -90.0 + 180.0 * (sr / n) / (height - 1) if height > 1 else -90.0
            out.append({"class": cls, "pixels": n, "area_fraction": area / whole if whole > 0 else 0.0, "lat": lat,
                        "lon": math.degrees(math.atan2(ssx, scx)), "row_min": rmin, "row_max": rmax, "crosses_seam": bool(seam), "root": root})
        return out


class EventMatcher:
    """Two event catalogues of the same frames matched on the device (dc_component_overlap + dc_event_scores, csrc/event_match.hip): which
    event of mask a overlaps which event of mask b and by how many pixels, how much of every event the other mask covers with the same
    class, and from that the detection scores per class -- hits and misses among b's events, false alarms and matched detections among
    a's.  With a = a prediction and b = its labels these are the counts behind POD, FAR and CSI; the same pairs link the events of two
    time steps.  An event is SCORED when it has at least max(min_pixels, 1) pixels and a row in its table; it is MATCHED when the other
    mask covers at least min_cover of it with its class (integer: cover * 1024 >= round(min_cover * 1024) * pixels, and cover >= 1).
    Coverage, not pairwise IoU, decides: a labelled river predicted as two fragments is still found.  The object owns the two catalogues
    `.a` and `.b`, the pair table (int64 [B, pair_cap, 3]), the coverage counts (int64 [B, cap] per side), the per-sample scores (int64
    [B, 2, 4]) and the running sums.  A call launches on the current stream and does not synchronise."""

    SCORE_FIELDS = ("hits", "misses", "false_alarms", "matched")

    def __init__(self, batch: int, height: int, width: int, connectivity: int = 8, wrap: bool = True, cap: int = 4096, pair_cap: int = 8192,
                 min_pixels: int = 0, min_cover: float = 0.5, device=None):
        if not 0.0 < float(min_cover) <= 1.0:
            raise L.DeepcamHipError(f"EventMatcher: min_cover must lie in (0, 1], got {min_cover}")
        if pair_cap < 1 or min_pixels < 0:
            raise L.DeepcamHipError("EventMatcher: pair_cap must be positive and min_pixels not negative")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.a = EventCatalog(batch, height, width, connectivity=connectivity, wrap=wrap, cap=cap, device=dev)
        self.b = EventCatalog(batch, height, width, connectivity=connectivity, wrap=wrap, cap=cap, device=dev)
        self.B, self.H, self.W, self.cap, self.pair_cap, self.min_pixels = batch, height, width, cap, pair_cap, int(min_pixels)
        self.cover_q = min(max(int(round(float(min_cover) * 1024)), 1), 1024)
        self._pairs = torch.zeros((batch, pair_cap, 3), dtype=torch.int64, device=dev)
        self._npairs = torch.zeros((batch, 2), dtype=torch.int32, device=dev)
        self._cover_a = torch.zeros((batch, cap), dtype=torch.int64, device=dev)
        self._cover_b = torch.zeros((batch, cap), dtype=torch.int64, device=dev)
        self._scores = torch.zeros((batch, 2, 4), dtype=torch.int64, device=dev)
        self.acc = torch.zeros(10, dtype=torch.int64, device=dev)
        nbytes = L.load().dc_component_overlap_workspace(batch, pair_cap)
        if nbytes == 0:
            raise L.DeepcamHipError(f"EventMatcher: pair_cap {pair_cap} is out of range")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._mask_b = None
        self._last_valid = 0

    def __call__(self, mask_a: torch.Tensor, mask_b: torch.Tensor, n_valid: Optional[int] = None) -> "EventMatcher":
        """mask_a: device uint8 [B, H, W]; mask_b: the same, or a label tensor (int64, int32) whose classes become bytes here.  Samples from
        n_valid on are padding: not read."""
        if mask_b.dtype in (torch.int64, torch.int32):
            mask_b = mask_b.to(torch.uint8)
        nv = self.B if n_valid is None else int(n_valid)
        a, b, st = self.a, self.b, L.stream_ptr()
        a(mask_a, n_valid=nv)
        b(mask_b, n_valid=nv)
        self._mask_b = mask_b                      # the converted bytes stay alive while the launches below may still read them
        L.call("dc_component_overlap", self.B, nv, self.H, self.W, L.dptr(mask_a), L.dptr(a._labels), L.dptr(a._ws), a.cap, L.dptr(mask_b),
               L.dptr(b._labels), L.dptr(b._ws), b.cap, self.pair_cap, L.dptr(self._pairs), L.dptr(self._npairs), L.dptr(self._cover_a),
               L.dptr(self._cover_b), L.dptr(self._ws), st)
        L.call("dc_event_scores", self.B, nv, a.cap, L.dptr(a._table), L.dptr(a._ncomp), L.dptr(self._cover_a), b.cap, L.dptr(b._table),
               L.dptr(b._ncomp), L.dptr(self._cover_b), L.dptr(self._npairs), self.min_pixels, self.cover_q, L.dptr(self._scores),
               L.dptr(self.acc), st)
        self._last_valid = nv
        return self

    @property
    def pair_table(self) -> torch.Tensor:
        """int64 [n_valid, pair_cap, 3] of the last call (a view): (rank a, rank b, pixels), device order, zero beyond the stored count"""
        return self._pairs[:self._last_valid]

    @property
    def pair_counts(self) -> torch.Tensor:
        """int32 [n_valid, 2] of the last call (a view): rows stored, overflow flag"""
        return self._npairs[:self._last_valid]

    @property
    def score_table(self) -> torch.Tensor:
        """int64 [n_valid, 2, 4] of the last call (a view): per class 1, 2 the SCORE_FIELDS"""
        return self._scores[:self._last_valid]

    @staticmethod
    def sort_pairs(rows: np.ndarray) -> np.ndarray:
        """the stored rows [n, 3] ordered by (rank a, rank b)"""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        return np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0]))])

    def pairs(self):
        """(rows, flags) on the host: per valid sample an int64 numpy array [n, 3] sorted by (rank a, rank b), and the overflow flags"""
        nv = self._last_valid
        if nv == 0:
            return [], []
        npairs = self._npairs[:nv].cpu().numpy()
        return [self.sort_pairs(p) for p in _filled_rows(self._pairs, [int(n) for n in npairs[:, 0]])], [int(f) for f in npairs[:, 1]]

    def cover(self):
        """(cover_a, cover_b) on the host: int64 numpy arrays [n_valid, cap], per component the pixels the other mask covers with its class"""
        nv = self._last_valid
        return self._cover_a[:nv].cpu().numpy(), self._cover_b[:nv].cpu().numpy()

    def scores(self) -> np.ndarray:
        """int64 numpy array [n_valid, 2, 4]: per sample and class the SCORE_FIELDS"""
        return self._scores[:self._last_valid].cpu().numpy()

    @staticmethod
    def join(pairs, rows_a, rows_b, height: int, width: int, min_pixels: int = 0):
        """Sorted pairs [n, 3] and the two catalogues' raw rows -> a list of dicts: `a`, `b` (EventCatalog.decode of the two rows),
        `class_a`, `class_b`, `pixels` (shared), `iou` (shared / union).  Pairs with an event below min_pixels are left out."""
        out = []
        for ra, rb, n in np.asarray(pairs, dtype=np.int64).reshape(-1, 3).tolist():
            if min(int(rows_a[ra][2]), int(rows_b[rb][2])) < max(min_pixels, 1):
                continue
            ea = EventCatalog.decode(rows_a[ra:ra + 1], height, width)[0]
            eb = EventCatalog.decode(rows_b[rb:rb + 1], height, width)[0]
            out.append({"a": ea, "b": eb, "class_a": ea["class"], "class_b": eb["class"], "pixels": n,
                        "iou": n / (ea["pixels"] + eb["pixels"] - n)})
        return out

    def matches(self, min_pixels: Optional[int] = None):
        """Per valid sample of the last call the joined pairs (join); min_pixels defaults to the matcher's."""
        mp = self.min_pixels if min_pixels is None else int(min_pixels)
        pairs, _ = self.pairs()
        _, rows_a = self.a.rows()
        _, rows_b = self.b.rows()
        return [self.join(p, ra, rb, self.H, self.W, mp) for p, ra, rb in zip(pairs, rows_a, rows_b)]

    def reset(self) -> None:
        L.call("dc_memset_async", L.dptr(self.acc), 0, 80, L.stream_ptr())

    @staticmethod
    def rates(hits: int, misses: int, false_alarms: int, matched: int) -> dict:
        """pod = hits / (hits + misses): the share of b's events found; far = false_alarms / (false_alarms + matched): the share of a's
        events that answer to nothing; csi = hits / (hits + misses + false_alarms).  None where the denominator is zero."""
        div = lambda n, d: n / d if d > 0 else None  # noqa: E731
        return {"pod": div(hits, hits + misses), "far": div(false_alarms, false_alarms + matched),
                "csi": div(hits, hits + misses + false_alarms)}

    @staticmethod
    def summarize(acc) -> dict:
        """the ten running sums -> {"samples", "truncated", "class_1": {...}, "class_2": {...}}: per class the SCORE_FIELDS and rates();
        truncated: some sample held more events than a table or more pairs than the pair table, so counts may be short"""
        acc = [int(v) for v in acc]
        out = {"samples": acc[8], "truncated": acc[9] != 0}
        for k in (0, 1):
            h, m, f, d = acc[4 * k:4 * k + 4]
            out[f"class_{k + 1}"] = {"hits": h, "misses": m, "false_alarms": f, "matched": d, **EventMatcher.rates(h, m, f, d),
                                     "truncated": acc[9] != 0}
        return out

    def result(self) -> dict:
        """summarize() of the sums since reset(): one device-to-host read"""
        return self.summarize(self.acc.cpu().tolist())


EVENT_FIELD_STATS = ("min", "max", "sum", "wsum", "nonfinite", "saturated")


def event_field_bits(minval, maxval) -> np.ndarray:
    """int32 [C]: the binary scale of dc_component_fields' sums per channel, from the dataset's recorded range (stats.h5: climate/minval,
    climate/maxval).  With m = max(|minval|, |maxval|): 39 - frexp(m)[1], and 0 where m is zero or not finite.  A value v inside the range
    is summed as rint(v * 2^bits) with |v * 2^bits| < 2^39; values up to twice outside the range still fit below the kernel's limit of
    2^40, larger ones are counted as saturated.  The quantum of the sums is 2^-bits: a sum of n values is within n * 2^-(bits + 1) of the
    real one (m = 1e5: bits 22, 1.2e-7 per value)."""
    lo = np.atleast_1d(np.asarray(minval, np.float64))
    hi = np.atleast_1d(np.asarray(maxval, np.float64))
    m = np.maximum(np.abs(lo), np.abs(hi))
    ok = np.isfinite(m) & (m > 0)
    return np.where(ok, 39 - np.frexp(np.where(ok, m, 1.0))[1], 0).astype(np.int32)


def event_field_key(values) -> np.ndarray:
    """uint32 keys of float32 values whose unsigned order is the values' order (-0.0 below +0.0, denormals in their places): the bits with
    the sign bit set for non-negative values, all bits flipped for negative ones.  The upper half of the min / max words."""
    u = np.asarray(values, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000)).astype(np.uint32)


def event_field_value(keys) -> np.ndarray:
    """float32 values of event_field_key's keys"""
    k = np.asarray(keys, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


class EventFields:
    """Per-event statistics of the raw input fields on the device (dc_component_fields, csrc/event_fields.hip): for every event of a
    catalogue and every channel the minimum and where it sits (a cyclone's pressure minimum is its centre), the maximum and where it sits
    (its strongest wind), the sum and the area-weighted sum (a river's mean water vapour).  The object owns the device scale_bits (int32
    [C], see event_field_bits) and the table (int64 [B, cap, C, 6], EVENT_FIELD_STATS; row k belongs to row k of the catalogue's table).
    Everything is exact and independent of the order in which pixels arrive.  A call must follow the catalogue's call on the same stream
    (it reads the catalogue's labels and rank map); it launches and does not synchronise."""

    def __init__(self, catalog: EventCatalog, channels: int, bits: Sequence[int], ldc: Optional[int] = None):
        ldc = int(channels if ldc is None else ldc)
        bits = [int(v) for v in np.asarray(bits).reshape(-1)]
        if not 1 <= int(channels) <= 32 or ldc < channels:
            raise L.DeepcamHipError(f"EventFields: channels must lie in [1, 32] and ldc must be at least channels, got {channels}, {ldc}")
        if len(bits) != channels:
            raise L.DeepcamHipError(f"EventFields: {len(bits)} scale bits for {channels} channels")
        if catalog.H * catalog.W > 1 << 22:
            raise L.DeepcamHipError("EventFields: H * W must be at most 2^22")
        self.catalog, self.C, self.ldc, self.bits = catalog, int(channels), ldc, bits
        dev = catalog._labels.device
        self._bits = torch.tensor(bits, dtype=torch.int32, device=dev)
        self._ftable = torch.zeros((catalog.B, catalog.cap, self.C, len(EVENT_FIELD_STATS)), dtype=torch.int64, device=dev)
        self._last_valid = 0

    def __call__(self, fields: torch.Tensor, n_valid: Optional[int] = None) -> "EventFields":
        """fields: contiguous device fp32 [B, H, W, ldc], physical units (InputPipeline.raw).  n_valid defaults to the catalogue's."""
        cat = self.catalog
        want = (cat.B, cat.H, cat.W, self.ldc)
        if fields.dtype != torch.float32 or tuple(fields.shape) != want or not fields.is_cuda or not fields.is_contiguous() \
                or fields.device != cat._labels.device:
            raise L.DeepcamHipError(f"EventFields: fields must be a contiguous fp32 tensor {list(want)} on {cat._labels.device}, got "
                                    f"{fields.dtype} {tuple(fields.shape)} on {fields.device}")
        nv = cat._last_valid if n_valid is None else int(n_valid)
        L.call("dc_component_fields", cat.B, nv, cat.H, cat.W, L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, L.dptr(fields), self.C, self.ldc,
               L.dptr(self._bits), L.dptr(cat._wy), L.dptr(self._ftable), L.stream_ptr())
        self._last_valid = nv
        return self

    @property
    def table(self) -> torch.Tensor:
        """int64 [n_valid, cap, C, 6] of the last call (a view): rows from min(count, cap) on are empty (-1, 0, 0, 0, 0, 0)"""
        return self._ftable[:self._last_valid]

    def rows(self):
        """On the host, per valid sample only the filled rows: int64 numpy arrays [min(total, cap), C, 6] (the catalogue's counts decide)"""
        nv = self._last_valid
        if nv == 0:
            return []
        return _filled_rows(self._ftable, self.catalog._fill(nv))

    def stats(self, min_pixels: int = 0):
        """Per valid sample a list aligned with catalog.events(min_pixels): per event a list over channels of dicts (decode)."""
        _, rows = self.catalog.rows()
        out = []
        for fr, r in zip(self.rows(), rows):
            keep = r[:, 2] >= max(min_pixels, 1)
            out.append(self.decode(fr[keep], r[keep], self.catalog.H, self.catalog.W, self.bits))
        return out

    FIELD_VALUES = ("min", "min_lat", "min_lon", "max", "max_lat", "max_lon", "mean", "area_mean")

    @staticmethod
    def values(frows, rows, height: int, width: int, bits) -> np.ndarray:
        """float64 [n, C, 8] (FIELD_VALUES): decode's numbers for whole arrays at once, NaN where decode gives None -- the same
        operations on the same operands, so the two agree to the bit (what predict.py stores as event_field_values)."""
        bits = np.asarray(bits, np.int64).reshape(-1)
        fr = np.asarray(frows, np.int64).reshape(-1, len(bits), len(EVENT_FIELD_STATS))
        rows = np.asarray(rows, np.int64).reshape(-1, len(EVENT_FIELDS))
        lat, lon = np.linspace(-90.0, 90.0, height), np.linspace(-180.0, 180.0, width)
        out = np.full(fr.shape[:2] + (8,), np.nan, np.float64)
        lo, hi = fr[..., 0].view(np.uint64), fr[..., 1].view(np.uint64)
        for k, (word, some) in enumerate(((lo, fr[..., 0] != -1), (hi, fr[..., 1] != 0))):
            p = (word & np.uint64(0xFFFFFFFF)).astype(np.int64)
            p = np.where(some, p if k == 0 else 0xFFFFFFFF - p, 0)
            val = event_field_value((word >> np.uint64(32)).astype(np.uint32)).astype(np.float64)
            out[..., 3 * k] = np.where(some, val, np.nan)
            out[..., 3 * k + 1] = np.where(some, lat[np.minimum(p // width, height - 1)], np.nan)
            out[..., 3 * k + 2] = np.where(some, lon[p % width], np.nan)
        n = rows[:, 2, None] - fr[..., 4] - fr[..., 5]
        area = rows[:, 3, None].astype(np.float64) * 2.0 ** -20
        with np.errstate(divide="ignore", invalid="ignore"):
            out[..., 6] = np.where(n > 0, np.ldexp(fr[..., 2].astype(np.float64), -bits) / n, np.nan)
            out[..., 7] = np.where(area > 0, fr[..., 3].astype(np.float64) / (np.ldexp(1.0, bits) * area), np.nan)
        return out

    @staticmethod
    def decode(frows, rows, height: int, width: int, bits):
        """Raw rows [n, C, 6] (EVENT_FIELD_STATS) and the events' own rows [n, 10] (EVENT_FIELDS) -> per event a list over channels of
        dicts: min, min_row, min_col, min_lat, min_lon, max, max_row, max_col, max_lat, max_lon (lat / lon through the linspaces of
        event_weight_tables), mean = sum * 2^-bits / (pixels - nonfinite - saturated), area_mean = wsum / (2^bits * area * 2^-20),
        nonfinite, saturated.  None where the row is empty (no finite value) or a divisor is zero."""
        frows = np.asarray(frows, np.int64)
        lat, lon = np.linspace(-90.0, 90.0, height), np.linspace(-180.0, 180.0, width)
        out = []
        for fr, r in zip(frows.tolist(), np.asarray(rows, np.int64).tolist()):
            pixels, area = r[2], r[3]
            per = []
            for ch, (lo, hi, s, ws, nonfinite, saturated) in enumerate(fr):
                d = {"nonfinite": nonfinite, "saturated": saturated}
                for name, word, empty in (("min", lo, -1), ("max", hi, 0)):
                    if word == empty:
                        d.update({name: None, name + "_row": None, name + "_col": None, name + "_lat": None, name + "_lon": None})
                        continue
                    word &= 0xFFFFFFFFFFFFFFFF
                    p = word & 0xFFFFFFFF if name == "min" else 0xFFFFFFFF - (word & 0xFFFFFFFF)
                    d.update({name: float(event_field_value(np.uint32(word >> 32))), name + "_row": p // width, name + "_col": p % width,
                              name + "_lat": float(lat[p // width]), name + "_lon": float(lon[p % width])})
                n = pixels - nonfinite - saturated
                d["mean"] = math.ldexp(float(s), -int(bits[ch])) / n if n > 0 else None
                d["area_mean"] = float(ws) / (math.ldexp(1.0, int(bits[ch])) * (area * 2.0 ** -20)) if area > 0 else None
                per.append(d)
            out.append(per)
        return out


EVENT_SHAPE_FIELDS = ("boundary_pixels", "faces_v", "faces_h", "s_x", "s_y", "s_z", "s_xx", "s_xy", "s_yy", "s_xz", "s_yz", "s_zz")
EVENT_SHAPE_VALUES = ("lat", "lon", "length_km", "width_km", "aspect", "orientation_deg", "perimeter_km", "area_km2", "compactness",
                      "boundary_pixels")
EVENT_FILTER_COUNTS = ("events_kept", "events_dropped", "pixels_kept", "pixels_dropped")
EARTH_RADIUS_KM = 6371.0


def event_shape_tables(height: int, width: int):
    """(rows int32 [6, H]: wy, rc2, rcs, rc3, rc2s, rcs2; cols int32 [5, W]: cx, sx, cxx, cxy, cyy) -- the tables of dc_component_shape.
    With cl / sl the cosine / sine of a row's latitude and co / so of a column's longitude: cl, cl^2, cl sl, cl^3, cl^2 sl, cl sl^2 and
    co, so, co^2, co so, so^2, each evaluated in float64, scaled by 2^20 and rounded to nearest (ties to even).  The latitudes are those
    of event_weight_tables (rows[0] is its wy).  The longitudes are the W columns of a PERIODIC grid, lon_c = -180 + 360 c / W: column
    W - 1 is one step west of column 0, as `wrap` has it, so a shape rolled across the seam keeps its moments.  event_weight_tables'
    linspace(-180, 180, W) holds the seam meridian twice (columns 0 and W - 1) and is left as it is for the catalogue."""
    lat = np.deg2rad(np.linspace(-90.0, 90.0, height))
    lon = np.deg2rad(-180.0 + 360.0 * np.arange(width) / width)
    cl, sl, co, so = np.cos(lat), np.sin(lat), np.cos(lon), np.sin(lon)
    q = lambda v: np.rint(v * EVENT_SCALE).astype(np.int32)  # noqa: E731
    rows = np.stack([q(cl), q(cl * cl), q(cl * sl), q(cl * cl * cl), q(cl * cl * sl), q(cl * sl * sl)])
    cols = np.stack([q(co), q(so), q(co * co), q(co * so), q(so * so)])
    return np.ascontiguousarray(rows), np.ascontiguousarray(cols)


class EventShape:
    """Geometry per event on the device (dc_component_shape, csrc/event_shape.hip): boundary pixels, perimeter faces, and the first and
    second moments of the event's pixels as area-weighted unit vectors on the sphere, all exact integer sums (EVENT_SHAPE_FIELDS; the
    header has the definition).  decode turns them into a spherical centroid, the length and width of the uniform strip with the same
    second moments, aspect, orientation, perimeter and compactness.  Built on an existing EventCatalog, as EventFields is; a call must
    follow the catalogue's call on the same stream, launches and does not synchronise.  The object owns the tables and the shape rows
    (int64 [B, cap, 12]: 96 bytes per event slot; row k belongs to row k of the catalogue's table)."""

    def __init__(self, catalog: EventCatalog):
        if catalog.H * catalog.W > 1 << 22:
            raise L.DeepcamHipError("EventShape: H * W must be at most 2^22")
        self.catalog = catalog
        dev = catalog._labels.device
        self.tables = event_shape_tables(catalog.H, catalog.W)
        self._rowt, self._colt = (torch.from_numpy(t).to(dev) for t in self.tables)
        self._shape = torch.zeros((catalog.B, catalog.cap, len(EVENT_SHAPE_FIELDS)), dtype=torch.int64, device=dev)
        self._last_valid = 0

    def __call__(self, n_valid: Optional[int] = None) -> "EventShape":
        """n_valid defaults to the catalogue's."""
        cat = self.catalog
        nv = cat._last_valid if n_valid is None else int(n_valid)
        L.call("dc_component_shape", cat.B, nv, cat.H, cat.W, L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, int(cat.wrap), L.dptr(self._rowt),
               L.dptr(self._colt), L.dptr(self._shape), L.stream_ptr())
        self._last_valid = nv
        return self

    @property
    def table(self) -> torch.Tensor:
        """int64 [n_valid, cap, 12] of the last call (a view): zero from min(count, cap) on"""
        return self._shape[:self._last_valid]

    def rows(self):
        """On the host, per valid sample only the filled rows: int64 numpy arrays [min(total, cap), 12] (the catalogue's counts decide)"""
        nv = self._last_valid
        if nv == 0:
            return []
        return _filled_rows(self._shape, self.catalog._fill(nv))

    def shapes(self):
        """Per valid sample of the last call a list of dicts (decode), one per row of the catalogue."""
        _, rows = self.catalog.rows()
        return [self.decode(s, r, self.catalog.H, self.catalog.W) for s, r in zip(self.rows(), rows)]

    @staticmethod
    def steps(height: int, width: int):
        """(dlat, dlon) in radians: the spacing of the rows and columns of event_shape_tables (rows pole to pole, columns periodic)"""
        return math.pi / max(height - 1, 1), 2.0 * math.pi / width

    ARC_MAX = 4.4934                               # radians: 1 - sin(t) / t grows up to here (tan t = t), well beyond half the globe

    @staticmethod
    def chord_moment(theta):
        """12 lambda+ of a uniform great-circle arc of angle theta (radians, numpy): 6 (1 - sin(theta) / theta) -- points on the unit
        sphere, second moment along the chord.  theta^2 (1 - theta^2 / 20 + ...) for short arcs (the series below 0.3, where the closed
        form cancels)."""
        t = np.asarray(theta, np.float64)
        t2 = t * t
        series = t2 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            closed = 6.0 * (1.0 - np.sin(t) / t)
        return np.where(t < 0.3, series, closed)

    @staticmethod
    def arc_angle(q):
        """the inverse of chord_moment on [0, ARC_MAX], by bisection (numpy): the angle of the great-circle arc whose 12 lambda+ is q"""
        q = np.asarray(q, np.float64)
        lo, hi = np.zeros_like(q), np.full_like(q, EventShape.ARC_MAX)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            below = EventShape.chord_moment(mid) < q
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        return 0.5 * (lo + hi)

    @staticmethod
    def moments(shape_rows, rows):
        """float64 numpy on the integers: (s0 [n], m [n, 3], C [n, 3, 3], lat [n], lon [n] in radians, lam_plus [n], lam_minus [n],
        theta [n]: the major axis' angle counter-clockwise from east, in radians) -- the header's decode formula.  Events whose zeroth
        moment is 0 (pixels on the pole rows only) give NaN moments and zero eigenvalues."""
        s = np.asarray(shape_rows, np.int64).reshape(-1, len(EVENT_SHAPE_FIELDS)).astype(np.float64)
        rows = np.asarray(rows, np.int64).reshape(-1, len(EVENT_FIELDS))
        s0 = rows[:, 3].astype(np.float64) * float(EVENT_SCALE)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = s[:, 3:6] / s0[:, None]
            second = np.empty((len(s), 3, 3), np.float64)
            for (i, j), f in zip(((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)), range(6, 12)):
                second[:, i, j] = second[:, j, i] = s[:, f] / s0
            cov = second - m[:, :, None] * m[:, None, :]
            norm = np.sqrt((m * m).sum(axis=1))
            c = np.where((norm > 0)[:, None], m / norm[:, None], np.array([1.0, 0.0, 0.0]))
            lat, lon = np.arcsin(np.clip(c[:, 2], -1.0, 1.0)), np.arctan2(c[:, 1], c[:, 0])
            zero = np.zeros_like(lat)
            e = np.stack([-np.sin(lon), np.cos(lon), zero], axis=1)
            n = np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], axis=1)
            cn = np.einsum("kij,kj->ki", cov, n)
            a, b, d = np.einsum("ki,kij,kj->k", e, cov, e), (e * cn).sum(axis=1), (n * cn).sum(axis=1)
            rad = np.sqrt(((a - d) / 2) ** 2 + b * b)
            lp, lm = np.maximum((a + d) / 2 + rad, 0.0), np.maximum((a + d) / 2 - rad, 0.0)
            theta = 0.5 * np.arctan2(2 * b, a - d)
        ok = s0 > 0
        return s0, m, cov, np.where(ok, lat, np.nan), np.where(ok, lon, np.nan), np.where(ok, lp, 0.0), np.where(ok, lm, 0.0), \
            np.where(ok, theta, np.nan)

    @staticmethod
    def values(shape_rows, rows, height: int, width: int) -> np.ndarray:
        """float64 [n, 10] (EVENT_SHAPE_VALUES): decode's numbers for whole arrays at once (what predict.py stores as
        event_shape_values).  NaN where the zeroth moment is 0 (lat, lon, orientation) or the perimeter is (compactness)."""
        s = np.asarray(shape_rows, np.int64).reshape(-1, len(EVENT_SHAPE_FIELDS))
        rows = np.asarray(rows, np.int64).reshape(-1, len(EVENT_FIELDS))
        _, _, _, lat, lon, lp, lm, theta = EventShape.moments(s, rows)
        dlat, dlon = EventShape.steps(height, width)
        out = np.empty((len(s), len(EVENT_SHAPE_VALUES)), np.float64)
        length, wid = EARTH_RADIUS_KM * EventShape.arc_angle(12.0 * lp), EARTH_RADIUS_KM * np.sqrt(12.0 * lm)
        perimeter = EARTH_RADIUS_KM * (dlat * s[:, 1].astype(np.float64) + dlon * s[:, 2].astype(np.float64) / EVENT_SCALE)
        area = EventFilter.area_km2(rows[:, 3].astype(np.float64), height, width)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, 0], out[:, 1] = np.degrees(lat), np.degrees(lon)
            out[:, 2], out[:, 3] = length, wid
            out[:, 4] = np.where(lm > 0, np.sqrt(lp / lm), np.inf)
            out[:, 5] = np.degrees(theta)                     # atan2 lies in (-pi, pi]: half of it in (-90, 90]
            out[:, 6], out[:, 7] = perimeter, area
            out[:, 8] = np.where(perimeter > 0, 4.0 * math.pi * area / (perimeter * perimeter), np.nan)
            out[:, 9] = s[:, 0]
        return out

    @staticmethod
    def decode(shape_rows, rows, height: int, width: int):
        """Shape rows [n, 12] (EVENT_SHAPE_FIELDS) and the events' own rows [n, 10] (EVENT_FIELDS) -> one dict per event with the keys of
        EVENT_SHAPE_VALUES, R = 6371 km: lat / lon of the spherical centroid in degrees; sqrt(12 lambda+) and sqrt(12 lambda-) are the
        sides of the uniform strip with the same second moments in chord space (not a skeleton length).  width_km = R sqrt(12 lambda-).
        length_km = R theta with 6 (1 - sin(theta) / theta) = 12 lambda+: the great-circle arc with that second moment (arc_angle) --
        R sqrt(12 lambda+) itself is the chord-space figure and falls short of a long thin event by theta^2 / 40, 2.7 % at 6700 km.
        aspect = sqrt(lambda+ / lambda-), the ratio of the strip's sides and the number the filter compares (inf at width 0);
        orientation_deg of the major axis, counter-clockwise from east, in (-90, 90]; perimeter_km =
        R (dlat faces_v + dlon faces_h / 2^20); area_km2 from the catalogue's area; compactness = 4 pi area / perimeter^2;
        boundary_pixels."""
        vals = EventShape.values(shape_rows, rows, height, width)
        out = []
        for v in vals:
            d = {k: float(x) for k, x in zip(EVENT_SHAPE_VALUES, v)}
            d["boundary_pixels"] = int(v[9])
            out.append(d)
        return out


class EventFilter:
    """A size and shape filter for the events of a mask, on the device (dc_event_select + dc_mask_select behind an EventCatalog and an
    EventShape): an event of class k is kept iff it has at least min_pixels[k] pixels, min_area_km2[k] of area, min_length_km[k] of length
    and min_aspect[k] of aspect (EventShape.decode's numbers; 0: the criterion is off), and the filtered mask keeps the pixels of kept
    events -- and of events beyond the catalogue's cap, for which nothing was evaluated.  Each threshold is a pair (class 1, class 2).
    `catalog` is the filter's own catalogue of the RAW mask; whatever consumes the filtered mask (another EventCatalog, a matcher, a
    tracker, ...) does so unchanged.  Nothing is copied to the host and nothing synchronises."""

    def __init__(self, catalog: EventCatalog, min_pixels=(0, 0), min_area_km2=(0, 0), min_length_km=(0, 0), min_aspect=(0, 0)):
        self.min_pixels, self.min_area_km2 = self._pair(min_pixels, "min_pixels"), self._pair(min_area_km2, "min_area_km2")
        self.min_length_km, self.min_aspect = self._pair(min_length_km, "min_length_km"), self._pair(min_aspect, "min_aspect")
        self.catalog = catalog
        self.shape = EventShape(catalog)
        dev = catalog._labels.device
        self.criteria = self.criteria_rows(catalog.H, catalog.W, self.min_pixels, self.min_area_km2, self.min_length_km, self.min_aspect)
        self._criteria = torch.from_numpy(self.criteria.view(np.int64).copy()).to(dev)
        self._keep = torch.zeros((catalog.B, catalog.cap), dtype=torch.uint8, device=dev)
        self._counts = torch.zeros((catalog.B, 2, len(EVENT_FILTER_COUNTS)), dtype=torch.int64, device=dev)
        self._out = torch.zeros((catalog.B, catalog.H, catalog.W), dtype=torch.uint8, device=dev)
        self._last_valid = 0

    @staticmethod
    def _pair(v, name):
        v = tuple(float(x) for x in (v if isinstance(v, (tuple, list, np.ndarray)) else (v, v)))
        if len(v) != 2 or any(not (x >= 0) or math.isinf(x) for x in v):
            raise L.DeepcamHipError(f"EventFilter: {name} takes two finite values >= 0 (class 1, class 2), got {v}")
        return v

    # -- the thresholds in the kernel's units, and back (the checker and the tests use the same ones)
    @staticmethod
    def pixel_area_km2(height: int, width: int) -> float:
        """km^2 of one pixel on the equator: R^2 dlat dlon"""
        dlat, dlon = EventShape.steps(height, width)
        return EARTH_RADIUS_KM * EARTH_RADIUS_KM * dlat * dlon

    @staticmethod
    def area_units(km2: float, height: int, width: int) -> int:
        """min_area: the smallest catalogue area (field 3: sum of 2^20 cos lat) that is at least km2"""
        return int(math.ceil(float(km2) / EventFilter.pixel_area_km2(height, width) * EVENT_SCALE))

    @staticmethod
    def area_km2(units, height: int, width: int):
        return units / float(EVENT_SCALE) * EventFilter.pixel_area_km2(height, width)

    @staticmethod
    def length_units(km: float) -> float:
        """min_len2 = chord_moment(km / R): length_km >= km  iff  12 lambda+ >= min_len2 (both sides of decode's arc_angle)"""
        theta = float(km) / EARTH_RADIUS_KM
        if not 0.0 <= theta <= EventShape.ARC_MAX:
            raise L.DeepcamHipError(f"EventFilter: a length threshold must lie in [0, {EARTH_RADIUS_KM * EventShape.ARC_MAX:.0f}] km, got {km}")
        return float(EventShape.chord_moment(theta))

    @staticmethod
    def length_km(len2: float) -> float:
        return EARTH_RADIUS_KM * float(EventShape.arc_angle(len2))

    @staticmethod
    def aspect_units(aspect: float) -> float:
        """min_aspect2 = aspect^2: decode's aspect >= aspect  iff  lambda+ >= min_aspect2 lambda-"""
        return float(aspect) ** 2

    @staticmethod
    def aspect(aspect2: float) -> float:
        return math.sqrt(aspect2)

    CRITERIA = np.dtype([("min_pixels", np.int64), ("min_area", np.int64), ("min_len2", np.float64), ("min_aspect2", np.float64)])

    @staticmethod
    def criteria_rows(height: int, width: int, min_pixels=(0, 0), min_area_km2=(0, 0), min_length_km=(0, 0), min_aspect=(0, 0)) -> np.ndarray:
        """the two rows dc_event_select takes (class 1, class 2), a numpy record array of dtype CRITERIA"""
        out = np.zeros(2, EventFilter.CRITERIA)
        for k in range(2):
            out[k] = (int(math.ceil(min_pixels[k])), EventFilter.area_units(min_area_km2[k], height, width),
                      EventFilter.length_units(min_length_km[k]), EventFilter.aspect_units(min_aspect[k]))
        return out

    def thresholds(self) -> dict:
        return {"min_pixels": list(self.min_pixels), "min_area_km2": list(self.min_area_km2), "min_length_km": list(self.min_length_km),
                "min_aspect": list(self.min_aspect)}

    def __call__(self, mask: torch.Tensor, n_valid: Optional[int] = None) -> torch.Tensor:
        """mask: device uint8 [B, H, W].  Returns the filtered mask [n_valid, H, W], a view of a buffer this object owns (mask_buffer is
        the whole of it; the next call overwrites it).  Samples from n_valid on are padding: neither read nor written."""
        cat = self.catalog
        cat(mask, n_valid=n_valid)
        nv = cat._last_valid
        self.shape(nv)
        st = L.stream_ptr()
        L.call("dc_event_select", cat.B, nv, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(self.shape._shape), L.dptr(self._criteria),
               L.dptr(self._keep), L.dptr(self._counts), st)
        L.call("dc_mask_select", cat.B, nv, cat.H, cat.W, L.dptr(mask), L.dptr(cat._labels), L.dptr(cat._ws), cat.cap, L.dptr(self._keep),
               L.dptr(self._out), L.dptr(self._counts), st)
        self._last_valid = nv
        return self._out[:nv]

    @property
    def mask_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the whole buffer the filtered masks are written to, padding samples included"""
        return self._out

    @property
    def keep(self) -> torch.Tensor:
        """uint8 [n_valid, cap] of the last call (a view): 1 for a kept event, 0 for a dropped one and for rows without an event"""
        return self._keep[:self._last_valid]

    def counts(self) -> torch.Tensor:
        """int64 [n_valid, 2, 4] of the last call (a view): per class EVENT_FILTER_COUNTS (events among the ranks below cap)"""
        return self._counts[:self._last_valid]


TRACK_STORE_FIELDS = ("frame", "rank") + EVENT_FIELDS
TRACK_FIELDS = ("id", "class", "events", "first_frame", "last_frame", "pixels", "peak", "area")


class EventTracker:
    """Events linked across time steps on the device (dc_track_append, dc_track_link, dc_track_resolve, csrc/tracks.hip): the frames
    given since reset() are one time series, frame numbers 0, 1, 2, ...; two events of consecutive frames are linked when they have the
    same class, share at least one pixel and each has at least max(min_pixels, 1) pixels; a track is a connected component of the events
    under these links (merges and splits stay in one track), its id the smallest event number it holds (include/deepcam_hip.h has the
    definitions).  Built on an existing EventCatalog, as EventFields is.  The object owns the state that survives from call to call --
    the four counters, the forest over event numbers, the store (int64 [event_cap, 12], TRACK_STORE_FIELDS) -- and one-frame copies of
    the last frame's mask, labels, rank map and first event number, because the caller's mask buffer and the catalogue's workspace are
    overwritten by the next call.  A call must follow the catalogue's call for that mask on the same stream; it launches and neither
    synchronises nor reads anything back.  tracks() / rows() resolve and read back only the filled parts."""

    def __init__(self, catalog: EventCatalog, event_cap: int = 1 << 19, track_cap: Optional[int] = None, min_pixels: int = 0):
        event_cap = int(event_cap)
        track_cap = event_cap if track_cap is None else int(track_cap)
        if not 1 <= event_cap <= 1 << 30:
            raise L.DeepcamHipError(f"EventTracker: event_cap must lie in [1, 2^30], got {event_cap}")
        if not 1 <= track_cap <= event_cap:
            raise L.DeepcamHipError(f"EventTracker: track_cap must lie in [1, event_cap], got {track_cap}")
        if int(min_pixels) < 0:
            raise L.DeepcamHipError("EventTracker: min_pixels must not be negative")
        if event_cap > ((1 << 43) - 1) // (catalog.H * catalog.W):
            raise L.DeepcamHipError(f"EventTracker: event_cap * H * W * 2^20 must stay below 2^63, got event_cap {event_cap} at "
                                    f"{catalog.H} x {catalog.W}")
        self.catalog, self.event_cap, self.track_cap, self.min_pixels = catalog, event_cap, track_cap, int(min_pixels)
        dev = catalog._labels.device
        H, W = catalog.H, catalog.W
        self._state = torch.zeros(4, dtype=torch.int64, device=dev)
        self._first = torch.zeros(catalog.B, dtype=torch.int64, device=dev)
        self._parent = torch.empty(event_cap, dtype=torch.int32, device=dev)
        self._store = torch.empty((event_cap, len(TRACK_STORE_FIELDS)), dtype=torch.int64, device=dev)
        self._track_of = torch.empty(event_cap, dtype=torch.int32, device=dev)
        self._tracks = torch.zeros((track_cap, len(TRACK_FIELDS)), dtype=torch.int64, device=dev)
        self._ntracks = torch.zeros(4, dtype=torch.int64, device=dev)
        self._ws = torch.empty(L.load().dc_track_workspace(event_cap), dtype=torch.uint8, device=dev)
        # the carry: the last valid frame of the call before
        self._c_mask = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
        self._c_labels = torch.zeros((1, H, W), dtype=torch.int32, device=dev)
        self._c_rank = torch.zeros((1, H, W), dtype=torch.int32, device=dev)
        self._c_first = torch.zeros(1, dtype=torch.int64, device=dev)
        self._carry = False
        self._frames = 0                           # frames given since reset(), counted on the host: the next call's frame0

    def __call__(self, mask: torch.Tensor, n_valid: Optional[int] = None) -> "EventTracker":
        """mask: the device uint8 [B, H, W] the catalogue was just called with.  n_valid defaults to the catalogue's and must equal it."""
        cat = self.catalog
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (cat.B, cat.H, cat.W) or not mask.is_cuda or not mask.is_contiguous() \
                or mask.device != cat._labels.device:
            raise L.DeepcamHipError(f"EventTracker: mask must be a contiguous uint8 tensor [{cat.B}, {cat.H}, {cat.W}] on {cat._labels.device}, "
                                    f"got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
        nv = cat._last_valid if n_valid is None else int(n_valid)
        if nv < 1 or nv != cat._last_valid:
            raise L.DeepcamHipError(f"EventTracker: call the catalogue on this mask first, with the same n_valid (its last call had "
                                    f"{cat._last_valid}, this one has {nv})")
        HW, st = cat.H * cat.W, L.stream_ptr()
        at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size())  # noqa: E731
        L.call("dc_track_append", cat.B, nv, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), self._frames, self.event_cap, L.dptr(self._state),
               L.dptr(self._first), L.dptr(self._parent), L.dptr(self._store), st)
        link = lambda n, a, b: L.call("dc_track_link", n, cat.H, cat.W, *a, *b, cat.cap, self.event_cap, self.min_pixels,  # noqa: E731
                                      L.dptr(self._store), L.dptr(self._parent), st)
        side = lambda k: (at(mask, k * HW), at(cat._labels, k * HW), at(cat._ws, 4 * k * HW), at(self._first, k))  # noqa: E731
        if nv > 1:
            link(nv - 1, side(0), side(1))
        if self._carry:
            link(1, (L.dptr(self._c_mask), L.dptr(self._c_labels), L.dptr(self._c_rank), L.dptr(self._c_first)), side(0))
        for dst, src in zip((self._c_mask, self._c_labels, self._c_rank, self._c_first), side(nv - 1)):
            L.call("dc_memcpy_async", L.dptr(dst), src, dst.numel() * dst.element_size(), st)
        self._carry = True
        self._frames += nv
        return self

    def cut(self) -> None:
        """A break in the sequence: the next frame is not linked to the one before it.  Frame numbering goes on."""
        self._carry = False

    def reset(self) -> None:
        """Forget every frame: the next one is frame 0."""
        L.call("dc_memset_async", L.dptr(self._state), 0, 32, L.stream_ptr())
        self._carry = False
        self._frames = 0

    def state(self) -> dict:
        """the four counters (one device-to-host read)"""
        s = [int(v) for v in self._state.cpu().tolist()]
        return {"events": s[0], "frames": s[1], "events_dropped": s[2], "frames_truncated": s[3]}

    def resolve(self) -> "EventTracker":
        """dc_track_resolve on the current stream: track_of, the track rows and the counts for the frames given so far.  Does not
        synchronise; may be called in the middle of a series."""
        L.call("dc_track_resolve", self.event_cap, self.track_cap, L.dptr(self._state), L.dptr(self._parent), L.dptr(self._store),
               L.dptr(self._track_of), L.dptr(self._tracks), L.dptr(self._ntracks), L.dptr(self._ws), L.stream_ptr())
        return self

    def track_counts(self) -> np.ndarray:
        """int64 [4] of the last resolve: tracks of any class, of class 1, of class 2 (not capped), rows stored"""
        return self._ntracks.cpu().numpy()

    def rows(self):
        """(state int64 [4], store rows int64 [n, 12], track_of int32 [n], track rows int64 [m, 8]) as numpy arrays: resolves, reads the
        counters, then only the filled parts."""
        self.resolve()
        state = self._state.cpu().numpy()
        n, m = int(state[0]), int(self._ntracks[3].item())
        return state, self._store[:n].cpu().numpy(), self._track_of[:n].cpu().numpy(), self._tracks[:m].cpu().numpy()

    def tracks(self, min_frames: int = 1):
        """The tracks of the frames given so far as a list of dicts (decode), those of fewer than min_frames frames left out."""
        _, store, track_of, tracks = self.rows()
        return self.decode(store, track_of, tracks, self.catalog.H, self.catalog.W, min_frames=min_frames)

    @staticmethod
    def decode(store, track_of, tracks, height: int, width: int, min_frames: int = 1):
        """Store rows [n, 12] (TRACK_STORE_FIELDS), track_of [n] and track rows [m, 8] (TRACK_FIELDS) -> one dict per track with at least
        min_frames frames, in row order: id, class, first_frame, last_frame, frames (last - first + 1), events, pixels, peak_pixels and
        peak_frame (the largest single event and its frame, the earliest among equals), area_fraction_sum (the events' area fractions
        summed) and path: per frame of the track its events' count, their pixels and the centroid lat / lon by EventCatalog.decode's
        formulas over the SUMMED columns, so two fragments of one frame give their joint centroid.  Needs no GPU."""
        store = np.asarray(store, np.int64).reshape(-1, len(TRACK_STORE_FIELDS))
        track_of = np.asarray(track_of, np.int64).reshape(-1)
        tracks = np.asarray(tracks, np.int64).reshape(-1, len(TRACK_FIELDS))
        wy = event_weight_tables(height, width)[0]
        whole = float(width) * float(wy.astype("int64").sum())
        order = np.argsort(track_of, kind="stable")
        lo = np.searchsorted(track_of[order], np.arange(len(tracks)), side="left")
        hi = np.searchsorted(track_of[order], np.arange(len(tracks)), side="right")
        out = []
        for t, row in enumerate(tracks.tolist()):
            tid, cls, nev, f0, f1, px, peak, area = row
            if f1 - f0 + 1 < min_frames:
                continue
            peak &= 0xFFFFFFFFFFFFFFFF
            ev = store[order[lo[t]:hi[t]]]
            path = []
            for f in np.unique(ev[:, 0]).tolist():
                n, sr, scx, ssx = (int(v) for v in ev[ev[:, 0] == f][:, [4, 6, 7, 8]].sum(axis=0))
                lat = -90.0 + 180.0 * (sr / n) / (height - 1) if height > 1 and n > 0 else -90.0
                path.append({"frame": f, "events": int((ev[:, 0] == f).sum()), "pixels": n, "lat": lat, "lon": math.degrees(math.atan2(ssx, scx))})
            out.append({"id": tid, "class": cls, "first_frame": f0, "last_frame": f1, "frames": f1 - f0 + 1, "events": nev, "pixels": px,
                        "peak_pixels": peak >> 32, "peak_frame": 0xFFFFFFFF - (peak & 0xFFFFFFFF),
                        "area_fraction_sum": area / whole if whole > 0 else 0.0, "path": path})
        return out


TRACK_STEP_FIELDS = ("track", "frame", "events", "pixels", "area", "sum_row", "sum_cx", "sum_sx")
TRACK_FIELD_STATS = ("min", "min_pixel", "max", "max_pixel")


class TrackFields:
    """Storm life cycles on the device (dc_track_fields_append, dc_track_cycles, csrc/tracks.hip): the join of an EventTracker (which
    events of which frames form one storm) and an EventFields of the same catalogue (every event's extremes and sums of the raw fields).
    Per track and frame -- a STEP -- the field rows of the track's events in that frame merged into one (for a cyclone and sea-level
    pressure the minimum's place is the conventional track position, its value the intensity), per track the lifetime extremes with the
    frame and place where they occurred (include/deepcam_hip.h has the definitions).  The object owns the field store (int64 [event_cap,
    C, 6]: 48 * C bytes per event slot next to the tracker's store, 403 MB at the tracker's default event_cap = 2^19 with 16 channels) and
    the output tables: offsets int64 [track_cap], steps int64 [step_cap, 8] (TRACK_STEP_FIELDS), step_fields int64 [step_cap, C, 6]
    (EVENT_FIELD_STATS), track_fields int64 [track_cap, C, 4] (TRACK_FIELD_STATS) and the four counters.  A call launches and neither
    synchronises nor reads anything back; reset() and cut() are the tracker's -- the state follows its counters.  rows() / cycles() resolve
    and read back only the filled parts."""

    def __init__(self, tracker: "EventTracker", fields: EventFields, step_cap: Optional[int] = None):
        if not isinstance(tracker, EventTracker) or not isinstance(fields, EventFields):
            raise L.DeepcamHipError("TrackFields: needs an EventTracker and an EventFields")
        if tracker.catalog is not fields.catalog:
            raise L.DeepcamHipError("TrackFields: the tracker and the fields must be built on the same EventCatalog")
        step_cap = tracker.event_cap if step_cap is None else int(step_cap)
        if not 1 <= step_cap <= (1 << 31) - 1:
            raise L.DeepcamHipError(f"TrackFields: step_cap must lie in [1, 2^31 - 1], got {step_cap}")
        self.tracker, self.fields, self.C, self.step_cap = tracker, fields, fields.C, step_cap
        dev = tracker._store.device
        i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
        self._fstore = torch.empty((tracker.event_cap, self.C, len(EVENT_FIELD_STATS)), dtype=torch.int64, device=dev)
        self._offsets = i64(tracker.track_cap)
        self._steps = i64(step_cap, len(TRACK_STEP_FIELDS))
        self._step_fields = i64(step_cap, self.C, len(EVENT_FIELD_STATS))
        self._track_fields = i64(tracker.track_cap, self.C, len(TRACK_FIELD_STATS))
        self._ncycles = i64(4)
        self._ws = torch.empty(max(L.load().dc_track_cycles_workspace(tracker.event_cap, tracker.track_cap), 256), dtype=torch.uint8, device=dev)

    def __call__(self) -> "TrackFields":
        """Files the field rows of the batch the tracker and the fields were just called with (both, on this stream, before this)."""
        trk, fld, cat = self.tracker, self.fields, self.tracker.catalog
        nv = cat._last_valid
        if nv < 1 or fld._last_valid != nv:
            raise L.DeepcamHipError(f"TrackFields: call the tracker and the fields on the same batch first (the catalogue's last call had "
                                    f"{nv} valid samples, the fields' {fld._last_valid})")
        L.call("dc_track_fields_append", cat.B, nv, cat.cap, L.dptr(cat._ncomp), L.dptr(trk._first), L.dptr(fld._ftable), self.C, trk.event_cap,
               L.dptr(self._fstore), L.stream_ptr())
        return self

    @staticmethod
    def class_mask(classes) -> int:
        mask = 0
        for c in classes:
            if int(c) not in (1, 2):
                raise L.DeepcamHipError(f"TrackFields: classes are 1 and 2, got {c}")
            mask |= 1 << int(c)
        if mask == 0:
            raise L.DeepcamHipError("TrackFields: no class selected")
        return mask

    def launch(self, min_frames: int = 1, classes=(1, 2)) -> "TrackFields":
        """dc_track_resolve and dc_track_cycles on the current stream, for the frames given so far.  Does not synchronise."""
        trk = self.tracker
        trk.resolve()
        L.call("dc_track_cycles", trk.event_cap, trk.track_cap, self.step_cap, self.C, max(int(min_frames), 0), self.class_mask(classes),
               L.dptr(trk._state), L.dptr(trk._store), L.dptr(trk._track_of), L.dptr(trk._tracks), L.dptr(trk._ntracks), L.dptr(self._fstore),
               L.dptr(self._offsets), L.dptr(self._steps), L.dptr(self._step_fields), L.dptr(self._track_fields), L.dptr(self._ncycles),
               L.dptr(self._ws), L.stream_ptr())
        return self

    def rows(self, min_frames: int = 1, classes=(1, 2)) -> dict:
        """launch(), then the counters and only the filled parts as numpy arrays: "counts" int64 [4] (tracks selected, step rows needed, step
        rows stored, tracks selected but not stored), "tracks" int64 [m, 8], "offsets" int64 [m], "steps" int64 [n, 8], "step_fields" int64
        [n, C, 6], "track_fields" int64 [m, C, 4], with m the tracker's stored track rows and n the stored step rows."""
        self.launch(min_frames, classes)
        counts = self._ncycles.cpu().numpy()
        m, n = int(self.tracker._ntracks[3].item()), int(counts[2])
        return {"counts": counts, "tracks": self.tracker._tracks[:m].cpu().numpy(), "offsets": self._offsets[:m].cpu().numpy(),
                "steps": self._steps[:n].cpu().numpy(), "step_fields": self._step_fields[:n].cpu().numpy(),
                "track_fields": self._track_fields[:m].cpu().numpy()}

    def cycles(self, min_frames: int = 1, classes=(1, 2), center_channel: Optional[int] = None):
        """The life cycles of the frames given so far as a list of dicts (decode)."""
        r = self.rows(min_frames, classes)
        cat = self.tracker.catalog
        return self.decode(r["tracks"], r["offsets"], r["steps"], r["step_fields"], r["track_fields"], cat.H, cat.W, self.fields.bits,
                           center_channel=center_channel)

    @staticmethod
    def decode(tracks, offsets, steps, step_fields, track_fields, height: int, width: int, bits, center_channel: Optional[int] = None):
        """Track rows [m, 8] (TRACK_FIELDS), offsets [m], step rows [n, 8] (TRACK_STEP_FIELDS), their field rows [n, C, 6]
        (EVENT_FIELD_STATS) and the lifetime rows [m, C, 4] (TRACK_FIELD_STATS) -> one dict per STORED track (offsets >= 0), in row order:
        id, class, first_frame, last_frame, frames, events, pixels, peak_pixels, peak_frame, area_fraction_sum as EventTracker.decode gives
        them; fields: per channel min, min_frame, min_row, min_col, min_lat, min_lon, the same for max (None where the track has no finite
        value), mean = the step sums added in Python integers * 2^-bits / the pixels that took part (None without any) and nonfinite,
        saturated; series: per frame of the track frame, events, pixels, the centroid lat / lon by EventCatalog.decode's formulas over the
        summed columns, and fields: the EventFields.decode entries of the merged row.  With center_channel = c every series entry also
        has center_lat / center_lon, the place of channel c's minimum (None where the step has no finite value).  Needs no GPU."""
        bits = [int(v) for v in np.asarray(bits).reshape(-1)]
        nch = len(bits)
        tracks = np.asarray(tracks, np.int64).reshape(-1, len(TRACK_FIELDS))
        offsets = np.asarray(offsets, np.int64).reshape(-1)
        steps = np.asarray(steps, np.int64).reshape(-1, len(TRACK_STEP_FIELDS))
        step_fields = np.asarray(step_fields, np.int64).reshape(-1, nch, len(EVENT_FIELD_STATS))
        track_fields = np.asarray(track_fields, np.int64).reshape(-1, nch, len(TRACK_FIELD_STATS))
        if center_channel is not None and not 0 <= int(center_channel) < nch:
            raise L.DeepcamHipError(f"TrackFields: center_channel must lie in [0, {nch}), got {center_channel}")
        lat, lon = np.linspace(-90.0, 90.0, height), np.linspace(-180.0, 180.0, width)
        wy = event_weight_tables(height, width)[0]
        whole = float(width) * float(wy.astype("int64").sum())
        out = []
        for t, row in enumerate(tracks.tolist()):
            off = int(offsets[t])
            if off < 0:
                continue
            tid, cls, nev, f0, f1, px, peak, area = row
            peak &= 0xFFFFFFFFFFFFFFFF
            st = steps[off:off + f1 - f0 + 1]
            sf = step_fields[off:off + f1 - f0 + 1]
            if len(st) != f1 - f0 + 1 or (st[:, 0] != t).any() or (st[:, 1] != np.arange(f0, f1 + 1)).any():
                raise L.DeepcamHipError(f"TrackFields.decode: the step rows of track row {t} are not its frames {f0} .. {f1}")
            # a step as one event row (EVENT_FIELDS): pixels, area and the centroid sums are the columns the decoders read
            pseudo = np.zeros((len(st), len(EVENT_FIELDS)), np.int64)
            pseudo[:, 1], pseudo[:, 2:7] = cls, st[:, 3:8]
            per_step = EventFields.decode(sf, pseudo, height, width, bits)
            series = []
            for (_, f, n_ev, n, _a, sr, scx, ssx), per in zip(st.tolist(), per_step):
                la = -90.0 + 180.0 * (sr / n) / (height - 1) if height > 1 and n > 0 else -90.0
                entry = {"frame": f, "events": n_ev, "pixels": n, "lat": la, "lon": math.degrees(math.atan2(ssx, scx)), "fields": per}
                if center_channel is not None:
                    entry["center_lat"], entry["center_lon"] = per[int(center_channel)]["min_lat"], per[int(center_channel)]["min_lon"]
                series.append(entry)
            life = []
            for ch, (wlo, plo, whi, phi) in enumerate(track_fields[t].tolist()):
                total = sum(int(v) for v in sf[:, ch, 2])
                nonfinite, saturated = int(sf[:, ch, 4].sum()), int(sf[:, ch, 5].sum())
                n = px - nonfinite - saturated
                d = {"nonfinite": nonfinite, "saturated": saturated, "mean": math.ldexp(float(total), -bits[ch]) / n if n > 0 else None}
                for name, word, p, empty in (("min", wlo, plo, -1), ("max", whi, phi, 0)):
                    if word == empty:
                        d.update({name: None, name + "_frame": None, name + "_row": None, name + "_col": None, name + "_lat": None,
                                  name + "_lon": None})
                        continue
                    word &= 0xFFFFFFFFFFFFFFFF
                    frame = word & 0xFFFFFFFF if name == "min" else 0xFFFFFFFF - (word & 0xFFFFFFFF)
                    d.update({name: float(event_field_value(np.uint32(word >> 32))), name + "_frame": frame, name + "_row": p // width,
                              name + "_col": p % width, name + "_lat": float(lat[p // width]), name + "_lon": float(lon[p % width])})
                life.append(d)
            out.append({"id": tid, "class": cls, "first_frame": f0, "last_frame": f1, "frames": f1 - f0 + 1, "events": nev, "pixels": px,
                        "peak_pixels": peak >> 32, "peak_frame": 0xFFFFFFFF - (peak & 0xFFFFFFFF),
                        "area_fraction_sum": area / whole if whole > 0 else 0.0, "fields": life, "series": series})
        return out


class Predictor:
    """Masks for unlabelled data: the eval forward on a forward-only engine (Engine(forward_only=True): the net's weights and running
    statistics through the shared arena, pooled activations) whose classifier leaves, per pixel, the first-max class as one byte
    (torch.max(outputs, 1)[1] of train_hdf5_ddp.py:458), optionally its softmax probability, and per sample the pixels of each class
    (bf16: dc_head_fwd_predict on the logits in registers; fp32: dc_head_fwd + dc_logits_predict).  Nothing here synchronises.
    events=True adds `.catalog`, an EventCatalog that runs on the mask of every call."""

    def __init__(self, net: DeepLabv3_plus, batch: int, height: int, width: int, confidence: bool = False, events: bool = False,
                 event_connectivity: int = 8, event_cap: int = 4096):
        if net.engine is None:
            raise L.DeepcamHipError("Predictor: materialize the model first (its parameters live in the primary engine's arena)")
        self.net, self.B, self.H, self.W = net, batch, height, width
        self.eng = Engine(batch, height, width, net.act_dtype, n_input=net.n_input, n_classes=net.n_classes, share_from=net.engine,
                          forward_only=True)
        dev = self.eng.device
        self._mask = torch.zeros((batch, height, width), dtype=torch.uint8, device=dev)
        self._conf = torch.zeros((batch, height, width), dtype=torch.float32, device=dev) if confidence else None
        self._counts = torch.zeros((batch, 3), dtype=torch.int64, device=dev)
        self._last_valid = 0
        self.store_logits = False       # bf16: also write the fp32 NCHW logits (the prediction needs them in registers only)
        self._eng_handle = _ops.engine_handle(self.eng)
        # events=True: the event catalogue of every mask (EventCatalog below), run behind the classifier on the same stream
        self.catalog = EventCatalog(batch, height, width, connectivity=event_connectivity, cap=event_cap, device=dev) if events else None

    def __call__(self, x: torch.Tensor, n_valid: Optional[int] = None) -> torch.Tensor:
        """x: the NCHW fp32 batch or the input pipeline's NHWC batch (Engine.forward); returns the uint8 mask [n_valid, H, W], a view of a
        buffer this object owns (the next call overwrites it).  The samples from n_valid on are padding: the network's body computes
        them, the classifier does not, and their bytes in the buffers stay as they were."""
        eng, B = self.eng, self.B
        nv = B if n_valid is None else int(n_valid)
        if not 0 < nv <= B:
            raise L.DeepcamHipError(f"Predictor: n_valid must lie in [1, {B}], got {n_valid}")
        L.call("dc_memset_async", L.dptr(self._counts), 0, 24 * nv, L.stream_ptr())
        eng.predict_args = {"n_valid": nv, "mask": self._mask, "conf": self._conf, "class_counts": self._counts,
                            "store_logits": self.store_logits}
        try:
            _ops.OPS.net_forward(x, self._eng_handle, False)
        finally:
            eng.predict_args = None
        self._last_valid = nv
        if self.catalog is not None:
            self.catalog(self._mask, n_valid=nv)
        return self._mask[:nv]

    @property
    def mask_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the whole buffer the masks are written to, padding samples included (what EventCatalog / EventMatcher take)"""
        return self._mask

    @property
    def confidence(self) -> Optional[torch.Tensor]:
        """fp32 [n_valid, H, W] of the last call: the predicted class's softmax probability (None unless built with confidence=True)"""
        return None if self._conf is None else self._conf[:self._last_valid]

    @property
    def class_counts(self) -> torch.Tensor:
        """int64 [n_valid, 3] of the last call: pixels per class and sample"""
        return self._counts[:self._last_valid]

    @property
    def logits(self) -> torch.Tensor:
        """the engine's fp32 NCHW logits of the last call (fp32 engines always; bf16 with store_logits=True), valid samples only"""
        return self.eng.logits[:self._last_valid]

    @property
    def logits_buffer(self) -> torch.Tensor:
        """fp32 [B, 3, H, W]: the whole buffer the logits are written to, padding samples included (what ProbabilitySkill takes)"""
        return self.eng.logits

    def close(self) -> None:
        self.eng.close()
        self._mask = self._conf = self._counts = self.catalog = None


# ------------------------------------------------------------------------------------------------------------------
# frame renderer (utils/visualizer.py: CamVisualizer.plot, called from train_hdf5_ddp.py:374-394,463-476)
# ------------------------------------------------------------------------------------------------------------------
def gall_rows(height: int, width: int) -> np.ndarray:
    """int32 [Ho]: the source row of every output row of a Gall stereographic picture `width` pixels wide, whose height over width is
    (1 + sqrt(2) / 2) * 2 / (sqrt(2) * pi): Ho = round(width * (2 + sqrt(2)) / (sqrt(2) * pi)), 885 for 1152.  Output row y shows the
    latitude 2 * atan(1 - 2 * (y + 1/2) / Ho); its source row is the nearest one of linspace(-90, 90, height).  North is at the top: the
    table runs from height - 1 down to 0.  The lower half mirrors the upper one (t[y] + t[Ho - 1 - y] = height - 1); with Ho odd the
    middle row shows the equator, which lies between two source rows when height is even."""
    ho = int(round(width * (2.0 + math.sqrt(2.0)) / (math.sqrt(2.0) * math.pi)))
    y = np.arange(ho, dtype=np.float64)
    lat = np.rad2deg(2.0 * np.arctan(1.0 - 2.0 * (y + 0.5) / ho))
    t = np.rint((lat + 90.0) / 180.0 * (height - 1)).astype(np.int64)
    half = ho // 2
    t[ho - half:] = (height - 1 - t[:half])[::-1]
    return np.clip(t, 0, height - 1).astype(np.int32)


def plate_rows(height: int) -> np.ndarray:
    """int32 [height]: every source row once, north (the last row) at the top"""
    return np.arange(height - 1, -1, -1, dtype=np.int32)


RENDER_BACKGROUND = (12, 20, 44)
_RAMP = ((0.0, (20, 40, 90)), (0.35, (30, 120, 160)), (0.7, (130, 200, 190)), (1.0, (250, 250, 235)))


def render_palette(n: int = 64) -> np.ndarray:
    """uint8 [n, 3]: the renderer's colour table for the normalised field, entry i for u = i / (n - 1).  A piecewise-linear ramp (_RAMP:
    deep blue, teal, pale green, near white) whose opacity u^0.75 grows with the value, composited over RENDER_BACKGROUND: dry air
    fades into the background, moist air stands out.  This project's own table; the reference's colour formula is not reproduced."""
    if not 1 <= int(n) <= 256:
        raise L.DeepcamHipError(f"render_palette: n must lie in [1, 256], got {n}")
    u = np.linspace(0.0, 1.0, int(n)) if n > 1 else np.asarray([1.0])
    stops = np.asarray([s[0] for s in _RAMP])
    ramp = np.stack([np.interp(u, stops, [s[1][k] for s in _RAMP]) for k in range(3)], axis=1)
    alpha = (u ** 0.75)[:, None]
    return np.rint(alpha * ramp + (1.0 - alpha) * np.asarray(RENDER_BACKGROUND, np.float64)).astype(np.uint8)


def graticule(rows, width: int, shift: int, parallels: float = 30, meridians: float = 60, height: Optional[int] = None):
    """(row_line uint8 [Ho], col_line uint8 [width]) for a table of source rows: 1 where a graticule line runs.  A parallel every
    `parallels` degrees strictly between the poles, on the output row whose source row is nearest to the parallel's (source rows are
    linspace(-90, 90, height); height defaults to the table's largest entry + 1).  A meridian every `meridians` degrees from longitude 0 =
    source column 0 (columns are longitudes 360 * c / width), on output column (c - shift) mod width.  0 switches either family off."""
    t = np.asarray(rows, np.int64).reshape(-1)
    if height is None:
        height = int(max(t.max(), 0)) + 1
    t = np.clip(t, 0, height - 1)
    row_line, col_line = np.zeros(len(t), np.uint8), np.zeros(width, np.uint8)
    if parallels and parallels > 0 and height > 1:
        k = 1
        while k * parallels < 90.0:
            for lat in (k * parallels, -k * parallels):
                row_line[int(np.argmin(np.abs(t - (lat + 90.0) / 180.0 * (height - 1))))] = 1
            k += 1
        row_line[int(np.argmin(np.abs(t - 0.5 * (height - 1))))] = 1
    if meridians and meridians > 0:
        k = 0
        while k * meridians < 360.0:
            col_line[(int(round(k * meridians / 360.0 * width)) - shift) % width] = 1
            k += 1
    return row_line, col_line


RENDER_COLOURS = {"missing": 0x404040, "line": 0x50FFFFFF, "class1": 0xFFFF4030, "class2": 0xFFFFE040}


def _c_int(v: int) -> int:
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}    # the element sizes of a class mask


class FrameRenderer:
    """The visualiser's picture on the device (dc_render_frames, csrc/render.hip): per sample `panels` panels stacked, the first with
    mask_a's classes outlined (the prediction), the second with mask_b's (the labels), over channel `channel` of the raw fields drawn
    through `palette` across [lo, hi].  projection: "gall" (gall_rows), "plate" (every row once) or an int32 array of source rows, north
    first; shift: the column roll, width // 2 by default (longitude 0 in the middle); outline: the outlines' width in source pixels, 1,
    3, 5 or 7; colours: RENDER_COLOURS with any of its entries replaced (missing 0xRRGGBB, the others 0xAARRGGBB).  The object owns the
    colour table, the row table, the graticule tables, the workspace and the output buffer.  A call launches on the current stream and
    does not synchronise; what it returns is a view of the output buffer, which the next call overwrites."""

    def __init__(self, batch: int, height: int, width: int, channel: int = 0, ldc: int = 16, lo: float = 0.0, hi: float = 1.0,
                 palette=None, projection="gall", outline: int = 3, panels: int = 2, colours: Optional[dict] = None, device=None,
                 shift: Optional[int] = None, parallels: float = 30, meridians: float = 60):
        if batch < 1 or height < 1 or width < 8 or height * width >= 1 << 31:
            raise L.DeepcamHipError("FrameRenderer: batch and height must be positive, width at least 8 and height * width below 2^31")
        if panels not in (1, 2) or outline not in (1, 3, 5, 7) or not 0 <= channel < ldc:
            raise L.DeepcamHipError(f"FrameRenderer: panels must be 1 or 2, outline 1, 3, 5 or 7 and channel in [0, ldc), got {panels}, "
                                    f"{outline}, {channel} of {ldc}")
        self.B, self.H, self.W, self.P, self.channel, self.ldc, self.outline = batch, height, width, panels, channel, ldc, outline
        span = np.float32(hi) - np.float32(lo)
        if not (np.isfinite(np.float32(lo)) and np.isfinite(span) and span > 0):
            raise L.DeepcamHipError(f"FrameRenderer: lo and hi must be finite with hi > lo in fp32, got {lo}, {hi}")
        self.lo = float(np.float32(lo))
        self.scale = float(np.float32(1.0) / span)
        self.palette = np.ascontiguousarray(render_palette() if palette is None else palette)
        if self.palette.dtype != np.uint8 or self.palette.ndim != 2 or self.palette.shape[1] != 3 or not 1 <= len(self.palette) <= 256:
            raise L.DeepcamHipError("FrameRenderer: palette must be uint8 [n, 3] with 1 <= n <= 256")
        if isinstance(projection, str):
            if projection not in ("gall", "plate"):
                raise L.DeepcamHipError(f"FrameRenderer: projection must be 'gall', 'plate' or a table of rows, got {projection!r}")
            self.rows = gall_rows(height, width) if projection == "gall" else plate_rows(height)
        else:
            self.rows = np.ascontiguousarray(np.asarray(projection, np.int32).reshape(-1))
        self.Ho = len(self.rows)
        if self.Ho < 1 or self.Ho * width >= 1 << 31:
            raise L.DeepcamHipError("FrameRenderer: the row table must hold at least one row and Ho * width stay below 2^31")
        self.shift = width // 2 if shift is None else int(shift)
        if not 0 <= self.shift < width:
            raise L.DeepcamHipError(f"FrameRenderer: shift must lie in [0, {width}), got {shift}")
        self.colours = dict(RENDER_COLOURS, **(colours or {}))
        if set(self.colours) != set(RENDER_COLOURS):
            raise L.DeepcamHipError(f"FrameRenderer: colours has the entries {sorted(RENDER_COLOURS)}")
        self.lines = graticule(self.rows, width, self.shift, parallels, meridians, height=height)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._lut = torch.from_numpy(self.palette).to(dev)
        dev = self.device = self._lut.device       # with its index, whatever form `device` came in
        self._rows = torch.from_numpy(self.rows).to(dev)
        self._row_line, self._col_line = (torch.from_numpy(t).to(dev) for t in self.lines)
        self._ws = torch.empty(max(L.load().dc_render_workspace(batch, panels, height, width), 256), dtype=torch.uint8, device=dev)
        self._out = torch.zeros((batch, panels, self.Ho, width, 3), dtype=torch.uint8, device=dev)

    def _mask(self, m: torch.Tensor, name: str) -> int:
        if m.dtype not in _BYTES or tuple(m.shape) != (self.B, self.H, self.W) or not m.is_cuda or m.device != self.device \
                or not m.is_contiguous():
            raise L.DeepcamHipError(f"FrameRenderer: {name} must be a contiguous uint8, int32 or int64 tensor [{self.B}, {self.H}, {self.W}] "
                                    f"on {self.device}, got {m.dtype} {tuple(m.shape)} on {m.device}")
        return _BYTES[m.dtype]

    def __call__(self, fields: torch.Tensor, mask_a: torch.Tensor, mask_b: Optional[torch.Tensor] = None,
                 n_valid: Optional[int] = None) -> torch.Tensor:
        """fields: contiguous device fp32 [B, H, W, ldc], physical units (InputPipeline.raw); mask_a (and, with two panels, mask_b): device
        uint8, int32 or int64 [B, H, W].  Returns uint8 [n_valid, panels * Ho, W, 3]: per sample the panels stacked."""
        want = (self.B, self.H, self.W, self.ldc)
        if fields.dtype != torch.float32 or tuple(fields.shape) != want or not fields.is_cuda or fields.device != self.device \
                or not fields.is_contiguous():
            raise L.DeepcamHipError(f"FrameRenderer: fields must be a contiguous fp32 tensor {list(want)} on {self.device}, got "
                                    f"{fields.dtype} {tuple(fields.shape)} on {fields.device}")
        if (mask_b is None) != (self.P == 1):
            raise L.DeepcamHipError(f"FrameRenderer: built for {self.P} panel(s): mask_b is given exactly when there are two")
        a_bytes = self._mask(mask_a, "mask_a")
        b_bytes = self._mask(mask_b, "mask_b") if mask_b is not None else 0
        nv = self.B if n_valid is None else int(n_valid)
        if not 0 < nv <= self.B:
            raise L.DeepcamHipError(f"FrameRenderer: n_valid must lie in [1, {self.B}], got {n_valid}")
        c = self.colours
        L.call("dc_render_frames", self.B, nv, self.H, self.W, L.dptr(fields), self.channel, self.ldc, self.lo, self.scale,
               L.dptr(self._lut), len(self.palette), L.dptr(mask_a), a_bytes, L.dptr(mask_b), b_bytes, L.dptr(self._rows), self.Ho,
               self.shift, L.dptr(self._row_line), L.dptr(self._col_line), _c_int(c["missing"]), _c_int(c["line"]), _c_int(c["class1"]),
               _c_int(c["class2"]), self.outline, L.dptr(self._out), L.dptr(self._ws), L.stream_ptr())
        return self._out[:nv].view(nv, self.P * self.Ho, self.W, 3)


# ---------------------------------------------------------------------------------------------- climatology: the maps over time
CLIMATOLOGY_ROWS = ("all", "class1", "class2")
CLIMATOLOGY_PRODUCTS = {"frequency": 0, "mean": 1, "share": 2}
CLIMATOLOGY_MAX_FRAMES = (1 << 31) - 1
CLIMATOLOGY_GROUPS = {"all": ("all",), "month": tuple(f"{m:02d}" for m in range(1, 13)), "season": ("DJF", "MAM", "JJA", "SON")}
_SEASON_OF_MONTH = (0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0)                      # DJF, MAM, JJA, SON
_DATE = re.compile(r"(\d{4})-(\d{2})-(\d{2})")


def climatology_group(name: str, by: str = "all") -> int:
    """The group of a file from its base name: by = "all": 0; "month": 0 .. 11; "season": DJF, MAM, JJA, SON -> 0 .. 3 (December is season
    0).  The date is the first YYYY-MM-DD in the name; a name without one (or with a month outside 1 .. 12) is an error unless by is
    "all"."""
    if by not in CLIMATOLOGY_GROUPS:
        raise L.DeepcamHipError(f"climatology_group: by must be 'all', 'month' or 'season', got {by!r}")
    if by == "all":
        return 0
    m = _DATE.search(os.path.basename(str(name)))
    month = int(m.group(2)) if m else 0
    if not 1 <= month <= 12:
        raise L.DeepcamHipError(f"climatology_group: no YYYY-MM-DD date in {name!r}")
    return month - 1 if by == "month" else _SEASON_OF_MONTH[month - 1]


class Climatology:
    """Occurrence and class-conditional field maps over time, accumulated on the device (dc_climatology_accumulate, dc_climatology_maps,
    csrc/climatology.hip): per group (1, 4 seasons, 12 months) how many frames a pixel spent inside class 1 / class 2, and per selected
    channel of the raw fields the sum and number of its values over all frames, over the class-1 frames and over the class-2 frames of the
    pixel -- the frequency of cyclones and rivers, the mean field inside them, the share of a field's total they account for.
    channels: indices into the ldc channels of a pixel (ldc defaults to the largest index + 1); bits: the sums' binary scale per SELECTED
    channel (event_field_bits).  The object owns frames (int64 [G]), count (int32 [G, 2, H, W]), sum (int64 [G, 3, H, W, C]) and n (int32
    [G, 3, H, W, C]); everything is an integer sum, so the state does not depend on how a sequence was cut into batches or ordered.
    Memory: G * H * W * (8 + 36 * C) bytes -- 8 for the two counts, 3 * (8 + 4) per selected channel.  768 x 1152 with 16 channels and
    one group: 884736 * 584 = 516.7 MB (12 months: 6.2 GB; without channels 7.1 MB per group).
    A call launches on the current stream and does not synchronise; state() and maps() read back."""

    def __init__(self, batch: int, height: int, width: int, channels: Sequence[int] = (), bits=None, ldc: Optional[int] = None,
                 groups: int = 1, device=None):
        channels = [int(c) for c in channels]
        C = len(channels)
        if batch < 1 or batch > 65535 or height < 1 or width < 1 or height * width >= 1 << 31:
            raise L.DeepcamHipError("Climatology: batch must lie in [1, 65535], height and width be positive and height * width below 2^31")
        if not 1 <= int(groups) <= 65536:
            raise L.DeepcamHipError(f"Climatology: groups must lie in [1, 65536], got {groups}")
        if C > 32:
            raise L.DeepcamHipError(f"Climatology: at most 32 channels, got {C}")
        ldc = int((max(channels) + 1 if C else 0) if ldc is None else ldc)
        if C and (min(channels) < 0 or max(channels) >= ldc):
            raise L.DeepcamHipError(f"Climatology: channels must lie in [0, {ldc}), got {channels}")
        bits = [] if bits is None else [int(v) for v in np.asarray(bits).reshape(-1)]
        if len(bits) != C:
            raise L.DeepcamHipError(f"Climatology: {len(bits)} scale bits for {C} channels")
        self.B, self.H, self.W, self.C, self.ldc, self.G = batch, height, width, C, ldc, int(groups)
        self.channels, self.bits = channels, bits
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._frames = torch.zeros((self.G,), dtype=torch.int64, device=dev)
        dev = self.device = self._frames.device
        self._count = torch.zeros((self.G, 2, height, width), dtype=torch.int32, device=dev)
        self._sum = torch.zeros((self.G, 3, height, width, C), dtype=torch.int64, device=dev) if C else None
        self._n = torch.zeros((self.G, 3, height, width, C), dtype=torch.int32, device=dev) if C else None
        self._bits = torch.tensor(bits, dtype=torch.int32, device=dev) if C else None
        # the identity over all ldc channels travels as a null table: the library then knows it on the host and may take its 16-byte loads
        self._chan = None if channels == list(range(ldc)) else torch.tensor(channels, dtype=torch.int32, device=dev)
        self._tables = {}                            # group tuple -> device int32 [B]: a time-sorted sequence produces few distinct ones
        self._products = {}                          # product tuple -> (device int32 [K, 3], out fp32 [G, H, W, K], contour uint8 [G, H, W])
        self.host_frames = [0] * self.G              # the device's `frames`, counted here too: the overflow bound needs no read-back

    def _group_table(self, groups, n_valid) -> tuple:
        nv = self.B if n_valid is None else int(n_valid)
        if not 0 <= nv <= self.B:
            raise L.DeepcamHipError(f"Climatology: n_valid must lie in [0, {self.B}], got {n_valid}")
        if groups is None or isinstance(groups, (int, np.integer)):
            table = [0 if groups is None else int(groups)] * self.B
        else:
            table = [int(g) for g in groups]
            if len(table) != self.B:
                raise L.DeepcamHipError(f"Climatology: {len(table)} groups for a batch of {self.B}")
        table = tuple(g if j < nv and g >= 0 else -1 for j, g in enumerate(table))
        if any(g >= self.G for g in table):
            raise L.DeepcamHipError(f"Climatology: group indices must be below {self.G}, got {list(table)}")
        return table

    def __call__(self, mask: torch.Tensor, fields: Optional[torch.Tensor] = None, groups=None, n_valid: Optional[int] = None) -> "Climatology":
        """mask: contiguous device uint8, int32 or int64 [B, H, W]; fields: contiguous device fp32 [B, H, W, ldc] in physical units
        (InputPipeline.raw), given exactly when channels were selected; groups: None (every frame to group 0), an int, or B ints, a
        negative one skipping its frame; frames from n_valid on are skipped."""
        if mask.dtype not in _BYTES or tuple(mask.shape) != (self.B, self.H, self.W) or not mask.is_cuda or mask.device != self.device \
                or not mask.is_contiguous():
            raise L.DeepcamHipError(f"Climatology: mask must be a contiguous uint8, int32 or int64 tensor [{self.B}, {self.H}, {self.W}] on "
                                    f"{self.device}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
        if (fields is None) != (self.C == 0):
            raise L.DeepcamHipError(f"Climatology: built for {self.C} channel(s): fields are given exactly when there are some")
        if fields is not None:
            want = (self.B, self.H, self.W, self.ldc)
            if fields.dtype != torch.float32 or tuple(fields.shape) != want or not fields.is_cuda or fields.device != self.device \
                    or not fields.is_contiguous():
                raise L.DeepcamHipError(f"Climatology: fields must be a contiguous fp32 tensor {list(want)} on {self.device}, got "
                                        f"{fields.dtype} {tuple(fields.shape)} on {fields.device}")
        table = self._group_table(groups, n_valid)
        added = [0] * self.G
        for g in table:
            if g >= 0:
                added[g] += 1
        if any(h + a > CLIMATOLOGY_MAX_FRAMES for h, a in zip(self.host_frames, added)):
            raise L.DeepcamHipError(f"Climatology: a group would pass {CLIMATOLOGY_MAX_FRAMES} frames, the bound of the int32 counts")
        if not any(added):
            return self
        dev_table = self._tables.get(table)
        if dev_table is None:
            dev_table = self._tables[table] = torch.tensor(table, dtype=torch.int32, device=self.device)
        L.call("dc_climatology_accumulate", self.B, self.H, self.W, self.G, L.dptr(mask), _BYTES[mask.dtype], L.dptr(fields), self.C,
               max(self.ldc, 1), L.dptr(self._chan), L.dptr(self._bits), L.dptr(dev_table), L.dptr(self._frames), L.dptr(self._count),
               L.dptr(self._sum), L.dptr(self._n), L.stream_ptr())
        self.host_frames = [h + a for h, a in zip(self.host_frames, added)]
        return self

    def reset(self) -> None:
        """zeroes the accumulators (in stream order)"""
        for t in (self._frames, self._count, self._sum, self._n):
            if t is not None:
                t.zero_()
        self.host_frames = [0] * self.G

    def state(self) -> dict:
        """the four accumulators on the host: frames int64 [G], count int32 [G, 2, H, W], sum int64 / n int32 [G, 3, H, W, C]"""
        empty = (self.G, 3, self.H, self.W, 0)
        return {"frames": self._frames.cpu().numpy(), "count": self._count.cpu().numpy(),
                "sum": self._sum.cpu().numpy() if self.C else np.zeros(empty, np.int64),
                "n": self._n.cpu().numpy() if self.C else np.zeros(empty, np.int32)}

    def product_table(self, products) -> np.ndarray:
        """int32 [K, 3] of products given as ("frequency", k), ("mean", c, row) or ("share", c, k): k the class 1 or 2, c the POSITION of
        a selected channel, row 0 / 1 / 2 or a name of CLIMATOLOGY_ROWS"""
        out = []
        for prod in products:
            kind, args = prod[0], list(prod[1:])
            if kind not in CLIMATOLOGY_PRODUCTS or len(args) != (1 if kind == "frequency" else 2):
                raise L.DeepcamHipError(f"Climatology: a product is ('frequency', k), ('mean', c, row) or ('share', c, k), got {prod!r}")
            if kind == "mean" and args[1] in CLIMATOLOGY_ROWS:
                args[1] = CLIMATOLOGY_ROWS.index(args[1])
            args = [int(a) for a in args] + [0] * (2 - len(args))
            ok = args[0] in (1, 2) if kind == "frequency" else 0 <= args[0] < self.C and (0 <= args[1] < 3 if kind == "mean" else args[1] in (1, 2))
            if not ok:
                raise L.DeepcamHipError(f"Climatology: product {prod!r} names a class, channel position or row that does not exist")
            out.append([CLIMATOLOGY_PRODUCTS[kind]] + args)
        if not 1 <= len(out) <= 256:
            raise L.DeepcamHipError(f"Climatology: between 1 and 256 products, got {len(out)}")
        return np.asarray(out, np.int32)

    def fields(self, products, t1: float = 0.1, t2: float = 0.1):
        """(fp32 [G, H, W, K], uint8 [G, H, W]) on the device, from dc_climatology_maps on the current stream, not synchronised: the
        products as the channels of a FrameRenderer(batch=G, ldc=K) input, and the contour mask (1 where the class-1 frequency >= t1, else
        2 where the class-2 frequency >= t2).  Both are buffers of the object, overwritten by the next call with the same products."""
        key = tuple(tuple(p) for p in products)
        if key not in self._products:
            table = self.product_table(products)
            self._products[key] = (torch.from_numpy(table).to(self.device),
                                   torch.empty((self.G, self.H, self.W, len(table)), dtype=torch.float32, device=self.device),
                                   torch.empty((self.G, self.H, self.W), dtype=torch.uint8, device=self.device))
        table, out, contour = self._products[key]
        L.call("dc_climatology_maps", self.G, self.H, self.W, self.C, L.dptr(self._frames), L.dptr(self._count), L.dptr(self._sum),
               L.dptr(self._n), L.dptr(self._bits), len(table), L.dptr(table), float(np.float32(t1)), float(np.float32(t2)), L.dptr(out),
               L.dptr(contour), L.stream_ptr())
        return out, contour

    def maps(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["frames"], s["count"], s["sum"], s["n"], self.bits, self.H, self.W)

    @staticmethod
    def occurrence(frames, count, height: int, width: int) -> dict:
        """decode()'s frequency, zonal_frequency and area_frequency, which need the counts alone"""
        frames = np.asarray(frames, np.int64).reshape(-1)
        count = np.asarray(count, np.int64).reshape(len(frames), 2, height, width)
        fr = frames.astype(np.float64)
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)  # noqa: E731
        rows = count.sum(axis=3)                                                # int64 [G, 2, H]
        wy = event_weight_tables(height, width)[0].astype(np.int64)
        return {"frequency": div(count.astype(np.float64), fr[:, None, None, None]),
                "zonal_frequency": div(rows.astype(np.float64), fr[:, None, None] * width),
                "area_frequency": div((rows * wy).sum(axis=2).astype(np.float64), fr[:, None] * (float(width) * float(wy.sum())))}

    @staticmethod
    def decode(frames, count, sum, n, bits, height: int, width: int) -> dict:
        """float64 maps from the raw integers, NaN where a divisor is zero: frequency [G, 2, H, W] = count / frames; mean [G, 3, H, W, C]
        = sum * 2^-bits / n; share [G, 2, H, W, C] = sum of class k / sum of all; zonal_frequency [G, 2, H], the mean frequency of a row;
        area_frequency [G, 2], the cos(lat)-weighted mean frequency with event_weight_tables' integer wy: sum_r wy[r] * (count summed
        along the row) / (frames * W * sum_r wy[r]) -- the share of the globe's area and time spent inside the class."""
        out = Climatology.occurrence(frames, count, height, width)
        G, C = len(out["area_frequency"]), len(np.asarray(bits).reshape(-1))
        total = np.asarray(sum, np.int64).reshape(G, 3, height, width, C).astype(np.float64)
        n = np.asarray(n, np.int64).reshape(G, 3, height, width, C)
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)  # noqa: E731
        scaled = np.ldexp(total, -np.asarray(bits, np.int32).reshape(-1)) if C else total
        out.update(mean=div(scaled, n.astype(np.float64)), share=div(total[:, 1:], total[:, :1]))
        return out


# ---------------------------------------------------------------------------------------------- storm-centred composites
COMPOSITE_COUNTS = ("composited", "no_center", "below_min_pixels", "other_class", "uncatalogued")
COMPOSITE_MAX_EVENTS = 1 << 21
COMPOSITE_MAX_RADIUS = 40
COMPOSITE_KEYS = ("events", "sum", "n", "inside", "rsum", "rn")


def composite_bits(minval, maxval) -> np.ndarray:
    """int32 [C]: the binary scale of dc_composite_accumulate's sums per channel, from the dataset's recorded range.  With m =
    max(|minval|, |maxval|): 27 - frexp(m)[1], and 0 where m is zero or not finite.  A value inside the range is summed as
    rint(v * 2^bits) with |q| < 2^27; values up to twice outside the range still fit below the kernel's limit of 2^28."""
    lo = np.atleast_1d(np.asarray(minval, np.float64))
    hi = np.atleast_1d(np.asarray(maxval, np.float64))
    m = np.maximum(np.abs(lo), np.abs(hi))
    ok = np.isfinite(m) & (m > 0)
    return np.where(ok, 27 - np.frexp(np.where(ok, m, 1.0))[1], 0).astype(np.int32)


def composite_radius_table(height: int, width: int, radius: int, bin_km: float, bins: int) -> np.ndarray:
    """uint8 [H][S][R + 1], S = 2 R + 1: entry (r0, d + R, a) is the distance bin floor(distance / bin_km) between the pixel centres
    (r0, c0) and (r0 + d, c0 + a) -- the great-circle distance by the haversine formula in float64, latitudes from linspace(-90, 90, H),
    a longitude step of 360 / W (the periodic grid of event_shape_tables), Earth radius EARTH_RADIUS_KM.  255 where the bin is >= bins or
    row r0 + d is off the grid.  bins <= 255."""
    height, width, radius, bins = int(height), int(width), int(radius), int(bins)
    if height < 1 or width < 1 or not 1 <= radius <= COMPOSITE_MAX_RADIUS or not 0 <= bins <= 255 or not float(bin_km) > 0:
        raise L.DeepcamHipError(f"composite_radius_table: height and width must be positive, radius in [1, {COMPOSITE_MAX_RADIUS}], bins in "
                                f"[0, 255] and bin_km positive, got {height}, {width}, {radius}, {bins}, {bin_km}")
    lat = np.deg2rad(np.linspace(-90.0, 90.0, height))
    d = np.arange(-radius, radius + 1)
    rows = np.arange(height)[:, None] + d[None, :]                              # [H, S]
    on = (rows >= 0) & (rows < height)
    lat1 = lat[:, None, None]
    lat2 = lat[np.clip(rows, 0, height - 1)][:, :, None]
    dlon = np.deg2rad(360.0 / width * np.arange(radius + 1))[None, None, :]
    hav = np.sin((lat2 - lat1) / 2.0) ** 2 + np.cos(lat1) * np.cos(lat2) * np.sin(dlon / 2.0) ** 2
    dist = 2.0 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.clip(hav, 0.0, 1.0)))
    k = np.floor(dist / float(bin_km))
    return np.where(on[:, :, None] & (k < bins), np.minimum(k, 255), 255).astype(np.uint8)


class StormComposite:
    """The fields in storm coordinates, accumulated on the device (dc_composite_centers, dc_composite_accumulate, csrc/composite.hip):
    around the centre of every selected event of an EventFields catalogue -- the pixel of the minimum (or maximum) of center_channel, a
    cyclone's pressure minimum -- a window of S x S grid pixels, S = 2 radius + 1, summed cell by cell over the events of a group, with
    the events' mean footprint and the sums per great-circle distance bin (bins of bin_km; bins = 0: no radial profile).
    channels: indices into the ldc channels of a pixel (None: all of them); bits: the binary scale per SELECTED channel (composite_bits;
    None: EventFields' bits less 12, which is the same number for a channel with a recorded range); classes: the event classes that are
    composited; groups: the frame groups G (climatology_group); intensity_edges: ascending finite values that cut the centre value into
    len + 1 bins (an event on an edge goes to the bin above), so that GT = G * (len + 1) composites are kept, index group * (len + 1) + bin;
    flip_south: southern events are reflected about their centre row, so that "up" is poleward and the rotation is northern; negate:
    selected-channel POSITIONS whose sign the reflection reverses (the meridional wind components).
    The object owns events (int64 [GT]), sum (int64 [GT, S, S, C]), n (int32 [GT, S, S, C]), inside (int32 [GT, S, S]), rsum / rn (int64
    [GT, NB, C]) and counts (int64 [5], COMPOSITE_COUNTS); everything is an integer sum, so the state does not depend on how a sequence was
    cut into batches or ordered.  A call must follow the catalogue's and the EventFields call of the same batch on the same stream; it
    launches and does not synchronise; state() and composites() read back."""

    def __init__(self, fields: "EventFields", center_channel: int, center_stat: str = "min", radius: int = 32, channels=None, bits=None,
                 classes=(1,), min_pixels: int = 0, groups: int = 1, intensity_edges=(), flip_south: bool = True, negate=(),
                 bin_km: float = 25.0, bins: int = 40):
        cat = fields.catalog
        if center_stat not in ("min", "max"):
            raise L.DeepcamHipError(f"StormComposite: center_stat must be 'min' or 'max', got {center_stat!r}")
        if not 0 <= int(center_channel) < fields.C:
            raise L.DeepcamHipError(f"StormComposite: center_channel must lie in [0, {fields.C}), got {center_channel}")
        radius = int(radius)
        if not 1 <= radius <= COMPOSITE_MAX_RADIUS or 2 * radius + 1 > cat.W:
            raise L.DeepcamHipError(f"StormComposite: radius must lie in [1, {COMPOSITE_MAX_RADIUS}] and 2 * radius + 1 may not exceed the "
                                    f"width {cat.W}, got {radius}")
        channels = list(range(fields.ldc)) if channels is None else [int(c) for c in channels]
        C_ = len(channels)
        if not 1 <= C_ <= 32 or min(channels) < 0 or max(channels) >= fields.ldc:
            raise L.DeepcamHipError(f"StormComposite: between 1 and 32 channels out of [0, {fields.ldc}), got {channels}")
        if bits is None:
            if max(channels) >= fields.C:
                raise L.DeepcamHipError("StormComposite: bits are needed for channels the EventFields object does not cover")
            bits = [fields.bits[c] - 12 for c in channels]
        bits = [int(v) for v in np.asarray(bits).reshape(-1)]
        if len(bits) != C_:
            raise L.DeepcamHipError(f"StormComposite: {len(bits)} scale bits for {C_} channels")
        classes = sorted({int(k) for k in classes})
        if not classes or any(k not in (1, 2) for k in classes):
            raise L.DeepcamHipError(f"StormComposite: classes must be a non-empty subset of (1, 2), got {classes}")
        if int(min_pixels) < 0:
            raise L.DeepcamHipError(f"StormComposite: min_pixels must not be negative, got {min_pixels}")
        edges = np.asarray(list(intensity_edges), np.float32).reshape(-1)
        if len(edges) > 255 or not np.all(np.isfinite(edges)) or np.any(np.diff(edges) < 0):
            raise L.DeepcamHipError(f"StormComposite: intensity_edges must be at most 255 finite ascending values, got {list(intensity_edges)}")
        if not 1 <= int(groups) or int(groups) * (len(edges) + 1) > 65536:
            raise L.DeepcamHipError(f"StormComposite: groups must be positive and groups * (edges + 1) at most 65536, got {groups}")
        negate = sorted({int(c) for c in negate})
        if any(not 0 <= c < C_ for c in negate):
            raise L.DeepcamHipError(f"StormComposite: negate holds positions of selected channels, [0, {C_}), got {negate}")
        if not 0 <= int(bins) <= 255 or not float(bin_km) > 0:
            raise L.DeepcamHipError(f"StormComposite: bins must lie in [0, 255] and bin_km be positive, got {bins}, {bin_km}")
        self.fields, self.catalog = fields, cat
        self.center_channel, self.center_stat, self.R, self.S = int(center_channel), center_stat, radius, 2 * radius + 1
        self.channels, self.bits, self.C, self.classes, self.min_pixels = channels, bits, C_, classes, int(min_pixels)
        self.G, self.edges, self.NE = int(groups), edges, len(edges)
        self.GT = self.G * (self.NE + 1)
        self.flip_south, self.negate, self.bin_km, self.NB = bool(flip_south), negate, float(bin_km), int(bins)
        self.class_mask = sum(1 << k for k in classes)
        self.negate_mask = sum(1 << c for c in negate)
        dev = self.device = cat._labels.device
        S, GT = self.S, self.GT
        self._events = torch.zeros((GT,), dtype=torch.int64, device=dev)
        self._sum = torch.zeros((GT, S, S, C_), dtype=torch.int64, device=dev)
        self._n = torch.zeros((GT, S, S, C_), dtype=torch.int32, device=dev)
        self._inside = torch.zeros((GT, S, S), dtype=torch.int32, device=dev)
        self._rsum = torch.zeros((GT, self.NB, C_), dtype=torch.int64, device=dev)
        self._rn = torch.zeros((GT, self.NB, C_), dtype=torch.int64, device=dev)
        self._counts = torch.zeros((len(COMPOSITE_COUNTS),), dtype=torch.int64, device=dev)
        self._centers = torch.full((cat.B, cat.cap), -1, dtype=torch.int32, device=dev)
        self._egroup = torch.full((cat.B, cat.cap), -1, dtype=torch.int32, device=dev)
        self._bits = torch.tensor(bits, dtype=torch.int32, device=dev)
        self._edges = torch.from_numpy(edges).to(dev) if self.NE else None
        # the identity over all ldc channels travels as a null table: the library then knows it on the host and may take its 16-byte loads
        self._chan = None if channels == list(range(fields.ldc)) else torch.tensor(channels, dtype=torch.int32, device=dev)
        self.radius_table = composite_radius_table(cat.H, cat.W, radius, bin_km, bins) if self.NB else None
        self._rbin = torch.from_numpy(self.radius_table).to(dev) if self.NB else None
        self._tables = {}                            # group tuple -> device int32 [B]
        self._last_valid = 0

    def _group_table(self, groups, nv: int) -> tuple:
        B = self.catalog.B
        if groups is None or isinstance(groups, (int, np.integer)):
            table = [0 if groups is None else int(groups)] * B
        else:
            table = [int(g) for g in groups]
            if len(table) != B:
                raise L.DeepcamHipError(f"StormComposite: {len(table)} groups for a batch of {B}")
        table = tuple(g if j < nv and g >= 0 else -1 for j, g in enumerate(table))
        if any(g >= self.G for g in table):
            raise L.DeepcamHipError(f"StormComposite: group indices must be below {self.G}, got {list(table)}")
        return table

    def __call__(self, raw_fields: torch.Tensor, groups=None, n_valid: Optional[int] = None) -> "StormComposite":
        """raw_fields: contiguous device fp32 [B, H, W, ldc], physical units (InputPipeline.raw) -- the tensor the EventFields call of this
        batch was given; groups: None (every frame to group 0), an int, or B ints, a negative one skipping its frame; n_valid defaults to
        the EventFields call's, frames from it on are skipped."""
        cat, ef = self.catalog, self.fields
        want = (cat.B, cat.H, cat.W, ef.ldc)
        if raw_fields.dtype != torch.float32 or tuple(raw_fields.shape) != want or not raw_fields.is_cuda or not raw_fields.is_contiguous() \
                or raw_fields.device != self.device:
            raise L.DeepcamHipError(f"StormComposite: fields must be a contiguous fp32 tensor {list(want)} on {self.device}, got "
                                    f"{raw_fields.dtype} {tuple(raw_fields.shape)} on {raw_fields.device}")
        nv = ef._last_valid if n_valid is None else int(n_valid)
        if not 0 <= nv <= cat.B:
            raise L.DeepcamHipError(f"StormComposite: n_valid must lie in [0, {cat.B}], got {n_valid}")
        table = self._group_table(groups, nv)
        self._last_valid = nv
        if nv == 0 or all(g < 0 for g in table):
            return self
        dev_table = self._tables.get(table)
        if dev_table is None:
            dev_table = self._tables[table] = torch.tensor(table, dtype=torch.int32, device=self.device)
        st = L.stream_ptr()
        L.call("dc_composite_centers", cat.B, nv, cat.H, cat.W, cat.cap, L.dptr(cat._table), L.dptr(cat._ncomp), L.dptr(ef._ftable), ef.C,
               self.center_channel, 0 if self.center_stat == "min" else 1, self.class_mask, self.min_pixels, L.dptr(dev_table), self.G,
               L.dptr(self._edges), self.NE, L.dptr(self._centers), L.dptr(self._egroup), L.dptr(self._counts), st)
        L.call("dc_composite_accumulate", cat.B, nv, cat.H, cat.W, cat.cap, self.R, self.GT, L.dptr(self._centers), L.dptr(self._egroup),
               L.dptr(cat._table), L.dptr(cat._labels), L.dptr(raw_fields), self.C, ef.ldc, L.dptr(self._chan), L.dptr(self._bits),
               _c_int(self.negate_mask), int(self.flip_south), L.dptr(self._rbin), self.NB, L.dptr(self._events), L.dptr(self._sum),
               L.dptr(self._n), L.dptr(self._inside), L.dptr(self._rsum) if self.NB else None, L.dptr(self._rn) if self.NB else None, st)
        return self

    @property
    def centers(self) -> torch.Tensor:
        """int32 [n_valid, cap] of the last call (a view): the centre pixel r0 * W + c0 of every composited event, -1 elsewhere"""
        return self._centers[:self._last_valid]

    @property
    def event_groups(self) -> torch.Tensor:
        """int32 [n_valid, cap] of the last call (a view): group * (edges + 1) + intensity bin of every composited event, -1 elsewhere"""
        return self._egroup[:self._last_valid]

    def reset(self) -> None:
        """zeroes the accumulators and the counts (in stream order)"""
        for t in (self._events, self._sum, self._n, self._inside, self._rsum, self._rn, self._counts):
            t.zero_()

    def state(self) -> dict:
        """the raw integers on the host (COMPOSITE_KEYS) and counts (a dict over COMPOSITE_COUNTS).  Raises when a group has reached
        COMPOSITE_MAX_EVENTS events: from there on the sums are no longer known to fit their words."""
        out = {"events": self._events.cpu().numpy(), "sum": self._sum.cpu().numpy(), "n": self._n.cpu().numpy(),
               "inside": self._inside.cpu().numpy(), "rsum": self._rsum.cpu().numpy(), "rn": self._rn.cpu().numpy()}
        if int(out["events"].max()) >= COMPOSITE_MAX_EVENTS:
            raise L.DeepcamHipError(f"StormComposite: a group has reached {COMPOSITE_MAX_EVENTS} events, the bound of the integer sums")
        out["counts"] = dict(zip(COMPOSITE_COUNTS, (int(v) for v in self._counts.cpu().tolist())))
        return out

    def composites(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(*(s[k] for k in COMPOSITE_KEYS), self.bits, self.bin_km)

    @staticmethod
    def decode(events, sum, n, inside, rsum, rn, bits, bin_km: float = 25.0) -> dict:
        """float64 from the raw integers: mean [GT, S, S, C] = sum * 2^-bits / n, NaN where n == 0; footprint [GT, S, S] = inside /
        events, NaN where events == 0; radial_mean [GT, NB, C] = rsum * 2^-bits / rn, NaN where rn == 0; radius_km [NB], the bin
        centres (k + 1/2) * bin_km; radius_of_max_km [GT, C], the centre of the bin with the largest finite radial mean -- the smallest
        such bin on ties --, NaN where no bin has a value."""
        bits = np.asarray(bits, np.int32).reshape(-1)
        events = np.asarray(events, np.int64).reshape(-1)
        total, n = np.asarray(sum, np.int64).astype(np.float64), np.asarray(n, np.int64).astype(np.float64)
        rsum, rn = np.asarray(rsum, np.int64).astype(np.float64), np.asarray(rn, np.int64).astype(np.float64)
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)  # noqa: E731
        radial = div(np.ldexp(rsum, -bits), rn)
        radius = (np.arange(radial.shape[1]) + 0.5) * float(bin_km)
        rmax = np.full((radial.shape[0], radial.shape[2]), np.nan)
        if radial.shape[1]:
            some = np.isfinite(radial).any(axis=1)
            first = np.argmax(np.where(np.isfinite(radial), radial, -np.inf), axis=1)    # argmax takes the first among equals
            rmax = np.where(some, radius[first], np.nan)
        return {"mean": div(np.ldexp(total, -bits), n), "footprint": div(np.asarray(inside, np.int64).astype(np.float64), events[:, None, None].astype(np.float64)),
                "radial_mean": radial, "radius_km": radius, "radius_of_max_km": rmax}


# ---------------------------------------------------------------------------------------------- verification skills: what they share
def _ratio(a, b):
    """a / b as a Python float, None where b == 0"""
    return None if b == 0 else a / b


def _two_words(words):
    """Python ints, nested as the leading axes, from int64 words [..., 2] = (lo, hi): (hi << 64) | lo with lo taken as unsigned"""
    words = np.asarray(words, np.int64)
    out = np.empty(words.size // 2, dtype=object)
    out[:] = [(int(hi) << 64) | (int(lo) & 0xFFFFFFFFFFFFFFFF) for lo, hi in words.reshape(-1, 2).tolist()]
    return out.reshape(words.shape[:-1]).tolist()


def _n_valid(who: str, n_valid: Optional[int], batch: int) -> int:
    nv = batch if n_valid is None else int(n_valid)
    if not 0 <= nv <= batch:
        raise L.DeepcamHipError(f"{who}: n_valid must lie in [0, {batch}], got {n_valid}")
    return nv


class _MaskSkill:
    """What the skills that score a predicted class mask against a labelled one share (FractionsSkill, DistanceSkill, DisplacementSkill,
    ScaleSkill): a batch of [B, H, W] frames with fewer than 2^31 pixels each, a band of rows row_range = (row0, row1), the check of
    the two masks (contiguous device uint8, int32 or int64, each side with its own element size), per-frame buffers of the last call
    and running totals since reset().  A subclass names the attributes of its per-frame buffers in `_frame` (the order of FRAME_KEYS, the
    datasets they are stored under) and of its totals in `_totals`, and makes the call in _score()."""

    FRAME_KEYS: tuple = ()
    _frame: tuple = ()
    _totals: tuple = ()

    def _geometry(self, batch: int, height: int, width: int, max_batch: int) -> None:
        if batch < 1 or batch > max_batch or height < 1 or width < 1 or height * width >= 1 << 31:
            raise L.DeepcamHipError(f"{type(self).__name__}: batch must lie in [1, {max_batch}], height and width be positive and "
                                    "height * width below 2^31")
        self.B, self.H, self.W, self._nv = batch, height, width, 0

    def _band(self, row_range) -> tuple:
        row0, row1 = (0, self.H) if row_range is None else (int(row_range[0]), int(row_range[1]))
        if not 0 <= row0 < row1 <= self.H:
            raise L.DeepcamHipError(f"{type(self).__name__}: row_range must satisfy 0 <= row0 < row1 <= {self.H}, got {row_range}")
        self.row_range = (row0, row1)
        return row0, row1

    def _check(self, t, name: str) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype not in _BYTES or tuple(t.shape) != (self.B, self.H, self.W) or not t.is_cuda \
                or t.device != self.device or not t.is_contiguous():
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise L.DeepcamHipError(f"{type(self).__name__}: {name} must be a contiguous uint8, int32 or int64 tensor "
                                    f"[{self.B}, {self.H}, {self.W}] on {self.device}, got {got}")

    def __call__(self, pred: torch.Tensor, truth: torch.Tensor, n_valid: Optional[int] = None):
        """pred, truth: contiguous device uint8, int32 or int64 [B, H, W], each side with its own element size; the frames from n_valid on
        are neither read nor written (FractionsSkill: not read, and their rows are zero).  Returns the object."""
        self._check(pred, "pred")
        self._check(truth, "truth")
        nv = _n_valid(type(self).__name__, n_valid, self.B)
        self._score(nv, L.dptr(pred), _BYTES[pred.dtype], L.dptr(truth), _BYTES[truth.dtype])
        self._nv = nv
        return self

    def frame_rows(self) -> tuple:
        """the per-frame buffers of the last call, in the order of FRAME_KEYS, each cut to [n_valid, ...]: views of the object's device
        buffers, not synchronised"""
        return tuple(getattr(self, name)[:self._nv] for name in self._frame)

    def reset(self) -> None:
        """zeroes the running totals (in stream order)"""
        for name in self._totals:
            getattr(self, name).zero_()


# ---------------------------------------------------------------------------------------------- neighbourhood verification
FSS_WINDOWS = (1, 3, 9, 17, 33, 65, 129)
FSS_MAX_WINDOW = 255
FSS_MAX_WINDOWS = 16
FSS_MAX_BATCH = 4095


def _fss(a: int, b: int, c: int):
    """1 - A / (B + C) from Python ints by true division (correctly rounded), None where B + C == 0"""
    return None if b + c == 0 else 1.0 - a / (b + c)


def fss_from_rows(rows):
    """The scores of integer rows [..., 3] = (A, B, C) as nested lists of the leading shape: 1 - A / (B + C) as a Python float from the
    exact integers, None where B + C == 0 (the class is absent from both masks)."""
    rows = np.asarray(rows)
    if rows.shape[-1:] != (3,):
        raise L.DeepcamHipError(f"fss_from_rows: the last axis must hold (A, B, C), got shape {rows.shape}")
    flat = rows.reshape(-1, 3).tolist()
    out = np.empty(len(flat), dtype=object)
    out[:] = [_fss(int(a), int(b), int(c)) for a, b, c in flat]
    return out.reshape(rows.shape[:-1]).tolist()


class FractionsSkill(_MaskSkill):
    """Neighbourhood verification on the device (dc_fss_score, csrc/fss.hip): per frame, class (1, 2) and window of n x n GRID PIXELS the
    integers (A, B, C) = (sum (F - O)^2, sum F^2, sum O^2), F and O the predicted and labelled pixel counts of the class inside the window
    around every pixel of the rows row_range = (row0, row1) -- columns periodic with wrap, rows beyond the poles empty -- and their running
    totals over all frames since reset() as two-word integers.  FSS = 1 - A / (B + C) (Roberts & Lean 2008) is decoded on the host from
    the exact integers; the pooled score of a run is 1 - sum A / (sum B + sum C).  windows: distinct odd sides in [1, 255], at most 16,
    with wrap also <= width.  No latitude weighting and no kilometres: row_range is the tool for a tropics-only score.
    Memory: a workspace of batch * S * height * width * 4 bytes, one packed word per pixel and window (dc_fss_workspace) -- 8 x 768 x 1152
    at the 7 default windows: 198.2 MB --, beside batch * (2 * S * 3 + 4) * 8 bytes of rows and a few hundred bytes of totals.
    A call launches on the current stream and does not synchronise; state() and result() read back."""

    FRAME_KEYS = ("fss", "fss_pixels")                # frame_rows(): int64 [n_valid, 2, S, 3], int64 [n_valid, 2, 2]
    _frame, _totals = ("_rows", "_pixels"), ("_total", "_total_pixels", "_frames")

    def __init__(self, batch: int, height: int, width: int, windows: Sequence[int] = FSS_WINDOWS, wrap: bool = True, row_range=None,
                 device=None):
        self._geometry(batch, height, width, FSS_MAX_BATCH)
        windows = [int(n) for n in windows]
        if not 1 <= len(windows) <= FSS_MAX_WINDOWS:
            raise L.DeepcamHipError(f"FractionsSkill: between 1 and {FSS_MAX_WINDOWS} windows, got {len(windows)}")
        for n in windows:
            if n % 2 == 0 or not 1 <= n <= FSS_MAX_WINDOW:
                raise L.DeepcamHipError(f"FractionsSkill: a window is an odd number of pixels in [1, {FSS_MAX_WINDOW}], got {n}")
            if wrap and n > width:
                raise L.DeepcamHipError(f"FractionsSkill: a periodic window must not be wider than the frame ({width}), got {n}")
        if len(set(windows)) != len(windows):
            raise L.DeepcamHipError(f"FractionsSkill: the windows must be distinct, got {windows}")
        self._band(row_range)
        self.S, self.windows, self.wrap = len(windows), windows, bool(wrap)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._radius = torch.tensor([(n - 1) // 2 for n in windows], dtype=torch.int32, device=dev)
        dev = self.device = self._radius.device
        self._rows = torch.zeros((batch, 2, self.S, 3), dtype=torch.int64, device=dev)
        self._pixels = torch.zeros((batch, 2, 2), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, self.S, 3, 2), dtype=torch.int64, device=dev)          # (lo, hi)
        self._total_pixels = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        size = L.load().dc_fss_workspace(batch, height, width, self.S)
        if size == 0:
            raise L.DeepcamHipError("FractionsSkill: dc_fss_workspace refused the shape")
        self._ws = torch.empty(size // 4, dtype=torch.int32, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_fss_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.S, L.dptr(self._radius),
               int(self.wrap), self.row_range[0], self.row_range[1], L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._total),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.dptr(self._ws), L.stream_ptr())

    @staticmethod
    def combine(total_words) -> list:
        """[2][S][3] Python ints from the int64 words [2, S, 3, 2] = (lo, hi): (hi << 64) | lo with lo taken as unsigned"""
        words = np.asarray(total_words, np.int64)
        if words.ndim != 4 or words.shape[0] != 2 or words.shape[2:] != (3, 2):
            raise L.DeepcamHipError(f"FractionsSkill: the totals are int64 [2, S, 3, 2], got shape {words.shape}")
        return _two_words(words)

    def state(self) -> dict:
        """on the host: total [2][S][3] as Python ints, pixels [2][2] ((pred, truth) per class) and frames as ints"""
        return {"total": self.combine(self._total.cpu().numpy()), "pixels": [[int(v) for v in row] for row in self._total_pixels.cpu().tolist()],
                "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["total"], s["pixels"], s["frames"], self.windows, self.row_range[1] - self.row_range[0], self.W)

    @staticmethod
    def decode(total, pixels, frames, windows, rows: int, width: int) -> dict:
        """Per class ("class_1", "class_2"), from the exact integers: fss, a list over the windows of the pooled 1 - sum A / (sum B + sum
        C), None where sum B + sum C == 0; base_rate = labelled pixels / (frames * rows * width), the share of the scored band the class
        covers; useful = 0.5 + base_rate / 2, the score above which a forecast is taken as skilful at that scale; skilful_window, the
        smallest window whose fss >= useful, else None.  Without a frame base_rate, useful and skilful_window are None."""
        windows = [int(n) for n in windows]
        cells = int(frames) * int(rows) * int(width)
        out = {}
        for k in range(2):
            scores = [_fss(*(int(v) for v in total[k][s])) for s in range(len(windows))]
            base = int(pixels[k][1]) / cells if cells > 0 else None
            useful = None if base is None else 0.5 + base / 2
            good = [n for n, f in zip(windows, scores) if useful is not None and f is not None and f >= useful]
            out[f"class_{k + 1}"] = {"fss": scores, "base_rate": base, "useful": useful, "skilful_window": min(good) if good else None}
        return out


# ---------------------------------------------------------------------------------------------- distance-map verification
DISTANCE_RADIUS = 64
DISTANCE_MAX_RADIUS = 127
DISTANCE_MAX_BATCH = 4095
DISTANCE_Q = 256                                  # dq = rint(sqrt(d^2) * DISTANCE_Q)


def distance_table(radius: int) -> np.ndarray:
    """int32 [R^2 + 2], the table dc_distance_score reads: entry v = ring(v) | dq(v) << 8 with ring(v) the smallest integer j with j^2 >= v
    (math.isqrt) and dq(v) = int(rint(sqrt(float64(v)) * 256)); the last entry (v = R^2 + 1, beyond the cap) has ring R + 1 and dq 0."""
    R = int(radius)
    if not 1 <= R <= DISTANCE_MAX_RADIUS:
        raise L.DeepcamHipError(f"distance_table: the radius must lie in [1, {DISTANCE_MAX_RADIUS}], got {radius}")
    table = np.zeros(R * R + 2, np.int32)
    for v in range(R * R + 1):
        ring = math.isqrt(v)
        ring += ring * ring < v
        table[v] = ring | int(np.rint(np.sqrt(np.float64(v)) * DISTANCE_Q)) << 8
    table[R * R + 1] = R + 1
    return table


class DistanceSkill(_MaskSkill):
    """Distance-map verification on the device (dc_distance_score, csrc/distance.hip): per frame, side (prediction, labels) and class (1, 2)
    the map of the squared Euclidean distance, in GRID PIXELS, to the nearest pixel of that side and class -- columns periodic with wrap,
    rows never --, capped: R^2 + 1 ("beyond") where nothing lies within `radius` = R.  From the maps, per class and direction (0 "miss": from
    every labelled pixel to the nearest predicted one; 1 "false alarm": the reverse) the sources per ring of distance, the sums of the
    distance (in 1/256 pixel) and of its square, and Baddeley's sum of squared map differences, as integers and as running totals over all
    frames since reset(); decode() turns them into the mean error distances, the (partial) Hausdorff distance, Baddeley's Delta and the hit
    rate and success ratio with a displacement of up to r pixels forgiven.  1 <= radius <= 127, with wrap also 2 radius + 1 <= width.
    No latitude weighting and no kilometres: row_range is the tool for a tropics-only score; it selects the sources and the Baddeley
    pixels, targets anywhere in the frame still count.  The single-word totals last 2^26 frames of 768 x 1152.
    Memory: a workspace of batch * height * width * 4 bytes (dc_distance_workspace; 28.3 MB at 8 x 768 x 1152), with keep_maps another
    batch * 4 * height * width * 2 bytes of uint16 maps (56.6 MB), beside batch * (4 * (R + 4) + 2) * 8 bytes of rows and the totals.
    A call launches on the current stream and does not synchronise; state() and result() read back."""

    FRAME_KEYS = ("distance", "distance_baddeley")    # frame_rows(): int64 [n_valid, 2, 2, R + 4], int64 [n_valid, 2]
    _frame, _totals = ("_rows", "_baddeley"), ("_total", "_total_baddeley", "_frames")

    def __init__(self, batch: int, height: int, width: int, radius: int = DISTANCE_RADIUS, wrap: bool = True, row_range=None,
                 keep_maps: bool = False, device=None):
        self._geometry(batch, height, width, DISTANCE_MAX_BATCH)
        R = int(radius)
        if not 1 <= R <= DISTANCE_MAX_RADIUS:
            raise L.DeepcamHipError(f"DistanceSkill: the radius must lie in [1, {DISTANCE_MAX_RADIUS}], got {radius}")
        if wrap and 2 * R + 1 > width:
            raise L.DeepcamHipError(f"DistanceSkill: a periodic window of 2 * {R} + 1 columns must not be wider than the frame ({width})")
        self._band(row_range)
        self.R, self.wrap, self.keep_maps = R, bool(wrap), bool(keep_maps)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._table = torch.from_numpy(distance_table(R)).to(dev)
        dev = self.device = self._table.device
        self._rows = torch.zeros((batch, 2, 2, R + 4), dtype=torch.int64, device=dev)
        self._baddeley = torch.zeros((batch, 2), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, 2, R + 4), dtype=torch.int64, device=dev)
        self._total_baddeley = torch.zeros((2, 2), dtype=torch.int64, device=dev)            # (lo, hi)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._maps = torch.zeros((batch, 2, 2, height, width), dtype=torch.uint16, device=dev) if keep_maps else None
        size = L.load().dc_distance_workspace(batch, height, width, R)
        if size == 0:
            raise L.DeepcamHipError("DistanceSkill: dc_distance_workspace refused the shape")
        self._ws = torch.empty(size // 4, dtype=torch.int32, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_distance_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.R, L.dptr(self._table),
               int(self.wrap), self.row_range[0], self.row_range[1], L.dptr(self._rows), L.dptr(self._baddeley), L.dptr(self._total),
               L.dptr(self._total_baddeley), L.dptr(self._frames), L.dptr(self._maps) if self._maps is not None else None,
               L.dptr(self._ws), L.stream_ptr())

    def maps(self) -> torch.Tensor:
        """uint16 [n_valid, 2 sides, 2 classes, H, W] of the last call (keep_maps): a view of the object's device buffer, not synchronised"""
        if self._maps is None:
            raise L.DeepcamHipError("DistanceSkill: maps() needs keep_maps=True")
        return self._maps[:self._nv]

    def state(self) -> dict:
        """on the host, as Python ints: total [2][2][R + 4], baddeley [2] (the two words combined) and frames"""
        return {"total": [[[int(v) for v in d] for d in cls] for cls in self._total.cpu().tolist()],
                "baddeley": _two_words(self._total_baddeley.cpu().numpy()), "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["total"], s["baddeley"], s["frames"], self.R, self.H, self.W, self.row_range)

    @staticmethod
    def decode(total, total_baddeley, frames, radius: int, height: int, width: int, row_range=None) -> dict:
        """Per class ("class_1", "class_2"), in float64 from the exact integers; distances in grid pixels; None wherever a denominator is 0:
        pixels {"labelled", "predicted"}; pod_within[r] and success_within[r] for r = 0 .. R, the share of labelled (predicted) pixels with a
        predicted (labelled) pixel within r -- r = 0 is the per-pixel POD and 1 - FAR; med_miss, med_false_alarm, the mean error distances
        sum dq / 256 / n over the sources within the cap, and rms_miss, rms_false_alarm; beyond_miss, beyond_false_alarm, the shares of
        sources beyond the cap; hausdorff, the largest non-empty ring over both directions, None when any source is beyond the cap or there
        is no source; hausdorff_q90, the larger over the directions that have sources of the smallest ring that, with the rings below it,
        holds 90 % of the direction's sources, None when that ring is beyond the cap; baddeley, sqrt(total / (frames * pixels of the band))
        / 256, Baddeley's Delta with p = 2 and cut-off R."""
        R = int(radius)
        row0, row1 = (0, int(height)) if row_range is None else (int(row_range[0]), int(row_range[1]))
        cells = int(frames) * (row1 - row0) * int(width)
        out = {}
        for k in range(2):
            entry, rings, quantiles = {}, [], []
            for d, (name, curve) in enumerate((("miss", "pod_within"), ("false_alarm", "success_within"))):
                cell = [int(v) for v in total[k][d]]
                if len(cell) != R + 4:
                    raise L.DeepcamHipError(f"DistanceSkill.decode: a row holds R + 4 = {R + 4} cells, got {len(cell)}")
                n, beyond = sum(cell[:R + 2]), cell[R + 1]
                within, cum = n - beyond, np.cumsum(np.asarray(cell[:R + 1], np.int64)).tolist()
                entry[curve] = [_ratio(c, n) for c in cum]
                entry[f"med_{name}"] = _ratio(cell[R + 2] / DISTANCE_Q, within)
                entry[f"rms_{name}"] = None if within == 0 else math.sqrt(cell[R + 3] / within)
                entry[f"beyond_{name}"] = _ratio(beyond, n)
                rings.append(cell[:R + 2])
                if n:
                    quantiles.append(next(j for j, c in enumerate(cum + [n]) if 10 * c >= 9 * n))
            entry["pixels"] = {"labelled": sum(rings[0]), "predicted": sum(rings[1])}
            occupied = [j for j in range(R + 2) if rings[0][j] or rings[1][j]]
            entry["hausdorff"] = occupied[-1] if occupied and occupied[-1] <= R else None
            entry["hausdorff_q90"] = max(quantiles) if quantiles and max(quantiles) <= R else None
            entry["baddeley"] = None if cells <= 0 else math.sqrt(int(total_baddeley[k]) / cells) / DISTANCE_Q
            out[f"class_{k + 1}"] = entry
        return out


def distance_from_rows(rows, baddeley, radius: int, height: int, width: int, row_range=None) -> list:
    """DistanceSkill.decode of single frames: rows int64 [n, 2, 2, R + 4] and baddeley int64 [n, 2] (what frame_rows() returns, on the
    host) give a list of n dictionaries, each the decode of that frame alone."""
    rows, baddeley = np.asarray(rows), np.asarray(baddeley)
    if rows.ndim != 4 or rows.shape[1:] != (2, 2, int(radius) + 4) or baddeley.shape != (rows.shape[0], 2):
        raise L.DeepcamHipError(f"distance_from_rows: rows [n, 2, 2, R + 4] and baddeley [n, 2], got shapes {rows.shape} and {baddeley.shape}")
    return [DistanceSkill.decode(r, b, 1, radius, height, width, row_range) for r, b in zip(rows.tolist(), baddeley.tolist())]


# ---------------------------------------------------------------------------------------------- displacement verification
DISPLACEMENT_RADIUS = 16
DISPLACEMENT_MAX_RADIUS = 63
DISPLACEMENT_MAX_BATCH = 4095


def displacement_best(table, radius: int):
    """(dy, dx, hits, kept[dy]) of one class's table [2 R + 1][2 R + 2] in Python ints: the most hits, ties to the smaller dy^2 + dx^2, then
    the smaller dy, then the smaller dx -- the order of dc_displacement_score's key; a table without hits gives (0, 0)."""
    R = int(radius)
    hits, _, dy, dx = max((int(table[dy + R][dx + R]), -(dy * dy + dx * dx), -dy, -dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    return -dy, -dx, hits, int(table[R - dy][2 * R + 1])


class DisplacementSkill(_MaskSkill):
    """Displacement verification on the device (dc_displacement_score, csrc/displacement.hip): per frame and class (1, 2) the overlap of the
    labelled mask with the predicted mask moved by every (dy, dx), |dy|, |dx| <= radius -- columns periodic, always; rows never: pixels
    moved over a pole are lost --, the predicted pixels each dy keeps inside the band, and the best shift, the one with the most hits: the
    rigid-shift part of the CRA method.  Integers, per frame and as running totals over all frames since reset(); decode() turns a table
    into the shift, the scores without and with it and the CRA decomposition of the error into displacement, volume and pattern.
    1 <= radius <= 63 and 2 radius + 1 <= width.  row_range is the band of LABEL rows scored (a tropics-only score); predicted pixels from
    anywhere in the frame may move into it.  No latitude weighting, no kilometres, no sub-pixel shifts.
    Memory: a workspace of bit planes (dc_displacement_workspace; 3.8 MB at 8 x 768 x 1152, R = 16) beside batch * 2 * (2 R + 1) * (2 R + 2)
    * 8 bytes of rows and the totals.  A call launches on the current stream and does not synchronise; state() and result() read back."""

    # frame_rows(): rows int64 [n_valid, 2, 2 R + 1, 2 R + 2], pixels int64 [n_valid, 2, 2], best int64 [n_valid, 2, 4]
    FRAME_KEYS = ("displacement", "displacement_pixels", "displacement_best")
    _frame, _totals = ("_rows", "_pixels", "_best"), ("_total", "_total_pixels", "_frames")

    def __init__(self, batch: int, height: int, width: int, radius: int = DISPLACEMENT_RADIUS, row_range=None, device=None):
        self._geometry(batch, height, width, DISPLACEMENT_MAX_BATCH)
        R = int(radius)
        if not 1 <= R <= DISPLACEMENT_MAX_RADIUS:
            raise L.DeepcamHipError(f"DisplacementSkill: the radius must lie in [1, {DISPLACEMENT_MAX_RADIUS}], got {radius}")
        if 2 * R + 1 > width:
            raise L.DeepcamHipError(f"DisplacementSkill: the window of 2 * {R} + 1 columns must not be wider than the frame ({width})")
        self._band(row_range)
        self.R = R
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        S = 2 * R + 1
        self._rows = torch.zeros((batch, 2, S, S + 1), dtype=torch.int64, device=dev)
        dev = self.device = self._rows.device
        self._pixels = torch.zeros((batch, 2, 2), dtype=torch.int64, device=dev)
        self._best = torch.zeros((batch, 2, 4), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, S, S + 1), dtype=torch.int64, device=dev)
        self._total_pixels = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        size = L.load().dc_displacement_workspace(batch, height, width, R)
        if size == 0:
            raise L.DeepcamHipError("DisplacementSkill: dc_displacement_workspace refused the shape")
        self._ws = torch.empty((size + 7) // 8, dtype=torch.int64, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_displacement_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.R, self.row_range[0],
               self.row_range[1], L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._best), L.dptr(self._total),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.dptr(self._ws), L.stream_ptr())

    def state(self) -> dict:
        """on the host, as Python ints: total [2][2 R + 1][2 R + 2], pixels [2][2] and frames"""
        return {"total": [[[int(v) for v in row] for row in cls] for cls in self._total.cpu().tolist()],
                "pixels": [[int(v) for v in cls] for cls in self._total_pixels.cpu().tolist()], "frames": int(self._frames.cpu()[0])}

    def result(self, surface: bool = False) -> dict:
        """decode() of the object's state: one common shift for all frames since reset(), the systematic displacement"""
        s = self.state()
        return self.decode(s["total"], s["pixels"], s["frames"], self.R, self.H, self.W, self.row_range, surface)

    @staticmethod
    def decode(total, pixels, frames, radius: int, height: int, width: int, row_range=None, surface: bool = False) -> dict:
        """Per class ("class_1", "class_2"), in float64 from the exact integers; None wherever a denominator is 0:
        pixels {"predicted" (whole frame), "labelled" (in the band)}; best, the raw integers [dy, dx, hits, kept[dy]] of the best shift;
        shift {"rows": dy, "cols": dx, "pixels": sqrt(dy^2 + dx^2), "lat_deg", "lon_deg"} by the steps of linspace(-90, 90, H) and
        linspace(-180, 180, W) -- row 0 is -90 degrees, a positive dy is poleward-north; at_edge, |dy| = R or |dx| = R: the window was too
        small; hits_unshifted, hits_shifted; csi, pod, far, each {"unshifted", "shifted"}, from hits, kept[dy] and labelled (CSI = hits /
        (kept[dy] + labelled - hits)); and the CRA decomposition for binary fields with N = frames * band rows * W: mse_total = (kept[0] +
        labelled - 2 hits[0][0]) / N, mse_shifted likewise at the best shift, mse_displacement = mse_total - mse_shifted, mse_volume =
        ((kept[dy] - labelled) / N)^2, mse_pattern = mse_shifted - mse_volume, and share {"displacement", "volume", "pattern"} of
        mse_total.  surface=True adds csi_surface, float64 [2 R + 1][2 R + 1], the CSI of every shift (NaN where undefined)."""
        R = int(radius)
        S = 2 * R + 1
        row0, row1 = (0, int(height)) if row_range is None else (int(row_range[0]), int(row_range[1]))
        N = int(frames) * (row1 - row0) * int(width)
        out = {}
        for k in range(2):
            table = [[int(v) for v in row] for row in total[k]]
            if len(table) != S or any(len(row) != S + 1 for row in table):
                raise L.DeepcamHipError(f"DisplacementSkill.decode: a table holds [2 R + 1][2 R + 2] = [{S}][{S + 1}] cells")
            predicted, labelled = int(pixels[k][0]), int(pixels[k][1])
            dy, dx, hits, kept = displacement_best(table, R)
            hits0, kept0 = table[R][R], table[R][S]
            entry = {"pixels": {"predicted": predicted, "labelled": labelled}, "best": [dy, dx, hits, kept],
                     "shift": {"rows": dy, "cols": dx, "pixels": math.sqrt(dy * dy + dx * dx),
                               "lat_deg": None if height < 2 else dy * 180.0 / (height - 1),
                               "lon_deg": None if width < 2 else dx * 360.0 / (width - 1)},
                     "at_edge": abs(dy) == R or abs(dx) == R, "hits_unshifted": hits0, "hits_shifted": hits}
            both = ((hits0, kept0), (hits, kept))
            entry["csi"] = {n: _ratio(h, kp + labelled - h) for n, (h, kp) in zip(("unshifted", "shifted"), both)}
            entry["pod"] = {n: _ratio(h, labelled) for n, (h, kp) in zip(("unshifted", "shifted"), both)}
            entry["far"] = {n: _ratio(kp - h, kp) for n, (h, kp) in zip(("unshifted", "shifted"), both)}
            if N > 0:
                mse_total, mse_shifted = (kept0 + labelled - 2 * hits0) / N, (kept + labelled - 2 * hits) / N
                volume = ((kept - labelled) / N) ** 2
                parts = {"displacement": mse_total - mse_shifted, "volume": volume, "pattern": mse_shifted - volume}
                entry.update(mse_total=mse_total, mse_shifted=mse_shifted, mse_displacement=parts["displacement"], mse_volume=volume,
                             mse_pattern=parts["pattern"], share={n: _ratio(v, mse_total) for n, v in parts.items()})
            else:
                entry.update(mse_total=None, mse_shifted=None, mse_displacement=None, mse_volume=None, mse_pattern=None,
                             share={"displacement": None, "volume": None, "pattern": None})
            if surface:
                t = np.asarray(table, np.float64)
                union = t[:, S:] + labelled - t[:, :S]
                entry["csi_surface"] = np.where(union > 0, t[:, :S] / np.where(union > 0, union, 1.0), np.nan)
            out[f"class_{k + 1}"] = entry
        return out


def displacement_from_rows(rows, pixels, radius: int, height: int, width: int, row_range=None, surface: bool = False) -> list:
    """DisplacementSkill.decode of single frames: rows int64 [n, 2, 2 R + 1, 2 R + 2] and pixels int64 [n, 2, 2] (what frame_rows()
    returns, on the host) give a list of n dictionaries, each the decode of that frame alone."""
    rows, pixels = np.asarray(rows), np.asarray(pixels)
    S = 2 * int(radius) + 1
    if rows.ndim != 4 or rows.shape[1:] != (2, S, S + 1) or pixels.shape != (rows.shape[0], 2, 2):
        raise L.DeepcamHipError(f"displacement_from_rows: rows [n, 2, 2 R + 1, 2 R + 2] and pixels [n, 2, 2], got shapes {rows.shape} and "
                                f"{pixels.shape}")
    return [DisplacementSkill.decode(r, p, 1, radius, height, width, row_range, surface) for r, p in zip(rows.tolist(), pixels.tolist())]


# ---------------------------------------------------------------------------------------------- scale-separation verification
SCALE_MAX_LEVELS = 8
SCALE_MAX_ORIGINS = 8
SCALE_MAX_BATCH = 4095
SCALE_LISTS = ("mse", "mse_share", "skill", "energy_pred", "energy_truth", "energy_rel_diff")


def scale_levels(rows_in_band: int, width: int) -> int:
    """the largest L <= 8 whose tile T = 2^L divides both the rows of the band and the width (7, T = 128, for 768 x 1152); 0 where one
    of them is odd, which ScaleSkill refuses"""
    L_ = 0
    while L_ < SCALE_MAX_LEVELS and int(rows_in_band) % (2 << L_) == 0 and int(width) % (2 << L_) == 0:
        L_ += 1
    return L_


def _scale_components(q) -> list:
    """the Haar components E_0 .. E_L as Fractions from the block sums Q_0 .. Q_L of one term: E_j = (4 Q_j - Q_{j+1}) / 4^(j+1) for
    j < L, E_L = Q_L / 4^L"""
    n = len(q) - 1
    return [Fraction(4 * q[j] - q[j + 1], 4 ** (j + 1)) for j in range(n)] + [Fraction(q[n], 4 ** n)]


def _float(v):
    return None if v is None else float(v)


class ScaleSkill(_MaskSkill):
    """Scale-separation verification on the device (dc_scale_score, csrc/scale.hip): the integers behind the intensity-scale skill score
    (Casati, Ross & Stephenson 2004; energies: Casati 2010).  Per frame, class (1, 2), column origin and level j = 0 .. levels the sums
    (A, B, C) = (sum (S_F - S_O)^2, sum S_F^2, sum S_O^2) over the disjoint blocks of side 2^j GRID PIXELS that tile the rows row_range
    from (row0, origin) on, S_F and S_O the predicted and labelled pixels of the class in a block -- columns periodic, always; rows never
    --, and their running totals over all frames since reset() as two-word integers.  decode() turns them, in exact arithmetic, into the
    squared error and the energies of the 2-D Haar components of scale 1, 2, ..., 2^levels pixels.  The tile T = 2^levels must divide
    both the rows of the band and the width; levels=None takes scale_levels(), the largest that does.  origins: 1 to 8 column offsets in
    [0, T) of the dyadic grid, scored in one pass: their spread shows how much a result owes to where the grid falls.  No latitude
    weighting, no kilometres, tiles instead of the whole domain, and "intensity" is the class, not a threshold ladder.
    Memory: batch * 2 * O * (levels + 1) * 3 * 8 bytes of rows and a workspace of 16 bytes per 64 x 64 tile and origin
    (dc_scale_workspace); no per-pixel buffer.  A call launches on the current stream and does not synchronise; state() and result() read
    back."""

    FRAME_KEYS = ("scale", "scale_pixels")            # frame_rows(): int64 [n_valid, 2, O, levels + 1, 3], int64 [n_valid, 2, 2]
    _frame, _totals = ("_rows", "_pixels"), ("_total", "_total_pixels", "_frames")

    def __init__(self, batch: int, height: int, width: int, levels: Optional[int] = None, origins: Sequence[int] = (0,), row_range=None,
                 device=None):
        self._geometry(batch, height, width, SCALE_MAX_BATCH)
        row0, row1 = self._band(row_range)
        lv = scale_levels(row1 - row0, width) if levels is None else int(levels)
        if levels is None and lv < 1:
            raise L.DeepcamHipError(f"ScaleSkill: levels=None needs an even number of rows in the band and an even width, got {row1 - row0} "
                                    f"and {width}")
        if not 1 <= lv <= SCALE_MAX_LEVELS:
            raise L.DeepcamHipError(f"ScaleSkill: levels must lie in [1, {SCALE_MAX_LEVELS}], got {levels}")
        T = 1 << lv
        if (row1 - row0) % T or width % T:
            raise L.DeepcamHipError(f"ScaleSkill: the tile 2^levels = {T} must divide the rows of the band ({row1 - row0}) and the width "
                                    f"({width})")
        try:
            origins = [int(c) for c in origins]
        except TypeError:
            raise L.DeepcamHipError(f"ScaleSkill: origins is a sequence of column offsets, got {origins!r}") from None
        if not 1 <= len(origins) <= SCALE_MAX_ORIGINS:
            raise L.DeepcamHipError(f"ScaleSkill: between 1 and {SCALE_MAX_ORIGINS} origins, got {len(origins)}")
        for c in origins:
            if not 0 <= c < T:
                raise L.DeepcamHipError(f"ScaleSkill: an origin is a column offset in [0, {T}), got {c}")
        self.L, self.O, self.origins = lv, len(origins), origins
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._origins = torch.tensor(origins, dtype=torch.int32, device=dev)
        dev = self.device = self._origins.device
        self._rows = torch.zeros((batch, 2, self.O, lv + 1, 3), dtype=torch.int64, device=dev)
        self._pixels = torch.zeros((batch, 2, 2), dtype=torch.int64, device=dev)
        self._total = torch.zeros((2, self.O, lv + 1, 3, 2), dtype=torch.int64, device=dev)          # (lo, hi)
        self._total_pixels = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        size = L.load().dc_scale_workspace(batch, height, width, lv, self.O)
        if size == 0:
            raise L.DeepcamHipError("ScaleSkill: dc_scale_workspace refused the shape")
        self._ws = torch.empty(size // 4, dtype=torch.int32, device=dev)

    def _score(self, nv: int, pred: int, pred_bytes: int, truth: int, truth_bytes: int) -> None:
        L.call("dc_scale_score", self.B, nv, self.H, self.W, pred, pred_bytes, truth, truth_bytes, self.L, self.O, L.dptr(self._origins),
               self.row_range[0], self.row_range[1], L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._total),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.dptr(self._ws), L.stream_ptr())

    @staticmethod
    def combine(total_words) -> list:
        """[2][O][levels + 1][3] Python ints from the int64 words [2, O, levels + 1, 3, 2] = (lo, hi): (hi << 64) | lo, lo unsigned"""
        words = np.asarray(total_words, np.int64)
        if words.ndim != 5 or words.shape[0] != 2 or words.shape[3:] != (3, 2):
            raise L.DeepcamHipError(f"ScaleSkill: the totals are int64 [2, O, levels + 1, 3, 2], got shape {words.shape}")
        return _two_words(words)

    def state(self) -> dict:
        """on the host: total [2][O][levels + 1][3] as Python ints, pixels [2][2] ((pred, truth) per class) and frames as ints"""
        return {"total": self.combine(self._total.cpu().numpy()), "pixels": [[int(v) for v in row] for row in self._total_pixels.cpu().tolist()],
                "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["total"], s["pixels"], s["frames"], self.L, self.row_range[1] - self.row_range[0], self.W, self.origins)

    @staticmethod
    def decode(total, pixels, frames, levels: int, rows_in_band: int, width: int, origins=None) -> dict:
        """Per class ("class_1", "class_2"), computed in exact arithmetic (Python ints and fractions.Fraction) from total [2][O][levels +
        1][3] and pixels [2][2]; every reported number is one float() of the exact value, None wherever a denominator is 0.  With N =
        frames * rows_in_band * width and Q_j one of A, B, C at level j, the Haar component of scale 2^j carries E_j = (4 Q_j - Q_{j+1}) /
        4^(j+1) for j < levels (the detail between block means of side 2^j and 2^(j+1)) and E_L = Q_L / 4^L (the father component: the
        TILE means, not the domain mean).  Per origin, lists over j = 0 .. levels: mse = E_j(A) / N, which sum to the per-pixel error
        rate; mse_share = E_j(A) / A_0; skill = 1 - mse (levels + 1) / mse_random with mse_random = p (1 - o) + o (1 - p), p and o the
        pooled predicted and labelled rates -- Casati's equipartition of the random error over the levels + 1 components;
        energy_pred = E_j(B) / N, energy_truth = E_j(C) / N, energy_rel_diff = (pred - truth) / (pred + truth).
        The entry holds pixels {"predicted", "labelled"}, base_rate = labelled / N, bias = predicted / labelled, mse_random, scales =
        [1, 2, ..., 2^levels], the six lists as the exact mean over the origins (energy_rel_diff from the mean energies), by_origin (a
        list of {"origin", the six lists}), origin_spread (max - min of mse[j] over the origins) and skilful_scale: the smallest 2^j from
        which the mean skill of every component up to levels - 1 is positive, else None."""
        n = int(levels)
        N = int(frames) * int(rows_in_band) * int(width)
        out = {}
        for k in range(2):
            table = [[[int(v) for v in level] for level in origin] for origin in total[k]]
            if not table or any(len(origin) != n + 1 or any(len(level) != 3 for level in origin) for origin in table):
                raise L.DeepcamHipError(f"ScaleSkill.decode: a class holds [O][levels + 1][3] = [O][{n + 1}][3] cells")
            O = len(table)
            names = list(range(O)) if origins is None else [int(c) for c in origins]
            if len(names) != O:
                raise L.DeepcamHipError(f"ScaleSkill.decode: {len(names)} origins for a table of {O}")
            predicted, labelled = int(pixels[k][0]), int(pixels[k][1])
            rnd = None if N == 0 else Fraction(predicted * (N - labelled) + labelled * (N - predicted), N * N)
            per = []                                  # per origin: the exact lists
            for origin in table:
                ea, eb, ec = (_scale_components([level[i] for level in origin]) for i in range(3))
                a0 = origin[0][0]
                per.append({"mse": [None if N == 0 else e / N for e in ea], "mse_share": [None if a0 == 0 else e / a0 for e in ea],
                            "energy_pred": [None if N == 0 else e / N for e in eb], "energy_truth": [None if N == 0 else e / N for e in ec]})
            mean = {name: [None if per[0][name][j] is None else sum(p[name][j] for p in per) / O for j in range(n + 1)] for name in per[0]}
            for entry in per + [mean]:
                entry["skill"] = [None if not rnd else 1 - m * (n + 1) / rnd for m in entry["mse"]]
                entry["energy_rel_diff"] = [None if p is None or p + t == 0 else (p - t) / (p + t)
                                            for p, t in zip(entry["energy_pred"], entry["energy_truth"])]
            good = None
            for j in range(n - 1, -1, -1):            # the component n is the father: tile means, not a scale's detail
                if mean["skill"][j] is None or mean["skill"][j] <= 0:
                    break
                good = 1 << j
            entry = {"pixels": {"predicted": predicted, "labelled": labelled}, "base_rate": None if N == 0 else labelled / N,
                     "bias": None if labelled == 0 else predicted / labelled, "mse_random": _float(rnd), "scales": [1 << j for j in range(n + 1)]}
            entry.update({name: [_float(v) for v in mean[name]] for name in SCALE_LISTS})
            entry["by_origin"] = [dict({"origin": c}, **{name: [_float(v) for v in p[name]] for name in SCALE_LISTS}) for c, p in zip(names, per)]
            entry["origin_spread"] = [None if N == 0 else float(max(p["mse"][j] for p in per) - min(p["mse"][j] for p in per))
                                      for j in range(n + 1)]
            entry["skilful_scale"] = good
            out[f"class_{k + 1}"] = entry
        return out


def scale_from_rows(rows, pixels, levels: int, rows_in_band: int, width: int, origins=None) -> list:
    """ScaleSkill.decode of single frames: rows int64 [n, 2, O, levels + 1, 3] and pixels int64 [n, 2, 2] (what frame_rows() returns, on
    the host) give a list of n dictionaries, each the decode of that frame alone."""
    rows, pixels = np.asarray(rows), np.asarray(pixels)
    if rows.ndim != 5 or rows.shape[1] != 2 or rows.shape[3:] != (int(levels) + 1, 3) or pixels.shape != (rows.shape[0], 2, 2):
        raise L.DeepcamHipError(f"scale_from_rows: rows [n, 2, O, levels + 1, 3] and pixels [n, 2, 2], got shapes {rows.shape} and "
                                f"{pixels.shape}")
    return [ScaleSkill.decode(r, p, 1, levels, rows_in_band, width, origins) for r, p in zip(rows.tolist(), pixels.tolist())]


# ---------------------------------------------------------------------------------------------- probabilistic verification
PROB_BINS = 20
PROB_MAX_BINS = 256
PROB_MAX_BATCH = 4095
PROB_MAX_PIXELS = 1 << 30
PROB_ONE = 65536                                  # q = rint(p * PROB_ONE)


def brier_from_rows(rows, pixels):
    """The Brier scores of single frames from ProbabilitySkill.frame_rows(): rows [..., 3] = sum (q_c - o_c * 65536)^2 per class, pixels
    [..., 3] = (scored, bad label, logit not finite); rows / (scored * 2^32) as nested lists of Python floats of rows' shape, None where no
    pixel was scored."""
    rows, pixels = np.asarray(rows), np.asarray(pixels)
    if rows.shape[-1:] != (3,) or pixels.shape != rows.shape:
        raise L.DeepcamHipError(f"brier_from_rows: rows and pixels must both be [..., 3], got {rows.shape} and {pixels.shape}")
    n = pixels.reshape(-1, 3)[:, 0].tolist()
    out = np.empty((len(n), 3), dtype=object)
    for i, (row, scored) in enumerate(zip(rows.reshape(-1, 3).tolist(), n)):
        out[i] = [_ratio(int(v), int(scored) << 32) for v in row]
    return out.reshape(rows.shape).tolist()


class ProbabilitySkill:
    """Probabilistic verification on the device (dc_prob_score, csrc/probskill.hip): from the classifier's fp32 logits and the labels, per
    class c the joint histogram of (probability bin, label == c) with the sum of the probabilities per cell, and the sum of the squared
    errors -- one streaming pass --, as integers: q_c = rint(softmax_c * 65536), bin = min(bins - 1, (q_c * bins) >> 16).  Running totals
    over all frames since reset(); the squared errors as two-word integers.  decode() turns the integers into the reliability diagram,
    the Brier score with Murphy's (1973) decomposition, ECE / MCE, and POD / POFD / CSI / bias per threshold k / bins with the ROC area
    (Mason 1982).  Pixels whose label is outside [0, 3) or whose logits are not finite are counted and left out.  No latitude weighting.
    Memory: (2 * 3 * 2 * bins * 2 + 2 * batch * 3 + 10) * 8 bytes.  A call launches on the current stream and does not synchronise; state()
    and result() read back."""

    FRAME_KEYS = ("prob", "prob_pixels")              # frame_rows(); the driver stores `brier` (brier_from_rows) in place of the raw rows

    def __init__(self, batch: int, height: int, width: int, bins: int = PROB_BINS, device=None):
        if batch < 1 or batch > PROB_MAX_BATCH or height < 1 or width < 1 or height * width > PROB_MAX_PIXELS:
            raise L.DeepcamHipError(f"ProbabilitySkill: batch must lie in [1, {PROB_MAX_BATCH}], height and width be positive and height * width at most 2^30")
        bins = int(bins)
        if not 1 <= bins <= PROB_MAX_BINS:
            raise L.DeepcamHipError(f"ProbabilitySkill: bins must lie in [1, {PROB_MAX_BINS}], got {bins}")
        self.B, self.H, self.W, self.K = batch, height, width, bins
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._hist = torch.zeros((3, 2, bins, 2), dtype=torch.int64, device=dev)
        dev = self.device = self._hist.device
        self._rows = torch.zeros((batch, 3), dtype=torch.int64, device=dev)
        self._pixels = torch.zeros((batch, 3), dtype=torch.int64, device=dev)
        self._total_hist = torch.zeros((3, 2, bins, 2), dtype=torch.int64, device=dev)
        self._total_sq = torch.zeros((3, 2), dtype=torch.int64, device=dev)                  # (lo, hi)
        self._total_pixels = torch.zeros((3,), dtype=torch.int64, device=dev)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._nv = 0

    def _check(self, t, name: str, dtypes, shape) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != shape or not t.is_cuda or t.device != self.device \
                or not t.is_contiguous():
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise L.DeepcamHipError(f"ProbabilitySkill: {name} must be a contiguous {' / '.join(str(d) for d in dtypes)} tensor "
                                    f"{list(shape)} on {self.device}, got {got}")

    def __call__(self, logits: torch.Tensor, labels: torch.Tensor, n_valid: Optional[int] = None) -> "ProbabilitySkill":
        """logits: contiguous device fp32 [B, 3, H, W]; labels: contiguous device uint8, int32 or int64 [B, H, W]; the frames from n_valid
        on are not read."""
        self._check(logits, "logits", (torch.float32,), (self.B, 3, self.H, self.W))
        self._check(labels, "labels", tuple(_BYTES), (self.B, self.H, self.W))
        nv = _n_valid("ProbabilitySkill", n_valid, self.B)
        L.call("dc_prob_score", self.B, nv, self.H, self.W, L.dptr(logits), L.dptr(labels), _BYTES[labels.dtype], self.K,
               L.dptr(self._hist), L.dptr(self._rows), L.dptr(self._pixels), L.dptr(self._total_hist), L.dptr(self._total_sq),
               L.dptr(self._total_pixels), L.dptr(self._frames), L.stream_ptr())
        self._nv = nv
        return self

    def frame_rows(self):
        """(int64 [n_valid, 3], int64 [n_valid, 3]) of the last call: per frame and class the sum of squared errors, and the pixel
        counters (scored, bad label, not finite); views of the object's device buffers, not synchronised"""
        return self._rows[:self._nv], self._pixels[:self._nv]

    def batch_hist(self) -> torch.Tensor:
        """int64 [3, 2, bins, 2] of the last call: class, outcome, bin, (n, sum q); the object's device buffer, not synchronised"""
        return self._hist

    def reset(self) -> None:
        """zeroes the running totals (in stream order)"""
        for t in (self._total_hist, self._total_sq, self._total_pixels, self._frames):
            t.zero_()

    @staticmethod
    def combine(words) -> list:
        """[3] Python ints from the int64 words [3, 2] = (lo, hi): (hi << 64) | lo with lo taken as unsigned (FractionsSkill's convention)"""
        words = np.asarray(words, np.int64)
        if words.shape != (3, 2):
            raise L.DeepcamHipError(f"ProbabilitySkill: the squared-error totals are int64 [3, 2], got shape {words.shape}")
        return _two_words(words)

    def state(self) -> dict:
        """on the host: hist int64 [3, 2, bins, 2], sq [3] as Python ints, pixels [3] and frames as ints"""
        return {"hist": self._total_hist.cpu().numpy(), "sq": self.combine(self._total_sq.cpu().numpy()),
                "pixels": [int(v) for v in self._total_pixels.cpu().tolist()], "frames": int(self._frames.cpu()[0])}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["hist"], s["sq"], s["pixels"], self.K)

    @staticmethod
    def decode(hist, sq, pixels, bins: int) -> dict:
        """Per class ("class_0", "class_1", "class_2"), in float64 from the exact integers hist [3][2][bins][2] = (n, sum q) per (outcome,
        bin), sq [3] and pixels [3]:
          n, base_rate (o = labelled share), mean_probability, brier = sq / (n * 2^32), brier_skill = 1 - brier / (o (1 - o)),
          reliability = sum_k n_k (f_k - o_k)^2 / n, resolution = sum_k n_k (o_k - o)^2 / n, uncertainty = o (1 - o) (Murphy 1973; f_k =
          sum q / n_k / 65536 the bin's mean forecast, o_k its observed frequency), ece = sum_k n_k |f_k - o_k| / n, mce = max_k |f_k - o_k|,
          curve {mean_probability, observed_frequency, n} per bin, sharpness n_k / n per bin,
          pod, pofd, csi, bias at the thresholds k / bins, k = 0 .. bins (the forecast is "bin >= k": k = 0 says yes everywhere, k = bins
          nowhere), auc by trapezoids over the (pofd, pod) points, best_csi and best_csi_threshold (the smallest among equals).
        A value is None where its denominator is zero.  "pixels" holds the three counters."""
        K = int(bins)
        h = np.asarray(hist, np.int64)
        if h.shape != (3, 2, K, 2):
            raise L.DeepcamHipError(f"ProbabilitySkill.decode: hist must be [3, 2, {K}, 2], got {h.shape}")
        h = h.tolist()
        out = {"bins": K, "pixels": {"scored": int(pixels[0]), "bad_label": int(pixels[1]), "not_finite": int(pixels[2])}}
        for c in range(3):
            n0, n1 = [cell[0] for cell in h[c][0]], [cell[0] for cell in h[c][1]]
            qk = [a[1] + b[1] for a, b in zip(h[c][0], h[c][1])]
            nk = [a + b for a, b in zip(n0, n1)]
            N0, N1 = sum(n0), sum(n1)
            N = N0 + N1
            base = _ratio(N1, N)
            unc = None if base is None else base * (1.0 - base)
            brier = _ratio(int(sq[c]), N << 32)
            fk = [_ratio(q, n * PROB_ONE) for q, n in zip(qk, nk)]
            ok = [_ratio(o, n) for o, n in zip(n1, nk)]
            full = [k for k in range(K) if nk[k]]
            rel = res = ece = mce = None
            if N:
                rel = sum(nk[k] * (fk[k] - ok[k]) ** 2 for k in full) / N
                res = sum(nk[k] * (ok[k] - base) ** 2 for k in full) / N
                ece = sum(nk[k] * abs(fk[k] - ok[k]) for k in full) / N
                mce = max(abs(fk[k] - ok[k]) for k in full)
            hits, alarms = [0] * (K + 1), [0] * (K + 1)     # labelled / unlabelled pixels in the bins >= k
            for k in range(K - 1, -1, -1):
                hits[k], alarms[k] = hits[k + 1] + n1[k], alarms[k + 1] + n0[k]
            pod = [_ratio(a, N1) for a in hits]
            pofd = [_ratio(b, N0) for b in alarms]
            csi = [_ratio(a, N1 + b) for a, b in zip(hits, alarms)]          # hits / (hits + misses + false alarms)
            bias = [_ratio(a + b, N1) for a, b in zip(hits, alarms)]
            auc = None
            if N0 and N1:
                auc = sum((pofd[k] - pofd[k + 1]) * (pod[k] + pod[k + 1]) / 2 for k in range(K))
            best = None
            for k in range(K + 1):
                if csi[k] is not None and (best is None or csi[k] > csi[best]):
                    best = k
            out[f"class_{c}"] = {
                "n": N, "base_rate": base, "mean_probability": _ratio(sum(qk), N * PROB_ONE), "brier": brier,
                "brier_skill": None if brier is None or not unc else 1.0 - brier / unc, "reliability": rel, "resolution": res,
                "uncertainty": unc, "ece": ece, "mce": mce, "curve": {"mean_probability": fk, "observed_frequency": ok, "n": nk},
                "sharpness": [_ratio(n, N) for n in nk], "pod": pod, "pofd": pofd, "csi": csi, "bias": bias, "auc": auc,
                "best_csi": None if best is None else csi[best], "best_csi_threshold": None if best is None else best / K}
        return out


# ---------------------------------------------------------------------------------------------- decision rule
DECISION_NEVER = PROB_ONE + 1                     # a threshold no q reaches
DECISION_COUNTS = ("class1_candidate_pixels", "class1_seed_pixels", "class1_kept_pixels", "class1_candidate_events", "class1_kept_events",
                   "class2_candidate_pixels", "class2_seed_pixels", "class2_kept_pixels", "class2_candidate_events", "class2_kept_events",
                   "nonfinite_pixels", "conflict_pixels")


def decision_q(p) -> int:
    """The threshold on q = rint(softmax * 65536) for the probability p: ceil(p * 65536) clamped to [0, 65537], so that q >= decision_q(p)
    iff q / 65536 >= p.  p > 1 gives 65537: never."""
    p = float(p)
    if math.isnan(p):
        raise L.DeepcamHipError("decision_q: the probability is NaN")
    if p > 1.0:
        return DECISION_NEVER
    return max(0, int(math.ceil(p * PROB_ONE)))


def decision_q_from_bin(k: int, bins: int) -> int:
    """The threshold on q that reproduces ProbabilitySkill's forecast "class c at threshold k / bins", min(bins - 1, (q * bins) >> 16) >= k:
    ceil(k * 65536 / bins) for k < bins, 65537 (never) for k == bins."""
    k, bins = int(k), int(bins)
    if not 1 <= bins <= PROB_MAX_BINS or not 0 <= k <= bins:
        raise L.DeepcamHipError(f"decision_q_from_bin: bins must lie in [1, {PROB_MAX_BINS}] and k in [0, bins], got k = {k}, bins = {bins}")
    return DECISION_NEVER if k == bins else -((-k * PROB_ONE) // bins)


class DecisionRule:
    """A mask from the classifier's fp32 logits by per-class probability thresholds with hysteresis, on the device (dc_logits_decide,
    dc_mask_components, dc_hysteresis_select; csrc/decide.hip) -- instead of the argmax, which the training's class weights bias on purpose.
    With q_c = rint(softmax_c * 65536), ProbabilitySkill's integer: class c in (1, 2) qualifies at a pixel iff q_c >= low[c]; the candidate
    class is the qualifying one, of two the one with the larger q (class 1 on equal q), else 0; a candidate pixel with q_c >= high[c] is a
    seed; the mask keeps the connected components of the candidates (one class, `connectivity` 4 or 8, periodic columns with `wrap`) that
    hold a seed.  A pixel with a logit that is not finite is background.  high=None, or high == low: plain thresholding, no component pass.
    low and high are pairs (class 1, class 2): a float is a probability (decision_q), an int is q itself, in [0, 65537]; 65537 is never.
    Memory with hysteresis: 4 * B * H * W bytes of planes (candidates, seeds, flags, mask) plus 4 * B * H * W bytes of labels plus the
    workspace of dc_mask_components; without: one plane of B * H * W bytes.  A call launches on the current stream and does not
    synchronise; the mask is whatever consumes a mask takes (EventFilter, EventCatalog, EventMatcher, FractionsSkill, ...)."""

    def __init__(self, batch: int, height: int, width: int, low=(0.5, 0.5), high=None, connectivity: int = 8, wrap: bool = True, device=None):
        if batch < 1 or batch > PROB_MAX_BATCH or height < 1 or width < 1 or height * width > PROB_MAX_PIXELS:
            raise L.DeepcamHipError(f"DecisionRule: batch must lie in [1, {PROB_MAX_BATCH}], height and width be positive and height * width at most 2^30")
        if connectivity not in (4, 8):
            raise L.DeepcamHipError(f"DecisionRule: connectivity must be 4 or 8, got {connectivity}")
        self.low = self._pair(low, "low")
        self.high = self.low if high is None else self._pair(high, "high")
        if any(h < l for l, h in zip(self.low, self.high)):
            raise L.DeepcamHipError(f"DecisionRule: a high threshold must not be below its low threshold, got low = {self.low}, high = {self.high} (q)")
        self.hysteresis = self.high != self.low
        self.B, self.H, self.W, self.connectivity, self.wrap = batch, height, width, connectivity, bool(wrap)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._counts = torch.zeros((batch, len(DECISION_COUNTS)), dtype=torch.int64, device=dev)
        dev = self.device = self._counts.device
        plane = lambda: torch.zeros((batch, height, width), dtype=torch.uint8, device=dev)  # noqa: E731
        self._cand = plane()
        self._seed = self._flags = self._out = self._labels = self._ws = None
        if self.hysteresis:
            self._seed, self._out = plane(), plane()
            self._flags = torch.zeros(max(L.load().dc_decide_workspace(batch, height, width), 256), dtype=torch.uint8, device=dev)
            self._labels = torch.zeros((batch, height, width), dtype=torch.int32, device=dev)
            self._ws = torch.empty(max(L.load().dc_mask_components_workspace(batch, height, width), 256), dtype=torch.uint8, device=dev)
        self._last_valid = 0

    @staticmethod
    def _pair(v, name):
        if not isinstance(v, (tuple, list, np.ndarray)) or len(v) != 2:
            raise L.DeepcamHipError(f"DecisionRule: {name} takes two values (class 1, class 2), got {v!r}")
        out = []
        for x in v:
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
                raise L.DeepcamHipError(f"DecisionRule: {name} takes probabilities (float) or q (int), got {x!r}")
            q = int(x) if isinstance(x, (int, np.integer)) else decision_q(x)
            if not 0 <= q <= DECISION_NEVER:
                raise L.DeepcamHipError(f"DecisionRule: a threshold q must lie in [0, {DECISION_NEVER}], got {name} = {x!r}")
            out.append(q)
        return tuple(out)

    @staticmethod
    def low_from_prob_skill(decoded) -> tuple:
        """(q class 1, q class 2) from best_csi_threshold: decoded is ProbabilitySkill.decode's dict, or a mapping with the `scalars`,
        `scalar_names` and `bins` arrays of a prob_skill.h5.  low[c] = decision_q_from_bin(round(best_csi_threshold_c * bins), bins);
        raises where a class has no threshold (None or NaN)."""
        if "scalars" in decoded:
            names = bytes(np.asarray(decoded["scalar_names"], np.uint8)).decode().split(",")
            col = names.index("best_csi_threshold")
            bins = int(np.asarray(decoded["bins"]).reshape(-1)[0])
            best = [float(np.asarray(decoded["scalars"])[c, col]) for c in (1, 2)]
        else:
            bins = int(decoded["bins"])
            best = [decoded[f"class_{c}"]["best_csi_threshold"] for c in (1, 2)]
        out = []
        for c, t in zip((1, 2), best):
            if t is None or math.isnan(t):
                raise L.DeepcamHipError(f"DecisionRule.from_prob_skill: class {c} has no best_csi_threshold (no pixel scored)")
            out.append(decision_q_from_bin(int(round(t * bins)), bins))
        return tuple(out)

    @classmethod
    def from_prob_skill(cls, decoded, batch: int, height: int, width: int, high=None, connectivity: int = 8, wrap: bool = True,
                        device=None) -> "DecisionRule":
        """The rule whose low thresholds are the best-CSI thresholds of a ProbabilitySkill result (low_from_prob_skill), typically of a
        validation split; as integers q they reproduce the scored forecasts bit for bit."""
        return cls(batch, height, width, low=cls.low_from_prob_skill(decoded), high=high, connectivity=connectivity, wrap=wrap, device=device)

    def thresholds(self) -> dict:
        """q and probability (q / 65536) per class (1, 2)"""
        return {"low_q": list(self.low), "high_q": list(self.high), "low": [q / PROB_ONE for q in self.low],
                "high": [q / PROB_ONE for q in self.high]}

    def __call__(self, logits: torch.Tensor, n_valid: Optional[int] = None) -> torch.Tensor:
        """logits: contiguous device fp32 [B, 3, H, W] (Predictor.logits_buffer).  Returns the uint8 mask [n_valid, H, W], a view of a buffer
        this object owns (mask_buffer is the whole of it; the next call overwrites it).  Samples from n_valid on are neither read nor
        written."""
        shape = (self.B, 3, self.H, self.W)
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or tuple(logits.shape) != shape or not logits.is_cuda \
                or logits.device != self.device or not logits.is_contiguous():
            got = f"{logits.dtype} {tuple(logits.shape)} on {logits.device}" if isinstance(logits, torch.Tensor) else type(logits).__name__
            raise L.DeepcamHipError(f"DecisionRule: logits must be a contiguous torch.float32 tensor {list(shape)} on {self.device}, got {got}")
        nv = self.B if n_valid is None else int(n_valid)
        if not 0 <= nv <= self.B:
            raise L.DeepcamHipError(f"DecisionRule: n_valid must lie in [0, {self.B}], got {n_valid}")
        st = L.stream_ptr()
        L.call("dc_logits_decide", self.B, nv, self.H, self.W, L.dptr(logits), self.low[0], self.low[1], self.high[0], self.high[1],
               L.dptr(self._cand), L.dptr(self._seed) if self.hysteresis else None, L.dptr(self._counts), st)
        self._last_valid = nv
        if nv and self.hysteresis:
            L.call("dc_mask_components", self.B, nv, self.H, self.W, L.dptr(self._cand), self.connectivity, int(self.wrap),
                   L.dptr(self._labels), L.dptr(self._ws), st)
            L.call("dc_hysteresis_select", self.B, nv, self.H, self.W, L.dptr(self._cand), L.dptr(self._seed), L.dptr(self._labels),
                   L.dptr(self._flags), L.dptr(self._out), L.dptr(self._counts), st)
        elif nv:                                  # plain thresholding: every candidate pixel is kept; no events are counted
            c = self._counts[:nv]
            c[:, 2], c[:, 7] = c[:, 0], c[:, 5]
        return self.mask_buffer[:nv]

    @property
    def mask_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the whole buffer the masks are written to, padding samples included (plain thresholding: the candidates')"""
        return self._out if self.hysteresis else self._cand

    @property
    def candidate_buffer(self) -> torch.Tensor:
        """uint8 [B, H, W]: the candidate classes, padding samples included"""
        return self._cand

    def counts(self) -> torch.Tensor:
        """int64 [n_valid, 12] of the last call (a device view, not synchronised): DECISION_COUNTS"""
        return self._counts[:self._last_valid]


# ---------------------------------------------------------------------------------------------- view ensemble
ENSEMBLE_MAX_MEMBERS = 63                         # a 6-bit vote field of the packed state plane
ENSEMBLE_MAX_WEIGHT_SUM = 65535                   # S_c <= sum of weights * 65537 stays below 2^32
ENSEMBLE_ROW = 208                                # 3 x 64 vote cells, then the 4 x 4 (first, pooled) cells
ENSEMBLE_CHANGED = 192


def seam_weights(width: int, roll: int, margin: int) -> np.ndarray:
    """The column weights of a member whose view is rolled by `roll`, uint16 [width] in SOURCE coordinates: min(d + 1, margin), d the
    distance of the pixel's VIEW column to the nearer edge of the view, where the convolutions pad with zeros.  margin = 1 gives all
    ones, the plain mean; a larger margin fades every member out towards its own seam, so that near longitude 0 the rolled views decide."""
    width, roll, margin = int(width), int(roll), int(margin)
    if width < 1 or not 0 <= roll < width or not 1 <= margin <= ENSEMBLE_MAX_WEIGHT_SUM:
        raise L.DeepcamHipError(f"seam_weights: width must be positive, roll in [0, width) and margin in [1, {ENSEMBLE_MAX_WEIGHT_SUM}], "
                                f"got width = {width}, roll = {roll}, margin = {margin}")
    view = (np.arange(width, dtype=np.int64) - roll) % width
    return np.minimum(np.minimum(view, width - 1 - view) + 1, margin).astype(np.uint16)


def view_input(raw: torch.Tensor, channels, shift: torch.Tensor, scale: torch.Tensor, roll: int = 0, flip: bool = False, negate=None,
               out: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """One view of the input on the device (dc_input_view_hwc): out[n, h, w, j] = scale[j] * (sign[j] * raw[n, src(h, w), channels[j]] -
    shift[j]) with src(h, w) = (H - 1 - h if flip else h, (w + roll) mod W) -- the input pipeline's normalisation on the rolled and
    mirrored fields.  raw, channels, shift, scale: data.InputPipeline's .raw (fp32 [B, H, W, Cfile]), .channels (device int32 [C], or None:
    the first C file channels), .shift and .scale (device fp32 [C]).  negate: None, the FILE channels whose sign is reversed (a mirrored
    hemisphere reverses the meridional winds), or a device fp32 [C] of +1 / -1.  out: the NHWC tensor [B, H, W, C] of `dtype` that takes
    the view (made when None; dtype defaults to out's, else fp32).  Launches on the current stream and does not synchronise."""
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.float32 or raw.dim() != 4 or not raw.is_cuda or not raw.is_contiguous():
        raise L.DeepcamHipError("view_input: raw must be a contiguous device fp32 tensor [B, H, W, Cfile]")
    B, H, W, cfile = raw.shape
    C_ = int(shift.numel())
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    if out is None:
        out = torch.empty((B, H, W, C_), dtype=dtype, device=raw.device)
    if tuple(out.shape) != (B, H, W, C_) or out.dtype != dtype or out.device != raw.device or not out.is_contiguous():
        raise L.DeepcamHipError(f"view_input: out must be a contiguous {dtype} tensor {[B, H, W, C_]} on {raw.device}")
    for t, name in ((shift, "shift"), (scale, "scale")):
        if t.dtype != torch.float32 or t.numel() != C_ or t.device != raw.device or not t.is_contiguous():
            raise L.DeepcamHipError(f"view_input: {name} must be a contiguous device fp32 tensor [{C_}]")
    if channels is not None and (channels.dtype != torch.int32 or channels.numel() != C_ or channels.device != raw.device):
        raise L.DeepcamHipError(f"view_input: channels must be None or a device int32 tensor [{C_}]")
    sign = negate
    if negate is not None and not isinstance(negate, torch.Tensor):
        file_channels = list(range(C_)) if channels is None else [int(c) for c in channels.cpu().tolist()]
        wanted = {int(c) for c in negate}
        sign = torch.tensor([-1.0 if c in wanted else 1.0 for c in file_channels], dtype=torch.float32, device=raw.device) if wanted else None
    if sign is not None and (sign.dtype != torch.float32 or sign.numel() != C_ or sign.device != raw.device or not sign.is_contiguous()):
        raise L.DeepcamHipError(f"view_input: negate as a tensor must be a contiguous device fp32 tensor [{C_}] of +1 / -1")
    L.call("dc_input_view_hwc", L.dtype_code(dtype), B, H, W, cfile, C_, L.dptr(channels), L.dptr(sign), L.dptr(raw), L.dptr(shift),
           L.dptr(scale), int(roll), int(bool(flip)), L.dptr(out), C_, L.stream_ptr())
    return out


class ViewEnsemble:
    """Seam-free, test-time-augmented prediction on the device (dc_ensemble_add, dc_ensemble_pool; csrc/ensemble.hip): the classifier's
    fp32 logits of several VIEWS of one batch -- the frame rolled by `roll` columns, an exact symmetry of the periodic grid that only the
    convolutions' zero padding breaks, and mirrored north-south (view_input makes them) -- pooled per pixel of the source frame.  Every
    member adds, per pixel, wt * q_c to three sums S_c (q_c = rint(softmax_c * 65536), ProbabilitySkill's and DecisionRule's integer; wt a
    weight per source column, seam_weights) and one vote for its first-max class; pool() turns the sums into ONE fp32 logits tensor, L_c =
    log(max(S_c, 1) / S_top): its first maximum is the class with the largest S, its softmax is S / sum S to within 0.75 / 65536, and
    predict_from_logits, ProbabilitySkill and DecisionRule take it as they take the classifier's.  A pixel at which a member's logits
    were not finite pools to NaN.  At most 63 members with a sum of their largest weights of at most 65535.  pool() also counts, per frame
    and as running totals since reset(), the pixels with exactly k votes for class c and the (member 0's class, pooled class) matrix.
    Memory: (16 + 12) * batch * height * width bytes.  Nothing here synchronises but a device tensor of weights (its extremes are read)."""

    def __init__(self, batch: int, height: int, width: int, device=None):
        if batch < 1 or batch > PROB_MAX_BATCH or height < 1 or width < 1 or height * width > PROB_MAX_PIXELS:
            raise L.DeepcamHipError(f"ViewEnsemble: batch must lie in [1, {PROB_MAX_BATCH}], height and width be positive and height * width at most 2^30")
        self.B, self.H, self.W = batch, height, width
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._state = torch.zeros((batch, 4, height, width), dtype=torch.int32, device=dev)       # uint32 words
        self.device = self._state.device
        self._logits = torch.zeros((batch, 3, height, width), dtype=torch.float32, device=self.device)
        self._rows = torch.zeros((batch, ENSEMBLE_ROW), dtype=torch.int64, device=self.device)
        self._totals = torch.zeros((ENSEMBLE_ROW,), dtype=torch.int64, device=self.device)
        self._frames = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._weights = {}                            # host arrays already uploaded: bytes -> (device tensor, largest weight)
        self.begin()
        self._pooled_members = self._pooled_valid = 0

    def begin(self) -> "ViewEnsemble":
        """the next add() is member 0 of a new batch"""
        self._members, self._weight_sum, self._nv = 0, 0, None
        return self

    @property
    def members(self) -> int:
        """the members added since begin()"""
        return self._members

    @property
    def state_buffer(self) -> torch.Tensor:
        """int32 [B, 4, H, W] holding the uint32 words of the state: S_0, S_1, S_2 and the packed plane (votes of class 0, 1, 2 in bits
        0-5, 6-11, 12-17, not-finite members in bits 18-23, member 0's class in bits 24-25)"""
        return self._state

    @property
    def logits_buffer(self) -> torch.Tensor:
        """fp32 [B, 3, H, W]: the whole buffer pool() writes, padding samples included"""
        return self._logits

    def _column_weights(self, weights):
        """(device uint16 [W] or None, the largest weight)"""
        if weights is None:
            return None, 1
        if isinstance(weights, torch.Tensor):
            if weights.dtype not in (torch.uint16, torch.int16) or tuple(weights.shape) != (self.W,) or not weights.is_contiguous():
                raise L.DeepcamHipError(f"ViewEnsemble: weights must be a contiguous uint16 tensor [{self.W}]")
            if weights.device == self.device:
                wide = weights.view(torch.int16).to(torch.int32) & 0xFFFF
                lo, hi, dev = int(wide.min()), int(wide.max()), weights
            else:
                return self._column_weights(weights.cpu().view(torch.int16).numpy().view(np.uint16))
        else:
            host = np.ascontiguousarray(weights)
            if host.dtype != np.uint16 or host.shape != (self.W,):
                raise L.DeepcamHipError(f"ViewEnsemble: weights must be uint16 [{self.W}], got {host.dtype} {host.shape}")
            key = host.tobytes()
            if key not in self._weights:
                self._weights[key] = (torch.from_numpy(host.view(np.int16).copy()).to(self.device), int(host.min()), int(host.max()))
            dev, lo, hi = self._weights[key]
        if lo < 1:
            raise L.DeepcamHipError("ViewEnsemble: every weight must be at least 1")
        return dev, hi

    def add(self, logits: torch.Tensor, roll: int = 0, flip: bool = False, weights=None, n_valid: Optional[int] = None) -> "ViewEnsemble":
        """One member: logits, contiguous device fp32 [B, 3, H, W] in the coordinates of the view (roll, flip) they were predicted on;
        weights None (1) or a device or host uint16 [W] per SOURCE column, at least 1.  The first add() after begin() or after
        construction is member 0 and overwrites the state; n_valid must be the same for every member of a batch."""
        shape = (self.B, 3, self.H, self.W)
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or tuple(logits.shape) != shape \
                or logits.device != self.device or not logits.is_contiguous():
            got = f"{logits.dtype} {tuple(logits.shape)} on {logits.device}" if isinstance(logits, torch.Tensor) else type(logits).__name__
            raise L.DeepcamHipError(f"ViewEnsemble: logits must be a contiguous torch.float32 tensor {list(shape)} on {self.device}, got {got}")
        nv = _n_valid("ViewEnsemble", n_valid, self.B)
        if self._nv is not None and nv != self._nv:
            raise L.DeepcamHipError(f"ViewEnsemble: member 0 of this batch had n_valid = {self._nv}, got {nv}")
        roll = int(roll)
        if not 0 <= roll < self.W:
            raise L.DeepcamHipError(f"ViewEnsemble: roll must lie in [0, {self.W}), got {roll}")
        dev_weights, largest = self._column_weights(weights)
        if self._members >= ENSEMBLE_MAX_MEMBERS:
            raise L.DeepcamHipError(f"ViewEnsemble: at most {ENSEMBLE_MAX_MEMBERS} members (a vote is a 6-bit field)")
        if self._weight_sum + largest > ENSEMBLE_MAX_WEIGHT_SUM:
            raise L.DeepcamHipError(f"ViewEnsemble: the members' largest weights may sum to at most {ENSEMBLE_MAX_WEIGHT_SUM} (S < 2^32), "
                                    f"got {self._weight_sum} + {largest}")
        L.call("dc_ensemble_add", self.B, nv, self.H, self.W, L.dptr(logits), roll, int(bool(flip)), L.dptr(dev_weights), self._members,
               L.dptr(self._state), L.stream_ptr())
        self._members, self._weight_sum, self._nv = self._members + 1, self._weight_sum + largest, nv
        return self

    def pool(self, n_valid: Optional[int] = None) -> torch.Tensor:
        """The pooled fp32 logits [B, 3, H, W] of the members added since begin(): the whole buffer (logits_buffer; samples from n_valid
        on are not written), overwritten by the next pool().  Adds the frames' counters to the running totals."""
        if self._members < 1:
            raise L.DeepcamHipError("ViewEnsemble: pool() needs at least one member")
        nv = self._nv if n_valid is None else _n_valid("ViewEnsemble", n_valid, self.B)
        if nv != self._nv:
            raise L.DeepcamHipError(f"ViewEnsemble: the members of this batch had n_valid = {self._nv}, got {nv}")
        L.call("dc_ensemble_pool", self.B, nv, self.H, self.W, self._members, L.dptr(self._state), L.dptr(self._logits), L.dptr(self._rows),
               L.dptr(self._totals), L.dptr(self._frames), L.stream_ptr())
        self._pooled_members, self._pooled_valid = self._members, nv
        return self._logits

    def frame_rows(self) -> torch.Tensor:
        """int64 [n_valid, 208] of the last pool(): per frame, word 64 c + k the pixels with exactly k votes for class c, word 192 + 4 i + j
        the pixels whose class in member 0 is i and in the pool j (3: not finite); a view of the object's device buffer, not synchronised"""
        return self._rows[:self._pooled_valid]

    def reset(self) -> None:
        """zeroes the running totals (in stream order)"""
        self._totals.zero_()
        self._frames.zero_()

    def state(self) -> dict:
        """on the host: totals [208] and frames as Python ints, members of the last pool()"""
        return {"totals": [int(v) for v in self._totals.cpu().tolist()], "frames": int(self._frames.cpu()[0]), "members": self._pooled_members}

    def result(self) -> dict:
        """decode() of the object's state"""
        s = self.state()
        return self.decode(s["totals"], s["frames"], s["members"])

    @staticmethod
    def decode(totals, frames: int, members: int) -> dict:
        """From the 208 integers: frames, members, pixels, not_finite (pixels at which a member's logits were not finite: they pool to
        NaN); per class ("class_0", "class_1", "class_2") vote_share (a list over k = 0 .. members: the share of pixels with exactly k
        votes for the class), mean_votes, gained (pixels the class has in the pooled mask and not in member 0's) and lost (the reverse);
        unanimous, the share of pixels on which all members name one class; changed, the 4 x 4 matrix [member 0's class][pooled class]
        with 3 = not finite.  A share is None without pixels."""
        t = [int(v) for v in np.asarray(totals).reshape(-1).tolist()]
        members = int(members)
        if len(t) != ENSEMBLE_ROW or not 0 <= members <= ENSEMBLE_MAX_MEMBERS:
            raise L.DeepcamHipError(f"ViewEnsemble.decode: totals must hold {ENSEMBLE_ROW} integers and members lie in [0, {ENSEMBLE_MAX_MEMBERS}]")
        pixels = sum(t[:64])                          # every pixel has some number of votes for class 0
        changed = [[t[ENSEMBLE_CHANGED + 4 * i + j] for j in range(4)] for i in range(4)]
        out = {"frames": int(frames), "members": members, "pixels": pixels, "not_finite": sum(row[3] for row in changed),
               "unanimous": _ratio(sum(t[64 * c + members] for c in range(3)), pixels) if members else None, "changed": changed}
        for c in range(3):
            votes = t[64 * c:64 * c + 64]
            out[f"class_{c}"] = {"vote_share": [_ratio(votes[k], pixels) for k in range(members + 1)],
                                 "mean_votes": _ratio(sum(k * n for k, n in enumerate(votes)), pixels),
                                 "gained": sum(changed[i][c] for i in range(4) if i != c),
                                 "lost": sum(changed[c][j] for j in range(4) if j != c)}
        return out
