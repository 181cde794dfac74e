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
The analysis classes live in the topic modules events, render, climate, skills and decide and are re-exported here.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from fractions import Fraction  # noqa: F401  (a name this module has always exposed)
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from . import ops as _ops
from .engine import Engine
# the re-exports: every name is defined once, in its topic module
from ._args import _BYTES, _c_int, _float, _n_valid, _ratio, _two_words  # noqa: F401
from .events import (EARTH_RADIUS_KM, EVENT_FIELD_STATS, EVENT_FIELDS, EVENT_FILTER_COUNTS, EVENT_SCALE, EVENT_SHAPE_FIELDS,  # noqa: F401
                     EVENT_SHAPE_VALUES, TRACK_COVER_FIELDS, TRACK_FIELD_STATS, TRACK_FIELDS, TRACK_PAIR_FIELDS, TRACK_STEP_FIELDS,
                     TRACK_STORE_FIELDS, EventCatalog, EventFields, EventFilter, EventMatcher, EventShape, EventTracker, TrackFields,
                     TrackMatcher, _filled_rows, event_field_bits, event_field_key, event_field_value, event_shape_tables,
                     event_weight_tables, great_circle_km)
from .render import _RAMP, RENDER_BACKGROUND, RENDER_COLOURS, FrameRenderer, gall_rows, graticule, plate_rows, render_palette  # noqa: F401
from .climate import (_DATE, _SEASON_OF_MONTH, CLIMATOLOGY_GROUPS, CLIMATOLOGY_MAX_FRAMES, CLIMATOLOGY_PRODUCTS,  # noqa: F401
                      CLIMATOLOGY_ROWS, COMPOSITE_COUNTS, COMPOSITE_KEYS, COMPOSITE_MAX_EVENTS, COMPOSITE_MAX_RADIUS, Climatology,
                      StormComposite, climatology_group, composite_bits, composite_radius_table)
from .skills import (DISPLACEMENT_MAX_BATCH, DISPLACEMENT_MAX_RADIUS, DISPLACEMENT_RADIUS, DISTANCE_MAX_BATCH,  # noqa: F401
                     DISTANCE_MAX_RADIUS, DISTANCE_Q, DISTANCE_RADIUS, FSS_MAX_BATCH, FSS_MAX_WINDOW, FSS_MAX_WINDOWS, FSS_WINDOWS, PROB_BINS,
                     PROB_MAX_BATCH, PROB_MAX_BINS, PROB_MAX_PIXELS, PROB_ONE, SCALE_LISTS, SCALE_MAX_BATCH, SCALE_MAX_LEVELS,
                     SCALE_MAX_ORIGINS, DisplacementSkill, DistanceSkill, FractionsSkill, ProbabilitySkill, ScaleSkill, _fss, _MaskSkill,
                     _scale_components, brier_from_rows, displacement_best, displacement_from_rows, distance_from_rows, distance_table,
                     fss_from_rows, scale_from_rows, scale_levels)
from .decide import (DECISION_COUNTS, DECISION_NEVER, ENSEMBLE_CHANGED, ENSEMBLE_MAX_MEMBERS, ENSEMBLE_MAX_WEIGHT_SUM,  # noqa: F401
                     ENSEMBLE_ROW, DecisionRule, ViewEnsemble, decision_q, decision_q_from_bin, seam_weights, view_input)

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
        # events=True: the event catalogue of every mask (events.EventCatalog), run behind the classifier on the same stream
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
