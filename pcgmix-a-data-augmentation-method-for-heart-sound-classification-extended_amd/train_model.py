"""Per-step training path of the reference's ``train_model.py`` (train_epoch, :490-589) on
MI355X: augment -> forward -> soft-target CE -> backward -> clip_grad_value_ -> Adam ->
OneCycleLR, one process per GPU with DistributedDataParallel over RCCL (the reference's
single-process ``nn.DataParallel``, train_model.py:385, is replaced).

What is kept: the loss (CELoss :45-54, SELCLoss :56-80), optimiser and scheduler setup
(:404-410), gradient value clipping (:557-558), the step counter that seeds the augmentation
(:105-109, :581), the per-epoch reseeding of the loader shuffle (:497), and the
``train_epoch`` signature.  What is deliberately not reproduced: the per-sample ``.item()``
loop (:542-552) — loss and hit counts stay on the device and are read once per epoch — and the
model zoo / plotting / pickling around the loop (out of scope).
"""
from __future__ import annotations

import os
import types
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import augmentations, augmentations2d, models, models2d

SPECTROGRAM_DATASETS = ("PhysioNet(spec128)", "UMC(spec128)", "UMC(spec64)")


class SoftCEFunction(torch.autograd.Function):
    """CELoss on a HIP device as one kernel each way (``pcgmix_soft_ce_{fwd,bwd}_f32``) instead of
    log_softmax, mul, sum, neg, mean and their five backward launches."""

    @staticmethod
    def forward(ctx, logits, target):
        import ctypes
        from . import _lib
        lib = _lib.load()
        logits = logits.contiguous()
        target = target.to(torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
        _lib.check(lib.pcgmix_soft_ce_fwd_f32(logits.data_ptr(), target.data_ptr(), loss.data_ptr(),
                                              logits.shape[0], logits.shape[1], stream),
                   "pcgmix_soft_ce_fwd_f32")
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, gout):
        import ctypes
        from . import _lib
        lib = _lib.load()
        logits, target = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        d = torch.empty_like(logits)
        stream = ctypes.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
        _lib.check(lib.pcgmix_soft_ce_bwd_f32(logits.data_ptr(), target.data_ptr(), gout.data_ptr(),
                                              d.data_ptr(), logits.shape[0], logits.shape[1],
                                              stream), "pcgmix_soft_ce_bwd_f32")
        return d, None


class CELoss(nn.Module):
    """Cross-entropy with soft targets: mean_b( -sum_c log_softmax(logits)[b,c] * t[b,c] )
    (train_model.py:45-54)."""

    def __init__(self, num_classes: int):
        super().__init__()
        self.num_classes = num_classes

    def forward(self, logits, target_ohe):
        if logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 \
                and logits.shape[0] > 0 and not target_ohe.requires_grad:
            return SoftCEFunction.apply(logits, target_ohe)
        return -(F.log_softmax(logits, dim=1) * target_ohe).sum(dim=1).mean()


def selc_keep_take(momentum: float):
    """The two float32 factors of ``m * soft + (1 - m) * pred`` as torch forms them from the Python
    scalar ``m``: ``1 - m`` is taken in double and THEN cast, so for m = 0.9 the second factor is
    ``float32(0.1)`` and not ``float32(1) - float32(0.9)`` (one ulp more)."""
    return np.float32(momentum), np.float32(1.0 - momentum)


class SELCFunction(torch.autograd.Function):
    """SELCLoss past its turning point (train_model.py:56-80) on a HIP device as one kernel each way
    (``pcgmix_selc_{fwd,bwd}_f32``): softmax, the momentum update of ``soft_labels[index]`` (in
    place, as the reference's side effect) and the loss against the updated rows; the backward
    reads the rows the forward stored, not ``soft_labels``.  ``index``: int64 (B,) on the device,
    distinct values; a value outside [0, N) leaves its row out (no update, zero loss and gradient)."""

    @staticmethod
    def forward(ctx, logits, index, soft_labels, momentum):
        import ctypes
        from . import _lib
        lib = _lib.load()
        logits = logits.contiguous()
        B, C = logits.shape
        if index.dtype != torch.int64 or index.shape != (B,) or index.device != logits.device \
                or not index.is_contiguous():
            raise ValueError("index must be a contiguous int64 (B,) tensor on the logits' device")
        if soft_labels.dtype != torch.float32 or soft_labels.dim() != 2 or soft_labels.shape[1] != C \
                or soft_labels.device != logits.device or not soft_labels.is_contiguous():
            raise ValueError("soft_labels must be a contiguous float32 (N, classes) tensor on the "
                             "logits' device")
        keep, take = selc_keep_take(momentum)
        rows = torch.empty_like(logits)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
        _lib.check(lib.pcgmix_selc_fwd_f32(logits.data_ptr(), index.data_ptr(), soft_labels.data_ptr(),
                                           soft_labels.shape[0], ctypes.c_float(keep),
                                           ctypes.c_float(take), rows.data_ptr(), loss.data_ptr(),
                                           B, C, stream), "pcgmix_selc_fwd_f32")
        ctx.save_for_backward(logits, rows)
        return loss

    @staticmethod
    def backward(ctx, gout):
        import ctypes
        from . import _lib
        lib = _lib.load()
        logits, rows = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        d = torch.empty_like(logits)
        stream = ctypes.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
        _lib.check(lib.pcgmix_selc_bwd_f32(logits.data_ptr(), rows.data_ptr(), gout.data_ptr(),
                                           d.data_ptr(), logits.shape[0], logits.shape[1], stream),
                   "pcgmix_selc_bwd_f32")
        return d, None, None, None


class SELCLoss(nn.Module):
    """train_model.py:56-80.  Plain CE until epoch ``es``; afterwards the self-ensembled soft
    labels.  With the reference's default (``es = num_epochs + 1`` unless the method contains
    'SELC', :394-402) it is CELoss.  Soft labels live on ``device`` (the reference hard-codes
    ``.cuda()``, :60).  On a HIP device the SELC phase is ``SELCFunction``; ``use_kernel = False``
    keeps the torch formulation (which is also what a CPU tensor gets)."""

    use_kernel = True     # SELC phase through the HIP kernels (False: torch ops; train_step then
                          # also leaves the fused Potes head + SELC node)

    def __init__(self, labels, num_classes: int, es: int = 10, momentum: float = 0.9,
                 device: Optional[torch.device] = None):
        super().__init__()
        labels = torch.as_tensor(np.asarray(labels), dtype=torch.long)
        soft = torch.zeros(len(labels), num_classes, dtype=torch.float)
        soft[torch.arange(len(labels)), labels] = 1
        self.register_buffer("soft_labels", soft.to(device) if device is not None else soft)
        self.num_classes, self.es, self.momentum = num_classes, es, momentum
        self.CEloss = CELoss(num_classes)

    def device_index(self, index) -> torch.Tensor:
        """``index`` as an int64 tensor next to the soft labels.  An index that arrives on the host
        (every loader hands over a host tensor) is checked there: outside [0, N) is an IndexError,
        before anything is launched.  A device tensor is taken as it is — the kernels leave a row
        with a bad index out, they never write outside ``soft_labels``."""
        if not (torch.is_tensor(index) and index.is_cuda):
            index = torch.as_tensor(index, dtype=torch.long).reshape(-1)
            n = self.soft_labels.shape[0]
            if index.numel() and (int(index.min()) < 0 or int(index.max()) >= n):
                raise IndexError(f"SELCLoss: sample index outside [0, {n})")
        return index.to(self.soft_labels.device, dtype=torch.long, non_blocking=True)

    def forward(self, logits, labels, index, epoch, mode):
        if mode == "test" or epoch <= self.es:
            return self.CEloss(logits, labels)
        index = self.device_index(index)
        if self.use_kernel and logits.is_cuda and logits.dtype == torch.float32 \
                and logits.dim() == 2 and logits.shape[0] > 0:
            return SELCFunction.apply(logits, index.contiguous(), self.soft_labels, self.momentum)
        pred = F.softmax(logits, dim=1)
        with torch.no_grad():
            self.soft_labels[index] = (self.momentum * self.soft_labels[index]
                                       + (1 - self.momentum) * pred.detach())
        return -(torch.log(pred) * self.soft_labels[index]).sum(dim=1).mean()


class step_counter_class:
    """train_model.py:105-109: the only source of augmentation randomness."""

    def __init__(self):
        self.count = 0

    def add(self):
        self.count += 1


class _ClipUpdate:
    """What ClipAdam and ClipSGD share; the first base, in front of the torch optimiser.  The
    multi-tensor launch of ``csrc/pcgmix_optim.hip`` takes host pointer tables (cached here) and
    can be the last node of a captured training step (``GraphedTrainStep``): kernel arguments are
    frozen at capture while OneCycleLR moves the group's scalars every step, so the captured launch
    reads them from device memory and ``next_hyper`` writes them on the host for the coming replay.
    A subclass names its three launches, says which state tensors are the tables' extra columns
    (``_columns``) and keeps ``step``, ``prepare_capture`` (which sets ``_cap_params``) and
    ``next_hyper``.  Gradients are NOT modified (torch's clip is in place; nothing downstream of
    the optimiser step reads them)."""

    EAGER_LAUNCH = DEV_LAUNCH = REDUCE_LAUNCH = None    # REDUCE_LAUNCH: the tape's fifth launch
    _STATE_WORDS = None                                 # what load_state_dict replaces, in words

    def __init__(self, params, clip_value, **kw):
        super().__init__(params, **kw)
        self.clip_value = float(clip_value or 0.0)
        self._tables = {}
        self._cap_params = self._cap_grads = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = {}                      # the state tensors were replaced
        self._adopt_loaded_state()
        if getattr(self, "_cap_params", None):
            raise RuntimeError(f"{type(self).__name__}: load the state before the step is captured "
                               f"(the graph holds the addresses of the old {self._STATE_WORDS})")

    def _adopt_loaded_state(self):
        pass

    def _table(self, gi, live, grads):
        """Host pointer tables of group ``gi`` in the order the entry points take them: (key, p, g,
        *state columns, n).  Cached; rebuilt when a parameter moved (the key), and dropped where a
        state tensor appears or is replaced (``_init_state``, ``load_state_dict``); an absent state
        tensor is a NULL entry.  The gradient pointers are rewritten in place."""
        import ctypes
        key = [p.data_ptr() for p in live]
        tab = self._tables.get(gi)
        if tab is None or tab[0] != key:
            arr = ctypes.c_void_p * len(live)
            cols = [[None if t is None else t.data_ptr() for t in col] for col in self._columns(live)]
            tab = (key, arr(*key), arr(), *[arr(*col) for col in cols],
                   (ctypes.c_longlong * len(live))(*[p.numel() for p in live]))
            self._tables[gi] = tab
        gptr = tab[2]
        for i, g in enumerate(grads):
            gptr[i] = g.data_ptr()
        return tab

    @staticmethod
    def _dense_grads(live):
        # flat iteration over raw memory: p, grad and the state tensors must share one dense layout
        return [p.grad if p.grad.stride() == p.stride() else torch.empty_like(p).copy_(p.grad)
                for p in live]

    def can_capture(self) -> bool:
        return len(self.param_groups) == 1

    @torch.no_grad()
    def capture_update(self, hyper_dev: torch.Tensor, deferred: Optional[dict] = None):
        """Inside the capture, after backward: the update of all ``prepare_capture`` tensors.

        ``deferred`` (``models.PotesStackFunction.defer_reduce`` after the backward): the Potes conv
        stack left its 212 gradient columns as G un-reduced partial rows.  When the stack's four
        parameter gradients are views of ``deferred["grads"]`` (autograd keeps the tensors the
        backward returned) the reduction runs as 212 extra blocks of this launch, each of which also
        updates its element; otherwise it is launched on its own first."""
        import ctypes
        from . import _lib
        lib = _lib.load()
        live = self._cap_params
        if any(p.grad is None for p in live):
            raise RuntimeError(f"{type(self).__name__}.capture_update: a prepared parameter has no "
                               "gradient")
        self._cap_grads = self._dense_grads(live)            # keep graph memory referenced
        self._opt_called = True      # the replays stand for step(): what LRScheduler's wrapper of it records
        args = (len(live), *self._table(0, live, self._cap_grads)[1:], hyper_dev.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(live[0].device).cuda_stream)
        if deferred and "partial" in deferred:
            grads, partial, G = deferred["grads"], deferred["partial"], int(deferred["G"])
            lo, hi = grads.data_ptr(), grads.data_ptr() + grads.numel() * 4
            covered = sum(g.numel() for g in self._cap_grads if lo <= g.data_ptr() < hi)
            self._cap_deferred = (partial, grads)            # referenced by the graph
            if covered == grads.numel() and len(live) <= 32:
                _lib.check(getattr(lib, self.REDUCE_LAUNCH)(
                    *args, partial.data_ptr(), grads.data_ptr(), G, stream), self.REDUCE_LAUNCH)
                return
            _lib.check(lib.pcgmix_potes_reduce_f32(partial.data_ptr(), grads.data_ptr(), G, stream),
                       "pcgmix_potes_reduce_f32")
        _lib.check(getattr(lib, self.DEV_LAUNCH)(*args, stream), self.DEV_LAUNCH)

    def _captured(self):
        """(parameter, the gradient tensor the captured update reads) pairs."""
        return zip(self._cap_params, self._cap_grads)


class ClipAdam(_ClipUpdate, torch.optim.Adam):
    """``clip_grad_value_(clip)`` + ``torch.optim.Adam`` (L2 weight decay) as one HIP launch for all
    parameters of a group (``pcgmix_adam_clip_multi_f32``).  Same state layout (``step``,
    ``exp_avg``, ``exp_avg_sq``) and param-group keys as torch's Adam, so OneCycleLR cycles ``lr``
    and ``betas`` on it unchanged and checkpoints interchange."""

    EAGER_LAUNCH = "pcgmix_adam_clip_multi_f32"
    DEV_LAUNCH = "pcgmix_adam_clip_multi_dev_f32"
    REDUCE_LAUNCH = "pcgmix_adam_clip_multi_reduce_dev_f32"
    _STATE_WORDS = "moment tensors"

    def __init__(self, params, lr, weight_decay=0.0, clip_value=0.0, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, clip_value, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._cap_step, self._cap_dirty = 0, False

    def _init_state(self, params):
        for p in params:
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self._tables = {}

    def _columns(self, live):
        return [self.state[p]["exp_avg"] for p in live], [self.state[p]["exp_avg_sq"] for p in live]

    @torch.no_grad()
    def step(self, closure=None):
        import ctypes
        from . import _lib
        lib = _lib.load()
        self._flush_captured_steps()
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            self._init_state(live)
            for p in live:
                self.state[p]["step"] += 1
            steps = {int(self.state[p]["step"]) for p in live}
            if len(steps) != 1:
                raise RuntimeError("ClipAdam: parameters of one group must share the step count")
            if self._cap_params:
                # an eager step between captured ones (train_epoch: a batch of another shape) counts
                # for the captured launches too: their bias corrections continue from here
                self._cap_step = next(iter(steps))
            tab = self._table(gi, live, self._dense_grads(live))
            stream = ctypes.c_void_p(torch.cuda.current_stream(live[0].device).cuda_stream)
            _lib.check(getattr(lib, self.EAGER_LAUNCH)(
                len(live), *tab[1:], ctypes.c_float(self.clip_value),
                ctypes.c_float(float(group["lr"])), ctypes.c_float(b1), ctypes.c_float(b2),
                ctypes.c_float(group["eps"]), ctypes.c_float(group["weight_decay"]),
                steps.pop(), stream), self.EAGER_LAUNCH)
        return None

    # ---- captured: the bias corrections move with the step count, which the host keeps ---------
    def prepare_capture(self, params):
        """Before the capture: allocate the moments of ``params`` (the tensors that will carry a
        gradient) — an allocation inside the capture would be re-zeroed by every replay."""
        self._flush_captured_steps()                 # re-capture: the state carries the live count
        self._init_state(params)
        steps = {int(self.state[p]["step"]) for p in params}
        if len(steps) != 1:
            raise RuntimeError("ClipAdam: parameters of one group must share the step count")
        self._cap_params = list(params)
        self._cap_step = steps.pop()

    def next_hyper(self, out8) -> None:
        """Host: the eight scalars of the NEXT update into ``out8`` (float32[8], numpy), from the
        param group as the scheduler left it; counts the step.  ``state[p]['step']`` is brought
        up to date lazily (``state_dict`` / an eager ``step``)."""
        import ctypes
        from . import _lib
        g = self.param_groups[0]
        self._cap_step += 1
        self._cap_dirty = True
        _lib.check(_lib.load().pcgmix_adam_hyper(
            ctypes.c_float(self.clip_value), ctypes.c_float(float(g["lr"])),
            ctypes.c_float(g["betas"][0]), ctypes.c_float(g["betas"][1]), ctypes.c_float(g["eps"]),
            ctypes.c_float(g["weight_decay"]), self._cap_step, out8.ctypes.data), "pcgmix_adam_hyper")

    def _flush_captured_steps(self):
        if getattr(self, "_cap_dirty", False):
            for p in self._cap_params:
                self.state[p]["step"].fill_(float(self._cap_step))
            self._cap_dirty = False

    def state_dict(self):
        self._flush_captured_steps()
        return super().state_dict()


class ClipSGD(_ClipUpdate, torch.optim.SGD):
    """``clip_grad_value_(clip)`` + ``torch.optim.SGD`` (momentum, L2 weight decay) as one HIP launch
    for all parameters of a group (``pcgmix_sgd_clip_multi_f32``; train_model.py:404-405, 557-558,
    566).  Same state (``momentum_buffer``) and param-group keys as torch's SGD, so OneCycleLR cycles
    ``lr`` and ``momentum`` on it unchanged and checkpoints interchange.  With momentum 0 no buffers
    exist and the state stays empty, as torch's does.  ``dampening``, ``nesterov`` and ``maximize``
    are refused: the kernel implements the reference's defaults."""

    EAGER_LAUNCH = "pcgmix_sgd_clip_multi_f32"
    DEV_LAUNCH = "pcgmix_sgd_clip_multi_dev_f32"
    REDUCE_LAUNCH = "pcgmix_sgd_clip_multi_reduce_dev_f32"
    _STATE_WORDS = "momentum buffers"

    def __init__(self, params, lr, weight_decay=0.0, clip_value=0.0, momentum=0.0, dampening=0.0,
                 nesterov=False, maximize=False):
        self._refuse(dict(dampening=dampening, nesterov=nesterov, maximize=maximize))
        super().__init__(params, clip_value, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self._cap_buffers = False

    @staticmethod
    def _refuse(group):
        if group.get("dampening", 0) != 0 or group.get("nesterov") or group.get("maximize"):
            raise NotImplementedError("ClipSGD: dampening, nesterov and maximize are not implemented "
                                      "(the reference trains with torch.optim.SGD's defaults)")

    def _adopt_loaded_state(self):
        for group in self.param_groups:
            self._refuse(group)
            for p in group["params"]:          # torch's buffer is a clone of the GRADIENT: its layout
                buf = self._buf(p)
                if buf is not None and buf.stride() != p.stride():
                    self.state[p]["momentum_buffer"] = torch.empty_like(p).copy_(buf)

    def _buf(self, p):
        return self.state.get(p, {}).get("momentum_buffer")     # (no state entry is created by asking)

    def _init_state(self, params):
        for p in params:
            if self._buf(p) is None:
                self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self._tables = {}

    def _columns(self, live):
        return ([self._buf(p) for p in live],)   # (None: no momentum so far — a NULL entry)

    @torch.no_grad()
    def step(self, closure=None):
        import ctypes
        from . import _lib
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            self._refuse(group)
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            mom = float(group["momentum"])
            if mom != 0.0:
                self._init_state(live)
            tab = self._table(gi, live, self._dense_grads(live))
            stream = ctypes.c_void_p(torch.cuda.current_stream(live[0].device).cuda_stream)
            _lib.check(getattr(lib, self.EAGER_LAUNCH)(
                len(live), *tab[1:], ctypes.c_float(self.clip_value),
                ctypes.c_float(float(group["lr"])), ctypes.c_float(mom),
                ctypes.c_float(group["weight_decay"]), stream), self.EAGER_LAUNCH)
        return None

    # ---- captured: SGD has no step count, nothing to carry between captures --------------------
    def prepare_capture(self, params):
        """Before the capture: allocate the momentum buffers of ``params`` when the group's momentum
        is not 0 (an allocation inside the capture would be re-zeroed by every replay)."""
        params = list(params)
        self._refuse(self.param_groups[0])
        if float(self.param_groups[0]["momentum"]) != 0.0:
            self._init_state(params)
        self._cap_params = params
        self._cap_buffers = all(self._buf(p) is not None for p in params)

    def next_hyper(self, out8) -> None:
        """Host: {clip, wd, momentum, lr} of the NEXT update into ``out8`` (float32[8], numpy), from
        the param group as the scheduler left it."""
        import ctypes
        from . import _lib
        g = self.param_groups[0]
        self._refuse(g)
        if float(g["momentum"]) != 0.0 and not self._cap_buffers:
            raise RuntimeError("ClipSGD: momentum became non-zero on a step that was captured without "
                               "momentum buffers; capture the step again")
        _lib.check(_lib.load().pcgmix_sgd_hyper(
            ctypes.c_float(self.clip_value), ctypes.c_float(float(g["lr"])),
            ctypes.c_float(float(g["momentum"])), ctypes.c_float(g["weight_decay"]),
            out8.ctypes.data), "pcgmix_sgd_hyper")


def selc_turning_point(args) -> int:
    """train_model.py:394-402."""
    if "SELC" in args.method and ("mixup" in args.method or "base" in args.method):
        return int(args.num_epochs * 0.4)
    return args.num_epochs + 1


# train_model.py:341-358: the ResNet9-1D size ladder, args.model -> filters
RESNET9_LADDER = {
    "resnet9-5k": (2, 4, 8, 16), "resnet9-15k": (4, 8, 16, 32), "resnet9-50k": (8, 16, 32, 64),
    "resnet9-150k": (16, 32, 64, 128), "resnet9-600k": (32, 64, 128, 256),
    "resnet9-1.4m": (64, 128, 192, 384), "resnet9-2.3m": (64, 128, 256, 512),
    "resnet9-5m": (96, 192, 384, 768), "resnet9-9m": (128, 256, 512, 1024),
}
# train_model.py:359-370: the Potes size ladder, args.model -> (factory, takes dataset, extra kwargs)
POTES_LADDER = {
    "Potes": ("CNN_potes_TS", True, {}),
    "Potes(noDropout)": ("CNN_potes_TS", True, {"dropout": 0.0}),
    "PotesBig64and32": ("CNN_potes_big64and32_TS", True, {}),
    "PotesBig128and64": ("CNN_potes_big128and64_TS", True, {}),
    "Potes0.1": ("CNN_potes_tenpercent_TS", False, {}),
    "Potes0.02": ("CNN_potes_twopercent_TS", False, {}),
}


def build_model(args) -> nn.Module:
    """The models of the hot path (train_model.py:296, 337-370: 'Potes', 'resnet9' and the two
    model-size ladders around them), head sized for ``args.sig_len`` (the reference hard-codes
    T = 2500).  Every Potes name runs its conv branch on a hand-written HIP stack: 'Potes' and
    'Potes(noDropout)' on the [8,4] kernels, 'Potes0.1' and 'Potes0.02' on the narrow ones, the two
    'PotesBig*' models on the f32-matrix-instruction ones (csrc/pcgmix_potes_big.hip).  Every
    ResNet9 width of the ladder (2 ... 1024) runs its BatchNorm + ReLU + pool through the HIP
    kernels, in training and in eval mode: they take C = 2 and every multiple of 4 up to 1024
    (``pcgmix_bnrp_supported``), so no ResNet9 name warns.  With PCGMIX_TRAIN_DETERMINISTIC=1 (or
    ``models.FUSED_CONV_TRAIN``) every Conv1d(k=3) of every ladder name runs on the project's
    fixed-order kernels: the matrix ones (csrc/pcgmix_conv3.hip, pcgmix_conv3_wgrad.hip), and for the
    2- and 8-channel layers of 'resnet9-5k' ... 'resnet9-50k' the narrow ones
    (csrc/pcgmix_conv3_narrow.hip, ``models.FUSED_CONV_NARROW``).  Without the switch those narrow
    layers keep MIOpen on every route."""
    sig_len = getattr(args, "sig_len", 2500)
    if args.dataset in SPECTROGRAM_DATASETS:
        if args.model != "resnet9":
            raise NotImplementedError(args.model)
        return models2d.ResNet9(num_classes=args.num_classes)
    if args.model in POTES_LADDER:
        factory, takes_dataset, kw = POTES_LADDER[args.model]
        kw = dict(kw, sig_len=None if sig_len == 2500 else sig_len)
        if takes_dataset:
            kw["dataset"] = args.dataset
        m = getattr(models, factory)(num_channels=args.num_channels, num_classes=args.num_classes, **kw)
        # cnn2..cnn4 are never called (reference models.py:444-455): their grads stay None in
        # the reference, so Adam and the clipper skip them; freezing them is equivalent and
        # keeps them out of the DDP reducer
        for name in ("cnn2", "cnn3", "cnn4"):
            for p in getattr(m, name).parameters():
                p.requires_grad_(False)
        return m
    if args.model == "resnet9":
        return models.ResNet9(in_channels=args.num_channels, num_classes=args.num_classes,
                              linear=models.resnet9_flat_features(sig_len))
    if args.model in RESNET9_LADDER:
        filters = RESNET9_LADDER[args.model]
        return models.ResNet9(in_channels=args.num_channels, num_classes=args.num_classes,
                              filters=filters,
                              linear=models.resnet9_flat_features(sig_len, filters[-1]))
    raise NotImplementedError(f"model {args.model!r} is outside the PCGmix hot path")


FUSED_SGD = True     # op='SGD' through ClipSGD where it applies; False: torch.optim.SGD (A/B timing, tests)


def make_optimizer(args, model: nn.Module):
    """train_model.py:404-410."""
    params = [p for p in model.parameters() if p.requires_grad]

    def dense(p):       # any non-overlapping dense layout: the kernel walks raw memory
        order = sorted(range(p.dim()), key=lambda d: (-p.stride(d), -p.size(d)))
        return p.numel() == 0 or p.permute(order).is_contiguous()
    hip_path = all(p.is_cuda and p.dtype == torch.float32 and dense(p) for p in params)
    if args.op == "SGD":
        if FUSED_SGD and hip_path:
            # clip + SGD in one HIP launch (train_step then skips clip_grad_value_)
            opt = ClipSGD(params, lr=args.lr_max, weight_decay=args.weight_decay,
                          clip_value=args.grad_clip)
        else:
            opt = torch.optim.SGD(params, lr=args.lr_max, weight_decay=args.weight_decay)
    elif args.op == "adam":
        if hip_path:
            # clip + Adam in one HIP pass per tensor (train_step then skips clip_grad_value_)
            opt = ClipAdam(params, lr=args.lr_max, weight_decay=args.weight_decay,
                           clip_value=args.grad_clip)
        else:
            opt = torch.optim.Adam(params, lr=args.lr_max, weight_decay=args.weight_decay)
    else:
        raise ValueError(args.op)
    sched = None
    if args.use_sched:
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr_max,
                                                    total_steps=args.num_steps)
    return opt, sched


def rank_and_world():
    """(rank, world size) of this process; (0, 1) without an initialised process group."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def wrap_distributed(model: nn.Module, device: torch.device) -> nn.Module:
    """One process per GPU; gradients are averaged by an all-reduce (RCCL over xGMI when the
    process group is 'nccl').  The whole model fits one bucket (<= 26 MB), so the single
    all-reduce overlaps the tail of backward.  BatchNorm statistics stay per rank, as they are
    per replica under the reference's DataParallel."""
    if rank_and_world()[1] == 1:
        return model
    ids = [device.index] if device.type == "cuda" else None
    return nn.parallel.DistributedDataParallel(model, device_ids=ids, bucket_cap_mb=64,
                                               gradient_as_bucket_view=True)


class FlatGradSync:
    """Gradient averaging over ranks without DDP's autograd hooks, so that forward + backward can
    live in a hipGraph: the gradients are packed into one flat buffer by ONE concat kernel (inside
    the captured region), summed by ONE all-reduce (RCCL over xGMI under 'nccl'; 0.8 MB for Potes,
    9.1 MB for ResNet9-1D — a single message per step, the size the per-link-bound ring wants),
    and the optimiser then reads views of that buffer.  The caller scales backward by 1/world
    (``backward_scale``) so the sum IS the mean on every backend.  BatchNorm buffers stay per
    rank, as under the reference's DataParallel (train_model.py:385)."""

    def __init__(self, model: nn.Module, device: torch.device):
        import torch.distributed as dist
        self.dist = dist
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.model, self.device = model, device
        self.params, self.flat, self.views, self._graph_grads = None, None, None, None
        if self.world > 1:                              # same start on every rank, as DDP does
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, 0)

    @property
    def backward_scale(self) -> float:
        return 1.0 / self.world

    def attach(self):
        """Call once after a first backward: fixes the set of parameters that receive gradients
        (CNN_potes allocates cnn2..cnn4 but never uses them) and allocates the flat buffer."""
        self.params = [p for p in self.model.parameters() if p.grad is not None]
        total = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(total, device=self.device, dtype=self.params[0].dtype)
        self.views, o = [], 0
        for p in self.params:
            self.views.append(self.flat[o:o + p.numel()].view_as(p))
            o += p.numel()

    def pack(self):
        """Concatenate the fresh gradients into the flat buffer (capturable: one kernel)."""
        self._graph_grads = [p.grad for p in self.params]            # keep graph memory referenced
        torch.cat([g.reshape(-1) for g in self._graph_grads], out=self.flat)

    def reduce_and_bind(self):
        """Sum over ranks and hand the optimiser the averaged gradients."""
        if self.world > 1:
            self.dist.all_reduce(self.flat)
        for p, v in zip(self.params, self.views):
            p.grad = v


def shard_batch(batch, rank: int, world: int):
    """Give rank r the r-th contiguous slice of every per-sample field (drop_last semantics of
    dataloader_physionet.py:227: the remainder is dropped)."""
    n = len(batch[0]) // world
    sl = slice(rank * n, (rank + 1) * n)
    return tuple(b[sl] for b in batch)


class _SeedView:
    __slots__ = ("count",)

    def __init__(self, count: int):
        self.count = count


def augmentation_counter(args, step_counter):
    """What ``augment()`` is given as its step counter.  The reference derives every random choice
    of a step from ``step_counter.count`` (train_model.py:507, augmentations.py:869-903), so under
    data parallelism every rank draws the same lambda, the same warp knots and the same
    permutation pattern.  ``args.rank_seed = True`` — NOT the reference's behaviour,
    off by default — gives rank r of w the seed ``count * w + r`` instead: distinct
    streams per rank that never collide across steps.  One process: unchanged."""
    if not getattr(args, "rank_seed", False):
        return step_counter
    rank, world = rank_and_world()
    if world == 1:
        return step_counter
    return _SeedView(int(step_counter.count) * world + rank)


def reseed_device_rng(args, device) -> None:
    """train_model.py:565: the reference calls ``torch.cuda.manual_seed_all(args.seed_fix)`` before
    every ``optimizer.step()``.  Its visible effect on a GPU is on the NEXT forward pass: the
    device generator restarts from the same position every step, so every step (and, under
    DataParallel, every replica) draws the same dropout masks.  Kept, for this process's device
    (one process per GPU); host-only, no launch.  ``args.seed_fix`` is set by ``train_model``
    (:217); loops that do not set it keep torch's running stream."""
    seed = getattr(args, "seed_fix", None)
    if seed is not None and device.type == "cuda":
        if getattr(args, "rank_seed", False):           # non-reference: per-rank dropout masks
            seed = int(seed) + rank_and_world()[0]
        torch.cuda.manual_seed(int(seed))


def fused_loss_model(model, criterion, data, target_ohe, epoch):
    """The CNN_potes whose head and loss can run as one autograd node for this step, or None:
    an unwrapped CNN_potes on the HIP path, a criterion in its plain-CE phase (CELoss, or SELCLoss
    up to its turning point, train_model.py:66-72), targets that need no gradient."""
    if not isinstance(model, models.CNN_potes) or target_ohe.requires_grad:
        return None
    if isinstance(criterion, SELCLoss):
        if epoch is None or epoch > criterion.es:
            return None
    elif not isinstance(criterion, CELoss):
        return None
    if not (data.dim() == 3 and model._fused_head(data) and data.shape[0] > 0):
        return None
    return model


LATENT_DDP_MESSAGE = ("latentmixup under torch.distributed is not supported: it runs the "
                      "model in two halves per step, which the DDP step does not handle")
LATENT_GRAPH_MESSAGE = ("latentmixup is not wired into the captured step: its per-step partners and "
                        "lambda have no slot in the graph's static block; use train_step")


def method_route(args):
    """``hostprep.route`` of ``args.method`` for the data set's dimensionality."""
    return augmentations.hostprep.route(args.method, args.dataset in SPECTROGRAM_DATASETS)


def latent_method(args) -> bool:
    """True when ``args.method`` reaches the reference's 1D ``latentmixup`` branch on a time-series
    dataset."""
    return method_route(args).family == "latent"


def cutpaste_graph_message(args) -> str:
    return (f"method {args.method!r} ({method_route(args).branch}) is not "
            f"wired into the captured step: its per-step segment tables have no slot in the graph's "
            f"static block; use train_step")


def capture_refusal(args) -> Optional[str]:
    """Why a step of ``args`` cannot be captured and stays with the eager ``train_step``
    (``GraphedTrainStep`` raises it, the drivers test it), or None.  The cut-and-paste family
    includes durmixrespscale and bare cutout."""
    if args.dataset in SPECTROGRAM_DATASETS:
        return "graphed step is wired for the 1D path"
    family = method_route(args).family
    if family == "latent":
        return LATENT_GRAPH_MESSAGE
    return cutpaste_graph_message(args) if family == "cutpaste" else None


def latent_fused_model(args, model, criterion, data, target_ohe, epoch):
    """The CNN_potes that runs a 1D ``latentmixup`` step inside its fused head (the blend happens in
    the tail kernel, ``CNN_potes.loss_and_logits(..., latent=...)``), or None when the step takes
    the drop-in path ``augment()`` + ``model(h, depth, 'second')``: any other model or a wrapped
    one, the SELC phase, targets that need a gradient, CPU tensors, ``args.model`` other than
    'Potes' (the only name whose depth is always 1) — or on request: ``args.latent_fused = False``
    or ``PCGMIX_NO_LATENT_FUSED`` in the environment (tests and A/B timing)."""
    if not latent_method(args) or getattr(args, "model", None) != "Potes":
        return None
    if not getattr(args, "latent_fused", True) or os.environ.get("PCGMIX_NO_LATENT_FUSED") is not None:
        return None
    return fused_loss_model(model, criterion, data, target_ohe, epoch)


def latent_host_step(args, data, target, target_ohe, step: int):
    """Host part of a fused 1D ``latentmixup`` step, exactly what ``augment()`` does in front of the
    model's first half (augmentations.py:1472-1497): gate, same-label partners, ``args.depth``,
    lambda from numpy's global stream; then the partners and their inverse go up in one copy.
    Returns ``(mix_dev, inv_dev, lam)``, or None when the gate rejects the step (``args.depth`` and
    numpy's stream untouched)."""
    labels = target.numpy() if not target.is_cuda \
        else (lambda: augmentations.labels_from_ohe(target_ohe))
    plan = augmentations.hostprep.latent_plan(args.method, args.model, labels, step, data.shape[0])
    if not plan.fired:
        return None
    args.depth = plan.depth
    with torch.cuda.device(data.device):
        mix_dev, inv_dev = augmentations.latent_partners(plan.mix, data.device)
    return mix_dev, inv_dev, float(plan.lam32)


def selc_phase(criterion, epoch) -> bool:
    """True when ``criterion`` is a SELCLoss past its turning point at ``epoch`` (train_model.py:72-80)."""
    return isinstance(criterion, SELCLoss) and epoch is not None and epoch > criterion.es


def selc_fused_model(model, criterion, data, target_ohe, epoch):
    """The CNN_potes that takes a SELC-phase step as head + SELC loss in one autograd node
    (``loss_and_logits(..., selc=...)``): the model ``fused_loss_model`` accepts in the CE phase,
    with ``SELCLoss.use_kernel`` on.  None otherwise (``criterion(...)`` then runs ``SELCFunction``)."""
    if not (selc_phase(criterion, epoch) and criterion.use_kernel):
        return None
    return fused_loss_model(model, criterion.CEloss, data, target_ohe, None)


def clips_outside_optimizer(args, optimizer) -> bool:
    """``clip_grad_value_`` as a pass of its own: ClipAdam and ClipSGD clip in their kernels."""
    return bool(args.grad_clip) and not isinstance(optimizer, _ClipUpdate)


def add_stats(stats: dict, loss, out, truth) -> None:
    """One step into ``stats``; ``truth`` is class indices (B,) or target rows (B, classes)."""
    with torch.no_grad():
        stats["loss_sum"] += loss
        stats["hits"] += (out.argmax(1) == (truth.argmax(1) if truth.dim() == 2 else truth)).sum()
        stats["seen"] += out.shape[0]


def train_step(args, model, batch, device, optimizer, scheduler, criterion, epoch, step_counter,
               stats: Optional[dict] = None, sync: Optional["FlatGradSync"] = None):
    """One iteration of the reference's batch loop (train_model.py:498-582) without host syncs.
    ``batch`` = (data, target, frames, wav, sig_qual, indices) as the reference's loaders yield
    it (dataloader_physionet.py:151-172).  Returns the loss tensor (on device, detached)."""
    data, target, frames, wav, _sig_qual, indices = batch
    data = data.to(device, non_blocking=True)
    target_ohe = F.one_hot(target, args.num_classes).to(device, non_blocking=True)
    aug = augmentations2d if args.dataset in SPECTROGRAM_DATASETS else augmentations
    latent = None
    fused = latent_fused_model(args, model, criterion, data, target_ohe, epoch)
    if fused is not None:
        # 1D latentmixup on the fused Potes path: the same launch chain as a plain step, the blend
        # of the hidden features happens inside the head's tail kernel
        latent = latent_host_step(args, data, target, target_ohe,
                                  int(augmentation_counter(args, step_counter).count))
    else:
        data, target_ohe, _, _ = aug.augment(args, data, target_ohe, frames, wav,
                                             augmentation_counter(args, step_counter), model, device, None,
                                             host_labels=target.numpy() if not target.is_cuda else None)
        fused = fused_loss_model(model, criterion, data, target_ohe, epoch) \
            if getattr(args, "depth", 0) == 0 else None
    selc_fused = selc_fused_model(model, criterion, data, target_ohe, epoch) \
        if fused is None and getattr(args, "depth", 0) == 0 else None
    if fused is not None:                   # head + loss as one autograd node (two launches, not four)
        loss, out = fused.loss_and_logits(data, target_ohe, latent=latent)
    elif selc_fused is not None:            # the same node with the SELC loss in the tail kernel
        loss, out = selc_fused.loss_and_logits(
            data, target_ohe,
            selc=(criterion.device_index(indices), criterion.soft_labels, criterion.momentum))
    else:
        out = model(data, depth=getattr(args, "depth", 0), pass_part="second")
        loss = criterion(out, target_ohe, indices, epoch, "train")
    args.depth = 0
    if sync is None:
        loss.backward()
    else:                                   # flat-buffer averaging instead of DDP hooks
        loss.backward(torch.full_like(loss, sync.backward_scale))
        if sync.params is None:
            sync.attach()
        sync.pack()
        sync.reduce_and_bind()
    if clips_outside_optimizer(args, optimizer):
        nn.utils.clip_grad_value_([p for p in model.parameters() if p.grad is not None],
                                  clip_value=args.grad_clip)
    reseed_device_rng(args, device)
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    if scheduler is not None:
        scheduler.step()
    step_counter.add()
    if stats is not None:
        add_stats(stats, loss.detach(), out, target_ohe)
    return loss.detach()


class _StaticBlock:
    """Everything small the captured step reads and the host decides per step, in ONE static block
    of float32 words: ``dev`` on the device and ``host``, its image in host memory.  A plain splice
    carries the image with its index block (``pcgmix_ctx_set_payload``: no copy of its own), other
    steps upload it with one H2D.  Layout, the same in both copies:

        words 0-1     dropout key (bits)
        words 2-3     unused
        words 4-11    the optimiser's eight scalars (``ClipAdam.next_hyper`` / ``ClipSGD.next_hyper``)
        from word 12  the class labels, one byte each, padded to a 16-byte granule
        behind them   the float targets (B, classes), padded to 4 words

    ``key``, ``hyper``, ``labels`` and ``targets`` are views of ``dev``; ``host_key`` ... of ``host``."""

    def __init__(self, batch_size: int, num_classes: int, device):
        self.shape = (batch_size, num_classes)
        self.targets_at = 12 + (batch_size + 15) // 16 * 4       # word offset of the float targets
        self.dev = torch.zeros(self.targets_at + (batch_size * num_classes + 3) // 4 * 4, device=device)
        self.host = np.zeros(self.dev.numel(), dtype=np.float32)
        self.key, self.hyper, self.labels, self.targets = self._views(self.dev, torch.int32, torch.uint8)
        self.host_key, self.host_hyper, self.host_labels, self.host_targets = \
            self._views(self.host, np.uint32, np.uint8)
        self.targets[:, 0] = 1                                 # one-hot rows until a step's own targets arrive

    def _views(self, words, key_dtype, byte_dtype):
        B, classes = self.shape
        return (words[0:2].view(key_dtype), words[4:12], words[12:self.targets_at].view(byte_dtype)[:B],
                words[self.targets_at:self.targets_at + B * classes].reshape(B, classes))

    def payload_bytes(self, labels_mode: bool) -> int:
        """What a step sends: up to the end of the label bytes, or the whole block."""
        return self.targets_at * 4 if labels_mode else self.host.nbytes


class GraphedTrainStep:
    """The same step as ``train_step`` with forward + loss + backward + gradient clipping
    captured once in a hipGraph (torch.cuda.CUDAGraph) and replayed: at bs=256 the eager Potes
    step issues ~40 launches and is host-bound (~1 ms wall for ~0.45 ms of GPU work).

    Stays eager, around the replay: the augmentation (its index data and lambda are kernel
    arguments that change every step; it writes straight into the graph's static input — plain
    splices, and the saliency-guided ones around the frozen model's own captured pass) and the
    scheduler.  The ClipAdam update is the graph's last node: OneCycleLR moves lr AND beta1 every
    step, so the captured launch reads its eight scalars from device memory (they travel with the
    step's payload); with op='SGD' ClipSGD takes the same place (lr and momentum move).  Under torch.distributed pass the UNWRAPPED model: gradients are packed into
    one flat buffer inside the graph, averaged by one eager all-reduce after the replay
    (``FlatGradSync``) — DDP's hooks cannot be captured — and the update is a SECOND small graph
    replayed behind the collective.  Needs static shapes (the loaders use drop_last=True).

    A step is captured for ONE phase of a ``SELCLoss``: ``selc=False`` (default) the plain-CE one,
    ``selc=True`` the phase past the turning point (train_model.py:72-80) — the fused Potes head with
    the SELC tail kernel, ``SELCFunction`` behind every other model.  The batch's sample indices go
    to a static int64 buffer before every replay (a copy of their own; the static block keeps its
    layout).  ``prepare`` refuses an epoch of the other phase."""

    use_tape = True      # direct launches instead of the graph replay where the step allows it
    _TAPE_LAUNCHES = ("pcgmix_potes_stack_fwd_save_f32", "pcgmix_potes_head_loss_fwd_f32",
                      "pcgmix_potes_head_loss_bwd_f32", "pcgmix_potes_stack_bwd_mask_f32",
                      "pcgmix_adam_clip_multi_reduce_dev_f32")

    def __init__(self, args, model, optimizer, scheduler, criterion, device, batch_size, channels,
                 sig_len, sync: Optional[FlatGradSync] = None, *, selc: bool = False):
        refusal = capture_refusal(args)
        if refusal is not None:
            raise NotImplementedError(refusal)
        if selc and not hasattr(criterion, "soft_labels"):
            raise ValueError("selc=True needs a criterion with soft_labels (SELCLoss)")
        self.args, self.model, self.opt, self.sched = args, model, optimizer, scheduler
        self.selc, self.crit = bool(selc), criterion
        # placeholder indices of the warm-up; every step's own arrive in ``prepare``
        self.index = torch.arange(batch_size, device=criterion.soft_labels.device) if selc else None
        self.ce = criterion.CEloss if hasattr(criterion, "CEloss") else criterion
        self.es = getattr(criterion, "es", None)
        self.device = device
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.x = torch.zeros(batch_size, channels, sig_len, device=device)
        self.block = _StaticBlock(batch_size, args.num_classes, device)
        self.t_u8, self.t = self.block.labels, self.block.targets
        self._rows = np.arange(batch_size)
        # Hard targets (everything but '(mixAll)') reach the fused Potes head+loss as class bytes:
        # the payload is then 48 + B bytes and travels in the splice kernel's ARGUMENTS with the
        # index block — no copy at all in front of the replay; other models / soft targets read the
        # float block (one H2D).
        self.labels_mode = bool(                               # same test as _fwd_bwd's
            isinstance(self.ce, CELoss) and not method_route(args).soft_targets
            and args.num_classes <= 255
            and fused_loss_model(model, self.ce, self.x, self.t, None) is not None)
        self._pay_bytes = self.block.payload_bytes(self.labels_mode)
        self.sync = sync
        self.bwd_seed = torch.full((), sync.backward_scale if sync else 1.0, device=device)
        self.rnd = self._dropout_buffer(batch_size)
        # The optimiser update is the graph's last node when nothing has to happen between
        # backward and update (no gradient all-reduce) and the optimiser can read its scalars
        # from the static block (ClipAdam, ClipSGD).
        # (``adam_in_graph``: the name is older than ClipSGD, which takes the same place)
        self.adam_in_graph = isinstance(optimizer, _ClipUpdate) and optimizer.can_capture() \
            and device.type == "cuda"
        self.graph_update = None        # with a sync: the update as a second graph behind the all-reduce
        self._warm_up()
        tape, fold = self._capture()
        self._adopt_tape(tape, fold)
        if self.adam_in_graph and sync is not None:
            self._capture_update_graph()

    def _dropout_buffer(self, batch_size):
        """Dropout inside a captured region costs two extra fill launches per replay (torch's
        graph-safe Philox state) on top of the mask kernels.  The Potes head reads random BYTES
        instead, from a static buffer that the conv stack's forward kernel fills as a side job
        (``pcgmix_potes_stack_fwd_save_f32``: a keyed counter hash).  The key is drawn on the host
        from torch's device generator — (seed, offset), offset advanced by 4 per step — so
        ``torch.cuda.manual_seed`` behaves as with nn.Dropout, the reference's reseeding before
        every optimiser step (``reseed_device_rng``) included.  Returns that buffer (handed to the
        model with the key's device words), or None for another model."""
        inner = self.model.module if hasattr(self.model, "module") else self.model
        if not (isinstance(inner, models.CNN_potes) and self.device.type == "cuda"):
            return None
        K = inner.dimreduc.in_features
        drop = inner.cnn1[1][3] if len(inner.cnn1[1]) > 3 else None
        n_rnd = models.head_dropout_bytes(batch_size, K, float(drop.p) if drop else 0.0)
        rnd = torch.empty((n_rnd + 15) // 16 * 16, dtype=torch.uint8, device=self.device)
        inner.dropout_bytes = rnd
        inner.dropout_key = self.block.key
        return rnd

    def _warm_up(self):
        """Three passes on the all-zero placeholder batch, on a side stream: they must leave no
        trace.  Weights are not updated (no optimiser step); BatchNorm running statistics and
        num_batches_tracked, and the device RNG stream the dropout masks come from, are put back
        afterwards, so a graphed run starts from exactly the state an eager run starts from."""
        import warnings
        device, sync = self.device, self.sync
        buffers = [(b, b.detach().clone()) for b in self.model.buffers()]
        if self.selc:                                   # the warm-up passes move the soft labels
            buffers.append((self.crit.soft_labels, self.crit.soft_labels.detach().clone()))
        rng = torch.cuda.get_rng_state(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        warn_always = torch.is_warn_always_enabled()
        torch.set_warn_always(True)                     # the stream-mismatch warning is a warn-once
        try:
            with warnings.catch_warnings(record=True) as caught, torch.cuda.stream(side):
                warnings.simplefilter("always")         # warm-up off the capture (no weight update)
                for _ in range(3):
                    self.opt.zero_grad(set_to_none=True)
                    self._fwd_bwd()
                if sync is not None and sync.params is None:    # once per sync: a second captured
                    sync.attach()                               # step (PipelinedTrainStep) shares it
                if self.adam_in_graph:
                    self.opt.prepare_capture([p for p in self.params if p.grad is not None])
        finally:
            torch.set_warn_always(warn_always)
        torch.cuda.current_stream(device).wait_stream(side)
        stale = [w for w in caught if "AccumulateGrad node's stream does not match" in str(w.message)]
        for w in caught:
            if w not in stale:
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        if stale:
            # An autograd graph built in an earlier pass over these parameters is still alive (a loss
            # or output tensor kept by the caller): its AccumulateGrad nodes belong to the stream of
            # that pass.  Backward under capture would then make THAT stream wait on an event of the
            # capturing stream; when it is the legacy default stream, hipStreamEndCapture walks a
            # null stream object and the process dies with SIGSEGV inside libamdhip64
            # (hip::Stream::EndCapture; reproduced with torch ops alone:
            # profiles/probes/capture_defer_probe.py 'puretorch').  Refuse here,
            # before any capture has begun.
            self.opt.zero_grad(set_to_none=True)
            raise RuntimeError(
                "GraphedTrainStep: an autograd graph from an earlier forward pass over this model's "
                "parameters is still alive (e.g. a non-detached loss/output tensor is still "
                "referenced).  Its AccumulateGrad nodes are bound to that pass's stream and would pull "
                "it into the capture (on ROCm: a crash in hipStreamEndCapture).  Drop those tensors "
                "(or .detach() them) before building the captured step.")
        with torch.no_grad():
            for b, saved in buffers:
                b.copy_(saved)
        torch.cuda.set_rng_state(rng, device)
        self.opt.zero_grad(set_to_none=True)

    def _capture(self):
        """Capture forward + loss + backward (+ the update when ClipAdam is the last node) into
        ``self.graph``.  Returns ``(tape, fold)``: the library launches recorded on the way (or
        None) and the conv stack's deferred-reduction record (or None)."""
        from . import _lib
        sync = self.sync
        if sync is not None and sync.world > 1:
            # no collective may be in flight while the graph is captured, and every rank must
            # capture (or fail) together
            torch.cuda.synchronize(self.device)
            sync.dist.barrier()
        self.graph = torch.cuda.CUDAGraph()
        # One rank, ClipAdam as the graph's last node: the conv stack's gradient reduction moves
        # into the optimiser launch (models.PotesStackFunction.defer_reduce).
        fold = {} if (self.adam_in_graph and sync is None
                      and os.environ.get("PCGMIX_NO_REDUCE_FOLD") is None) else None
        # The fused Potes step is five library launches and nothing else (forward, head + loss,
        # feature pass, weight gradients, reduction + update: profiles/r3_train_step_timeline.txt).
        # They are recorded while the capture makes them; ``launch`` then issues them DIRECTLY on the
        # current stream instead of replaying the hipGraph — the graph's launch leaves ~5 us of idle
        # GPU per step that back-to-back kernel launches do not (130.8 -> 125.7 us,
        # profiles/probes/tape_vs_graph.py).  The graph object stays: it owns the buffers.
        want_tape = (self.use_tape and fold is not None and self.labels_mode
                     and isinstance(self.model, models.CNN_potes)
                     and os.environ.get("PCGMIX_NO_TAPE") is None)
        tape = [] if want_tape else None
        # thread_local: HIP calls of other threads (RCCL's watchdog) must not abort the capture
        with _lib.capture_without_gc(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            models.PotesStackFunction.defer_reduce = fold
            _lib.TAPE = tape
            try:
                self.loss, self.out = self._fwd_bwd()
                if self.adam_in_graph and sync is None:
                    self.opt.capture_update(self.block.hyper, deferred=fold)
            finally:
                models.PotesStackFunction.defer_reduce = None
                _lib.TAPE = None
        return tape, fold

    def _adopt_tape(self, tape, fold) -> None:
        """``self.tape``: the recorded launches when they are the whole capture, else None."""
        self.tape = None
        # (a tape is recorded only with the update in the graph; the fifth launch is the optimiser's
        # own — _TAPE_LAUNCHES names ClipAdam's)
        if tape is not None and [t[0] for t in tape] == [*self._TAPE_LAUNCHES[:4], self.opt.REDUCE_LAUNCH] \
                and self._tape_covers_capture(tape, fold):
            import ctypes
            # pointer tables are snapshotted: ClipAdam re-uses its ctypes arrays for the next capture
            # (a second slot of PipelinedTrainStep), a graph node would have copied them too
            snap = lambda v: type(v)(*v) if isinstance(v, ctypes.Array) else v      # noqa: E731
            self.tape = [(name, fn, tuple(snap(v) for v in a[:-1])) for name, fn, a in tape]

    def _capture_update_graph(self) -> None:
        """N > 1: [forward + backward + pack] | one eager all-reduce | [clip + Adam].  The update
        reads the averaged gradients through views of the flat buffer and its eight scalars from
        the static block — an N-rank step issues exactly the launches of the one-rank step plus
        the collective, and no Python optimiser code runs between them."""
        from . import _lib
        for p, v in zip(self.sync.params, self.sync.views):
            p.grad = v
        self.graph_update = torch.cuda.CUDAGraph()
        with _lib.capture_without_gc(), torch.cuda.graph(self.graph_update, capture_error_mode="thread_local"):
            self.opt.capture_update(self.block.hyper)

    def _tape_covers_capture(self, tape, fold) -> bool:
        """The tape replaces the graph only if the five recorded launches ARE the capture: no
        torch-side kernel may sit between them (an AccumulateGrad clone of a head gradient, a
        dense copy of a stride-mismatched gradient — the tape would skip it and the update would
        read stale memory).  Checked at build time: every gradient the captured update reads must
        be (a view of) the very buffer one of the recorded launches was handed — the backward
        launches' outputs, or the deferred-reduction block the update launch fills."""
        import ctypes
        import warnings
        written = set()
        for _name, _fn, a in tape:
            for v in a[:-1]:
                if isinstance(v, int) and v > 4096:
                    written.add(v)
                elif isinstance(v, ctypes.c_void_p) and v.value:
                    written.add(v.value)
        for p, g in self.opt._captured():
            # (gradients are views: the head's small ones of one block, the stack's of the deferred
            # block — compare the storage a launch was handed, not the view's own address)
            if g is not p.grad or g.untyped_storage().data_ptr() not in written:
                warnings.warn("GraphedTrainStep: the capture holds work besides the five library "
                              "launches (a gradient of %s is not written by them directly); "
                              "replaying the hipGraph instead of launching directly"
                              % (tuple(p.shape),))
                return False
        return True

    def _fwd_bwd(self):
        fused = fused_loss_model(self.model, self.ce, self.x, self.t, None) \
            if isinstance(self.ce, CELoss) else None
        if self.selc:
            selc = (self.index, self.crit.soft_labels, self.crit.momentum)
            if fused is not None:
                loss, out = fused.loss_and_logits(self.x, self.t, selc=selc)
            else:
                out = self.model(self.x, depth=0, pass_part="second")
                loss = SELCFunction.apply(out, *selc)
        elif fused is not None:
            loss, out = fused.loss_and_logits(self.x, self.t_u8 if self.labels_mode else self.t)
        else:
            out = self.model(self.x, depth=0, pass_part="second")
            loss = self.ce(out, self.t)
        loss.backward(self.bwd_seed)
        if self.sync is not None and self.sync.params is not None:
            self.sync.pack()
        elif clips_outside_optimizer(self.args, self.opt):
            nn.utils.clip_grad_value_(self.params, clip_value=self.args.grad_clip)
        return loss.detach(), out.detach()

    def _next_key(self) -> None:
        """This step's dropout key from torch's device generator (host only, no launch)."""
        z = models.next_dropout_key(self.device)
        self.block.host_key[0] = z & 0xFFFFFFFF
        self.block.host_key[1] = z >> 32

    def step(self, batch, epoch, step_counter, stats: Optional[dict] = None, next_batch=None):
        """One training step: ``prepare`` (augmentation into the static input, payload) then
        ``launch`` (replay, optimiser, scheduler, counters) on the current stream.  ``next_batch``
        is ``PipelinedTrainStep.step``'s lookahead: accepted and unused, one call form for both."""
        self.prepare(batch, epoch, step_counter)
        return self.launch(step_counter, stats)

    def prepare(self, batch, epoch, step_counter):
        """First half of a step, everything in front of the replay: the host image of the static
        block (targets, dropout key, Adam scalars — read from generator / optimiser state as the
        PREVIOUS step's ``launch`` left it, so prepare(k+1) must follow launch(k) on the host) and
        the augmentation launches, which write this object's static input and block on the
        CURRENT stream.  ``PipelinedTrainStep`` runs it on a side stream for batch k+1 while the
        graph of batch k replays."""
        from . import hostprep, _lib, saliency as _saliency
        data, target, frames, wav, _sq, idx = batch
        if (self.es is not None and epoch > self.es) != self.selc:
            raise NotImplementedError(
                f"this step was captured for the {'SELC' if self.selc else 'plain-CE'} phase and epoch "
                f"{epoch} belongs to the other one; capture a step with selc={not self.selc}")
        args, block = self.args, self.block
        data = data.to(self.device, non_blocking=True)
        if self.selc:                                   # host-checked, then one copy of its own
            self.index.copy_(self.crit.device_index(idx), non_blocking=True)
        frames_np = augmentations._as_numpy_frames(frames)
        B, C, T = data.shape
        step = int(augmentation_counter(args, step_counter).count)
        # host image of the static block: one-hot float targets, dropout key, Adam scalars
        labels_np = target.numpy() if not target.is_cuda else target.cpu().numpy()
        if self.labels_mode:
            block.host_labels[:] = labels_np
        else:
            block.host_targets.fill(0.0)
            block.host_targets[self._rows, labels_np] = 1.0
        if self.rnd is not None and self.model.training:
            self._next_key()
        if self.adam_in_graph:
            self.opt.next_hyper(block.host_hyper)
        recipe = hostprep.plain_recipe(args.method, False)
        srec = hostprep.salopt_recipe(args.method) if recipe is None else None
        lib, ctx = _lib.load(), augmentations.step_context(data.device.index)
        _lib.check(lib.pcgmix_ctx_set_payload(ctx, block.host.ctypes.data, self._pay_bytes,
                                              block.dev.data_ptr()), "pcgmix_ctx_set_payload")
        plan, t_ohe = hostprep.MixPlan(fired=False), None
        if recipe is not None and B > 0:                # plain splice: one library call
            fired = augmentations.gate_passes(recipe, args.method, step, data.device.index)
            if fired:                                   # ... which carries the payload along
                augmentations.splice_plain(recipe, data, labels_np, frames_np, step, out=self.x)
        elif srec is not None and B > 0:
            # Saliency-guided splice with same-label partners (BASELINE config 3; augmentations.py:
            # 874-928): seed + boundaries + this step's payload in the arguments of one launch,
            # the frozen saliency model's captured pass, then search + splice straight into the
            # training graph's static input — the whole step stays on the stream, no host wait.
            fired = hostprep.gate_fires(args.method, step)
            if fired:
                g = _saliency.step_graph(args, data, args.num_classes)
                if g is None:
                    raise RuntimeError("the captured saliency pass is unavailable (saliency.USE_GRAPHS "
                                       "is off or the stream is capturing)")
                with torch.cuda.device(self.device):
                    augmentations._salopt_step(srec, g, data, None, labels_np, frames_np, step,
                                               out=self.x)
        else:
            if method_route(args).family != "passthrough":
                plan = hostprep.make_plan(args.method, labels_np, frames_np, wav, step, B, C,
                                          sample_rate=getattr(args, "sample_rate", None), sig_len=T)
            fired = plan.fired
            if fired:
                sal = None
                if plan.salopt_mode is not None:        # salopt with '(samePCG)' & co.: general path
                    t_ohe = F.one_hot(target, args.num_classes).to(self.device, non_blocking=True)
                    sal = _saliency.get_saliency_maps(args, self.device, data, t_ohe, frames_np)
                augmentations.apply_plan(plan, data, frames_np, sal, out=self.x)
        if not fired:
            self.x.copy_(data, non_blocking=True)
        # any other step: the payload goes on its own (no-op when the splice took it)
        _lib.check(lib.pcgmix_ctx_flush_payload(
            ctx, torch.cuda.current_stream(self.device).cuda_stream), "pcgmix_ctx_flush_payload")
        if plan.fired and plan.mix_all:                 # float blend of the one-hot rows
            if t_ohe is None:
                t_ohe = F.one_hot(target, args.num_classes).to(self.device, non_blocking=True)
            self.t.copy_(augmentations.blend_targets(t_ohe, plan))

    def launch(self, step_counter, stats: Optional[dict] = None):
        """Second half: replay the captured forward + backward (+ update), the gradient all-reduce
        and update graph under torch.distributed, scheduler, step counter, statistics."""
        if self.tape is not None:
            import ctypes
            st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for name, fn, a in self.tape:
                err = fn(*a, st)
                if err:
                    from . import _lib
                    _lib.check(err, name)
        else:
            self.graph.replay()
        reseed_device_rng(self.args, self.device)
        if self.graph_update is not None:
            self.sync.reduce_and_bind()
            self.graph_update.replay()
        elif not self.adam_in_graph:
            if self.sync is not None:
                self.sync.reduce_and_bind()
                if clips_outside_optimizer(self.args, self.opt):
                    nn.utils.clip_grad_value_(self.sync.params, clip_value=self.args.grad_clip)
            self.opt.step()
        if self.sched is not None:
            self.sched.step()
        step_counter.add()
        if stats is not None:
            add_stats(stats, self.loss, self.out, self.t_u8 if self.labels_mode else self.t)
        return self.loss


class PipelinedTrainStep:
    """Two ``GraphedTrainStep`` slots over the same model / optimiser, used alternately so that the
    augmentation of batch k+1 runs on a side stream WHILE the captured training graph of batch k
    replays on the main stream.

    The augmentation of a batch depends on that batch, its labels and the step count only
    (train_model.py:507: ``augment(args, data, target_ohe, frames, wav, step_counter, ...)``), never
    on the weights being trained — the saliency-guided methods use a FROZEN model
    (saliency.py:26-51) — so it can run ahead by one batch without changing a single value; it is
    the data-loader prefetch the reference does not have.  For BASELINE config 3 the augmentation
    (frozen forward + input gradient + search + splice, ~160 us) is as long as the training graph
    (~147 us) and both are issue/latency-bound kernels that leave the other room: measured
    309 -> 225 us per step with the two on separate streams (profiles/probes/overlap_probe.py);
    for the plain splice (10 us) the cross-stream hand-overs cost more than the overlap gains
    (148 -> 166 us), so ``train_model`` uses this class for the saliency-guided methods only.

    Host order is unchanged — prepare(k+1) follows launch(k), so dropout keys, Adam scalars,
    scheduler and step counter advance exactly as in the sequential loop — only the STREAM of the
    augmentation launches differs.  Buffer hazards: slot s's static input / block are rewritten
    by prepare(k+2) only after the replay of batch k (same slot) has finished (event), and a replay
    waits for its slot's prepare (event).

        pipe = PipelinedTrainStep(args, model, opt, sched, crit, device, B, C, T, sync=...)
        for batch, nxt in pipe.pairs(loader):           # or: pipe.step(batch, epoch, sc, stats, nxt)
            pipe.step(batch, epoch, step_counter, stats, next_batch=nxt)
    """

    def __init__(self, *a, **kw):
        self.slots = [GraphedTrainStep(*a, **kw), GraphedTrainStep(*a, **kw)]
        self.device = self.slots[0].device
        self.side = torch.cuda.Stream(self.device)
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]     # slot prepared (side stream)
        self.done = [torch.cuda.Event(), torch.cuda.Event()]      # slot's replay finished (main stream)
        self._fetched = torch.cuda.Event()
        self.cur = 0
        self.prepared = None            # id() of the batch already prepared into slot `cur`

    @property
    def loss(self):
        return self.slots[self.cur ^ 1].loss          # the step that ran last

    @property
    def x(self):
        return self.slots[0].x                        # (shape of the static input)

    @staticmethod
    def pairs(loader):
        """(batch, next batch or None) over ``loader`` — the one-batch lookahead ``step`` wants."""
        it = iter(loader)
        try:
            cur = next(it)
        except StopIteration:
            return
        for nxt in it:
            yield cur, nxt
            cur = nxt
        yield cur, None

    def _prepare_on_side(self, slot, batch, epoch, step_counter, fetched):
        self.side.wait_event(fetched)                   # the batch itself (loader gather, main stream)
        self.side.wait_event(self.done[slot])           # the slot's previous replay has read its buffers
        with torch.cuda.stream(self.side):
            self.slots[slot].prepare(batch, epoch, step_counter)
            self.ready[slot].record(self.side)
        if batch[0].is_cuda:    # allocated on the main stream (loader gather), read on the side stream
            batch[0].record_stream(self.side)

    def step(self, batch, epoch, step_counter, stats: Optional[dict] = None, next_batch=None):
        main = torch.cuda.current_stream(self.device)
        s = self.cur
        if self.prepared != id(batch):                  # first step, or the caller gave no lookahead
            # inline, on the main stream.  Both slots' prepares share the cached saliency graph
            # (seed, boundaries, activations, map) and the per-device step context (search
            # workspace): the side stream's prepare(k+1) must not start before THIS prepare's last
            # kernel has read them, so the hand-over point below is recorded behind it.
            self.slots[s].prepare(batch, epoch, step_counter)
        else:
            main.wait_event(self.ready[s])
        if next_batch is not None:
            # next_batch exists already (the caller's lookahead fetched it before this call): mark the
            # point on the main stream BEFORE this step's graph — and behind an inline prepare — so
            # that the side stream waits for the batch (and the shared saliency buffers) and not for
            # the graph it is meant to overlap
            self._fetched.record(main)
        self.prepared = None
        loss = self.slots[s].launch(step_counter, stats)
        self.done[s].record(main)
        if next_batch is not None:
            self._prepare_on_side(s ^ 1, next_batch, epoch, step_counter, self._fetched)
            self.prepared = id(next_batch)
        self.cur = s ^ 1
        return loss


def captured_step_class(args, pipeline: bool = True):
    """Two pipelined slots for the saliency-guided methods (297 -> 258 us per step), one slot for
    the rest (plain splice: 148 -> 166 us if pipelined, profiles/r3_pipeline_ab.txt); the reasons
    are in ``PipelinedTrainStep``'s docstring."""
    return PipelinedTrainStep if pipeline and "(salopt" in args.method else GraphedTrainStep


def _no_epoch_step():
    return None


class _EpochStep:
    """(key, captured step) kept on the model by ``train_epoch``.  A copy or a pickle of the model
    must not drag the graph along: both see ``None`` in its place."""
    __slots__ = ("key", "step")

    def __init__(self, key, step):
        self.key, self.step = key, step

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_no_epoch_step, ())


def _epoch_graphed_step(args, model, optimizer, scheduler, criterion, device, epoch, batch):
    """The captured step ``train_epoch`` replays instead of calling ``train_step``, or None when
    the step has to stay eager.  A caller of the reference's ``train_epoch`` hands over exactly
    what ``GraphedTrainStep`` needs; the graph is built at the first batch and kept for as long as
    model, optimiser, scheduler, criterion, method and batch shape stay the same objects/values
    (the reference creates them once per run, train_model.py:293-410).  ``args.hipgraph = False``
    switches it off.  Eager: CPU, whatever ``capture_refusal`` names, wrapped (DataParallel/DDP)
    models, a criterion other than ``SELCLoss``, an active process group (use ``train_model()`` /
    ``FlatGradSync`` there).  The step belongs to one phase of the criterion: at the first epoch past
    ``criterion.es`` the plain-CE step is dropped and a SELC-phase one is captured in its place
    (``ClipAdam.prepare_capture`` carries the live step count across)."""
    if not getattr(args, "hipgraph", True) or device.type != "cuda":
        return None
    if capture_refusal(args) is not None or not isinstance(criterion, SELCLoss):
        return None
    if not isinstance(model, (models.CNN_potes, models.ResNet9_myrtle)):
        return None
    if rank_and_world()[1] > 1:
        return None
    data = batch[0]
    if data.dim() != 3:
        return None
    phase = epoch > criterion.es
    key = (id(optimizer), id(scheduler), id(criterion), tuple(data.shape), args.method,
           args.num_classes, device, phase)
    hit = model.__dict__.get("_pcgmix_epoch_step")      # kept ON the model: dies with it (a module-
    if hit is None or hit.key != key:                   # level table would keep model and graph alive)
        B, C, T = data.shape
        cls = captured_step_class(args)
        model.__dict__["_pcgmix_epoch_step"] = hit = None   # the other phase's graph goes first
        hit = _EpochStep(key, cls(args, model, optimizer, scheduler, criterion, device, B, C, T,
                                  selc=phase))
        model.__dict__["_pcgmix_epoch_step"] = hit
    return hit.step


def _run_epoch(args, model, batches, device, optimizer, scheduler, criterion, epoch, step_counter,
               captured, eager, lrs: Optional[list] = None):
    """The batches of one epoch (train_model.py:496-586) for ``train_epoch`` and ``train_model``.
    ``captured(...same arguments as _epoch_graphed_step...)`` gives the captured step or None at the
    first batch; it runs every batch of its static shape, with one batch of lookahead.  ``eager``
    (``train_step`` or None) runs the others; None makes such a batch an error (``train_model``
    under a captured step: an eager step there would skip ``FlatGradSync``'s gradient averaging).
    ``lrs`` collects the learning rate in front of every step.  Returns (stats, steps run)."""
    model.train()
    torch.manual_seed(args.seed * 635410 + step_counter.count)      # :497 fixes this epoch's shuffle
    stats = {"loss_sum": torch.zeros((), device=device),
             "hits": torch.zeros((), device=device, dtype=torch.long), "seen": 0}
    n_batches, graphed = 0, None

    def fits(b):
        return tuple(b[0].shape) == tuple(graphed.x.shape)

    for batch, nxt in PipelinedTrainStep.pairs(batches):            # one batch of lookahead
        if lrs is not None:
            lrs.append(optimizer.param_groups[0]["lr"])
        if n_batches == 0:
            graphed = captured(args, model, optimizer, scheduler, criterion, device, epoch, batch)
        if graphed is not None and fits(batch):
            last = not step_counter.count + 1 < getattr(args, "num_steps", float("inf"))   # :584-586
            ahead = nxt if (not last and nxt is not None and fits(nxt)) else None
            graphed.step(batch, epoch, step_counter, stats, next_batch=ahead)
        elif eager is not None:
            eager(args, model, batch, device, optimizer, scheduler, criterion, epoch, step_counter, stats)
        else:
            raise RuntimeError(f"batch of shape {tuple(batch[0].shape)} does not fit the captured "
                               f"step's {tuple(graphed.x.shape)}")
        n_batches += 1
        if not step_counter.count < args.num_steps:                  # :584-586
            break
    return stats, n_batches


def train_epoch(args, model, train_loader, device, optimizer, scheduler, criterion, epoch,
                step_counter, variability_counter=None, EXPERIMENT_ARGS=None):
    """Reference signature (train_model.py:490).  Returns (mean loss, accuracy, lr per step).
    On a GPU the step is the captured one (``_epoch_graphed_step``): the same values as
    ``train_step`` at three times its rate; batches of another shape (a loader without
    drop_last) fall back to the eager step."""
    lrs = []
    stats, n_batches = _run_epoch(args, model, train_loader, device, optimizer, scheduler, criterion,
                                  epoch, step_counter, _epoch_graphed_step, train_step, lrs)
    loss = float(stats["loss_sum"]) / max(1, n_batches)              # the only host syncs
    acc = float(stats["hits"]) / max(1, stats["seen"])
    return loss, acc, lrs


class performance_metrics_class:
    """The reference's result collector (train_model.py:178-195): a dict of lists with the same
    thirteen keys and the same ``add(key, value)``."""

    def __init__(self):
        self.dict = {k: [] for k in ("steps", "epochs", "times", "train_loss", "train_accuracy",
                                     "test_loss", "test_accuracy", "test_specificity",
                                     "test_sensitivity", "test_precision", "test_recall", "test_f1",
                                     "test_rocauc")}

    def add(self, string, value):
        self.dict[string].append(value)


FUSED_EVAL = True    # evaluation through the HIP eval kernels (predict_recordings) where they apply
                     # (False: the torch formulation below, for A/B; a switch like models.FUSED_BN)
EVAL_MAX_CLASSES = 8


class EvalPlan:
    """Host-side plan of one evaluation pass (train_model.py:615-632): from the recording name and
    the label of every heart cycle, in the order the loader yields them, the recordings numbered by
    first appearance (``names``), the label of each recording's FIRST cycle (``labels``), its cycle
    count (``counts``), and the CSR pair the segments kernel walks: ``order`` (N) int32 — the cycle
    rows grouped by recording, within a recording in loader order (a stable permutation) — and
    ``rec_start`` (R+1) int32.  ``cycle_labels`` (N) uint8 are the per-cycle label bytes of the loss.

    ``device_side(device, C)`` holds the device copies of ``order``, ``rec_start`` and the label bytes
    and the (N,C) / (N) / (R,C) buffers of the pass: uploaded or allocated once per (device, C),
    counted in ``uploads``.  ``ResidentLoader(shuffle=False)`` is immutable and yields the same order
    every time: its plan is cached on the loader (``loader.eval_plan``)."""

    def __init__(self, names, labels):
        names = np.asarray(list(names), dtype=object)
        lab = np.asarray(labels, dtype=np.int64).reshape(-1)
        if len(names) != len(lab):
            raise ValueError("EvalPlan: one label per recording name")
        if len(lab) and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("EvalPlan: labels must fit a byte")
        self.n = int(len(lab))
        if self.n:
            _uniq, first, inv = np.unique(names.astype(str), return_index=True, return_inverse=True)
            by_first = np.argsort(first, kind="stable")          # recording id = rank of its first cycle
            rank = np.empty(len(first), dtype=np.int64)
            rank[by_first] = np.arange(len(first))
            ids = rank[np.asarray(inv).reshape(-1)]
            first = first[by_first]
        else:
            ids, first = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.ids = ids
        self.names = [str(names[i]) for i in first]
        self.labels = lab[first]
        self.counts = np.bincount(ids, minlength=len(first)).astype(np.int64)
        self.order = np.argsort(ids, kind="stable").astype(np.int32)
        self.rec_start = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.cycle_labels = lab.astype(np.uint8)
        self.validate()
        self.uploads = 0
        self._device = {}

    @property
    def recordings(self) -> int:
        return len(self.names)

    def validate(self) -> None:
        """What the segments kernel relies on (it clamps besides): ``order`` a permutation of the N
        rows, ``rec_start`` non-decreasing from 0 to N."""
        if not np.array_equal(np.sort(self.order), np.arange(self.n)):
            raise ValueError("EvalPlan: order is not a permutation of the cycle rows")
        rs = self.rec_start
        if rs[0] != 0 or rs[-1] != self.n or (np.diff(rs) < 0).any():
            raise ValueError("EvalPlan: rec_start is not a CSR offset vector over the cycle rows")

    def device_side(self, device, C: int):
        key = (str(device), int(C))
        side = self._device.get(key)
        if side is None:
            N, R = self.n, self.recordings
            side = types.SimpleNamespace(
                order=torch.from_numpy(self.order).to(device),
                rec_start=torch.from_numpy(self.rec_start).to(device),
                labels=torch.from_numpy(self.cycle_labels).to(device),
                prob=torch.empty((N, C), dtype=torch.float32, device=device),
                loss_rows=torch.empty(N, dtype=torch.float32, device=device),
                vote=torch.empty(N, dtype=torch.uint8, device=device),
                # [loss_rec f64 (R) | mean_p f32 (R,C) | votes i32 (R,C)]: one buffer, one copy to the host
                out=torch.empty(8 * R + 8 * R * C, dtype=torch.uint8, device=device))
            self.uploads += 3
            self._device[key] = side
        return side


def _eval_labels_ok(labels, C: int) -> None:
    labels = np.asarray(labels)
    if labels.size and (labels.min() < 0 or labels.max() >= C):
        raise ValueError(f"predict_recordings: label outside [0, {C})")


def fused_eval_applies(args, device, criterion) -> bool:
    """Whether ``test_data_accuracy`` builds its metrics from ``predict_recordings``: a GPU, at most
    eight classes, and a loss the row rule computes — none, ``CELoss``, or ``SELCLoss`` (whose
    'test' mode is its ``CEloss``)."""
    return (FUSED_EVAL and torch.device(device).type == "cuda" and 1 <= args.num_classes <= EVAL_MAX_CLASSES
            and (criterion is None or type(criterion) in (CELoss, SELCLoss)))


@torch.no_grad()
def predict_recordings(args, model, loader, device, criterion=None):
    """Recording-level inference (train_model.py:591-647) through the HIP eval kernels: per batch the
    model's logits -> softmax, row loss and vote in the launch that forms them
    (``pcgmix_potes_head_eval_f32`` behind the conv stack for an unwrapped ``CNN_potes`` on its fused
    path, ``pcgmix_eval_rows_f32`` behind ``model(data)`` for everything else), rows landing at the
    batch's offset in the plan's buffers; then ONE ``pcgmix_eval_segments_f32`` launch and ONE copy to
    the host.  Nothing synchronises per batch.  The per-recording sums run in loader order: the same
    bits on every call.

    Returns a dict: ``names`` (recordings by first appearance), ``labels`` (first cycle's label),
    ``counts``, ``mean_proba`` (R,C) float32, ``votes`` (R,C) int32, ``loss_sum`` (sum of the row
    cross entropies, recordings added in order; None without a criterion), ``n`` (cycles seen).
    ``criterion``: None, ``CELoss`` or ``SELCLoss``.  The model is put in eval mode; the loader is
    iterated exactly once.  A label >= ``args.num_classes`` is a ValueError before the batch that
    carries it launches anything (with a cached plan: before any launch)."""
    import ctypes
    from . import _lib
    device = torch.device(device)
    C = int(args.num_classes)
    if device.type != "cuda":
        raise ValueError("predict_recordings runs on a HIP device (test_data_accuracy covers the CPU)")
    if not 1 <= C <= EVAL_MAX_CLASSES:
        raise ValueError(f"predict_recordings: 1..{EVAL_MAX_CLASSES} classes, got {C}")
    if not (criterion is None or type(criterion) in (CELoss, SELCLoss)):
        raise ValueError("predict_recordings computes the cross entropy of CELoss / SELCLoss('test'); "
                         f"got {type(criterion).__name__}")
    model.eval()
    lib = _lib.load()
    want_loss = criterion is not None
    cacheable = hasattr(loader, "eval_plan") and not getattr(loader, "shuffle", True)
    plan = loader.eval_plan if cacheable else None
    if cacheable and plan is None:
        plan = loader.eval_plan = EvalPlan(loader.wav, loader.label.numpy())
    batches = loader
    if plan is None and not hasattr(loader, "dataset"):
        batches = list(loader)                     # (the one iteration: how many rows there are)
        cap = sum(len(b[1]) for b in batches)
    elif plan is None:
        cap = len(loader.dataset)
    if plan is not None:
        if want_loss:
            _eval_labels_ok(plan.cycle_labels, C)
        side = plan.device_side(device, C)
        prob, loss_rows, vote = side.prob, side.loss_rows, side.vote
    else:
        prob = torch.empty((cap, C), dtype=torch.float32, device=device)
        loss_rows = torch.empty(cap, dtype=torch.float32, device=device)
        vote = torch.empty(cap, dtype=torch.uint8, device=device)
        seen_wav, seen_lab = [], []
    potes = isinstance(model, models.CNN_potes)
    n = 0
    for data, target, _frames, wav, _sq, _idx in batches:
        b = int(data.shape[0])
        if b == 0:
            continue
        if plan is not None:
            if n + b > plan.n:
                raise ValueError("predict_recordings: the loader yields more rows than its cached plan")
            lab_ptr = side.labels.data_ptr() + n if want_loss else None
        else:
            if n + b > cap or len(wav) != b or len(target) != b:
                raise ValueError("predict_recordings: the loader yields more rows than len(loader.dataset)")
            lab_host = target.detach().to("cpu", torch.int64).reshape(-1)
            if want_loss:
                _eval_labels_ok(lab_host.numpy(), C)
            seen_wav.extend(wav)
            seen_lab.append(lab_host)
            lab_dev = lab_host.to(torch.uint8).to(device, non_blocking=True) if want_loss else None
            lab_ptr = lab_dev.data_ptr() if want_loss else None
        data = data.to(device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        outs = (prob.data_ptr() + 4 * n * C, loss_rows.data_ptr() + 4 * n, vote.data_ptr() + n)
        if potes and data.dim() == 3 and model._fused_head(data):
            c1, c2 = model.cnn1[0][0], model.cnn1[1][0]
            rows = data[:, :4, :].reshape(b * 4, data.shape[2]).contiguous()
            # detached weights: ``ctx.needs_input_grad`` follows the inputs' ``requires_grad`` even under
            # no_grad, and the conv stack would take its routing-saving forward for a backward nobody runs
            feat = models.PotesStackFunction.apply(rows, c1.weight.detach(), c1.bias.detach(),
                                                   c2.weight.detach(), c2.bias.detach()).reshape(b, -1)
            K = int(feat.shape[1])
            w1, w2 = model.dimreduc.weight.detach().contiguous(), model.linear.weight.detach().contiguous()
            b1, b2 = model.dimreduc.bias, model.linear.bias
            partial = torch.empty((lib.pcgmix_skinny_linear_splits(b, K), b, 20), dtype=torch.float32,
                                  device=device)
            _lib.check(lib.pcgmix_potes_head_eval_f32(
                feat.data_ptr(), w1.data_ptr(), b1.detach().data_ptr() if b1 is not None else None,
                w2.data_ptr(), b2.detach().data_ptr() if b2 is not None else None, lab_ptr,
                partial.data_ptr(), None, *outs, b, K, C, stream), "pcgmix_potes_head_eval_f32")
        else:
            out = model(data)
            if out.dim() != 2 or out.shape != (b, C):
                raise ValueError(f"predict_recordings: the model returned {tuple(out.shape)}, "
                                 f"expected ({b}, {C})")
            out = out.to(torch.float32).contiguous()
            _lib.check(lib.pcgmix_eval_rows_f32(out.data_ptr(), lab_ptr, *outs, b, C, stream),
                       "pcgmix_eval_rows_f32")
        n += b
    if plan is None:
        plan = EvalPlan(seen_wav, torch.cat(seen_lab).numpy() if seen_lab else [])
        order = torch.from_numpy(plan.order).to(device)
        rec_start = torch.from_numpy(plan.rec_start).to(device)
        R = plan.recordings
        out_buf = torch.empty(8 * R + 8 * R * C, dtype=torch.uint8, device=device)
    else:
        if n != plan.n:
            raise ValueError("predict_recordings: the loader yields fewer rows than its cached plan")
        order, rec_start, out_buf, R = side.order, side.rec_start, side.out, plan.recordings
    if R:
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        base = out_buf.data_ptr()
        _lib.check(lib.pcgmix_eval_segments_f32(
            prob.data_ptr(), loss_rows.data_ptr(), vote.data_ptr(), order.data_ptr(),
            rec_start.data_ptr(), base + 8 * R, base + 8 * R + 4 * R * C, base, n, R, C, stream),
            "pcgmix_eval_segments_f32")
    host = out_buf.cpu().numpy()                       # the pass's one copy to the host (and its sync)
    loss_rec = host[:8 * R].view(np.float64)
    mean_p = host[8 * R:8 * R + 4 * R * C].view(np.float32).reshape(R, C)
    votes = host[8 * R + 4 * R * C:].view(np.int32).reshape(R, C)
    loss_sum = None
    if want_loss:
        loss_sum = 0.0
        for v in loss_rec.tolist():                    # recordings in order, in double
            loss_sum += v
    return {"names": list(plan.names), "labels": plan.labels.copy(), "counts": plan.counts.copy(),
            "mean_proba": mean_p, "votes": votes, "loss_sum": loss_sum, "n": n}


@torch.no_grad()
def _collect_recordings_torch(args, model, test_loader, device, criterion, majority):
    """The torch formulation of the per-recording collection (the CPU, other criteria, more than
    eight classes, ``FUSED_EVAL = False``): per-recording sums as segmented sums on the device
    (index_add).  Returns (mean_p, votes or None, recording labels, loss sum or None, cycles)."""
    model.eval()
    rec_ids: dict = {}
    rec_label: dict = {}
    parts = []
    loss_sum = torch.zeros((), device=device, dtype=torch.float64)
    n = 0
    for data, target, _frames, wav, _sq, _idx in test_loader:
        data = data.to(device)
        out = model(data)
        prob = F.softmax(out, dim=1)
        for w, t in zip(wav, target.tolist()):
            rec_label.setdefault(rec_ids.setdefault(w, len(rec_ids)), t)   # first cycle's label
        ids = torch.tensor([rec_ids[w] for w in wav], device=device)
        parts.append((ids, prob))
        if criterion is not None:               # :608-609, accumulated on the device
            loss_sum += criterion(out, F.one_hot(target, args.num_classes).to(device),
                                  None, None, "test").double() * len(target)
        n += len(target)
    R = len(rec_ids)
    acc_p = torch.zeros(R, args.num_classes, device=device)
    acc_n = torch.zeros(R, device=device)
    votes = torch.zeros(R, args.num_classes, device=device, dtype=torch.long)
    for ids, prob in parts:
        acc_p.index_add_(0, ids, prob)
        acc_n.index_add_(0, ids, torch.ones_like(ids, dtype=torch.float))
        if majority:
            votes.index_add_(0, ids, F.one_hot(prob.argmax(1), args.num_classes))
    mean_p = (acc_p / acc_n[:, None]).cpu().numpy()
    lab = np.asarray([rec_label[i] for i in range(R)])
    return (mean_p, votes.cpu().numpy() if majority else None, lab,
            float(loss_sum) if criterion is not None else None, n)


@torch.no_grad()
def test_data_accuracy(args, model, test_loader, device, criterion=None, epoch=None,
                       performance=None):
    """Evaluation as train_model.py:591-670, reference signature ``(args, model, test_loader,
    device, criterion, epoch, performance)`` (called that way at :455): per recording, average
    the softmax of its heart cycles and take the argmax (:623-633); with '(class_majority)' in
    ``args.method`` the recording's class is the majority of its cycles' arg-max votes, a 0/1 tie
    going to class 1 (:634-647).  Accuracy / sensitivity / specificity / precision / recall / F1
    over recordings, ROC-AUC of the mean class-1 probability.  On a GPU, with at most eight classes
    and no criterion, ``CELoss`` or ``SELCLoss``, the per-recording numbers come from
    ``predict_recordings`` (HIP eval kernels, fixed-order sums; ``FUSED_EVAL``); otherwise from
    the torch formulation (``_collect_recordings_torch``).

    With a ``performance`` object (anything with the reference's ``add(key, value)``,
    :194-195) the eight ``test_*`` values are appended to it in the reference's order
    (:651-669) and the function returns None, as the reference does.  Without one it returns
    the same numbers as a dict.  ``epoch`` is accepted and unused, as in the reference.

    Under '(class_majority)' the reference never collects the mean probabilities, so its own
    ``roc_auc_score`` line (:667) raises IndexError after the other seven values have been
    appended: with ``performance`` this function does exactly that; the dict form carries
    ``rocauc = None`` on that branch."""
    majority = "(class_majority)" in getattr(args, "method", "")
    if fused_eval_applies(args, device, criterion):
        rec = predict_recordings(args, model, test_loader, device, criterion)
        mean_p, votes, lab, loss_sum, n = (rec["mean_proba"], rec["votes"], np.asarray(rec["labels"]),
                                           rec["loss_sum"], rec["n"])
    else:
        mean_p, votes, lab, loss_sum, n = _collect_recordings_torch(args, model, test_loader, device,
                                                                     criterion, majority)
    R = len(lab)
    if majority:
        pred = np.zeros(R, dtype=np.int64)
        for r, c in enumerate(votes):
            c = np.trim_zeros(c, "b") if c.any() else c[:1]          # what np.bincount returns
            pred[r] = 1 if (len(c) == 2 and c[0] == c[1]) else int(np.argmax(c))
    else:
        pred = mean_p.argmax(1)
    tp = int(((pred == 1) & (lab == 1)).sum()); tn = int(((pred == 0) & (lab == 0)).sum())
    fp = int(((pred == 1) & (lab == 0)).sum()); fn = int(((pred == 0) & (lab == 1)).sum())
    prec = tp / max(1, tp + fp)
    rec = tp / max(1, tp + fn)
    # ROC-AUC of the class-1 mean probability (Mann-Whitney U with average ranks for ties)
    auc = None
    if 0 < lab.sum() < R and not majority:
        score = mean_p[:, 1]
        order = np.argsort(score, kind="mergesort")
        ranks = np.empty(R)
        ranks[order] = np.arange(1, R + 1)
        for v in np.unique(score):
            tie = score == v
            ranks[tie] = ranks[tie].mean()
        n1 = int(lab.sum())
        auc = float((ranks[lab == 1].sum() - n1 * (n1 + 1) / 2) / (n1 * (R - n1)))
    n_total = len(test_loader.dataset) if hasattr(test_loader, "dataset") else n      # :653
    ev = {"accuracy": 100.0 * float((pred == lab).sum()) / max(1, R), "sensitivity": 100.0 * rec,
          "specificity": 100.0 * tn / max(1, tn + fp), "precision": prec, "recall": rec,
          "f1": 2 * prec * rec / max(1e-12, prec + rec), "rocauc": auc, "recordings": R,
          "loss": loss_sum / max(1, n_total) if criterion is not None else None}
    if performance is None:
        return ev
    for key in ("accuracy", "loss", "specificity", "sensitivity", "f1", "precision", "recall"):
        performance.add("test_" + key, ev[key])                                       # :651-666
    if majority:
        raise IndexError("'(class_majority)' collects no mean probabilities: the reference's "
                         "roc_auc_score line (train_model.py:667) fails the same way")
    performance.add("test_rocauc", auc)                                               # :667-668
    return None


def train_model(args, dataset, device, use_graph: bool = True, log=print, pipeline: bool = True):
    """The reference's run driver (train_model.py:197-488) reduced to the hot path: seeds (:216-223),
    loaders (:244-248), model (:293-386), criterion/optimiser/scheduler (:390-410), the epoch loop
    (:428-478) with evaluation at the reference's 11 "plot epochs", and ``model.pth`` written with the
    reference's DataParallel key prefix (:481-482) so that saliency-guided runs of either code
    base can load it (saliency.py:50).  Plots, the pickle of the performance dict and the model
    zoo are out of scope.  Returns the performance dict.

    ``dataset`` is the dictionary ``dataloader_physionet.file2dict`` returns (time series:
    ``args.dataset = 'PhysioNet'``; log-mel images, one per cycle: ``'PhysioNet(spec128)'``,
    train_model.py:228-233 -> ``dataloader_physionet2d``); it is selected by ``physionet_dataloader``
    and kept resident on ``device``.  The step runs as a captured
    hipGraph (``use_graph``); under torch.distributed each rank trains on its shard of every batch
    and gradients are averaged by one all-reduce per step (``FlatGradSync`` around the graph, DDP
    for the eager step)."""
    import random
    import time as _time

    from . import dataloader_physionet as dlp
    from . import saliency as _sal

    spectro = args.dataset == "PhysioNet(spec128)"
    if args.dataset != "PhysioNet" and not spectro:
        raise NotImplementedError("train_model drives the PhysioNet time-series and spectrogram paths")
    rank, world = rank_and_world()
    if spectro and world > 1:
        from . import hostprep
        if hostprep.select_method(args.method, is2d=True) == "latentmixup":
            # two half passes of the DDP-wrapped model in one iteration (augmentations2d.py:523 and
            # the training step's 'second' pass): refused rather than reduced twice or not at all
            raise NotImplementedError(LATENT_DDP_MESSAGE)
    if not spectro and latent_method(args) and world > 1:
        raise NotImplementedError(LATENT_DDP_MESSAGE)
    seed_fix = 4                                                   # :217
    args.seed_fix = seed_fix
    torch.manual_seed(seed_fix)
    random.seed(seed_fix)
    np.random.seed(seed_fix)
    args.device = device
    if not hasattr(args, "classical_space"):
        args.classical_space = False
    if spectro:                                                    # :228-233
        from . import dataloader_physionet2d as dlp2
        loaders = dlp2.physionet_dataloader(args, dataset)
    else:
        loaders = dlp.physionet_dataloader(args, dataset)
    train_loader, train_labels = loaders.run("train", seed_fix)
    test_loader = loaders.run("valid" if args.valid else "test", None)
    args.sig_len = int(train_loader.data.shape[-1])
    torch.manual_seed(seed_fix)                                    # :293 initial weights
    model = build_model(args).to(device)
    args.num_steps = args.num_epochs * (len(train_loader.dataset) // args.batch_size)   # :390
    criterion = SELCLoss(train_labels, args.num_classes, es=selc_turning_point(args), device=device)
    # (the spectrogram step is 80 ms of MIOpen convolutions: nothing for a graph to win, it stays eager)
    # Under torch.distributed a run that reaches the SELC phase stays eager: every rank owns a copy of
    # the soft labels and sees its shard's indices only.
    graphable = use_graph and device.type == "cuda" and capture_refusal(args) is None \
        and (world == 1 or args.num_epochs <= criterion.es)
    if not graphable:
        model = wrap_distributed(model, device)
    optimizer, scheduler = make_optimizer(args, model)
    step_counter = step_counter_class()
    graphed, graphed_selc = None, None

    def capture_step(selc):
        return captured_step_class(args, pipeline)(
            args, model, optimizer, scheduler, criterion, device,
            args.batch_size // world, args.num_channels, args.sig_len,
            sync=FlatGradSync(model, device) if world > 1 else None, selc=selc)
    performance = performance_metrics_class()                                           # :421
    perf = performance.dict
    plot_epochs = set(np.linspace(1, args.num_epochs, 11).astype("int").tolist())       # :424
    args.depth = 0
    t_sum = 0.0
    for epoch in range(1, args.num_epochs + 1):
        if graphable and graphed_selc != (epoch > criterion.es):     # first epoch, and the first past es
            graphed = None                                           # (the old graph goes first)
            graphed_selc = epoch > criterion.es
            model.train()                    # the evaluation of the epoch before left it in eval mode
            graphed = capture_step(graphed_selc)
        t0 = _time.time()
        batches = (shard_batch(b, rank, world) for b in train_loader) if world > 1 else train_loader
        stats, n_batches = _run_epoch(
            args, model, batches, device, optimizer, scheduler, criterion, epoch, step_counter,
            lambda *_: graphed, train_step if graphed is None else None)
        t_sum += _time.time() - t0
        if epoch in plot_epochs:
            performance.add("epochs", epoch)                                            # :447-455
            performance.add("steps", step_counter.count)
            performance.add("train_loss", float(stats["loss_sum"]) / max(1, n_batches))
            performance.add("train_accuracy", 100.0 * float(stats["hits"]) / max(1, stats["seen"]))
            try:
                test_data_accuracy(args, model, test_loader, device, criterion, epoch, performance)
            except IndexError:                    # '(class_majority)': the reference stops here (:667)
                performance.add("test_rocauc", None)
            performance.add("times", t_sum)
            if rank == 0 and log is not None:
                log(f"epoch {epoch:3d} step {step_counter.count:6d} train loss "
                    f"{perf['train_loss'][-1]:.4f} acc {perf['train_accuracy'][-1]:.1f}%  "
                    f"test acc {perf['test_accuracy'][-1]:.1f}%")
    out_dir = getattr(args, "EXPERIMENTS", None)
    if out_dir and rank == 0:
        exp = _sal.experiment_dir(args)
        os.makedirs(exp, exist_ok=True)
        inner = model.module if hasattr(model, "module") else model
        torch.save({"module." + k: v for k, v in inner.state_dict().items()},
                   os.path.join(exp, "model.pth"))
    perf["model"] = model
    return perf


class SyntheticCycleLoader:
    """Stands in for physionet_dataloader(...).run('train') (dataloader_physionet.py:204-229):
    yields the same 6-tuple (data, target, frames, wav, sig_qual, index) of CPU tensors, shuffled
    with torch's global generator and ``drop_last=True``, from a synthetic pool."""

    def __init__(self, pool, batch_size: int):
        self.x, self.frames, self.labels, self.wav = pool
        self.batch_size = batch_size
        self.dataset = range(len(self.labels))

    def __len__(self):
        return len(self.labels) // self.batch_size

    def __iter__(self):
        perm = torch.randperm(len(self.labels))
        for i in range(len(self)):
            idx = perm[i * self.batch_size:(i + 1) * self.batch_size]
            ii = idx.numpy()
            yield (torch.from_numpy(self.x[ii]), torch.from_numpy(self.labels[ii]),
                   torch.from_numpy(self.frames[ii]), tuple(self.wav[j] for j in ii),
                   torch.ones(len(ii), dtype=torch.long), idx)
