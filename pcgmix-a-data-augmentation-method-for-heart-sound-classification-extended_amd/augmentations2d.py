"""Drop-in replacement for the reference's ``augmentations2d.augment`` (augmentations2d.py:267,
called from train_model.py:505): one cached ``hostprep.route(args.method, True)`` lookup, then one
branch on the route's family — the ``durratiomixup`` splice (:397-427) and its mask variants, the
comparison baselines, bare ``cutout``; a branch of the reference that is not served raises
NotImplementedError (a bare ``mixup`` that nothing behind it catches among them).

The mask variants ``durmixcutout(t,f)``, ``durmixtimemask(t)``, ``durmixfreqmask(f)``
(augmentations2d.py:286-395): the same splice followed by a zeroed rectangle, fused into the same
kernel launch as one extra predicate.

Spectrogram batches are (B, 1, F, W); the four heart states are ranges of the last (time)
axis and ``frames`` holds their boundaries in spectrogram columns.  The splice is the 1D one
applied to every frequency row, so the same kernel runs with C = F rows and T = W columns
(augmentations2d.py:206-221).  alpha is fixed to 1 and only same-label partners exist in 2D
(augmentations2d.py:410-411).  ``(saloptenv)durratiomixup`` / ``(saloptsum)durratiomixup`` place the
shorter state inside the longer one by saliency (augmentations2d.py:125-204, 416-423): maps from the
frozen ResNet9-2D 'base' checkpoint through ``saliency.get_saliency_maps(dim=2)``, then the 1D
displacement search and offset splice.

The paper's spectrogram comparison baselines (augmentations2d.py:461-617) run through the same
call, with the reference's return values (csrc/pcgmix_baselines.hip, csrc/pcgmix_cutpaste.hip):

    timemask(t)[+p]            columns [int(u1*f[-1]), int(u2*f[-1])) of every row and channel
                               zeroed IN PLACE; returns ``data`` itself, ``[]``, None
    freqmask(f)[+p]            rows [h1, h2) of every channel zeroed IN PLACE; same return
    mixup(same) / mixup(mix)   data*lam + data[mix]*(1-lam) in fp32 on a new tensor; '(mix)'
                               blends the targets too; returns (new, targets, mix, None)
    cutmix, (rand)cutmix       own columns up to f1[cut], the partner's behind them, zeros after
                               ``min(.., F)``; the new tensor is (B, C, F, F) as the reference's
                               ``torch.zeros((size, C, F, F))``; returns (new, targets, mix, cut)
    durratiocutmix             systole and diastole columns from the partner (needs W == F)
    (rand)durratiocutmix       the reference's row-slicing quirk: whole frequency rows swapped
    latentmixup[+p]            ``model(data, depth, 'first')`` blended with the same-label partners'
                               features through a differentiable HIP blend; sets ``args.depth``

    cutout[(t,f)][+p]          durmixcutout's rectangle without the splice (augmentations2d.py:429-459):
                               rows [h1, h2) x columns [int(u1*f[-1]), int(u2*f[-1])) of every
                               channel zeroed IN PLACE; returns ``data`` itself, ``[]``, None
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, hostprep
from . import augmentations as _aug1d           # (its _native_step is read per call: tests switch it)
from .augmentations import (LatentBlend, _as_numpy_frames, _batch_dense, _blend_planes, _check_data,  # noqa: F401
                            _label_source, _raw_stream, apply_plan, blend_targets, gate_passes,
                            latent_blend, splice_plain, upload_array)


def zero_rects_(data: torch.Tensor, rect: np.ndarray) -> torch.Tensor:
    """``data[b, :, r0:r1, c0:c1] = 0`` in place for the (B, 4) int32 host rectangles."""
    B, C, F, W = data.shape
    if B == 0:
        return data
    area = int(((rect[:, 1] - rect[:, 0]).clip(0) * (rect[:, 3] - rect[:, 2]).clip(0)).max())
    if area == 0:
        return data
    with torch.cuda.device(data.device):
        dev = upload_array(np.ascontiguousarray(rect, dtype=np.int32), data.device)
        _lib.check(_lib.load().pcgmix_zero_rects_f32(data.data_ptr(), dev.data_ptr(), B, C, F, W, area,
                                                     ctypes.c_void_p(_raw_stream(data.device))), "pcgmix_zero_rects_f32")
    return data


def piecewise_rows(data: torch.Tensor, segs: np.ndarray, mix: np.ndarray, axis: int,
                   out_cols: int) -> torch.Tensor:
    """New (B, C, F, out_cols) tensor from the (B, 5, 4) segment table (cutmix, durratiocutmix)."""
    B, C, F, W = data.shape
    out = torch.empty((B, C, F, out_cols), dtype=data.dtype, device=data.device)
    if B == 0:
        return out
    with torch.cuda.device(data.device):
        # one upload: the table, then the partners
        host = np.concatenate([np.ascontiguousarray(segs, dtype=np.int32).reshape(-1),
                               np.asarray(mix, dtype=np.int32)])
        dev = upload_array(host, data.device)
        _lib.check(_lib.load().pcgmix_piecewise_rows_f32(
            data.data_ptr(), out.data_ptr(), dev.data_ptr(), dev.data_ptr() + segs.size * 4, axis,
            B, C, F, W, out_cols, ctypes.c_void_p(_raw_stream(data.device))), "pcgmix_piecewise_rows_f32")
    return out


def _augment_baseline2d(args, name, data, target_ohe, frames, step: int, model, host_labels):
    """One call of the spectrogram baseline ``name`` (augmentations2d.py:461-617)."""
    _check_data(data, 4)
    B, C, F, W = data.shape
    if name == "latentmixup" and getattr(args, "model", None) != "resnet9":
        # the reference sets max_model_depth for 'resnet9' only (augmentations2d.py:520-521)
        raise NotImplementedError(f"latentmixup: the reference defines the mixing depth for "
                                  f"args.model == 'resnet9' only, got {getattr(args, 'model', None)!r}")
    frames_np = _as_numpy_frames(frames)
    labels = _label_source(target_ohe, host_labels)
    plan = hostprep.make_plan(args.method, labels, frames_np, None, step, B, C, is2d=True, n_cols=W,
                              n_freq=F)
    if not plan.fired:
        return data, target_ohe, [], None
    kind = plan.kind
    if kind in ("timemask2d", "freqmask2d"):
        return zero_rects_(data, plan.zero_rect), target_ohe, [], None
    if kind == "mixup2d":
        out = torch.empty_like(data)
        if B:
            with torch.cuda.device(data.device):
                mix = upload_array(plan.mix.astype(np.int32), data.device)
                _blend_planes(data, out, mix, float(plan.lam32))
        if plan.mix_all:
            target_ohe = blend_targets(target_ohe, plan)
        return out, target_ohe, plan.mix, None
    if kind in ("cutmix2d", "durratiocutmix2d"):
        out = piecewise_rows(data, plan.segs, plan.mix, plan.seg_axis, plan.out_cols)
        return out, target_ohe, plan.mix, plan.cut
    if kind == "latentmixup2d":
        if model is None:
            raise ValueError("latentmixup needs the model (augment(..., model, ...))")
        args.depth = plan.depth
        h = model(data, depth=plan.depth, pass_part="first")
        return latent_blend(h, plan.mix, plan.lam32), target_ohe, plan.mix, None
    raise NotImplementedError(kind)                                        # pragma: no cover


def _augment_cutout2d(args, data, target_ohe, frames, step: int):
    """Bare ``cutout[(t,f)]`` (augmentations2d.py:429-459): durmixcutout's rectangle without the
    splice — no partners, no lambda, numpy's global stream untouched — zeroed IN PLACE in every
    channel; returns ``data`` itself."""
    _check_data(data, 4)
    B, C, F, W = data.shape
    plan = hostprep.cutpaste_plan(args.method, None, _as_numpy_frames(frames), None, step, B, C, W,
                                  is2d=True, n_freq=F, n_cols=W)
    if not plan.fired:
        return data, target_ohe, [], None
    return zero_rects_(data, plan.zero_rect), target_ohe, [], None


def _augment_splice2d(args, route, data, target_ohe, frames, wav, step: int, device, host_labels):
    """One call of ``durratiomixup`` or a mask variant (augmentations2d.py:286-427)."""
    _check_data(data, 4)
    B, Cc, F, W = data.shape
    plain = route.plain
    if plain.__class__ is tuple and B > 0:             # durratiomixup: one library call
        rows = data.view(B, Cc * F, W)
        native = _aug1d._native_step
        if native is not None and _lib.TAPE is None:   # the compiled armed step, as augmentations.augment
            done = native(plain, rows, target_ohe, frames, step, host_labels)
            if done is not None:                       # (a rejected gate hands `rows` itself back)
                return (data if done[0] is rows else done[0].view(B, Cc, F, W)), target_ohe, done[2], None
        if not gate_passes(plain, args.method, step, data.device.index):
            return data, target_ohe, [], None
        out, mix = splice_plain(plain, rows, host_labels, frames, step, target_ohe=target_ohe)
        return out.view(B, Cc, F, W), target_ohe, mix, None
    if isinstance(plain, Exception):
        raise plain
    frames_np = _as_numpy_frames(frames)
    plan = hostprep.make_plan(args.method, _label_source(target_ohe, host_labels), frames_np, wav, step,
                              B, Cc * F, is2d=True, n_cols=W)
    if not plan.fired:
        return data, target_ohe, [], None
    sal = None
    if plan.salopt_mode is not None:
        # '(saloptenv)durratiomixup' / '(saloptsum)…' on spectrograms (augmentations2d.py:416-423):
        # the frozen ResNet9-2D's input gradient -> (B, W) maps (saliency.get_saliency_maps, dim=2),
        # then the same displacement search and offset splice as in 1D, with C = F rows, T = W columns
        from . import saliency
        sal = saliency.get_saliency_maps(args, device, data, target_ohe, frames_np, dim=2)
    out = apply_plan(plan, data.view(B, Cc * F, W), frames_np, sal).view(B, Cc, F, W)
    return out, target_ohe, plan.mix, None


def augment(args, data, target_ohe, frames, wav, step_counter, model, device, RESULTS_ARGS,
            host_labels=None):
    step = int(step_counter.count)
    route = hostprep.route(args.method, True)
    family = route.family
    if family == "splice":
        return _augment_splice2d(args, route, data, target_ohe, frames, wav, step, device, host_labels)
    if family == "passthrough":
        return data, target_ohe, [], None
    if family == "baseline":
        return _augment_baseline2d(args, route.branch, data, target_ohe, frames, step, model, host_labels)
    if family == "cutpaste":
        return _augment_cutout2d(args, data, target_ohe, frames, step)
    raise NotImplementedError(route.refusal)
