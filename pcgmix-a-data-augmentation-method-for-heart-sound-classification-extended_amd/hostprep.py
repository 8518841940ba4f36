"""Host prologue of one PCGmix augmentation call: everything that is integer or random.

Which augmentation a method string selects is decided in ONE place: ``route(method, is2d)`` walks the
reference's if-chain (``_CHAIN_1D`` / ``_CHAIN_2D``, stated once, in the reference's order) and
returns a cached ``Route``: the branch reached, the family that serves it ("passthrough", "splice",
"baseline", "cutpaste", "latent", "refused") and the splice's recipes.  ``select_method``,
``plain_recipe``, ``salopt_recipe``, ``latent_recipe``, ``cutpaste_recipe`` and ``soft_targets`` are
views of it; both ``augment()``s and the training steps branch on ``Route.family``.

The reference derives all randomness of a step from ``step_counter.count`` through CPython's
``random.Random`` and numpy's legacy global ``RandomState`` (augmentations.py:869, 936, 500-514,
659-666, 677).  Those streams *define* parity, are O(B) work, and are therefore kept on the
host and called in the reference's order:

    Random(step).uniform          probability gate                 augmentations.py:869-872
    Random(step).sample per group partner permutation              augmentations.py:500-514
    np.random.seed(step); beta    lambda (global numpy stream!)    augmentations.py:659-666
    Random(step).randint          '(rand)' placement offsets       augmentations.py:305-337
    np.random.normal              magnitude-warp knots             augmentations.py:677

The spectrogram baselines (augmentations2d.py:461-617) draw from the same streams: the gate,
same-label partners (or ``Random(step).sample`` for ``mixup(mix)``), ``get_lambda`` for mixup and
latentmixup only, ``Random(step+131071)`` / ``Random(step+13119)`` for the mask sizes and
positions, ``Random(step*131071).randint(1, 3)`` for ``(rand)cutmix``'s cut and
``Random(step).randint(1, 3)`` for latentmixup's depth.

The heart-cycle cut-and-paste family, ``durmixrespscale`` and bare ``cutout`` (augmentations.py:
734-775, 983-1000, 1101-1213, 1285-1316, 1569-1616; augmentations2d.py:429-459) are planned by
``cutpaste_plan``: the gate, partners by label / recording / data set /
(label, length bin), ``Random(step).randint(1, 3)`` or ``Random(step*131071).randint(1, 3)`` for
the cut, ``Random(step + i*131071)`` for the 'cutout' suffix; only ``durmixrespscale`` touches
numpy's global stream (``get_lambda``).

The result is a small ``MixPlan`` of index/scalar data that the device kernels consume; no
waveform data is touched here.
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib

# Methods this package implements: the PCGmix splices (augmentations.py:864, 931) and the paper's
# 1D comparison baselines (augmentations.py:777, 807, 829, 1002, 1026).
SPLICE_METHODS_1D = ("durmixmagwarp", "durratiomixup")
BASELINE_METHODS_1D = ("respiratoryscale", "timemask", "mixup", "timewarp", "magnitudewarp")
PCGMIX_METHODS_1D = SPLICE_METHODS_1D + BASELINE_METHODS_1D
# the PCGmix splice and its mask variants on spectrograms (augmentations2d.py:286, 328, 364, 397)
PCGMIX_METHODS_2D = ("durmixcutout", "durmixtimemask", "durmixfreqmask", "durratiomixup")
# the paper's spectrogram comparison baselines (augmentations2d.py:461, 487, 510, 538, 574, 599)
BASELINE_METHODS_2D = ("timemask", "freqmask", "latentmixup", "mixup", "cutmix", "durratiocutmix")

# Names planned by ``cutpaste_plan`` (1D: augmentations.py:734, 983, 1101, 1121, 1153, 1184, 1285,
# 1569; 2D: augmentations2d.py:429).
CUTPASTE_METHODS_1D = ("durmixrespscale", "wav-durratiocutmix", "durratiocutmix", "lengthcutmix",
                       "datasetcutmix", "wavcutmix", "labelcutmix", "cutout")
CUTPASTE_METHODS_2D = ("cutout",)
CUTPASTE_KINDS = ("cutpaste", "mixscale", "cutout", "cutout2d")      # MixPlan.kind of a cutpaste_plan


def _branch(name, line, cond=None):
    """One branch of the reference's if-chain: its name, the source line it restates, and its
    condition on the method string (a bare substring test unless given)."""
    return name, line, cond or (lambda m: name in m)


# The reference's if-chains, each stated ONCE, whole and in the reference's order; ``route`` is the
# only function that walks them.  Every branch returns, except 'mixup' (see ``route``).  A method
# string that holds none of a chain's names is passed through (augmentations.py:731-732,
# augmentations2d.py:283-284: the names of ``methods_implemented`` all contain one of these).
_CHAIN_1D = (                                                         # augmentations.py
    _branch("durmixrespscale", 734), _branch("respiratoryscale", 777), _branch("timemask", 807),
    _branch("mixup", 829, lambda m: "mixup" in m and "latentmixup" not in m and "durratiomixup" not in m),
    _branch("durmixmagwarp", 864), _branch("durratiomixup", 931), _branch("wav-durratiocutmix", 983),
    _branch("timewarp", 1002), _branch("magnitudewarp", 1026), _branch("gaussiannoise", 1050),
    _branch("(UMC-subset)durratiocutmix", 1080, lambda m: "(UMC-subset)durratiocutmix" in m
            and "(plus)" not in m and "(plusplus)" not in m),
    _branch("durratiocutmix", 1101, lambda m: "durratiocutmix" in m and "(plus)" not in m
            and "(plusplus)" not in m and "(UMC" not in m and "wav-durratiocutmix" not in m),
    _branch("lengthcutmix", 1121), _branch("datasetcutmix", 1153),
    _branch("wavcutmix", 1184, lambda m: "wavcutmix" in m and "durratiowavcutmix" not in m),
    _branch("lc-nointrusion", 1215), _branch("labelcutmix", 1285), _branch("swapsysdia", 1318),
    _branch("cont-cutmix", 1356), _branch("saliency-cutmix", 1396), _branch("latentmixup", 1472),
    _branch("cutmix", 1508, lambda m: "cutmix" in m and "saliency" not in m and "label" not in m),
    _branch("cutout", 1569, lambda m: "cutout" in m and "saliency" not in m),
    _branch("s1s2mask", 1618, lambda m: m == "s1s2mask"),
)
_CHAIN_2D = (                                                         # augmentations2d.py
    _branch("durmixcutout", 286), _branch("durmixtimemask", 328), _branch("durmixfreqmask", 364),
    _branch("durratiomixup", 397),
    _branch("cutout", 429, lambda m: "cutout" in m and "durmixcutout" not in m),
    _branch("timemask", 461, lambda m: "timemask" in m and "durmixtimemask" not in m),
    _branch("freqmask", 487, lambda m: "freqmask" in m and "durmixfreqmask" not in m),
    _branch("latentmixup", 510),
    _branch("mixup", 538, lambda m: "mixup" in m and "durratiomixup" not in m and "latentmixup" not in m),
    _branch("cutmix", 574, lambda m: "cutmix" in m and "durratiocutmix" not in m),
    _branch("durratiocutmix", 599),
)
# Who serves a branch: "splice" and "baseline" go through plain_recipe / salopt_recipe / make_plan,
# "cutpaste" through cutpaste_plan, "latent" (1D) through latent_plan; any other branch is refused.
_FAMILY_1D = {**dict.fromkeys(SPLICE_METHODS_1D, "splice"), **dict.fromkeys(BASELINE_METHODS_1D, "baseline"),
              **dict.fromkeys(CUTPASTE_METHODS_1D, "cutpaste"), "latentmixup": "latent"}
_FAMILY_2D = {**dict.fromkeys(PCGMIX_METHODS_2D, "splice"), **dict.fromkeys(BASELINE_METHODS_2D, "baseline"),
              **dict.fromkeys(CUTPASTE_METHODS_2D, "cutpaste")}
_UNSUPPORTED_SELECTORS = ("(sameCVD)", "(closestbins=", "(closestknn=")


@dataclass
class MixPlan:
    """Index/scalar description of one augmentation step (host memory only)."""
    fired: bool
    name: str = ""
    step: int = 0
    mix: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))   # (B,) partner of b
    lam64: float = float("nan")                # np.random.beta result
    lam32: np.float32 = np.float32("nan")      # what multiplies the waveforms
    rand_off: Optional[np.ndarray] = None      # int32 (B,4) for '(rand)'
    salopt_mode: Optional[int] = None          # 0 = '(saloptenv', 1 = '(saloptsum'
    knots: Optional[np.ndarray] = None         # float64 (B, n_knots, C) as numpy drew them
    n_knots: int = 0
    mix_all: bool = False                      # '(mixAll)': targets are blended too
    zero_rect: Optional[np.ndarray] = None     # int32 (B,4) [row0,row1,col0,col1): 2D mask variants
    spans: Optional[np.ndarray] = None         # int32 (B,2) [t0,t1): timemask, zeroed in place
    scale_row: Optional[np.ndarray] = None     # float64 (T,): respiratoryscale's sinusoid
    is2d: bool = False                         # a spectrogram plan (augmentations2d.augment)
    cut: Optional[int] = None                  # cutmix: the state boundary it cuts at (1..3)
    depth: int = 0                             # latentmixup: the model depth it mixes at (1..3)
    segs: Optional[np.ndarray] = None          # int32 (B,5,4) {lo,hi,src,shift}: cutmix / durratiocutmix
    seg_axis: int = 0                          # 0: segments along the columns, 1: along F ('(rand)')
    out_cols: int = 0                          # width of the new tensor (cutmix: F, augmentations2d.py:589)
    junctions: Optional[np.ndarray] = None     # int32 (B,4) {c1, c2, ov, 0}: the '(smooth)' cross-fade
    span_rows: int = 0                         # cutout: rows per sample that carry a span of their own
                                               # (1, or C for '(ch)': spans is then (B*C, 2))
    # Which device path applies the plan, set where the plan is made: "splice" (durratiomixup /
    # durmixmagwarp and the 2D mask variants), the 1D baseline's name, the 2D baseline's name with a
    # "2d" suffix ("timemask2d", "cutmix2d", ...: a 2D timemask is a rectangle per channel, never the
    # 1D span path), or one of CUTPASTE_KINDS: "cutpaste" (segment table + junction), "mixscale"
    # (durmixrespscale: splice x row), "cutout" (1D spans, in place), "cutout2d" (rectangles, in place).
    kind: str = ""

    def __post_init__(self):
        if not self.kind:                      # a plan built by hand from a branch name
            self.kind = _plan_kind(route(self.name, self.is2d), self.is2d)


@dataclass(frozen=True)
class Route:
    """Where the reference's if-chain sends one method string, and who serves it here."""
    branch: Optional[str]     # name of the branch reached; None: no branch returns (or none is named)
    family: str               # "passthrough" | "splice" | "baseline" | "cutpaste" | "latent" | "refused"
    plain: object = None      # plain_recipe's tuple, None, or the exception its parsers raised
    salopt: object = None     # salopt_recipe's tuple, None, or the exception it raised
    soft_targets: bool = False
    refusal: str = ""         # "refused": why


def _recorded(fn, *args):
    """``fn(*args)``, or the exception a malformed parameter makes it raise: ``route`` itself never
    raises, the function that owns the answer does (``_value``)."""
    try:
        return fn(*args)
    except (ValueError, IndexError, NotImplementedError) as exc:
        return exc


def _value(answer):
    if isinstance(answer, Exception):
        raise answer.with_traceback(None)      # the cached object: do not pile tracebacks up on it
    return answer


@functools.lru_cache(maxsize=256)
def route(method: str, is2d: bool) -> Route:
    """One walk of the reference's if-chain for ``method``: the first branch that returns.  Every
    branch draws the same gate (``Random(step).uniform(0, 1) < p``), so the one branch that falls
    through — ``mixup`` without '(same)' or '(mix)', augmentations.py:829-862, augmentations2d.py:
    547-572 — leaves the decision to the next one.  Never raises: what is not served is "refused"."""
    chain = _CHAIN_2D if is2d else _CHAIN_1D
    soft = "(mixAll)" in method                                # augmentations.py:915-917, 978-980
    if not any(name in method for name, _, _ in chain):
        return Route(None, "passthrough", soft_targets=soft)   # augmentations.py:731-732
    branch = line = None
    for name, at, cond in chain:
        if cond(method) and (name != "mixup" or "(same)" in method or "(mix)" in method):
            branch, line = name, at
            break
    family = (_FAMILY_2D if is2d else _FAMILY_1D).get(branch, "refused")
    refusal = ""
    if branch is None:
        refusal = f"method {method!r} names a reference augmentation but reaches no branch that returns"
    elif family == "refused":
        refusal = (f"method {method!r} reaches the reference's branch {branch!r} (line {line}), which is "
                   f"not served: the reference's 2-tuple branches, manifold-*, (UMC-subset) and "
                   f"gaussiannoise are out of scope")
    elif not is2d:
        sel = next((s for s in _UNSUPPORTED_SELECTORS if s in method), None)
        if family == "splice" and sel is not None:
            refusal = f"partner selector {sel!r} is out of scope (SURVEY.md §2)"
        elif branch == "cutout" and "manifold" in method:
            refusal = "manifold-cutout needs max_depth, which the reference binds for FCN only"
        elif branch == "latentmixup" and ("durratiocutmix" in method or "wavcutmix" in method):
            # stricter than :1472: such a string gets past :1080 / :1101 / :1184 only through their
            # exclusions ('(plus)', '(UMC', 'durratiowavcutmix') and has been refused from the start
            refusal = f"method {method!r}: latentmixup next to a durratiocutmix / wavcutmix variant is not served"
    if refusal:
        return Route(branch, "refused", soft_targets=soft, refusal=refusal)
    if family == "baseline":
        soft = soft or (branch == "mixup" and "(same)" not in method)       # 'mixup(mix)', :857
    if family != "splice":
        return Route(branch, family, soft_targets=soft)
    return Route(branch, family, _recorded(_plain, method, branch, is2d),
                 None if is2d else _recorded(_salopt, method, branch), soft)


def _plan_kind(r: Route, is2d: bool) -> str:
    if r.family != "baseline":
        return "splice"
    return r.branch + "2d" if is2d else r.branch


def _waveform_route(method: str, is2d: bool) -> Route:
    """``route`` for the callers that go on to launch a splice or a baseline (or nothing, on
    passthrough): every other family raises NotImplementedError."""
    r = route(method, is2d)
    if r.family in ("refused", "cutpaste", "latent"):
        raise NotImplementedError(r.refusal or f"method {method!r} ({r.branch}) is not an augmentation of "
                                  f"the waveform that make_plan() serves: see cutpaste_plan() / latent_plan()")
    return r


def select_method(method: str, is2d: bool) -> Optional[str]:
    """Which splice or baseline branch the reference's if-chain reaches, or None for passthrough.

    Raises NotImplementedError for reference augmentations outside this package's scope — and for
    the cut-and-paste family and 1D latentmixup, which ``cutpaste_recipe`` / ``latent_recipe`` name."""
    return _waveform_route(method, is2d).branch


@functools.lru_cache(maxsize=256)
def parse_probability(method: str) -> float:
    """Text after the last '+' (augmentations.py:865-868)."""
    parts = method.split("+")
    return float(parts[-1]) if len(parts) > 1 else 1.0


@functools.lru_cache(maxsize=256)
def parse_alpha(method: str, name: str) -> float:
    """'(alpha=a)' immediately in front of the method name (augmentations.py:897-899)."""
    parts = method.split("(alpha=")
    return float(parts[1].split(")" + name)[0]) if len(parts) > 1 else 1.0


@functools.lru_cache(maxsize=256)
def parse_warp(method: str, name: str):
    """'durmixmagwarp(sigma,knot)' (augmentations.py:919-923) and 'magnitudewarp(sigma,knot)'
    (:1039-1042), defaults 0.2, 4; 'timewarp(sigma,knot)' (:1015-1018), defaults 0.05, 2.  As in the
    reference, the knot count is read behind the method string's FIRST comma."""
    sigma, knot = (0.05, 2) if name == "timewarp" else (0.2, 4)
    parts = method.split(name + "(")
    if len(parts) > 1:
        sigma = float(parts[1].split(",")[0])
        knot = int(method.split(",")[1].split(")")[0])
    return sigma, knot


def parse_magwarp(method: str):
    return parse_warp(method, "durmixmagwarp")


@functools.lru_cache(maxsize=256)
def parse_timemask(method: str) -> float:
    """'timemask(max)' (augmentations.py:816-819): default 0.2, clamped to [0, 1]."""
    parts = method.split("timemask(")
    if len(parts) > 1:
        return min(max(float(parts[1].split(")")[0]), 0), 1)
    return 0.2


@functools.lru_cache(maxsize=256)
def parse_respscale(method: str, name: str = "respiratoryscale"):
    """'respiratoryscale(min,max)' (augmentations.py:791-795) or, with ``name``,
    'durmixrespscale(min,max)' (:760-764) in breaths per minute -> (min, max) in Hz: min through
    float(), max through int() and from behind the string's FIRST comma — so
    'respiratoryscale(12,20.5)' raises ValueError as the reference does."""
    lo, hi = 12 / 60, 20 / 60
    parts = method.split(name + "(")
    if len(parts) > 1:
        lo = float(parts[1].split(",")[0]) / 60
        hi = int(method.split(",")[1].split(")")[0]) / 60
    return lo, hi


def parse_durmixrespscale(method: str):
    return parse_respscale(method, "durmixrespscale")


def mask_spans(method: str, frames: np.ndarray, step: int, sig_len: int) -> np.ndarray:
    """timemask's zeroed span per sample (augmentations.py:816-826): ``gap =
    Random(step+131071).uniform(0, max)``, ``f1 = Random(step+13119).uniform(0, 1-gap)``, span
    ``[int(f1*beat), int((f1+gap)*beat))`` with ``beat = frames[b, -1]``; int32 (B, 2), clipped
    to the row as the reference's slice is."""
    gap = random.Random(step + 131071).uniform(0, parse_timemask(method))
    frac1 = random.Random(step + 13119).uniform(0, 1 - gap)
    frac2 = frac1 + gap
    beat = np.asarray(frames)[:, -1].astype(np.float64)
    spans = np.empty((beat.shape[0], 2), dtype=np.int64)
    spans[:, 0] = (frac1 * beat).astype(np.int64)              # int() truncation
    spans[:, 1] = (frac2 * beat).astype(np.int64)
    return np.clip(spans, 0, sig_len).astype(np.int32)


def respiration_row(band, step: int, sig_len: int, sample_rate) -> np.ndarray:
    """The sinusoid of respiratoryscale / durmixrespscale (augmentations.py:796-799, 765-768) for
    ``band`` = (min, max) in Hz, with numpy as the reference builds it: the gate's own ``u =
    Random(step).random()`` gives rate = min + (max-min)*u and phase = 2*pi*u
    (``Random(step).uniform`` twice on fresh generators)."""
    lo, hi = band
    u = _lib.load().pcgmix_py_uniform01(int(step))
    rate = lo + (hi - lo) * u
    phase = 0 + (2 * np.pi - 0) * u
    t = np.linspace(0, sig_len / sample_rate, sig_len)
    return np.sin(2 * np.pi * rate * t + phase)


def _plain(method: str, name: str, is2d: bool):
    """Route.plain of a splice branch."""
    if is2d:
        if name != "durratiomixup" or "(salopt" in method:
            return None
        return name, parse_probability(method), 1.0, 0.0, 0          # augmentations2d.py:411
    if any(t in method for t in ("(rand)", "(salopt", "(samePCG)", "(sameDataset)", "(mixAll)")):
        return None
    sigma, knot = parse_warp(method, name) if name == "durmixmagwarp" else (0.0, -2)
    return name, parse_probability(method), parse_alpha(method, name), sigma, knot + 2


def _salopt(method: str, name: str):
    """Route.salopt of a 1D splice branch."""
    if "(salopt" not in method or any(t in method for t in ("(samePCG)", "(sameDataset)", "(mixAll)")):
        return None
    mode = _salopt_mode(method)
    sigma, knot = parse_warp(method, name) if name == "durmixmagwarp" else (0.0, -2)
    return mode, parse_alpha(method, name), sigma, knot + 2


def _salopt_mode(method: str) -> int:
    if "(saloptenv" in method:
        return 0
    if "(saloptsum" in method:
        return 1
    raise NotImplementedError("only (saloptenv…) and (saloptsum…) exist in the reference")


def plain_recipe(method: str, is2d: bool):
    """(name, p, alpha, sigma, knots) when ``method`` is a plain splice — same-label partners, no
    '(rand)' offsets, no saliency, no 2D mask — i.e. what ``pcgmix_augment_plain_f32`` does in
    one call; None otherwise (the general ``make_plan`` path handles those)."""
    return _value(_waveform_route(method, is2d).plain)


def salopt_recipe(method: str):
    """(mode, alpha, sigma, knots) when ``method`` is a saliency-guided splice with same-label
    partners — what ``pcgmix_ctx_salopt_begin/_finish`` do around the saliency pass; None otherwise
    ('(samePCG)', '(sameDataset)', '(mixAll)': the general ``make_plan`` path)."""
    return _value(_waveform_route(method, False).salopt)


# max_model_depth of the reference's 1D branch (augmentations.py:1484-1493) for the models served here
LATENT_MAX_DEPTH_1D = {"Potes": 1, "resnet9": 3}


def latent_recipe(method: str):
    """``(p,)`` when the reference's 1D if-chain reaches its ``latentmixup`` branch for ``method``
    (augmentations.py:1472-1506), None otherwise.  latentmixup leaves the waveform alone and needs
    the model, so it is a family of its own (``latent_plan``) and ``select_method`` refuses it."""
    return (parse_probability(method),) if route(method, False).family == "latent" else None


def latent_depth(model_name, step: int) -> int:
    """``Random(step).randint(1, max_model_depth)`` (augmentations.py:1494).  Models for which the
    reference leaves ``max_model_depth`` unbound (it fails there) are refused."""
    top = LATENT_MAX_DEPTH_1D.get(model_name)
    if top is None:
        raise NotImplementedError(f"latentmixup: the mixing depth is defined for args.model in "
                                  f"{tuple(LATENT_MAX_DEPTH_1D)} only, got {model_name!r}")
    return 1 + int(_lib.load().pcgmix_py_randint0(int(step), top - 1))


def latent_plan(method: str, model_name, labels, step: int, batch: int) -> MixPlan:
    """Host draws of one 1D latentmixup step in the reference's order (augmentations.py:1477-1497):
    gate, same-label partners, depth, then ``get_lambda(alpha=1)`` — numpy's global stream is
    reseeded only when the gate fires.  ``labels``: array or zero-argument callable (asked after
    the gate).  ``plan.mix`` are the partners, ``plan.depth`` the model depth, ``plan.lam64/32``."""
    recipe = latent_recipe(method)
    if recipe is None:
        raise ValueError(f"{method!r} does not reach the reference's 1D latentmixup branch")
    if LATENT_MAX_DEPTH_1D.get(model_name) is None:
        latent_depth(model_name, step)                         # raises
    if not (recipe[0] >= 1.0 or gate_fires(method, step)):
        return MixPlan(fired=False, step=step)
    plan = MixPlan(fired=True, name="latentmixup", step=step, kind="latent")
    plan.mix = shuffle_within_groups(_host_labels(labels, batch).astype(np.int64, copy=False), step)
    plan.depth = latent_depth(model_name, step)
    plan.lam64, _ = draw_lambda_knots(step, 1.0, 0.0, 0)
    plan.lam32 = np.float32(plan.lam64)
    return plan


def soft_targets(method: str) -> bool:
    """True when a fired step blends the one-hot targets into floats: '(mixAll)' (augmentations.py:
    915-917, 978-980) and 'mixup(mix)' (:857).  A training step then needs the float targets."""
    return route(method, False).soft_targets


def gate_fires(method: str, step: int) -> bool:
    """Fresh ``Random(step)``; the method runs iff u < p (augmentations.py:869-872).  The draw is
    the library's bit-exact restatement of ``random.Random(step).uniform(0, 1)``."""
    return _lib.load().pcgmix_py_uniform01(int(step)) < parse_probability(method)


def shuffle_within_groups(keys, step: int) -> np.ndarray:
    """Partner permutation: group positions by key and permute every group with a fresh
    ``Random(step).sample`` (augmentations.py:500-514).  The draw itself runs in the library's
    exact restatement of CPython's sampler (pcgmix_partner_permutation_i64): ~10x cheaper than
    ``random.sample`` and bit-identical to it (tests/test_host_logic.py)."""
    if isinstance(keys, np.ndarray) and keys.dtype.kind in "iu":
        lo, hi = (int(keys.min()), int(keys.max())) if keys.size else (0, 0)
        if hi - lo < 4096:                      # class labels: ids are the labels themselves
            gid, n_groups = keys - lo, hi - lo + 1          # (empty groups are allowed)
        else:
            uniq, gid = np.unique(keys, return_inverse=True)
            n_groups = int(uniq.shape[0])
    else:
        table: dict = {}
        gid = np.fromiter((table.setdefault(k, len(table)) for k in keys), dtype=np.int32,
                          count=len(keys))
        n_groups = len(table)
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    mix = np.empty(gid.shape[0], dtype=np.int64)
    lib = _lib.load()
    _lib.check(lib.pcgmix_partner_permutation_i64(gid.ctypes.data, gid.shape[0], n_groups,
                                                  int(step), mix.ctypes.data),
               "pcgmix_partner_permutation_i64")
    return mix


def partner_indices(method: str, labels: np.ndarray, wav: Sequence[str], step: int,
                    is2d: bool = False) -> np.ndarray:
    """Partner selection with the reference's override order (augmentations.py:877-896)."""
    labels = np.asarray(labels).reshape(-1)
    mix = shuffle_within_groups(labels.astype(np.int64, copy=False), step)  # same label
    if is2d:
        return mix                                                          # augmentations2d.py:410
    if "(samePCG)" in method:                                               # augmentations.py:528
        mix = shuffle_within_groups(list(wav), step)
    if "(sameDataset)" in method:                                           # augmentations.py:542
        mix = shuffle_within_groups([f"{w[0]}_{int(t)}" for w, t in zip(wav, labels)], step)
    if "(mixAll)" in method:                                                # augmentations.py:883
        mix = shuffle_within_groups(np.zeros(len(labels), dtype=np.int64), step)  # one group
    return mix


def rand_offsets(frames: np.ndarray, mix: np.ndarray, step: int, states=(0, 1, 2, 3)) -> np.ndarray:
    """'(rand)': offset of the shorter state inside the longer one,
    ``Random(step).randint(0, |gap|)`` with a fresh generator per (sample, state), so the value
    depends on (step, |gap|) only (augmentations.py:305-337): one library draw per distinct gap.
    int32 (B, 4); only the columns of ``states`` are drawn, the others are 0 ('(rand)durratiocutmix'
    needs systole and diastole only, augmentations2d.py:236, 243)."""
    lens = np.diff(frames, axis=1)
    cols = list(states)
    gap = np.abs(lens[mix] - lens)[:, cols]
    lib = _lib.load()
    uniq, inv = np.unique(gap, return_inverse=True)
    vals = np.array([lib.pcgmix_py_randint0(int(step), int(g)) for g in uniq], dtype=np.int32)
    out = np.zeros(lens.shape, dtype=np.int32)
    out[:, cols] = vals[inv].reshape(gap.shape)
    return out


def mask_rectangles(method: str, name: str, frames: np.ndarray, step: int, n_rows: int,
                    n_cols: int) -> np.ndarray:
    """Zeroed rectangle per sample for durmixcutout / durmixtimemask / durmixfreqmask
    (augmentations2d.py:309-323, 348-358, 384-394) and the plain timemask / freqmask (:476-484,
    :500-507): region sizes from ``Random(step+131071).uniform``, positions from
    ``Random(step+13119).uniform``; the time span is a fraction of each sample's own cycle length
    (``int(frac * f[-1])``), the frequency span is one row range for the whole batch,
    ``h1 = int(n_rows * u)``, ``h2 = min(n_rows, h1 + int(gap * n_rows))``.  ``n_rows`` is the row
    axis the caller's kernel applies the rectangle to: the durmix variants pass the flattened
    (channel, frequency) axis of the splice (the reference's images have one channel), the plain
    names F (``spec_dim1 = data.shape[2]``), applied within every channel as ``d[:, h1:h2]`` does.
    Columns are not clipped here."""
    def clamp01(v):
        return min(max(v, 0), 1)
    t_max = f_max = 0.2
    key = (name[len("durmix"):] if name.startswith("durmix") else name) + "("
    parts = method.split(key)
    if len(parts) > 1:
        if name == "durmixcutout":
            t_max = clamp01(float(parts[1].split(",")[0]))
            f_max = clamp01(float(method.split(",")[1].split(")")[0]))
        else:
            t_max = f_max = clamp01(float(parts[1].split(")")[0]))
    B = frames.shape[0]
    rect = np.zeros((B, 4), dtype=np.int32)
    rect[:, 1] = n_rows
    rect[:, 3] = n_cols
    if name in ("durmixcutout", "durmixtimemask", "timemask"):
        gap = random.Random(step + 131071).uniform(0, t_max)
        frac1 = random.Random(step + 13119).uniform(0, 1 - gap)
        frac2 = frac1 + gap
        beat = frames[:, 4].astype(np.float64)
        rect[:, 2] = (frac1 * beat).astype(np.int64)          # int() truncation
        rect[:, 3] = (frac2 * beat).astype(np.int64)
    if name in ("durmixcutout", "durmixfreqmask", "freqmask"):
        fgap = random.Random(step + 131071).uniform(0, f_max)
        h1 = int(n_rows * random.Random(step + 13119).uniform(0, 1 - fgap))
        rect[:, 0] = h1
        rect[:, 1] = min(n_rows, h1 + int(fgap * n_rows))
    return rect


# ---- numpy's global stream: lambda and the warp knots ---------------------------------------------
_NPDRAW = None        # (handle, lam, knots pointer, hit) of the process-wide draw object
_NP_GLOBAL = None     # (bit generator of numpy's global RandomState, address of its MT19937 state)


def _npdraw():
    global _NPDRAW
    if _NPDRAW is None:
        import ctypes
        import os
        h = ctypes.c_void_p()
        look = max(0, min(3, int(os.environ.get("PCGMIX_NPDRAW_LOOKAHEAD", "2"))))
        if _lib.load().pcgmix_npdraw_create(ctypes.byref(h), look):
            raise RuntimeError("pcgmix_npdraw_create failed")
        _NPDRAW = (h, ctypes.c_double(), ctypes.c_void_p(), ctypes.c_int())
    return _NPDRAW


def _numpy_global_state():
    """(lock, address) of the MT19937 state behind ``np.random.seed/beta/normal``, or None when
    the global RandomState runs on another bit generator (``np.random.set_bit_generator``)."""
    global _NP_GLOBAL
    bg = np.random.get_bit_generator()
    if _NP_GLOBAL is None or _NP_GLOBAL[0] is not bg:
        addr = bg.ctypes.state_address if type(bg).__name__ == "MT19937" else None
        _NP_GLOBAL = (bg, bg.lock, addr)
    return _NP_GLOBAL[1], _NP_GLOBAL[2]


def draw_lambda_knots(step: int, alpha: float, sigma: float, count: int):
    """``np.random.seed(step); lam = np.random.beta(alpha, alpha)`` (augmentations.py:661-663) and,
    for ``count`` > 0, ``np.random.normal(1.0, sigma, count)`` right behind it (:677) — the same
    doubles, and numpy's GLOBAL stream left exactly where the reference leaves it (asserted by
    tests/test_host_logic.py against numpy itself).  Returns (lam, knots) with knots = the host
    address of ``count`` float64 (library memory, valid until the next call), an ndarray on the
    fallback path, or None.

    The 6144 normals of a (256, 6, 4) block cost numpy ~110 us per step — ten times the kernel they
    feed.  The library restates the legacy stream (csrc/pcgmix_nprand.hip) and draws the blocks of
    the NEXT steps on worker threads (they depend on (step, alpha, sigma, count) only); a matching
    call picks its block up and writes the final generator state into numpy's own state memory.
    Outside that restatement's contract (alpha <= 0: the reference does not seed; alpha > 1:
    gamma-based beta; an odd count: numpy's Gaussian cache would be left full; a foreign bit
    generator) the draws are numpy's own calls."""
    if count == 0 and alpha > 0.0:          # plain splice: numpy's own two calls, nothing else (0.5 us less)
        np.random.seed(step)
        return float(np.random.beta(alpha, alpha)), None
    lock, addr = _numpy_global_state()
    if 0.0 < alpha <= 1.0 and count > 0 and not (count & 1) and addr is not None \
            and 0 <= step <= 0xFFFFFFFF:
        import ctypes
        h, lam, kp, hit = _npdraw()
        np.random.seed(step)                # key (overwritten below) AND the empty Gaussian cache
        with lock:
            err = _lib.load().pcgmix_npdraw_step(h, step, alpha, sigma, count, addr,
                                                 ctypes.byref(lam), ctypes.byref(kp), ctypes.byref(hit))
        if err:
            raise RuntimeError("pcgmix_npdraw_step refused a draw inside its contract")
        return lam.value, kp.value
    if alpha > 0.0:
        np.random.seed(step)                # global stream, as the reference (side effect kept)
        lam = float(np.random.beta(alpha, alpha))
    else:
        lam = 1.0
    knots = np.random.normal(loc=1.0, scale=sigma, size=count) if count else None
    return lam, knots


def knots_array(knots, shape) -> np.ndarray:
    """``draw_lambda_knots``'s knots as an owned float64 array of ``shape`` (as numpy fills it)."""
    if isinstance(knots, np.ndarray):
        return knots.reshape(shape)
    import ctypes
    n = int(np.prod(shape))
    return np.frombuffer((ctypes.c_double * n).from_address(knots), dtype=np.float64).reshape(shape).copy()


def validate_frames(frames: np.ndarray, sig_len: int) -> None:
    """The reference silently mis-slices (and usually raises a shape error) when a cycle runs
    past the padded length; refuse such input up front."""
    if frames.ndim != 2 or frames.shape[1] != 5:
        raise ValueError(f"frames must be (B, 5), got {frames.shape}")
    if frames.size == 0:
        return
    if (frames[:, 1:] < frames[:, :-1]).any() or int(frames.min()) < 0:
        raise ValueError("frames must be non-decreasing and non-negative")
    if int(frames.max()) > sig_len:
        raise ValueError(f"heart cycle ends at {int(frames.max())} > signal length {sig_len}")


def make_plan(method: str, labels, frames: np.ndarray, wav: Sequence[str], step: int,
              batch: int, channels: int, is2d: bool = False, n_cols: int = 0,
              sample_rate=None, sig_len: Optional[int] = None,
              n_freq: Optional[int] = None) -> MixPlan:
    """Everything random/integer for one step, in the reference's RNG order.

    ``labels`` may be an array or a zero-argument callable returning one: they are needed only
    when the gate fires (on a GPU they cost a device->host sync, augmentations.py:501), so a
    callable lets rejected steps skip the sync.  ``sample_rate`` (``args.sample_rate``) and
    ``sig_len`` (T) are needed by respiratoryscale; timemask clips its spans to ``sig_len``.
    The 2D baselines need the image's F (``n_freq``) and W (``n_cols``); ``channels`` is then C."""
    r = _waveform_route(method, is2d)
    name = r.branch
    if name is None or not gate_fires(method, step):
        return MixPlan(fired=False, step=step)
    if frames.shape[0] != batch:
        raise ValueError("labels/frames do not match the batch size")
    plan = MixPlan(fired=True, name=name, step=step, is2d=is2d, kind=_plan_kind(r, is2d))
    if is2d and plan.kind != "splice":
        if n_freq is None or n_cols <= 0:
            raise ValueError("2D baselines need make_plan(..., n_freq=F, n_cols=W)")
        return _baseline_plan_2d(plan, method, labels, frames, step, batch, int(n_freq), int(n_cols))
    if plan.kind != "splice":
        return _baseline_plan(plan, method, labels, frames, step, batch, channels, sample_rate,
                              sig_len)
    # numpy's global stream first (lambda, then the warp knots right behind it): neither depends
    # on the labels, and python's random.Random (partners, offsets, masks) is a separate stream,
    # so the order BETWEEN the two streams is free — a callable `labels` that has to wait for the
    # GPU is asked as late as possible, after the ~0.1 ms of normal draws.
    alpha = 1.0 if is2d else parse_alpha(method, name)                      # augmentations2d.py:411
    sigma, knot = parse_warp(method, name) if (not is2d and name == "durmixmagwarp") else (0.0, -2)
    # seed -> beta (augmentations.py:661-663) -> normal right behind it (:677)
    plan.lam64, knots = draw_lambda_knots(step, alpha, sigma, batch * (knot + 2) * channels)
    plan.lam32 = np.float32(plan.lam64)                                     # augmentations.py:903
    if knot + 2:
        plan.n_knots = knot + 2
        plan.knots = knots_array(knots, (batch, knot + 2, channels))
    plan.mix = partner_indices(method, _host_labels(labels, batch), wav, step, is2d)
    if is2d and name != "durratiomixup":
        plan.zero_rect = mask_rectangles(method, name, frames, step, channels, n_cols)
    if not is2d and "(rand)" in method and "(salopt" not in method:
        plan.rand_off = rand_offsets(frames, plan.mix, step)
    # saliency-guided placement: 1D augmentations.py:905-913; 2D only under durratiomixup
    # (augmentations2d.py:416-423 — the mask variants never look at '(salopt')
    if (not is2d or name == "durratiomixup") and "(salopt" in method:
        plan.salopt_mode = _salopt_mode(method)
    if not is2d:
        plan.mix_all = "(mixAll)" in method
    return plan


def _baseline_plan(plan: MixPlan, method: str, labels, frames: np.ndarray, step: int, batch: int,
                   channels: int, sample_rate, sig_len: Optional[int]) -> MixPlan:
    """make_plan's part for the comparison baselines; the gate has fired."""
    name = plan.name
    if name == "mixup":
        # get_lambda(alpha=1): np.random.seed(step); beta(1, 1) (augmentations.py:841, 851)
        plan.lam64, _ = draw_lambda_knots(step, 1.0, 0.0, 0)
        plan.lam32 = np.float32(plan.lam64)
        labels = _host_labels(labels, batch)
        if "(same)" in method:                                    # augmentations.py:840
            plan.mix = shuffle_within_groups(labels.astype(np.int64, copy=False), step)
        else:                                                     # '(mix)', augmentations.py:850
            plan.mix = shuffle_within_groups(np.zeros(batch, dtype=np.int64), step)
            plan.mix_all = True
    elif name in ("magnitudewarp", "timewarp"):
        sigma, knot = parse_warp(method, name)
        if not 2 <= knot + 2 <= 64:
            raise ValueError(f"{name}: {knot + 2} spline knots, the kernels take 2..64")
        # np.random.normal(1, sigma, (B, knot+2, C)) from numpy's global stream AS IT IS: no
        # reseeding (augmentations.py:677, 688)
        _, knots = draw_lambda_knots(step, 0.0, sigma, batch * (knot + 2) * channels)
        plan.n_knots = knot + 2
        plan.knots = knots_array(knots, (batch, knot + 2, channels)) if knots is not None \
            else np.zeros((0, knot + 2, channels))
    elif name == "timemask":
        plan.spans = mask_spans(method, frames, step, 2**31 - 1 if sig_len is None else sig_len)
    elif name == "respiratoryscale":
        if sample_rate is None or sig_len is None:
            raise ValueError("respiratoryscale needs make_plan(..., sample_rate=, sig_len=)")
        plan.scale_row = respiration_row(parse_respscale(method), step, int(sig_len), sample_rate)
    return plan


def _host_labels(labels, batch: int) -> np.ndarray:
    if callable(labels):
        labels = labels()
    labels = np.asarray(labels).reshape(-1)
    if labels.shape[0] != batch:
        raise ValueError("labels/frames do not match the batch size")
    return labels


def _baseline_plan_2d(plan: MixPlan, method: str, labels, frames: np.ndarray, step: int, batch: int,
                      F: int, W: int) -> MixPlan:
    """make_plan's part for the spectrogram baselines (augmentations2d.py:461-617); the gate has
    fired.  numpy's global stream is drawn by mixup and latentmixup only (get_lambda)."""
    name = plan.name
    if name in ("timemask", "freqmask"):                          # :476-484, :500-507
        rect = mask_rectangles(method, name, frames, step, F, W)
        rect[:, 2:] = np.clip(rect[:, 2:], 0, W)                  # the reference's slice clips
        plan.zero_rect = rect
        return plan
    lib = _lib.load()
    if name == "mixup" and "(same)" not in method:                # '(mix)': Random(step).sample, :560
        plan.mix = shuffle_within_groups(np.zeros(batch, dtype=np.int64), step)
        plan.mix_all = True
    else:                                                         # get_same_label_mix_indices
        plan.mix = shuffle_within_groups(_host_labels(labels, batch).astype(np.int64, copy=False), step)
    if name in ("mixup", "latentmixup"):
        if name == "latentmixup":                                 # Random(step).randint(1, 3), :522
            plan.depth = 1 + int(lib.pcgmix_py_randint0(int(step), 2))
        plan.lam64, _ = draw_lambda_knots(step, 1.0, 0.0, 0)      # get_lambda(alpha=1), :527, :551
        plan.lam32 = np.float32(plan.lam64)
        return plan
    # cutmix / durratiocutmix read state boundaries: refused beyond the image, as the splice does
    validate_frames(np.asarray(frames), W)
    f1 = np.asarray(frames, dtype=np.int64)
    if name == "cutmix":
        plan.cut = 1 + int(lib.pcgmix_py_randint0(int(step) * 131071, 2)) if "(rand)" in method else 2
        plan.segs = cutmix_segments(f1, plan.mix, plan.cut, F)
        plan.out_cols = F
        return plan
    if W != F:
        # data_new is (B, C, F, F) (augmentations2d.py:609) and receives a (C, F, W) d1.clone():
        # torch refuses the assignment unless W == F
        raise ValueError(f"durratiocutmix: the reference writes (C, F, W) = (.., {F}, {W}) samples into "
                         f"(C, F, F) slots, which torch refuses unless W == F")
    plan.out_cols = W
    if "(rand)" in method:
        plan.segs = rand_keepdur_segments(f1, plan.mix, rand_offsets(f1, plan.mix, step, (1, 3)), F)
        plan.seg_axis = 1
    else:
        plan.segs = keepdur_segments(f1, plan.mix, W)
    return plan


_OWN, _PARTNER, _ZERO = 0, 1, 2        # PCGMIX_PIECE_* (include/pcgmix_hip.h)


def _segment_table(bounds, kinds, shifts) -> np.ndarray:
    """int32 (B, 5, 4) {lo, hi, src, shift} from the 6 boundaries (B each) of 5 contiguous segments."""
    B = bounds[0].shape[0]
    segs = np.zeros((B, 5, 4), dtype=np.int32)
    for k in range(5):
        segs[:, k, 0] = bounds[k]
        segs[:, k, 1] = bounds[k + 1]
        segs[:, k, 2] = kinds[k]
        segs[:, k, 3] = shifts[k]
    return segs


def cutmix_segments(frames: np.ndarray, mix: np.ndarray, cut: int, F: int) -> np.ndarray:
    """cutmix_multidim_tensors (augmentations2d.py:34-51) as a column table of the (F, F) output:
    ``[0, f1[cut])`` own, ``[f1[cut], last)`` the partner from ``f2[cut]`` on, zero behind ``last =
    min(f1[cut] + f2[4] - f2[cut], F)`` — the cap is spec_dim2 = data.shape[2] = F, not W.  With
    ``f1[cut] > F`` (possible when F < W) the reference's own-part assignment has mismatched shapes:
    ValueError, as torch raises there."""
    f2 = frames[mix]
    a = frames[:, cut]
    if (a > F).any():
        raise ValueError(f"cutmix: a cut at column {int(a.max())} > F = {F}: the reference copies "
                         f"{int(a.max())} columns into an F-column slot and torch raises")
    last = np.minimum(a + f2[:, 4] - f2[:, cut], F)
    full = np.full_like(a, F)
    zero = np.zeros_like(a)
    return _segment_table((zero, a, last, full, full, full), (_OWN, _PARTNER, _ZERO, _ZERO, _ZERO),
                          (zero, f2[:, cut] - a, zero, zero, zero))


def keepdur_segments(frames: np.ndarray, mix: np.ndarray, W: int) -> np.ndarray:
    """cutmix_keepdur_multidim_tensors without '(rand)' (augmentations2d.py:225-231): systole and
    diastole columns, over the shorter of the two lengths, from the partner; a column table."""
    f2 = frames[mix]
    n_sys = np.minimum(frames[:, 2] - frames[:, 1], f2[:, 2] - f2[:, 1])
    n_dia = np.minimum(frames[:, 4] - frames[:, 3], f2[:, 4] - f2[:, 3])
    s0, d0 = frames[:, 1], frames[:, 3]
    zero = np.zeros_like(s0)
    return _segment_table((zero, s0, s0 + n_sys, d0, d0 + n_dia, np.full_like(s0, W)),
                          (_OWN, _PARTNER, _OWN, _PARTNER, _OWN),
                          (zero, f2[:, 1] - s0, zero, f2[:, 3] - d0, zero))


def rand_keepdur_segments(frames: np.ndarray, mix: np.ndarray, off: np.ndarray, F: int) -> np.ndarray:
    """'(rand)durratiocutmix' (augmentations2d.py:232-248) as a table along F: the reference slices
    ``d_new[:, a:b]`` on a (C, F, W) sample, so it swaps whole FREQUENCY rows ``[a, b)`` (every column)
    with the partner's rows at a shift.  ``off`` = ``rand_offsets``: ``Random(step).randint(0, |gap|)``
    with ``gap = len2 - len1``; gap >= 0 shifts the partner's rows, gap < 0 the sample's own.  With
    W == F and boundaries within W, both sides of every slice lie inside the image, so torch never
    clips one side differently from the other."""
    f2 = frames[mix]
    out = []
    for k in (1, 3):                                   # systole, diastole
        l1 = frames[:, k + 1] - frames[:, k]
        l2 = f2[:, k + 1] - f2[:, k]
        ge = l2 - l1 >= 0
        s = off[:, k].astype(np.int64)
        t0 = np.where(ge, frames[:, k], frames[:, k] + s)
        src0 = np.where(ge, f2[:, k] + s, f2[:, k])
        out.append((t0, t0 + np.minimum(l1, l2), src0 - t0))
    (a0, a1, sa), (b0, b1, sb) = out
    zero = np.zeros_like(a0)
    return _segment_table((zero, a0, a1, b0, b1, np.full_like(a0, F)),
                          (_OWN, _PARTNER, _OWN, _PARTNER, _OWN),
                          (zero, sa, zero, sb, zero))


# ---- the cut-and-paste family, durmixrespscale and bare cutout --------------------------------------
_KEEPDUR_1D = ("wav-durratiocutmix", "durratiocutmix")
CUTPASTE_MAX_OVERLAP = 10          # PCGMIX_CUTPASTE_MAX_OVERLAP: cutmix_multidim_tensors' overlap=10


def cutpaste_recipe(method: str, is2d: bool = False) -> Optional[str]:
    """The branch name when the reference's if-chain reaches, for ``method``, one of the branches
    ``cutpaste_plan`` serves — the heart-cycle cut-and-paste methods, ``durmixrespscale`` and bare
    ``cutout`` in 1D (``CUTPASTE_METHODS_1D``), bare ``cutout`` in 2D — and None otherwise (an
    earlier branch takes the string, or a later one, or none)."""
    r = route(method, is2d)
    return r.branch if r.family == "cutpaste" else None


@functools.lru_cache(maxsize=16)
def sigmoid_table() -> np.ndarray:
    """float64 (10, 20): row ov-1 holds the reference's ``sigmoid(ov)`` (augmentations.py:668-672) in
    its first 2*ov entries, computed with numpy as the reference computes it."""
    tab = np.zeros((CUTPASTE_MAX_OVERLAP, 2 * CUTPASTE_MAX_OVERLAP), dtype=np.float64)
    for ov in range(1, CUTPASTE_MAX_OVERLAP + 1):
        row = np.array([1.0 / (1.0 + np.exp(-x)) for x in np.linspace(-8, 8, ov * 2)])
        row[0] = 0
        row[-1] = 1
        tab[ov - 1, :2 * ov] = row
    tab.setflags(write=False)
    return tab


def length_bin_keys(method: str, labels: np.ndarray, frames: np.ndarray, batch_size: int) -> np.ndarray:
    """get_same_length_mix_indices' grouping key (augmentations.py:558-575): (label, length bin) with
    ``num_bins = batch_size//100`` ('(5bins)', '(10bins)'), the bins through numpy itself."""
    lengths = [int(v) for v in frames[:, -1]]
    num_bins = int(batch_size) // 100
    if "(5bins)" in method:
        num_bins = 5
    if "(10bins)" in method:
        num_bins = 10
    bins = np.linspace(np.min(lengths) - 1, np.max(lengths) + 1, num_bins + 1)
    bins_inds = np.digitize(lengths, bins).astype(np.int64)
    return labels.astype(np.int64) * (int(bins_inds.max()) + 1) + bins_inds


def cutout_spans(frames: np.ndarray, step: int, sig_len: int, channels: int, per_channel: bool) -> np.ndarray:
    """Bare 1D cutout (augmentations.py:1594-1615): int32 (B, 2), or (B*C, 2) for '(ch)'.  The
    parameters in the method string are ignored, as the reference ignores them."""
    beat = np.asarray(frames)[:, -1].astype(np.float64)
    if per_channel:
        fr = np.array([sorted(random.Random(step + i * 131071 + c * 524287).uniform(0, 1) for i in range(2))
                       for c in range(channels)])                              # (C, 2)
        spans = (fr[None, :, :] * beat[:, None, None]).astype(np.int64).reshape(-1, 2)
    else:
        gap = random.Random(step + 131071).uniform(0, 0.05)
        frac1 = random.Random(step + 13119).uniform(0, 1 - gap)
        frac2 = frac1 + gap
        spans = np.stack([(frac1 * beat).astype(np.int64), (frac2 * beat).astype(np.int64)], axis=1)
    return np.clip(spans, 0, sig_len).astype(np.int32)


def cutmix_cutout_segments(frames: np.ndarray, mix: np.ndarray, cut: int, T: int, cut_frac) -> np.ndarray:
    """``cutmix_segments`` with the 'cutout' suffix of the four 1D cutmix branches (e.g. :1143-1148):
    ``[int(cf0*last), int(cf1*last))`` zeroed after the paste, ``last`` = the new cycle's end."""
    f2 = frames[mix]
    a = frames[:, cut]
    last = np.minimum(a + f2[:, 4] - f2[:, cut], T)
    z0 = (cut_frac[0] * last.astype(np.float64)).astype(np.int64)              # int() truncation
    z1 = (cut_frac[1] * last.astype(np.float64)).astype(np.int64)
    pts = np.sort(np.stack([np.zeros_like(a), a, z0, z1, last], axis=1), axis=1)
    B = a.shape[0]
    segs = np.zeros((B, 5, 4), dtype=np.int32)
    for k in range(5):
        lo = pts[:, k]
        hi = pts[:, k + 1] if k < 4 else np.full_like(a, T)
        zero = ((lo >= z0) & (lo < z1)) | (lo >= last)
        partner = ~zero & (lo >= a)
        segs[:, k, 0] = lo
        segs[:, k, 1] = hi
        segs[:, k, 2] = np.where(zero, _ZERO, np.where(partner, _PARTNER, _OWN))
        segs[:, k, 3] = np.where(partner, f2[:, cut] - a, 0)
    return segs


def smooth_junctions(frames: np.ndarray, mix: np.ndarray, cut: int) -> np.ndarray:
    """'(smooth)' (augmentations.py:41-51): int32 (B, 4) {f1[cut], f2[cut], ov, 0} with ``ov = min(10,
    f1[cut], f2[4]-f2[cut], f1[4]-f1[cut], f2[cut])``.  ``ov == 0`` makes the reference index an empty
    array inside ``sigmoid``: IndexError, raised here before anything is launched."""
    f2 = frames[mix]
    a, c2 = frames[:, cut], f2[:, cut]
    ov = np.minimum.reduce([np.full_like(a, CUTPASTE_MAX_OVERLAP), a, f2[:, 4] - c2, frames[:, 4] - a, c2])
    if (ov <= 0).any():
        raise IndexError("(smooth): a part next to the junction is empty (overlap 0); the reference "
                         "raises IndexError in sigmoid(0)")
    return np.stack([a, c2, ov, np.zeros_like(a)], axis=1).astype(np.int32)


def _validate_cycles(frames: np.ndarray, sig_len: int) -> None:
    validate_frames(frames, sig_len)
    if frames.size and (frames[:, 0] != 0).any():
        raise ValueError("frames[:, 0] must be 0 (a heart cycle starts at its first sample)")


def cutpaste_plan(method: str, labels, frames: np.ndarray, wav: Optional[Sequence[str]], step: int,
                  batch: int, channels: int, sig_len: int, is2d: bool = False,
                  batch_size: Optional[int] = None, sample_rate=None, n_freq: Optional[int] = None,
                  n_cols: int = 0) -> MixPlan:
    """Host part of one step of a ``cutpaste_recipe`` method, in the reference's RNG order: gate,
    partners, cut, 'cutout' fractions; for durmixrespscale gate, partners, ``get_lambda`` (numpy's
    global stream, only when the gate fires), '(rand)' offsets, the sinusoid.  ``labels``: array or
    zero-argument callable (asked after the gate).  1D: ``sig_len`` = T; ``batch_size`` =
    ``args.batch_size`` (lengthcutmix), ``sample_rate`` = ``args.sample_rate`` (durmixrespscale).
    2D: ``n_freq`` = F, ``n_cols`` = W."""
    r = route(method, is2d)
    if r.family != "cutpaste":
        raise ValueError(f"{method!r} reaches none of the branches cutpaste_plan serves")
    name = r.branch
    if not gate_fires(method, step):
        return MixPlan(fired=False, step=step)
    frames = np.asarray(frames)
    if frames.ndim != 2 or frames.shape != (batch, 5):
        raise ValueError("labels/frames do not match the batch size")
    kind = "cutout2d" if is2d else name if name == "cutout" else \
        "mixscale" if name == "durmixrespscale" else "cutpaste"
    plan = MixPlan(fired=True, name=name, step=step, is2d=is2d, kind=kind)
    if is2d:                                                   # augmentations2d.py:429-459
        if n_freq is None or n_cols <= 0:
            raise ValueError("2D cutout needs cutpaste_plan(..., n_freq=F, n_cols=W)")
        rect = mask_rectangles(method, "durmixcutout", frames, step, int(n_freq), int(n_cols))
        rect[:, 2:] = np.clip(rect[:, 2:], 0, int(n_cols))     # the reference's slice clips
        plan.zero_rect = rect
        return plan
    if name == "cutout":                                       # :1569-1616
        per_ch = "(ch)" in method
        plan.spans = cutout_spans(frames, step, sig_len, channels, per_ch)
        plan.span_rows = channels if per_ch else 1
        return plan
    _validate_cycles(frames, sig_len)
    f1 = frames.astype(np.int64, copy=False)
    lab = lambda: _host_labels(labels, batch).astype(np.int64, copy=False)   # noqa: E731
    if name == "durmixrespscale":                              # :734-775
        if "(sameCVD)" in method:
            raise NotImplementedError("partner selector '(sameCVD)' needs the reference's private CVD table")
        if sample_rate is None:
            raise ValueError("durmixrespscale needs cutpaste_plan(..., sample_rate=)")
        plan.mix = shuffle_within_groups(lab(), step)
        plan.lam64, _ = draw_lambda_knots(step, 1.0, 0.0, 0)   # get_lambda(alpha=1)
        plan.lam32 = np.float32(plan.lam64)
        if "(rand)" in method:
            plan.rand_off = rand_offsets(f1, plan.mix, step)
        plan.scale_row = respiration_row(parse_respscale(method, name), step, int(sig_len), sample_rate)
        return plan
    if wav is None and name in ("wav-durratiocutmix", "wavcutmix", "datasetcutmix"):
        raise ValueError(f"{name} groups the batch by recording: it needs wav")
    if name in ("wav-durratiocutmix", "wavcutmix"):            # get_same_wav_mix_indices, :528
        if len(wav) != batch:
            raise ValueError("wav does not match the batch size")
        plan.mix = shuffle_within_groups(list(wav), step)
    elif name == "datasetcutmix":                              # get_same_dataset_mix_indices, :542
        if len(wav) != batch:
            raise ValueError("wav does not match the batch size")
        plan.mix = shuffle_within_groups([f"{w[0]}_{int(t)}" for w, t in zip(wav, lab())], step)
    elif name == "lengthcutmix":                               # get_same_length_mix_indices, :558
        if batch_size is None:
            raise ValueError("lengthcutmix needs args.batch_size (cutpaste_plan(..., batch_size=))")
        plan.mix = shuffle_within_groups(length_bin_keys(method, lab(), f1, batch_size), step) \
            if batch else np.zeros(0, np.int64)
    else:                                                      # get_same_label_mix_indices
        plan.mix = shuffle_within_groups(lab(), step)
    if name in _KEEPDUR_1D:                                    # cutmix_keepdur_multidim_tensors, :340
        if "(rand)" in method:
            plan.segs = rand_keepdur_segments(f1, plan.mix, rand_offsets(f1, plan.mix, step, (1, 3)),
                                              sig_len)
        else:
            plan.segs = keepdur_segments(f1, plan.mix, sig_len)
        return plan
    lib = _lib.load()
    plan.cut = 2                                               # cutmix_multidim_tensors, :30
    if "(rand)" in method:                                     # :1139 / :1303
        seed = int(step) * 131071 if name == "labelcutmix" else int(step)
        plan.cut = 1 + int(lib.pcgmix_py_randint0(seed, 2))
    if "cutout" in method:
        cut_frac = sorted(random.Random(step + i * 131071).uniform(0, 1) for i in range(2))
        plan.segs = cutmix_cutout_segments(f1, plan.mix, plan.cut, sig_len, cut_frac)
    else:
        plan.segs = cutmix_segments(f1, plan.mix, plan.cut, sig_len)
    if "(smooth)" in method:
        plan.junctions = smooth_junctions(f1, plan.mix, plan.cut)
    return plan


def _gpu_numa_node(torch, index):
    pr = torch.cuda.get_device_properties(index)
    bus = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
    with open("/sys/bus/pci/devices/%s/numa_node" % bus) as f:
        return bus, int(f.read())


def _slice_for(cpus, ordinal, n_cpus):
    """``n_cpus`` of a node's CPU list for the ``ordinal``-th GPU of that node.  The first half of
    the list are the physical cores where SMT siblings are listed behind them; the node's first
    eight CPUs (interrupts, housekeeping) are left alone when there is room."""
    phys = cpus[:max(2, len(cpus) // 2)]
    n = max(2, min(n_cpus, len(phys)))
    usable = phys[8:] if len(phys) - 8 >= n else phys
    slot = ordinal % max(1, len(usable) // n)
    return usable[slot * n:(slot + 1) * n]


def bind_host_threads(device_index: int = 0, local_rank: int = 0, n_cpus: int = 8) -> str:
    """Pin the calling process to ``n_cpus`` CPUs of the NUMA node its GPU hangs off (a slice of its
    own for each GPU of that node), and say what was done.  Threads created afterwards — the
    draw-ahead workers of §3.6 — inherit the mask.  The strict-signature step is a host loop with one
    device->host hand-over per call: left to the scheduler on a two-socket box the process migrates
    between 256 CPUs and the step is 22.7-24.4 us; on four CPUs next to the GPU 20.4-20.5 us, on the
    remote socket 22.6-22.7 (MI355X box, ``profiles/r4_host_affinity.txt``).  The reference does not
    pin anything; a launcher would normally do this (``numactl``), ``torch.distributed.run`` does
    not.  ``local_rank`` only breaks ties where the other GPUs' nodes cannot be read.  No-op (with
    the reason in the returned string) wherever the topology cannot be read or leaves fewer than two
    CPUs."""
    import os
    if not hasattr(os, "sched_setaffinity"):
        return "no affinity API"
    try:
        import torch
        bus, node = _gpu_numa_node(torch, device_index)
        if node < 0:
            return "GPU %s reports no NUMA node" % bus
        try:        # which of this node's GPUs am I (device properties only: no context is created)
            ordinal = sum(1 for j in range(device_index) if _gpu_numa_node(torch, j)[1] == node)
        except Exception:
            ordinal = local_rank
        with open("/sys/devices/system/node/node%d/cpulist" % node) as f:
            cpus = []
            for part in f.read().strip().split(","):
                if "-" in part:
                    a, b = part.split("-")
                    cpus += list(range(int(a), int(b) + 1))
                elif part:
                    cpus.append(int(part))
    except Exception as exc:                                   # no sysfs, no such device, ...
        return "topology not readable (%s)" % type(exc).__name__
    allowed = os.sched_getaffinity(0)
    cpus = [c for c in cpus if c in allowed]
    if len(cpus) < 2:
        return "fewer than two CPUs of node %d allowed" % node
    chosen = _slice_for(cpus, ordinal, n_cpus)
    os.sched_setaffinity(0, chosen)
    return "GPU %s on NUMA node %d: pinned to CPUs %d-%d" % (bus, node, chosen[0], chosen[-1])
