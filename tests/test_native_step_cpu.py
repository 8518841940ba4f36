"""The compiled entry point of the armed plain step (csrc/pcgmix_pystep.cpp) without a GPU: it is built and
bound, it declines every input it does not serve — returning None and raising nothing, so the Python path
reports what it always reported — and a declined call leaves every reference count where it was."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, augmentations, hostprep

B = 6
PLAIN = hostprep.plain_recipe("durratiomixup", False)
GATED = hostprep.plain_recipe("durratiomixup+0.5", False)
WARP = hostprep.plain_recipe("durmixmagwarp(0.2,4)", False)


def _good():
    """Arguments that only lack a HIP device."""
    return dict(recipe=PLAIN, data=torch.zeros(B, 2, 16), ohe=torch.zeros(B, 2, dtype=torch.int64),
                frames=torch.zeros(B, 5, dtype=torch.int64), step=3, host_labels=None)


def _call(a):
    return augmentations._native_step(a["recipe"], a["data"], a["ohe"], a["frames"], a["step"], a["host_labels"])


INELIGIBLE = {
    "data on the CPU": {},
    "data float64": {"data": torch.zeros(B, 2, 16, dtype=torch.float64)},
    "data not contiguous": {"data": torch.zeros(B, 16, 2).transpose(1, 2)},
    "data 2-D": {"data": torch.zeros(B, 16)},
    "data no tensor": {"data": np.zeros((B, 2, 16), np.float32)},
    "empty batch": {"data": torch.zeros(0, 2, 16), "ohe": torch.zeros(0, 2, dtype=torch.int64),
                    "frames": torch.zeros(0, 5, dtype=torch.int64)},
    "one-hot int32": {"ohe": torch.zeros(B, 2, dtype=torch.int32)},
    "one-hot 1-D": {"ohe": torch.zeros(B, dtype=torch.int64)},
    "one-hot of another batch": {"ohe": torch.zeros(B + 1, 2, dtype=torch.int64)},
    "frames (B, 4)": {"frames": torch.zeros(B, 4, dtype=torch.int64)},
    "frames int32": {"frames": torch.zeros(B, 5, dtype=torch.int32)},
    "frames int32 ndarray": {"frames": np.zeros((B, 5), np.int32)},
    "frames (B, 4) ndarray": {"frames": np.zeros((B, 4), np.int64)},
    "frames strided ndarray": {"frames": np.zeros((B, 10), np.int64)[:, ::2]},
    "frames a list": {"frames": [[0, 1, 2, 3, 4]] * B},
    "host labels given": {"host_labels": np.zeros(B, np.int64)},
    "recipe with knots": {"recipe": WARP},
    "no recipe": {"recipe": None},
    "step -1": {"step": -1},
    "step 2**32": {"step": 2 ** 32},
    "step no int": {"step": 3.0},
}


def test_module_is_built_and_bound():
    assert _lib.native_step_loaded()
    assert augmentations._native_step is sys.modules[_lib.__package__ + "._pcgmix_step"].step
    assert PLAIN == ("durratiomixup", 1.0, 1.0, 0.0, 0) and GATED[1] == 0.5 and WARP[4] > 0


@pytest.mark.parametrize("case", sorted(INELIGIBLE))
def test_ineligible_input_is_declined(case):
    a = dict(_good(), **INELIGIBLE[case])
    assert _call(a) is None
    a["recipe"] = GATED if a["recipe"] is PLAIN else a["recipe"]
    assert _call(a) is None


def test_taped_step_is_declined(monkeypatch):
    monkeypatch.setattr(_lib, "TAPE", [])
    assert _call(_good()) is None
    assert _lib.TAPE == []


def test_wrong_argument_count_is_an_error():
    with pytest.raises(TypeError):
        augmentations._native_step(PLAIN)


def test_declined_calls_leave_every_reference_count_alone():
    cases = [dict(_good(), **INELIGIBLE[k]) for k in sorted(INELIGIBLE)]
    objs = [v for a in cases for v in a.values() if v is not None and not isinstance(v, (int, float))]
    step = augmentations._native_step
    for a in cases:                               # once, so that anything cached on first use exists
        _call(a)
    before = [sys.getrefcount(o) for o in objs]
    none_before = sys.getrefcount(None)
    n = 100000 // len(cases) + 1
    for a in cases:
        r, d, o, f, s, h = a["recipe"], a["data"], a["ohe"], a["frames"], a["step"], a["host_labels"]
        for _ in range(n):
            step(r, d, o, f, s, h)
    del r, d, o, f, s, h
    assert [sys.getrefcount(o) for o in objs] == before
    assert abs(sys.getrefcount(None) - none_before) < 100       # (each decline returns None: handed back)


def test_python_path_reports_what_the_module_declines():
    """Declined means the existing code speaks: the error of a CPU tensor is augment()'s own."""
    from conftest import Args, StepCounter
    a = _good()
    with pytest.raises(ValueError, match="must live on a HIP device"):
        augmentations.augment(Args("durratiomixup"), a["data"], a["ohe"], a["frames"], None, StepCounter(3), None,
                              torch.device("cpu"), "")


def test_native_step_switch_is_one_attribute(monkeypatch):
    from conftest import Args, StepCounter
    monkeypatch.setattr(augmentations, "_native_step", None)
    a = _good()
    with pytest.raises(ValueError, match="must live on a HIP device"):
        augmentations.augment(Args("durratiomixup"), a["data"], a["ohe"], a["frames"], None, StepCounter(3), None,
                              torch.device("cpu"), "")


def test_abort_of_a_null_context_is_refused():
    """pcgmix_augment_plain_abort: hipErrorInvalidValue (1) for NULL; a context with nothing open answers 0
    (tests/test_native_step_gpu.py: a context needs a device)."""
    lib = _lib.load()
    assert lib.pcgmix_augment_plain_abort(None) == 1
    assert lib.pcgmix_abi_version() == _lib.ABI_VERSION == 25
    assert ctypes.cast(lib.pcgmix_augment_plain_abort, ctypes.c_void_p).value
