"""The compiled entry point of the armed plain step against libtorch (csrc/pcgmix_pystep.cpp), without a GPU:
the module is linked against torch's libraries and refuses to load into a process that has not imported
torch; tensors it reaches through THPVariable_Unpack — subclasses, tensors that require grad — are served as
the Python path serves them or declined, never raised; and declined calls leave every reference count alone."""
import os
import subprocess
import sys

import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, augmentations, hostprep

B = 6
PLAIN = hostprep.plain_recipe("durratiomixup", False)
GATED = hostprep.plain_recipe("durratiomixup+0.5", False)


class Wrapped(torch.Tensor):
    """A subclass whose every torch call goes through __torch_function__ (and would raise there)."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        raise AssertionError("the step module reached a tensor subclass through torch: %r" % (func,))


class Plain(torch.Tensor):
    """A subclass that changes nothing."""


def _args(**over):
    a = dict(recipe=PLAIN, data=torch.zeros(B, 2, 16), ohe=torch.zeros(B, 2, dtype=torch.int64),
             frames=torch.zeros(B, 5, dtype=torch.int64), step=3, host_labels=None)
    a.update(over)
    return a


def _call(a):
    return augmentations._native_step(a["recipe"], a["data"], a["ohe"], a["frames"], a["step"], a["host_labels"])


def _cases():
    """Inputs that go through the new unpacking; none can be served here (no HIP device), so all are declined."""
    return {
        "data subclass": _args(data=torch.zeros(B, 2, 16).as_subclass(Wrapped)),
        "one-hot subclass": _args(ohe=torch.zeros(B, 2, dtype=torch.int64).as_subclass(Wrapped)),
        "frames subclass": _args(frames=torch.zeros(B, 5, dtype=torch.int64).as_subclass(Wrapped)),
        "data requires grad": _args(data=torch.zeros(B, 2, 16, requires_grad=True)),
        "data a Parameter": _args(data=torch.nn.Parameter(torch.zeros(B, 2, 16))),
        "data a view that requires grad": _args(data=torch.zeros(B, 2, 32, requires_grad=True)[:, :, :16]),
        "data on the meta device": _args(data=torch.zeros(B, 2, 16, device="meta")),
        "frames on the meta device": _args(frames=torch.zeros(B, 5, dtype=torch.int64, device="meta")),
        "frames 0-d": _args(frames=torch.zeros((), dtype=torch.int64)),
        "data 0-d": _args(data=torch.zeros(())),
        "plain CPU tensors": _args(),
    }


def test_module_names_torch_libraries_among_its_dependencies():
    assert _lib.native_step_loaded()
    with open(_lib.STEP_MODULE_PATH, "rb") as f:
        image = f.read()
    for name in (b"libtorch_python.so", b"libtorch_cpu.so", b"libc10.so"):
        assert name in image, name
    assert os.path.dirname(torch.__file__).encode() in image          # the rpath to torch/lib


def test_module_loads_only_after_torch():
    """A fresh interpreter that has not imported torch gets an ImportError, not a half-working module."""
    code = ("import importlib.util, sys\n"
            "spec = importlib.util.spec_from_file_location('_pcgmix_step', sys.argv[1])\n"
            "try:\n"
            "    importlib.util.module_from_spec(spec)\n"
            "except ImportError as e:\n"
            "    print('refused:', e)\n"
            "else:\n"
            "    print('loaded')\n"
            "print('torch' in sys.modules)\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.STEP_MODULE_PATH], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("refused:") and lines[-1] == "False", r.stdout
    assert "torch" in sys.modules and sys.modules[_lib.__package__ + "._pcgmix_step"].ABI_VERSION == _lib.ABI_VERSION


@pytest.mark.parametrize("case", sorted(_cases()))
def test_unpacked_inputs_are_declined_never_raised(case):
    a = _cases()[case]
    assert _call(a) is None
    assert _call(dict(a, recipe=GATED)) is None


def test_subclass_and_grad_inputs_reach_the_python_path():
    """Declined means augment() speaks: for CPU inputs of either kind that is its own device error."""
    from conftest import Args, StepCounter
    for a in (_args(data=torch.zeros(B, 2, 16).as_subclass(Plain)), _cases()["data requires grad"]):
        assert _call(a) is None
        with pytest.raises(ValueError, match="must live on a HIP device"):
            augmentations.augment(Args("durratiomixup"), a["data"], a["ohe"], a["frames"], None, StepCounter(3),
                                  None, torch.device("cpu"), "")


def test_declined_calls_leave_every_reference_count_alone():
    cases = list(_cases().values())
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
