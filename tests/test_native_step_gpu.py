"""The armed plain step through the compiled entry point (csrc/pcgmix_pystep.cpp) against the Python path
of the same process (``augmentations._native_step = None``): outputs bit for bit, partners, numpy's and
``random``'s streams, ownership, the errors — and the ways out of a waiting kernel, which now go through
pcgmix_augment_plain_abort on both paths.  The kernel is the same on both sides, so the shapes are chosen
for the argument marshalling: the smoke shape, a small odd one, the upper B of the armed form, and one B
above it, where begin answers PCGMIX_NOT_ARMED and the module must hand the step back."""
import ctypes
import random
import sys
import time

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, augmentations, augmentations2d, hostprep, synthetic
from conftest import Args, StepCounter
from oracle import pcgmix_oracle as O

pytestmark = pytest.mark.gpu

METHOD = "durratiomixup"
GATED = "durratiomixup+0.5"
LAST_STEP = 2 ** 32 - 1


def _stats(device):
    out = (ctypes.c_longlong * 3)()
    _lib.check(_lib.load().pcgmix_ctx_armed_stats(augmentations.step_context(device.index), out), "stats")
    return list(out)                               # armed steps | checked after a sync | kernels given up


def _batch(B, C, T, classes, seed):
    """Random rows and any monotone boundaries inside [0, T]; every class column exists."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, C, T)).astype(np.float32)
    frames = np.sort(rs.randint(0, T + 1, (B, 5)), axis=1).astype(np.int64)
    labels = rs.randint(0, classes, B).astype(np.int64)
    return x, frames, labels, ["a%04d" % i for i in range(B)]


_CASES = {}


def _case(name, device):
    """(x, frames, labels, wav, data, tgt) of a shape of the table, made once and never changed."""
    if name not in _CASES:
        if name == "smoke":
            x, frames, labels, wav = synthetic.make_batch(16, 4, 2500, seed=5)
            classes = 2
        else:
            B, C, T, classes = {"odd": (5, 1, 64, 3), "top": (256, 1, 8, 2), "over": (257, 1, 8, 2)}[name]
            x, frames, labels, wav = _batch(B, C, T, classes, seed=B + T)
        data = torch.from_numpy(x).to(device)
        tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), classes).to(device)
        _CASES[name] = (x, frames, labels, wav, data, tgt)
    return _CASES[name]


def _augment(mod, method, data, tgt, frames, wav, step, device):
    return mod.augment(Args(method), data, tgt, frames, wav, StepCounter(step), None, device, "")


def _both_paths(monkeypatch, mod, method, data, tgt, frames, wav, step, device):
    """The step through augment() with the module and without it, each from the same numpy / random state;
    returns both results with the stream states they left."""
    assert _lib.native_step_loaded() and augmentations._native_step is not None
    got = []
    for native in (True, False):
        with monkeypatch.context() as m:
            if not native:
                m.setattr(augmentations, "_native_step", None)
            np.random.seed(12345)
            np.random.standard_normal(3)           # (a Gaussian cached: seed() must drop it on both paths)
            random.seed(99)
            py_state = random.getstate()
            before = _stats(device)
            res = _augment(mod, method, data, tgt, frames, wav, step, device)
            after = _stats(device)
            assert random.getstate() == py_state, "the step touched random's global stream"
            got.append((res, np.random.get_state(), [a - b for a, b in zip(after, before)]))
    return got


def _same_np_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("name", ["smoke", "odd", "top", "over"])
@pytest.mark.parametrize("step", [0, 3, LAST_STEP])
@pytest.mark.parametrize("as_tensor", [True, False], ids=["tensor", "ndarray"])
def test_native_step_equals_python_path(name, step, as_tensor, device, monkeypatch):
    x, frames_np, labels, wav, data, tgt = _case(name, device)
    frames = torch.from_numpy(frames_np) if as_tensor else frames_np
    (nat, nat_np, nat_d), (py, py_np, py_d) = _both_paths(monkeypatch, augmentations, METHOD, data, tgt, frames,
                                                          wav, step, device)
    assert torch.equal(nat[0], py[0]) and nat[0] is not data and nat[0].data_ptr() != py[0].data_ptr()
    assert nat[1] is tgt and py[1] is tgt and nat[3] is None
    assert isinstance(nat[2], np.ndarray) and nat[2].dtype == np.int64 and nat[2].shape == (data.shape[0],)
    assert np.array_equal(nat[2], py[2])
    assert _same_np_state(nat_np, py_np)
    np.random.seed(step)
    np.random.beta(1.0, 1.0)
    assert _same_np_state(nat_np, np.random.get_state()), "numpy's stream is not where the reference leaves it"
    armed = 0 if name == "over" else 1             # B = 257: begin answers not-armed, the one-call route runs
    assert nat_d == [armed, 0, 0] and py_d == [armed, 0, 0]
    if name == "smoke":
        ref = O.augment(METHOD, x, labels, frames_np, wav, step)
        assert np.array_equal(nat[2], ref["mix"])
        assert float(np.abs(nat[0].cpu().numpy() - ref["y"]).max()) <= 1e-4


def test_module_itself_serves_the_step(device):
    """Not through augment(): the module's answer is the tuple, so the comparisons above are not two runs of
    the Python path.  Above the armed B it declines after begin answered not-armed."""
    x, frames, labels, wav, data, tgt = _case("smoke", device)
    recipe = hostprep.plain_recipe(METHOD, False)
    before = _stats(device)
    res = augmentations._native_step(recipe, data, tgt, torch.from_numpy(frames), 3, None)
    assert res is not None and len(res) == 4 and _stats(device)[0] - before[0] == 1
    ref = O.augment(METHOD, x, labels, frames, wav, 3)
    assert np.array_equal(res[2], ref["mix"]) and float(np.abs(res[0].cpu().numpy() - ref["y"]).max()) <= 1e-4
    x, frames, labels, wav, data, tgt = _case("over", device)
    before = _stats(device)
    assert augmentations._native_step(recipe, data, tgt, frames, 3, None) is None
    assert _stats(device) == before


def test_probability_gate(device, monkeypatch):
    x, frames_np, labels, wav, data, tgt = _case("odd", device)
    frames = torch.from_numpy(frames_np)
    fired = next(s for s in range(64) if hostprep.gate_fires(GATED, s))
    rejected = next(s for s in range(64) if not hostprep.gate_fires(GATED, s))
    (nat, nat_np, nat_d), (py, py_np, py_d) = _both_paths(monkeypatch, augmentations, GATED, data, tgt, frames,
                                                          wav, fired, device)
    assert torch.equal(nat[0], py[0]) and np.array_equal(nat[2], py[2]) and _same_np_state(nat_np, py_np)
    assert nat_d == [1, 0, 0] and py_d == [1, 0, 0]
    (nat, nat_np, nat_d), (py, py_np, py_d) = _both_paths(monkeypatch, augmentations, GATED, data, tgt, frames,
                                                          wav, rejected, device)
    for res in (nat, py):
        assert res[0] is data and res[1] is tgt and res[2] == [] and res[3] is None
    assert _same_np_state(nat_np, py_np) and nat_d == [0, 0, 0] and py_d == [0, 0, 0]
    np.random.seed(12345)
    np.random.standard_normal(3)
    assert _same_np_state(nat_np, np.random.get_state()), "a rejected step moved numpy's stream"


def test_spectrogram_route(device, monkeypatch):
    B, Cc, F, W = 8, 1, 16, 32
    x, frames_np, labels, wav = _batch(B, Cc * F, W, 2, seed=41)
    data = torch.from_numpy(x.reshape(B, Cc, F, W)).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    frames = torch.from_numpy(frames_np)
    (nat, nat_np, nat_d), (py, py_np, py_d) = _both_paths(monkeypatch, augmentations2d, METHOD, data, tgt, frames,
                                                          wav, 9, device)
    assert nat[0].shape == data.shape and torch.equal(nat[0], py[0]) and not torch.equal(nat[0], data)
    assert np.array_equal(nat[2], py[2]) and _same_np_state(nat_np, py_np) and nat_d == [1, 0, 0] == py_d
    ref = O.augment(METHOD, x.reshape(B, Cc, F, W), labels, frames_np, wav, 9)
    assert np.array_equal(nat[2], ref["mix"]) and np.array_equal(nat[0].cpu().numpy(), ref["y"])
    rejected = next(s for s in range(64) if not hostprep.gate_fires(GATED, s))
    (nat, _, nat_d), (py, _, _) = _both_paths(monkeypatch, augmentations2d, GATED, data, tgt, frames, wav, rejected,
                                              device)
    assert nat[0] is data and py[0] is data and nat[2] == [] and nat_d == [0, 0, 0]


def test_ownership(device):
    x, frames_np, labels, wav, data, tgt = _case("odd", device)
    frames = torch.from_numpy(frames_np)
    recipe = hostprep.plain_recipe(METHOD, False)
    counts = [sys.getrefcount(o) for o in (recipe, data, tgt, frames)]
    res = augmentations._native_step(recipe, data, tgt, frames, 4, None)
    out, mix = res[0], res[2]
    del res
    assert sys.getrefcount(out) == 2 and sys.getrefcount(mix) == 2
    assert [sys.getrefcount(o) for o in (recipe, data, tgt, frames)] == counts
    want = hostprep.shuffle_within_groups(labels, 4)
    del out, frames
    torch.cuda.synchronize()
    assert np.array_equal(mix, want) and mix.flags.writeable and (mix.flags.owndata or mix.base is not None)


@pytest.mark.parametrize("what", ["data float64", "one-hot int32", "frames (B, 4)", "frames a list",
                                  "host labels", "knots", "step 2**32", "taped"])
def test_ineligible_input_on_the_device_is_declined_before_any_launch(what, device, monkeypatch):
    x, frames_np, labels, wav, data, tgt = _case("odd", device)
    a = [hostprep.plain_recipe(METHOD, False), data, tgt, torch.from_numpy(frames_np), 3, None]
    if what == "data float64":
        a[1] = data.double()
    elif what == "one-hot int32":
        a[2] = tgt.int()
    elif what == "frames (B, 4)":
        a[3] = torch.from_numpy(frames_np[:, :4].copy())
    elif what == "frames a list":
        a[3] = frames_np.tolist()
    elif what == "host labels":
        a[5] = labels
    elif what == "knots":
        a[0] = hostprep.plain_recipe("durmixmagwarp(0.2,4)", False)
    elif what == "step 2**32":
        a[4] = 2 ** 32
    else:
        monkeypatch.setattr(_lib, "TAPE", [])
    before = _stats(device)
    assert augmentations._native_step(*a) is None
    assert _stats(device) == before and _lib.TAPE in (None, [])


def _synchronize_seconds():
    t0 = time.perf_counter()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _equals_oracle(name, step, device):
    x, frames, labels, wav, data, tgt = _case(name, device)
    y, _, mix, _ = _augment(augmentations, METHOD, data, tgt, torch.from_numpy(frames), wav, step, device)
    ref = O.augment(METHOD, x, labels, frames, wav, step)
    return np.array_equal(mix, ref["mix"]) and float(np.abs(y.cpu().numpy() - ref["y"]).max()) <= 1e-4


def test_step_beyond_numpys_seed_range(device):
    """Step 2**32: the module declines before the launch; the Python path launches, numpy refuses the seed
    (the reference's ValueError), and the waiting kernel is released at once, not by its 1 s timeout."""
    x, frames, labels, wav, data, tgt = _case("smoke", device)
    torch.cuda.synchronize()
    with pytest.raises(ValueError) as caught:
        _augment(augmentations, METHOD, data, tgt, torch.from_numpy(frames), wav, 2 ** 32, device)
    took = _synchronize_seconds()
    print(f"synchronize after the refused step: {took * 1e3:.2f} ms")
    with pytest.raises(ValueError) as numpys:
        np.random.seed(2 ** 32)
    assert str(caught.value) == str(numpys.value)
    assert took < 0.2
    assert _equals_oracle("smoke", 7, device)


@pytest.mark.parametrize("native", [True, False], ids=["module", "python"])
def test_exception_between_begin_and_finish_releases_the_kernel(native, device, monkeypatch):
    """numpy's beta raises once, after the launch (it is looked up per call on both paths): the exception
    reaches the caller, pcgmix_augment_plain_abort has released the kernel, the next step is exact."""
    x, frames, labels, wav, data, tgt = _case("smoke", device)
    if not native:
        monkeypatch.setattr(augmentations, "_native_step", None)

    class Boom(Exception):
        pass

    def beta(*a, **k):
        raise Boom("no lambda today")

    torch.cuda.synchronize()
    before = _stats(device)
    with monkeypatch.context() as m:
        m.setattr(np.random, "beta", beta)
        with pytest.raises(Boom, match="no lambda today"):
            _augment(augmentations, METHOD, data, tgt, torch.from_numpy(frames), wav, 5, device)
    took = _synchronize_seconds()
    print(f"synchronize after the abort: {took * 1e3:.2f} ms")
    after = _stats(device)
    assert took < 0.2
    assert after[2] - before[2] == 1 and after[0] == before[0]
    assert _lib.load().pcgmix_augment_plain_abort(augmentations.step_context(device.index)) == 0   # nothing open
    assert _stats(device) == after
    assert _equals_oracle("smoke", 5, device)
    assert _stats(device)[0] - after[0] == 1


def test_malformed_boundaries_raise_the_same_on_both_paths(device, monkeypatch):
    x, frames, labels, wav, data, tgt = _case("smoke", device)
    bad = frames.copy()
    bad[3, 4] = data.shape[2] + 1
    seen = []
    for native in (True, False):
        with monkeypatch.context() as m:
            if not native:
                m.setattr(augmentations, "_native_step", None)
            with pytest.raises(ValueError) as caught:
                _augment(augmentations, METHOD, data, tgt, torch.from_numpy(bad), wav, 2, device)
            seen.append((type(caught.value), str(caught.value)))
            assert _synchronize_seconds() < 0.2
    assert seen[0] == seen[1] and seen[0][1] == "heart cycle ends beyond the signal length"
    assert _equals_oracle("smoke", 2, device)
