"""The armed step's host half end to end (csrc/pcgmix_host.hip armed_finish): the label bytes the kernel left
are grouped as they are, the partners drawn in lock step, the records written from the packed tables.  The
armed path is chosen per process, so each side runs in a fresh child: the default, and PCGMIX_NO_ARMED=1 (the
two-launch path).  Both run the same strict-signature augment() steps; outputs and partners must be
bit-identical between them, and the partners equal CPython's own ``random.Random(step).sample`` per label
group.  One step with malformed boundaries after the launch: the error comes back at once (the waiting kernel
is released, not timed out) and the next step is exact.  (The records' placement in device memory behind a
large BAR, which these cases were first written for, was measured and not kept: DESIGN.md 3.6.)"""
import ctypes
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from conftest import ROOT, Args, StepCounter

pytestmark = pytest.mark.gpu

WARP = "durmixmagwarp(0.2,4)"
CASES = [("durratiomixup", 3, 1, 64), ("durratiomixup", 5, 4, 260), ("durratiomixup", 64, 1, 4096),
         ("durratiomixup", 65, 4, 2052), ("durratiomixup", 256, 4, 5000), (WARP, 5, 4, 260), (WARP, 64, 1, 4096)]
STEP = 3
PATHS = {"armed": {}, "unarmed": {"PCGMIX_NO_ARMED": "1"}}


def _batch(B, C, T):
    """Row 0: an empty cycle at an odd position; row 1: a cycle that reaches T; the rest: odd edges."""
    rs = np.random.RandomState(1000 * B + 10 * C + T)
    x = rs.standard_normal((B, C, T)).astype(np.float32)
    labels = rs.randint(0, 2, B).astype(np.int64)
    frames = np.empty((B, 5), np.int64)
    for b in range(B):
        lo = int(rs.randint(1, T // 3 + 1)) | 1
        hi = T if b == 1 else int(rs.randint(lo, T + 1))
        cuts = np.sort(rs.randint(lo, hi + 1, 3))
        frames[b] = [lo] * 5 if b == 0 else [lo, cuts[0], cuts[1], cuts[2], hi]
    assert (np.diff(frames, axis=1) >= 0).all() and frames.min() >= 0 and frames.max() <= T
    return x, labels, frames, ["a%04d" % i for i in range(B)]


def child_main(out_path):
    """Runs in the child: every case once, then the malformed step and the case behind it again."""
    import torch
    from pcgmix_amd import _lib, augmentations
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def step(method, x, labels, frames, wav):
        tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(dev)
        y, _, mix, _ = augmentations.augment(Args(method), torch.from_numpy(x).to(dev), tgt, torch.from_numpy(frames),
                                             wav, StepCounter(STEP), None, dev, "")
        return y.cpu().numpy(), np.asarray(mix)

    res = {}
    for i, (method, B, C, T) in enumerate(CASES):
        res["y%d" % i], res["mix%d" % i] = step(method, *_batch(B, C, T))
    x, labels, frames, wav = _batch(5, 4, 260)
    bad = frames.copy()
    bad[3, 4] = 261
    t0 = time.perf_counter()
    try:
        step("durratiomixup", x, labels, bad, wav)
        refused = False
    except ValueError:
        refused = True
    torch.cuda.synchronize()                   # returns: nobody is waiting any more
    res["refused"], res["refusal_seconds"] = refused, time.perf_counter() - t0
    res["y_after"], res["mix_after"] = step("durratiomixup", x, labels, frames, wav)
    stats = (ctypes.c_longlong * 3)()
    ctx = augmentations.step_context(0)
    _lib.check(lib.pcgmix_ctx_armed_stats(ctx, stats), "stats")
    res["stats"] = np.array(list(stats))
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    """The two children side by side, each with a time limit of its own."""
    tmp = tmp_path_factory.mktemp("armed_records")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_armed_records_gpu as t; t.child_main(sys.argv[1])"
            % (ROOT, os.path.join(ROOT, "tests")))
    flags = ["-s"] if sys.flags.no_user_site else []
    procs = {}
    for name, extra in PATHS.items():
        env = {k: v for k, v in os.environ.items() if k != "PCGMIX_NO_ARMED"}
        env.update(extra)
        procs[name] = subprocess.Popen([sys.executable] + flags + ["-c", code, str(tmp / (name + ".npz"))], env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        try:
            log, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert p.returncode == 0, "%s child: exit %d\n%s" % (name, p.returncode, log[-2000:])
        out[name] = dict(np.load(tmp / (name + ".npz")))
    return out


def test_each_child_ran_the_path_it_was_asked_for(runs):
    n = len(CASES) + 1                                       # and the step behind the refusal
    assert int(runs["unarmed"]["stats"][0]) == 0
    assert int(runs["armed"]["stats"][0]) == n, "a strict-signature step did not take the armed kernel"
    assert int(runs["armed"]["stats"][1]) == 0, "records were late"


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s-%d-%d-%d" % c for c in CASES])
def test_armed_and_two_launch_path_agree_bit_for_bit(runs, i):
    y, mix = runs["unarmed"]["y%d" % i], runs["unarmed"]["mix%d" % i]
    assert not np.isnan(y).any() and y.shape == tuple(CASES[i][1:])
    assert np.array_equal(runs["armed"]["mix%d" % i], mix)
    assert np.array_equal(runs["armed"]["y%d" % i].view(np.int32), y.view(np.int32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s-%d-%d-%d" % c for c in CASES])
def test_partners_equal_the_cpu_draw(runs, i):
    _, B, C, T = CASES[i]
    labels = _batch(B, C, T)[1]
    want = np.full(B, -1, dtype=np.int64)
    for key in dict.fromkeys(labels.tolist()):
        members = np.flatnonzero(labels == key).tolist()
        want[members] = random.Random(STEP).sample(members, len(members))
    for name in PATHS:
        assert np.array_equal(runs[name]["mix%d" % i], want), name


def test_malformed_boundaries_after_the_launch(runs):
    i = CASES.index(("durratiomixup", 5, 4, 260))
    for name in PATHS:
        r = runs[name]
        assert bool(r["refused"]), name
        assert float(r["refusal_seconds"]) < 0.5, "%s: the kernel waited for its time-out" % name
        assert np.array_equal(r["mix_after"], r["mix%d" % i]), name
        assert np.array_equal(r["y_after"].view(np.int32), r["y%d" % i].view(np.int32)), name
