"""Host side of the evaluation pass: ``train_model.EvalPlan`` against a dict restatement of the
reference's per-recording collection (train_model.py:615-632), the binding of the three eval entry
points, and ``test_data_accuracy`` on the CPU (which keeps the torch formulation)."""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib
from pcgmix_amd import dataloader_physionet as dlp
from pcgmix_amd import train_model as tm

EVAL_SYMBOLS = ("pcgmix_eval_rows_f32", "pcgmix_potes_head_eval_f32", "pcgmix_eval_segments_f32")


def dict_walk(batches):
    """train_model.py:615-632 restated: recordings keyed by first appearance, each holding the rows
    of its cycles in the order the loader yielded them, and the label of its first cycle."""
    rows, first_label = {}, {}
    row = 0
    for names, labels in batches:
        for w, t in zip(names, labels):
            if w not in rows:
                rows[w] = [row]
                first_label[w] = int(t)
            else:
                rows[w].append(row)
            row += 1
    return rows, first_label


def batched(names, labels, bs):
    return [(names[i:i + bs], labels[i:i + bs]) for i in range(0, len(names), bs)]


def case_interleaved():
    names = ["b", "a", "b", "c", "a", "b", "c", "a", "d", "b"]
    return names, [1, 0, 1, 1, 0, 0, 1, 1, 0, 1]        # 'b' and 'a' change label later: the first counts


def case_random(n, n_rec, seed):
    rs = np.random.RandomState(seed)
    ids = rs.randint(0, n_rec, n)
    return [f"r{7 * i % n_rec:03d}" for i in ids], rs.randint(0, 3, n).tolist()


CASES = {
    "interleaved": (case_interleaved(), 4),             # 10 rows, batch 4: ragged last batch, 'b' split
    "split_across_batches": ((["x"] * 5 + ["y"] * 2 + ["x"] * 3, [1] * 5 + [0] * 2 + [1] * 3), 3),
    "one_cycle_recordings": (([f"s{i}" for i in range(7)], [i % 2 for i in range(7)]), 3),
    "single_recording": ((["only"] * 6, [1] * 6), 4),
    "random_ragged": (case_random(103, 17, 1), 40),
    "names_sort_differently": ((["10", "9", "10", "100", "9"], [0, 1, 0, 1, 1]), 2),
    "empty": (([], []), 4),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_matches_the_dict_walk(case):
    (names, labels), bs = CASES[case]
    rows, first_label = dict_walk(batched(names, labels, bs))
    plan = tm.EvalPlan(names, labels)
    N, R = len(names), len(rows)
    assert plan.n == N and plan.recordings == R
    assert plan.names == list(rows)                                   # by first appearance
    assert plan.labels.tolist() == [first_label[w] for w in rows]     # the first cycle's label
    assert plan.counts.tolist() == [len(v) for v in rows.values()]
    assert plan.order.dtype == np.int32 and plan.rec_start.dtype == np.int32
    assert plan.order.shape == (N,) and plan.rec_start.shape == (R + 1,)
    assert plan.rec_start[0] == 0 and plan.rec_start[-1] == N
    for r, w in enumerate(rows):
        seg = plan.order[plan.rec_start[r]:plan.rec_start[r + 1]].tolist()
        assert seg == rows[w]                                         # loader order within a recording
        assert seg == sorted(seg)                                     # ... i.e. a STABLE grouping
    assert sorted(plan.order.tolist()) == list(range(N))              # a permutation of the rows
    assert plan.cycle_labels.dtype == np.uint8 and plan.cycle_labels.tolist() == list(labels)
    assert plan.ids.tolist() == [list(rows).index(w) for w in names]


def test_plan_refuses_bad_input_and_validates_itself():
    with pytest.raises(ValueError):
        tm.EvalPlan(["a", "b"], [0])
    with pytest.raises(ValueError):
        tm.EvalPlan(["a"], [256])
    with pytest.raises(ValueError):
        tm.EvalPlan(["a"], [-1])
    plan = tm.EvalPlan(["a", "b", "a"], [0, 1, 0])
    plan.validate()
    plan.order[0] = plan.order[1]
    with pytest.raises(ValueError):
        plan.validate()
    plan = tm.EvalPlan(["a", "b", "a"], [0, 1, 0])
    plan.rec_start[1] = 3
    plan.rec_start[2] = 2
    with pytest.raises(ValueError):
        plan.validate()


def test_eval_entry_points_are_bound_and_abi_is_unchanged():
    lib = _lib.load()
    for n in EVAL_SYMBOLS:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert _lib.ABI_VERSION == 25 and lib.pcgmix_abi_version() == 25


def test_entry_points_refuse_before_any_launch():
    """Argument checks that return before a device call: they run without a GPU."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)
    inval = 1                                                          # hipErrorInvalidValue
    for C in (0, 9, -1):
        assert lib.pcgmix_eval_rows_f32(p, None, p, p, p, 4, C, None) == inval
        assert lib.pcgmix_eval_segments_f32(p, p, p, p, p, p, p, p, 4, 2, C, None) == inval
        assert lib.pcgmix_potes_head_eval_f32(p, p, p, p, p, None, p, None, p, p, p, 4, 96, C, None) == inval
    assert lib.pcgmix_eval_rows_f32(p, None, p, p, p, 0, 2, None) == 0         # B == 0: nothing to do
    assert lib.pcgmix_eval_rows_f32(p, None, p, p, p, -1, 2, None) == inval
    assert lib.pcgmix_eval_rows_f32(None, None, p, p, p, 4, 2, None) == inval
    assert lib.pcgmix_eval_segments_f32(p, p, p, p, p, p, p, p, 0, 0, 2, None) == 0   # R == 0
    assert lib.pcgmix_eval_segments_f32(p, p, p, p, p, p, p, p, 0, 2, 2, None) == inval
    assert lib.pcgmix_eval_segments_f32(p, p, p, None, p, p, p, p, 4, 2, 2, None) == inval
    assert lib.pcgmix_potes_head_eval_f32(p, p, p, p, p, None, p, None, p, p, p, 4, 98, 2, None) == inval  # K % 4
    assert lib.pcgmix_potes_head_eval_f32(p, p, p, p, p, None, p, None, None, p, p, 4, 96, 2, None) == inval


def small_pool(n=24, T=64):
    rs = np.random.RandomState(3)
    x = rs.standard_normal((n, 4, T)).astype(np.float32)
    frames = np.tile(np.asarray([0, 10, 20, 30, 40], dtype=np.int64), (n, 1))
    wav = [f"w{i // 3:02d}" for i in range(n)]
    labels = np.asarray([(i // 3) % 2 for i in range(n)], dtype=np.int64)
    return x, frames, labels, wav


class Fixed(torch.nn.Module):
    """Logits that depend on the input only: class-1 score = mean of the first channel."""

    def forward(self, x):
        s = x[:, 0, :].mean(dim=1)
        return torch.stack([-s, s], dim=1)


def test_cpu_evaluation_keeps_the_torch_path(monkeypatch):
    """On the CPU ``test_data_accuracy`` never reaches ``predict_recordings``, whatever the switch
    says, and returns the same numbers either way."""
    x, frames, labels, wav = small_pool()
    loader = dlp.ResidentLoader(x, labels, frames, wav, np.ones(len(labels)), batch_size=10,
                                shuffle=False, drop_last=False)
    assert loader.eval_plan is None

    class A:
        num_classes = 2
        method = "base"

    def boom(*a, **k):
        raise AssertionError("predict_recordings called on the CPU")
    monkeypatch.setattr(tm, "predict_recordings", boom)
    crit = tm.SELCLoss(np.zeros(4, int), 2)        # the criterion the run driver evaluates with
    monkeypatch.setattr(tm, "FUSED_EVAL", True)
    cpu = torch.device("cpu")
    assert not tm.fused_eval_applies(A, cpu, crit)
    on = tm.test_data_accuracy(A, Fixed(), loader, cpu, crit)
    monkeypatch.setattr(tm, "FUSED_EVAL", False)
    off = tm.test_data_accuracy(A, Fixed(), loader, cpu, crit)
    assert on == off and on["recordings"] == 8
    assert loader.eval_plan is None


def test_fused_eval_gate():
    class A:
        num_classes = 2
    cuda = torch.device("cuda:0")
    assert tm.fused_eval_applies(A, cuda, None)
    assert tm.fused_eval_applies(A, cuda, tm.CELoss(2))
    assert tm.fused_eval_applies(A, cuda, tm.SELCLoss(np.zeros(4, int), 2))
    assert not tm.fused_eval_applies(A, cuda, torch.nn.CrossEntropyLoss())

    class Sub(tm.CELoss):
        pass
    assert not tm.fused_eval_applies(A, cuda, Sub(2))            # a subclass may compute something else
    A.num_classes = 9
    assert not tm.fused_eval_applies(A, cuda, None)


def test_predict_recordings_refuses_what_it_cannot_compute():
    class A:
        num_classes = 2
    with pytest.raises(ValueError):
        tm.predict_recordings(A, Fixed(), [], torch.device("cpu"))
