"""The evaluation pass on the GPU: the three eval entry points against float64 / numpy restatements
of train_model.py:591-670, and ``predict_recordings`` / ``test_data_accuracy`` end to end against
the torch formulation (``FUSED_EVAL = False``)."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models, synthetic
from pcgmix_amd import dataloader_physionet as dlp
from pcgmix_amd import train_model as tm

pytestmark = pytest.mark.gpu

INVALID = 1                                     # hipErrorInvalidValue


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ pcgmix_eval_rows_f32
def make_logits(B, C, seed):
    """Random rows plus, where B has room for them (B >= 3 has all three): row 0 at +-80 (the max
    subtraction), row 1 all equal (vote 0), row 2 with its two largest logits one ulp apart."""
    rs = np.random.RandomState(seed)
    l = (3.0 * rs.standard_normal((B, C))).astype(np.float32)
    l[0] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0).astype(np.float32)
    if B > 1:
        l[1] = np.float32(0.37)
    if B > 2 and C > 1:
        l[2] = np.float32(-2.0)
        l[2, C - 1] = np.float32(1.0)
        l[2, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    return l, rs.randint(0, C, B).astype(np.uint8)


def run_rows(device, logits, labels):
    lib = _lib.load()
    B, C = logits.shape
    lg = torch.from_numpy(logits).to(device)
    lb = torch.from_numpy(labels).to(device) if labels is not None else None
    prob = torch.full((B, C), -7.0, device=device)
    loss = torch.full((B,), -7.0, device=device)
    vote = torch.full((B,), 99, dtype=torch.uint8, device=device)
    err = lib.pcgmix_eval_rows_f32(ptr(lg), ptr(lb), ptr(prob), ptr(loss), ptr(vote), B, C,
                                   stream_of(device))
    return err, prob.cpu().numpy(), loss.cpu().numpy(), vote.cpu().numpy()


@pytest.mark.parametrize("C", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 255, 256, 257])
def test_eval_rows(B, C, device):
    logits, labels = make_logits(B, C, 100 * B + C)
    err, prob, loss, vote = run_rows(device, logits, labels)
    assert err == 0
    l64 = logits.astype(np.float64)
    e = np.exp(l64 - l64.max(1, keepdims=True))
    p64 = e / e.sum(1, keepdims=True)
    # one expf at <= 1-2 ulp, a sum of <= 8 terms and one division: relative error < ~7e-7, p <= 1
    d = np.abs(prob - p64).max()
    print(f"B={B} C={C} max |prob - f64| = {d:.3g}")
    assert d <= 2e-6
    s = np.abs(prob.astype(np.float64).sum(1) - 1.0).max()
    print(f"   max |row sum - 1| = {s:.3g}")
    assert s <= 4e-7 * C
    want = -(l64[np.arange(B), labels] - l64.max(1) - np.log(e.sum(1)))     # (finite where p underflows)
    dl = np.abs(loss - want)
    print(f"   max loss error = {dl.max():.3g}")
    assert (dl <= 1e-6 * np.abs(want) + 1e-6).all()
    assert np.array_equal(vote, np.argmax(prob, axis=1))        # the vote of the float32 p it wrote
    if B > 1:
        assert vote[1] == 0 and np.all(prob[1] == prob[1, 0])   # all-equal row
    # labels = NULL: zero losses, everything else the same bits
    err, prob2, loss2, vote2 = run_rows(device, logits, None)
    assert err == 0 and np.array_equal(prob2, prob) and np.array_equal(vote2, vote)
    assert np.array_equal(loss2, np.zeros(B, np.float32))


def test_eval_rows_refusals(device):
    logits, labels = make_logits(4, 8, 1)
    wide = np.concatenate([logits, logits[:, :1]], axis=1)              # C = 9
    err, prob, loss, vote = run_rows(device, wide, labels)
    assert err == INVALID
    assert (prob == -7.0).all() and (loss == -7.0).all() and (vote == 99).all()
    lib = _lib.load()
    t = torch.full((4,), -7.0, device=device)
    v = torch.full((4,), 99, dtype=torch.uint8, device=device)
    assert lib.pcgmix_eval_rows_f32(ptr(t), None, ptr(t), ptr(t), ptr(v), 0, 2, stream_of(device)) == 0
    torch.cuda.synchronize()
    assert (t == -7.0).all() and (v == 99).all()                        # B = 0 launched nothing


# ------------------------------------------------------------------ pcgmix_potes_head_eval_f32
@pytest.mark.parametrize("K", [models.potes_flat_features(30), models.potes_flat_features(2500)])
@pytest.mark.parametrize("B", [1, 4, 5, 9, 257])
def test_potes_head_eval(B, K, device):
    assert K in (96, 9968)
    lib = _lib.load()
    st = stream_of(device)
    if K == 9968:
        assert lib.pcgmix_skinny_linear_splits(B, K) > 16       # the unrolled partial loop of the tail
    for C in (2, 3):
        g = torch.Generator().manual_seed(1000 * B + K + C)
        x = torch.randn(B, K, generator=g).to(device)
        w1 = (torch.randn(20, K, generator=g) / K ** 0.5).to(device)
        b1 = (0.1 * torch.randn(20, generator=g)).to(device)
        w2 = (0.7 * torch.randn(C, 20, generator=g)).to(device)
        b2 = (0.1 * torch.randn(C, generator=g)).to(device)
        labels = torch.randint(0, C, (B,), generator=g).to(torch.uint8).to(device)
        ks = lib.pcgmix_skinny_linear_splits(B, K)
        new = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device=device)   # noqa: E731
        partial, z, ref = new(ks, B, 20), new(B, 20), new(B, C)
        _lib.check(lib.pcgmix_potes_head_fwd_f32(
            ptr(x), None, ctypes.c_float(1.0), 0, 8, ptr(w1), ptr(b1), None, ctypes.c_float(1.0), 0,
            ptr(w2), ptr(b2), ptr(partial), ptr(z), ptr(ref), B, K, C, st), "head_fwd")
        partial2, logits, prob, loss, vote = new(ks, B, 20), new(B, C), new(B, C), new(B), new(B, dt=torch.uint8)
        _lib.check(lib.pcgmix_potes_head_eval_f32(
            ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(labels), ptr(partial2), ptr(logits),
            ptr(prob), ptr(loss), ptr(vote), B, K, C, st), "head_eval")
        assert torch.equal(logits, ref)                         # the same bits as the training head
        rprob, rloss, rvote = new(B, C), new(B), new(B, dt=torch.uint8)
        _lib.check(lib.pcgmix_eval_rows_f32(ptr(ref), ptr(labels), ptr(rprob), ptr(rloss), ptr(rvote),
                                            B, C, st), "eval_rows")
        assert torch.equal(prob, rprob) and torch.equal(loss, rloss) and torch.equal(vote, rvote)
        assert float(loss.min()) > 0.0 and int(vote.max()) < C
        # logits = NULL is accepted and changes nothing else
        prob3, loss3, vote3 = new(B, C), new(B), new(B, dt=torch.uint8)
        _lib.check(lib.pcgmix_potes_head_eval_f32(
            ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(labels), ptr(partial2), None,
            ptr(prob3), ptr(loss3), ptr(vote3), B, K, C, st), "head_eval")
        assert torch.equal(prob3, prob) and torch.equal(loss3, loss) and torch.equal(vote3, vote)


# ------------------------------------------------------------------ pcgmix_eval_segments_f32
SEG_COUNTS = (1, 2, 3, 64, 65, 300)


@pytest.mark.parametrize("C", [2, 3, 8])
def test_eval_segments_exact(C, device):
    lib = _lib.load()
    rs = np.random.RandomState(40 + C)
    ids = rs.permutation(np.repeat(np.arange(len(SEG_COUNTS)), SEG_COUNTS))   # interleaved cycles
    N, R = len(ids), len(SEG_COUNTS)
    names = [f"rec{i}" for i in ids]
    plan = tm.EvalPlan(names, np.zeros(N, int))
    assert sorted(plan.counts.tolist()) == sorted(SEG_COUNTS)
    prob = rs.random_sample((N, C)).astype(np.float32)
    prob /= prob.sum(1, keepdims=True).astype(np.float32)
    loss = (5.0 * rs.random_sample(N)).astype(np.float32)
    vote = rs.randint(0, C, N).astype(np.uint8)
    dev = lambda a: torch.from_numpy(a).to(device)                            # noqa: E731
    dprob, dloss, dvote, dorder, dstart = dev(prob), dev(loss), dev(vote), dev(plan.order), dev(plan.rec_start)
    results = []
    for _ in range(2):
        mean_p = torch.full((R, C), -7.0, device=device)
        votes = torch.full((R, C), -7, dtype=torch.int32, device=device)
        loss_rec = torch.full((R,), -7.0, dtype=torch.float64, device=device)
        _lib.check(lib.pcgmix_eval_segments_f32(
            ptr(dprob), ptr(dloss), ptr(dvote), ptr(dorder), ptr(dstart), ptr(mean_p), ptr(votes),
            ptr(loss_rec), N, R, C, stream_of(device)), "eval_segments")
        results.append((mean_p.cpu().numpy(), votes.cpu().numpy(), loss_rec.cpu().numpy()))
    mean_p, votes, loss_rec = results[0]
    for r, name in enumerate(plan.names):                       # the reference's dict, in loader order
        rows = [i for i in range(N) if names[i] == name]
        want = np.mean([prob[i] for i in rows], axis=0)         # train_model.py:627
        assert want.dtype == np.float32
        assert np.array_equal(mean_p[r].view(np.int32), want.view(np.int32)), (r, len(rows))
        assert np.array_equal(votes[r], np.bincount(vote[rows], minlength=C))
        run = 0.0
        for i in rows:
            run += float(loss[i])
        assert loss_rec[r] == run
    for a, b in zip(results[0], results[1]):                    # the same bits on every call
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ end to end
POOL_SEED = 14
POOL_SIZES = [2, 14, 3, 11, 8, 8, 1, 13, 10, 6, 12, 8]         # 96 cycles in 12 recordings


def eval_pool(seed=POOL_SEED):
    x, frames, _labels, _ = synthetic.make_batch(96, 4, 2500, sample_rate=1000, seed=seed)
    wav, lab = [], []
    for r, n in enumerate(POOL_SIZES):
        wav += [f"{'abcdef'[r % 6]}{r:04d}"] * n
        lab += [r % 2] * n
    order = np.random.RandomState(seed).permutation(96)        # recordings spread over the batches
    return x[order], frames[order], np.asarray(lab, dtype=np.int64)[order], [wav[i] for i in order]


def make_args(model, method="base"):
    return argparse.Namespace(dataset="PhysioNet", model=model, method=method, num_classes=2,
                              num_channels=4, sig_len=2500)


def make_model(name, device):
    """Freshly initialised.  An untrained Potes head is nearly undecided (|p0 - p1| ~ 1e-4): its last
    layer is scaled up so that votes and arg-max decisions have a margin two softmax roundings
    cannot cross (checked on the CPU with the torch path for POOL_SEED: no recording's top-2 gap of
    the mean probabilities is below 1e-4, no cycle's below 1e-4, and no two recordings' class-1
    scores are closer than 1e-6)."""
    torch.manual_seed(3)
    model = tm.build_model(make_args(name))
    if isinstance(model, models.CNN_potes):
        with torch.no_grad():
            model.linear.weight.mul_(25.0)
    return model.to(device)


def make_loader(kind, pool, device):
    x, frames, labels, wav = pool
    if kind == "resident":
        return dlp.ResidentLoader(x, labels, frames, wav, np.ones(96), batch_size=40, shuffle=False,
                                  drop_last=False, device=device)
    return tm.SyntheticCycleLoader((x, frames, labels, wav), 40)


@pytest.fixture(scope="module")
def pool():
    return eval_pool()


def both_paths(fn, monkeypatch):
    """fn() under FUSED_EVAL on and off, each from the same torch seed; returns the two results and
    the two generator states after the call."""
    out = []
    for fused in (True, False):
        monkeypatch.setattr(tm, "FUSED_EVAL", fused)
        torch.manual_seed(77)
        res = fn()
        out.append((res, torch.get_rng_state().clone()))
    return out


@pytest.mark.parametrize("kind", ["resident", "synthetic"])
@pytest.mark.parametrize("name", ["Potes", "resnet9-5k"])
def test_evaluation_matches_the_torch_path(name, kind, pool, device, monkeypatch):
    model = make_model(name, device)
    crit = tm.SELCLoss(np.zeros(96, int), 2, es=99, device=device)
    loader = make_loader(kind, pool, device)
    for method in ("base", "base(class_majority)"):
        args = make_args(name, method)
        (on, rng_on), (off, rng_off) = both_paths(
            lambda: tm.test_data_accuracy(args, model, loader, device, crit), monkeypatch)
        assert torch.equal(rng_on, rng_off)                    # the loader was iterated once, as before
        assert on["recordings"] == off["recordings"] and on["recordings"] >= 11
        for k in ("accuracy", "specificity", "sensitivity", "precision", "recall", "f1"):
            assert abs(on[k] - off[k]) <= 1e-9, (method, k, on[k], off[k])
        print(f"{name} {kind} {method}: loss {on['loss']!r} vs {off['loss']!r}, auc {on['rocauc']!r}")
        assert abs(on["loss"] - off["loss"]) <= 1e-5
        if "majority" in method:
            assert on["rocauc"] is None and off["rocauc"] is None
        else:
            assert abs(on["rocauc"] - off["rocauc"]) <= 1e-12
    # mean probabilities against the torch formulation's
    monkeypatch.setattr(tm, "FUSED_EVAL", True)
    torch.manual_seed(77)
    rec = tm.predict_recordings(make_args(name), model, loader, device, crit)
    torch.manual_seed(77)
    mean_p, _votes, lab, loss_sum, n = tm._collect_recordings_torch(make_args(name), model, loader, device,
                                                                   crit, False)
    assert rec["n"] == n == (96 if kind == "resident" else 80)
    assert np.array_equal(rec["labels"], lab) and len(rec["names"]) == len(lab)
    assert rec["counts"].sum() == n and rec["votes"].sum() == n
    d = np.abs(rec["mean_proba"] - mean_p).max()
    print(f"{name} {kind}: max |mean_proba - torch| = {d:.3g}")
    assert d <= 2e-6
    assert abs(rec["loss_sum"] - loss_sum) <= 1e-5 * n
    # the fixed-order sums: the same bits on a second call
    torch.manual_seed(77)
    again = tm.predict_recordings(make_args(name), model, loader, device, crit)
    assert again["mean_proba"].tobytes() == rec["mean_proba"].tobytes()
    assert again["loss_sum"] == rec["loss_sum"] and np.array_equal(again["votes"], rec["votes"])


class Scripted(torch.nn.Module):
    """Logits (-s, s) with s = the cycle's first sample: the test writes the votes into the data."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(()))

    def forward(self, x):
        s = x[:, 0, 0] * self.scale
        return torch.stack([-s, s], dim=1)


def scripted_batches():
    """Three recordings over two ragged batches: 'tie' has two cycles voting 0 and 1 (class 1 under
    '(class_majority)', train_model.py:642-643, though its mean probability says 0), 'zero' votes
    0, 0, 1, 'one' votes 1."""
    wav = ["tie", "zero", "one", "zero", "tie", "zero"]
    s = np.asarray([-3.0, -1.0, 2.0, -1.0, 0.5, 0.25], dtype=np.float32)
    lab = np.asarray([1, 0, 1, 0, 1, 0], dtype=np.int64)
    x = np.zeros((6, 4, 16), dtype=np.float32)
    x[:, 0, 0] = s
    cut = lambda a, i, j: torch.from_numpy(a[i:j])             # noqa: E731
    return [(cut(x, i, j), cut(lab, i, j), None, tuple(wav[i:j]), None, None) for i, j in ((0, 4), (4, 6))]


def test_class_majority_tie_and_performance_appends(device, monkeypatch):
    monkeypatch.setattr(tm, "FUSED_EVAL", True)
    model = Scripted().to(device)
    crit = tm.SELCLoss(np.zeros(6, int), 2, es=99, device=device)
    rec = tm.predict_recordings(make_args("x"), model, scripted_batches(), device, crit)
    assert rec["names"] == ["tie", "zero", "one"] and rec["labels"].tolist() == [1, 0, 1]
    assert rec["votes"].tolist() == [[1, 1], [2, 1], [0, 1]] and rec["counts"].tolist() == [2, 3, 1]
    assert rec["mean_proba"][0, 0] > rec["mean_proba"][0, 1]            # the mean rule says class 0
    mean = tm.test_data_accuracy(make_args("x", "base"), model, scripted_batches(), device, crit)
    maj = tm.test_data_accuracy(make_args("x", "base(class_majority)"), model, scripted_batches(), device, crit)
    assert abs(mean["accuracy"] - 200.0 / 3.0) <= 1e-9 and maj["accuracy"] == 100.0   # the tie goes to class 1
    assert maj["rocauc"] is None and mean["rocauc"] is not None
    perf = tm.performance_metrics_class()
    with pytest.raises(IndexError):
        tm.test_data_accuracy(make_args("x", "base(class_majority)"), model, scripted_batches(), device,
                              crit, 1, perf)
    got = {k: v for k, v in perf.dict.items() if v}
    assert sorted(got) == sorted("test_" + k for k in ("accuracy", "loss", "specificity", "sensitivity",
                                                       "f1", "precision", "recall"))
    assert all(len(v) == 1 for v in got.values()) and perf.dict["test_rocauc"] == []
    monkeypatch.setattr(tm, "FUSED_EVAL", False)
    off = tm.test_data_accuracy(make_args("x", "base(class_majority)"), model, scripted_batches(), device, crit)
    for k in ("accuracy", "specificity", "sensitivity", "precision", "recall", "f1"):
        assert abs(maj[k] - off[k]) <= 1e-9
    assert abs(maj["loss"] - off["loss"]) <= 1e-5


def test_model_comes_back_in_eval_mode_without_grads(pool, device, monkeypatch):
    monkeypatch.setattr(tm, "FUSED_EVAL", True)
    for name in ("Potes", "resnet9-5k"):
        model = make_model(name, device).train()
        rec = tm.predict_recordings(make_args(name), model, make_loader("resident", pool, device), device)
        assert rec["loss_sum"] is None and rec["n"] == 96
        assert not model.training
        assert all(p.grad is None for p in model.parameters())


def test_bad_label_is_refused_on_the_host(pool, device, monkeypatch):
    monkeypatch.setattr(tm, "FUSED_EVAL", True)
    x, frames, labels, wav = pool
    bad = labels.copy()
    bad[50] = 2
    model = Scripted().to(device)
    crit = tm.CELoss(2)
    tape = _lib.TAPE = []
    try:
        with pytest.raises(ValueError):
            tm.predict_recordings(make_args("x"), model,
                                  dlp.ResidentLoader(x, bad, frames, wav, np.ones(96), 40, False, False, device),
                                  device, crit)
    finally:
        _lib.TAPE = None
    assert tape == []                                          # refused before any launch


# ------------------------------------------------------------------ launch shape
def test_launch_shape_and_plan_cache(pool, device, monkeypatch):
    monkeypatch.setattr(tm, "FUSED_EVAL", True)
    model = make_model("Potes", device)
    crit = tm.SELCLoss(np.zeros(96, int), 2, es=99, device=device)
    loader = make_loader("resident", pool, device)
    args = make_args("Potes")
    tm.predict_recordings(args, model, loader, device, crit)    # builds and uploads the plan
    plan = loader.eval_plan
    assert isinstance(plan, tm.EvalPlan) and plan.uploads == 3
    side = plan.device_side(device, 2)
    ptrs = [t.data_ptr() for t in (side.order, side.rec_start, side.labels, side.prob, side.out)]
    tape = _lib.TAPE = []
    try:
        rec = tm.predict_recordings(args, model, loader, device, crit)
    finally:
        _lib.TAPE = None
    names = [t[0] for t in tape]
    assert names == ["pcgmix_potes_stack_fwd_f32", "pcgmix_potes_head_eval_f32"] * 3 + ["pcgmix_eval_segments_f32"]
    assert loader.eval_plan is plan and plan.uploads == 3       # nothing uploaded the second time
    side = plan.device_side(device, 2)
    assert ptrs == [t.data_ptr() for t in (side.order, side.rec_start, side.labels, side.prob, side.out)]
    assert rec["n"] == 96 and len(rec["names"]) == 12
