"""CPU tests of the train loops' monitoring numbers (cmpc-refseg_amd/hostutil.py): compute_accuracy against the reference's own results
on the six stored inputs (tests/golden/ref_processing_tools.npz, iou/{i}/scores|labels|accuracy), accuracy_from_counts, TrainLog against
a literal per-step loop of the driver's formulas (CMPC_video/trainval_video.py:102-121), and cmpc_train_accuracy's argument checks
before anything is launched (the library loads without a GPU)."""
import importlib
import math
import os

import numpy as np
import pytest

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
L = importlib.import_module("cmpc-refseg_amd._lib")

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_processing_tools.npz")


def _cases():
    z = np.load(GOLD)
    return [(z["iou/%d/scores" % i], z["iou/%d/labels" % i], z["iou/%d/accuracy" % i]) for i in range(int(z["iou/n"]))]


@pytest.mark.timeout(60)
def test_compute_accuracy_equals_the_reference_on_its_six_inputs():
    cases = _cases()
    assert len(cases) == 6
    for i, (s, l, want) in enumerate(cases):
        assert (l != 0).any() and (l == 0).any() and not (s == 0).any(), i      # both classes present, no score on the boundary
        got = HU.compute_accuracy(s, l)
        assert all(isinstance(v, float) for v in got)
        assert got == tuple(float(v) for v in want), (i, got, want)             # the same integer sums and one division: ==, no allowance


@pytest.mark.timeout(60)
def test_accuracy_from_counts():
    cases = _cases()
    for i, (s, l, want) in enumerate(cases):
        c = HU.accuracy_counts(s, l)
        assert c.dtype == np.int64 and c.shape == (4,) and c[0] + c[1] == s.size
        assert c[0] == (l != 0).sum() and c[2] == ((s >= 0) & (l != 0)).sum() and c[3] == ((s < 0) & (l == 0)).sum()
        assert HU.accuracy_from_counts(c) == tuple(float(v) for v in want), i
        assert HU.accuracy_from_counts(c[None]) == tuple(float(v) for v in want), i
    # a batch: the sums over its samples, i.e. compute_accuracy over all the batch's pixels
    s0, l0, _ = cases[1]
    s1, l1, _ = cases[4]
    both = HU.accuracy_from_counts(np.stack([HU.accuracy_counts(s0, l0), HU.accuracy_counts(s1, l1)]))
    assert both == HU.compute_accuracy(np.concatenate([s0.reshape(-1), s1.reshape(-1)]), np.concatenate([l0.reshape(-1), l1.reshape(-1)]))
    for bad in (np.zeros((2, 3), np.int64), np.zeros((4,), np.float32), np.zeros((1, 2, 4), np.int64)):
        with pytest.raises(ValueError):
            HU.accuracy_from_counts(bad)


@pytest.mark.timeout(60)
def test_accuracy_edge_rules():
    # no negative pixel: accuracy_neg is the reference's 0 / 0; accuracy_pos keeps its / (num_pos + 1)
    s = np.array([[1.0, -1.0], [2.0, 3.0]], np.float32)
    a, p, n = HU.compute_accuracy(s, np.ones((2, 2), np.float32))
    assert (a, p) == (3 / 4, 3 / 5) and math.isnan(n)
    a, p, n = HU.accuracy_from_counts(np.array([[4, 0, 3, 0]]))
    assert (a, p) == (3 / 4, 3 / 5) and math.isnan(n)
    # no positive pixel: accuracy_pos = 0 / 1
    assert HU.compute_accuracy(s, np.zeros((2, 2), np.float32)) == (1 / 4, 0.0, 1 / 4)
    # 0.0, -0.0 and NaN are not < 0: predicted positive
    z = np.array([0.0, -0.0, np.nan, -1e-30], np.float32)
    assert HU.accuracy_counts(z, np.array([1, 1, 1, 1])).tolist() == [4, 0, 3, 0]
    assert HU.accuracy_counts(z, np.array([0, 0, 0, 0])).tolist() == [0, 4, 0, 1]
    with pytest.raises(ValueError):
        HU.compute_accuracy(np.zeros((2, 2)), np.zeros((2, 3)))


class _Counted:
    """A stand-in for a device scalar / count tensor that counts how often its value crosses to the host."""
    reads = 0

    def __init__(self, v):
        self.v = v

    def __float__(self):
        _Counted.reads += 1
        return float(self.v)

    def cpu(self):
        _Counted.reads += 1
        return self.v


@pytest.mark.timeout(60)
def test_train_log_equals_the_per_step_loop_and_reads_lazily():
    rng = np.random.default_rng(7)
    steps, every, decay = 250, 100, 0.99
    loss = rng.uniform(0.1, 2.0, steps).astype(np.float32)
    lr = np.float32(0.00025) * (1 - np.arange(steps) / 1000.0).astype(np.float32)
    counts = []
    for _ in range(steps):
        n_pos = int(rng.integers(0, 1600))
        n_neg = 1600 - n_pos
        counts.append(np.array([[n_pos, n_neg, int(rng.integers(0, n_pos + 1)), int(rng.integers(0, n_neg + 1))]], np.int64))
    # the driver's loop, literally (trainval_video.py:102-121)
    cls_loss_avg = avg_all = avg_pos = avg_neg = 0.0
    want = {}
    for n_iter in range(steps):
        cls_loss_val, lr_val = float(loss[n_iter]), float(lr[n_iter])
        n_pos, n_neg, c_pos, c_neg = (int(v) for v in counts[n_iter][0])
        accuracy_all, accuracy_pos, accuracy_neg = (c_pos + c_neg) / (n_pos + n_neg), c_pos / (n_pos + 1), c_neg / n_neg
        cls_loss_avg = decay * cls_loss_avg + (1 - decay) * cls_loss_val
        avg_all = decay * avg_all + (1 - decay) * accuracy_all
        avg_pos = decay * avg_pos + (1 - decay) * accuracy_pos
        avg_neg = decay * avg_neg + (1 - decay) * accuracy_neg
        if n_iter % every == 0:
            want[n_iter] = ['iter = %d, loss (cur) = %f, loss (avg) = %f, lr = %f' % (n_iter, cls_loss_val, cls_loss_avg, lr_val),
                            'iter = %d, accuracy (cur) = %f (all), %f (pos), %f (neg)' % (n_iter, accuracy_all, accuracy_pos, accuracy_neg),
                            'iter = %d, accuracy (avg) = %f (all), %f (pos), %f (neg)' % (n_iter, avg_all, avg_pos, avg_neg)]
    final = (cls_loss_avg, avg_all, avg_pos, avg_neg)

    log = HU.TrainLog(iters_per_log=every, decay=decay)
    _Counted.reads = 0
    got = {}
    for n_iter in range(steps):
        before = _Counted.reads
        log.add(n_iter, _Counted(loss[n_iter]), _Counted(lr[n_iter]), _Counted(counts[n_iter]))
        assert _Counted.reads == before                                        # add() only stores
        lines = log.lines(n_iter)
        if n_iter % every == 0:
            got[n_iter] = lines
            assert _Counted.reads == 3 * (n_iter + 1)                          # everything up to this step, each value once
        else:
            assert lines == [] and _Counted.reads == before                    # nothing is read before a line is due
    assert sorted(got) == [0, 100, 200] and got == want
    assert _Counted.reads == 3 * 201
    log.flush()
    assert _Counted.reads == 3 * steps
    assert (log.cls_loss_avg, log.avg_accuracy_all, log.avg_accuracy_pos, log.avg_accuracy_neg) == final
    log.flush()
    assert _Counted.reads == 3 * steps                                         # nothing is read twice
    with pytest.raises(ValueError):
        HU.TrainLog(iters_per_log=0)
    with pytest.raises(ValueError):
        HU.TrainLog(iters_per_log=10).lines(0)                                 # a line for a step that was never added


P = 64          # a non-NULL stand-in for device pointers: every call below must fail before anything is launched


@pytest.mark.timeout(60)
def test_train_accuracy_rejects_invalid_arguments():
    lib = L.load()

    def bad(rc, word=b"train_accuracy"):
        return rc == -1 and word in lib.cmpc_last_error()

    assert bad(lib.cmpc_train_accuracy(None, P, 1, 8, 8, 64, 64, P, None))
    assert bad(lib.cmpc_train_accuracy(P, None, 1, 8, 8, 64, 64, P, None))
    assert bad(lib.cmpc_train_accuracy(P, P, 1, 8, 8, 64, 64, None, None))
    for B in (0, -1, L.EVAL_MAX_BATCH + 1):
        assert bad(lib.cmpc_train_accuracy(P, P, B, 8, 8, 64, 64, P, None), b"outside")
    for h, w, H, W in ((0, 8, 64, 64), (8, 0, 64, 64), (8, 8, 0, 64), (8, 8, 64, 0), (-1, 8, 64, 64), (8, 8, 64, -3)):
        assert bad(lib.cmpc_train_accuracy(P, P, 2, h, w, H, W, P, None)), (h, w, H, W)
    assert bad(lib.cmpc_train_accuracy(P, P, 2, 65, 8, 64, 64, P, None), b"larger")
    assert bad(lib.cmpc_train_accuracy(P, P, 2, 8, 65, 64, 64, P, None), b"larger")
