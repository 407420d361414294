"""CPU tests of mask propagation: the symbols and their bindings, the argument validation of cmpc_label_propagate / cmpc_prop_fuse (before
anything is launched: the library loads without a GPU, and the fake pointers would fault if anything ran), hostutil.propagation_plan by
hand, the float64 restatement (tests/propagate_ref.py) on a shifted field, and the share of pixels that
tests/test_gpu_propagate.py::test_mask_case_against_the_float64_chain excludes on tests/propagate_ref.mask_case's seeded inputs."""
import importlib

import numpy as np
import pytest

from tests import propagate_ref as R
from tests import test_segment_host as TS

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("cmpc_label_propagate", "cmpc_label_propagate_workspace", "cmpc_prop_fuse"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.cmpc_abi_version() == L.ABI_VERSION == 4            # additive: new symbols, no layout change
    assert L.PROP_MAX_SOURCES == 4 and L.POOL_MAX_POSITIONS == 1 << 21 and L.PROP_MAX_ROWS == 65535 and L.PROP_MIN_TEMPERATURE == 1e-6
    import ctypes
    assert ctypes.sizeof(L.PropItem) == 4 * (2 + 2 * L.PROP_MAX_SOURCES)


def test_workspace_size_formula():
    for n, h, w in [(1, 1, 1), (8, 40, 40), (32, 4, 4), (3, 7, 9)]:
        assert EV.prop_workspace(n, h, w) == n * (1 + L.PROP_MAX_SOURCES) * h * w * 4
    assert EV.prop_workspace(1, L.PROP_MAX_ROWS, 1) == 5 * L.PROP_MAX_ROWS * 4
    for bad in [(0, 4, 4), (33, 4, 4), (1, 0, 4), (1, 4, 0), (1, 2048, 2048), (1, L.PROP_MAX_ROWS + 1, 1)]:
        with pytest.raises(L.CmpcError, match="label_propagate_workspace"):
            EV.prop_workspace(*bad)
    assert L.load().cmpc_label_propagate_workspace(1, 4, 4, None) == -1


def _item(tgt=0, srcs=((1, 0),)):
    it = L.PropItem()
    it.tgt, it.nsrc = tgt, len(srcs)
    for k, (f, l) in enumerate(srcs[: L.PROP_MAX_SOURCES]):
        it.src[k], it.label[k] = f, l
    return it


def _prop(lib, dt=1, feat=64, stride=None, frames=3, labels=64, n_labels=2, items=None, n=None, h=4, w=6, C=16, radius=2, t=0.07, out=64,
          peak=64, ws=64, ws_bytes=None):
    items = [_item(), _item(2, ((0, 1), (1, 0)))] if items is None else items
    n = len(items) if n is None else n
    arr = (L.PropItem * max(len(items), 1))(*items) if items != "null" else None
    stride = h * w * C if stride is None else stride
    ws_bytes = (1 << 20) if ws_bytes is None else ws_bytes
    return lib.cmpc_label_propagate(dt, feat, stride, frames, labels, n_labels, arr, n, h, w, C, radius, t, out, peak, ws, ws_bytes, None)


def test_label_propagate_rejects_invalid_arguments_before_launch():
    """Every call passes fake pointers: had a kernel been launched (or a pointer been followed) the process would fault."""
    lib = L.load()

    def bad(word, **kw):
        assert _prop(lib, **kw) == -1, kw
        msg = lib.cmpc_last_error()
        assert b"label_propagate" in msg and word in msg, (kw, msg)
    for p in ("feat", "labels", "out", "ws"):
        bad(b"NULL", **{p: None})
    bad(b"NULL", items="null", n=1)
    for n in (0, -1, L.EVAL_MAX_BATCH + 1):
        bad(b"outside", n=n)
    for kw in (dict(h=0), dict(w=0), dict(h=-3)):
        bad(b"empty", **kw)
    bad(b"positions", h=2048, w=2048)
    bad(b"rows", h=L.PROP_MAX_ROWS + 1, w=1)                       # a tall thin grid: more rows than a launch has workgroup rows
    for C in (0, 4, 12, 1001):
        bad(b"multiple of 8", C=C)
    for dt in (3, -1):
        bad(b"dtype", dt=dt)
    for kw in (dict(frames=0), dict(n_labels=0)):
        bad(b"empty bank", **kw)
    for stride in (4 * 6 * 16 - 8, 4 * 6 * 16 + 4, -8, 0):
        bad(b"stride", stride=stride)
    for t in (0.0, -0.07, float("nan"), float("inf"), 1e-30, 0.99e-6):     # a tiny one would take c / temperature out of float32
        bad(b"temperature", t=t)
    it0, it5 = _item(), _item(0, ((1, 0),) * 5)
    it0.nsrc, it5.nsrc = 0, 5
    bad(b"sources", items=[it0])
    bad(b"sources", items=[_item(), it5])
    for it in (_item(3), _item(-1)):
        bad(b"target frame", items=[it])
    for it in (_item(0, ((3, 0),)), _item(0, ((1, 0), (-1, 0)))):
        bad(b"source frame", items=[_item(), it])
    for it in (_item(0, ((1, 2),)), _item(0, ((1, 0), (1, 0), (1, -1)))):
        bad(b"label", items=[it])
    need = EV.prop_workspace(2, 4, 6)
    bad(b"workspace", ws_bytes=need - 1)
    bad(b"workspace", ws_bytes=0)
    for kw in (dict(feat=72), dict(ws=72), dict(labels=66), dict(out=66), dict(peak=65)):
        bad(b"aligned", **kw)
    # an index past nsrc is not looked at, and peak may be NULL: these would pass the checks, so they are not tried here (they would launch)


def test_prop_fuse_rejects_invalid_arguments_before_launch():
    lib = L.load()

    def call(own=64, prop=64, n=2, h=5, w=7, H=40, W=56, alpha=0.5, fused=64):
        return lib.cmpc_prop_fuse(own, prop, n, h, w, H, W, alpha, fused, None)
    for kw in (dict(own=None), dict(prop=None), dict(fused=None)):
        assert call(**kw) == -1 and b"prop_fuse" in lib.cmpc_last_error() and b"NULL" in lib.cmpc_last_error()
    for n in (0, -2, L.EVAL_MAX_BATCH + 1):
        assert call(n=n) == -1 and b"outside" in lib.cmpc_last_error()
    for kw in (dict(h=0), dict(w=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == -1 and b"empty" in lib.cmpc_last_error()
    assert call(h=2048, w=2048) == -1 and b"too large" in lib.cmpc_last_error()
    for alpha in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(alpha=alpha) == -1 and b"alpha" in lib.cmpc_last_error()
    for kw in (dict(own=66), dict(prop=65), dict(fused=67)):
        assert call(**kw) == -1 and b"aligned" in lib.cmpc_last_error()


def test_wrappers_reject_host_arrays_and_bad_items():
    with pytest.raises(ValueError):
        EV.label_propagate(np.zeros((2, 2, 2, 8), np.float32), np.zeros((1, 2, 2), np.float32), [(0, [(1, 0)])])
    with pytest.raises(ValueError):
        EV.prop_fuse(np.zeros((1, 8, 8), np.float32), np.zeros((1, 2, 2), np.float32), 0.5)
    its = EV.prop_items([(0, [(1, 0)]), (2, [(0, 1), (1, 0), (3, 2), (4, 3)])])
    assert [(i.tgt, i.nsrc, list(i.src), list(i.label)) for i in its] == [(0, 1, [1, 0, 0, 0], [0, 0, 0, 0]), (2, 4, [0, 1, 3, 4], [1, 0, 2, 3])]
    for bad in ([(0, [])], [(0, [(1, 0)] * 5)], [3], [(0, [1])]):
        with pytest.raises(ValueError, match="item 0"):
            EV.prop_items(bad)


# ---- hostutil.propagation_plan ---------------------------------------------------------------------------------------------------------
def test_propagation_plan_by_hand():
    ids = list(range(8))
    # reach from both sides, nearest first; frames 6 and 7 are out of reach of every pivot and left out
    assert HU.propagation_plan(ids, [1, 3]) == {0: [1], 2: [1, 3], 4: [3], 5: [3]}
    # ties go to the lower frame, whatever the order the pivots come in
    assert HU.propagation_plan(ids, [4, 0], 2) == {1: [0], 2: [0, 4], 3: [4], 5: [4], 6: [4]}
    assert HU.propagation_plan(ids, [0, 4], 3)[2] == [0, 4] and HU.propagation_plan(ids, [0, 4], 3)[3] == [4, 0]
    assert HU.propagation_plan(ids, [2, 4, 6], 3, max_sources=2)[3] == [2, 4] and HU.propagation_plan(ids, [2, 4, 6], 3)[3] == [2, 4, 6]
    assert HU.propagation_plan(ids, [2, 4, 6], 3, max_sources=1) == {0: [2], 1: [2], 3: [2], 5: [4], 7: [6]}
    # num_propagate = 0: nobody receives; no pivots: nobody receives; every frame a pivot: nobody receives
    assert HU.propagation_plan(ids, [1, 3], 0) == {} and HU.propagation_plan(ids, []) == {} and HU.propagation_plan(ids, ids) == {}
    # distance is the position in frame_ids, not the difference of the ids
    assert HU.propagation_plan([10, 20, 30, 40, 50], [10], 2) == {20: [10], 30: [10]}
    assert HU.propagation_plan([5, 3, 9], [9], 1) == {3: [9]}
    # what find_pivot_frames gives with the same num_propagate leaves no frame out
    for p in (1, 2, 3):
        piv = HU.find_pivot_frames(np.random.default_rng(p).uniform(0, 1, (17, 5)), p)
        plan = HU.propagation_plan(range(17), piv, p)
        assert sorted(list(plan) + piv) == list(range(17)) and all(1 <= len(v) <= 4 for v in plan.values())
    with pytest.raises(ValueError, match="pivot 9"):
        HU.propagation_plan(ids, [1, 9])
    for kw in (dict(num_propagate=-1), dict(max_sources=0)):
        with pytest.raises(ValueError):
            HU.propagation_plan(ids, [1], **kw)
    with pytest.raises(ValueError, match="twice"):
        HU.propagation_plan([1, 2, 1], [1])


# ---- the float64 restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0, 0), (2, -1), (-3, 3), (1, 2)])
def test_reference_gives_back_a_shifted_label(shift):
    """A source field of random unit vectors and a target that is the field shifted by (dy, dx) inside the radius: at temperature 0.01
    every target whose origin lies in the grid receives the label of that origin, within the bound."""
    dy, dx = shift
    h, w, C, radius, T = 9, 11, 64, 3, 0.01
    rng = np.random.default_rng(3)
    src = R.l2_normalize(rng.normal(0, 1, (h, w, C)))
    tgt = R.l2_normalize(rng.normal(0, 1, (h, w, C)))
    ys, xs = np.mgrid[0:h, 0:w]
    oy, ox = ys + dy, xs + dx
    ok = (oy >= 0) & (oy < h) & (ox >= 0) & (ox < w)
    tgt[ok] = src[oy[ok], ox[ok]]
    label = rng.uniform(0, 1, (1, h, w))
    out, peak, cnt = R.propagate(np.stack([src, tgt]), label, [(1, [(0, 0)])], radius, T)
    lim = R.bound(C, cnt[0], T, 1.0)
    assert ok.sum() >= (h - 3) * (w - 3)
    assert np.all(np.abs(out[0][ok] - label[0][oy[ok], ox[ok]]) <= lim[ok])
    assert np.all(np.abs(peak[0][ok] - 1.0) <= R.delta(C))
    assert cnt.max() == (2 * radius + 1) ** 2 and cnt.min() == (radius + 1) ** 2


def test_reference_fuse_and_bound_by_hand():
    own = np.array([[[0.25, 0.5], [0.75, 1.0]]], np.float32)
    prop = np.array([[[0.5]]], np.float32)
    ref, lim = R.fuse(own, prop, 0.5)
    assert np.array_equal(ref, 0.5 * own + 0.25) and np.all(lim > 0) and np.all(lim < 30 * R.U)
    ref0, lim0 = R.fuse(own, prop, 0.0)
    assert np.array_equal(ref0, own.astype(np.float64)) and not lim0.any()
    u, M = R.upsample(np.array([[[0.0, 1.0], [2.0, 3.0]]]), 4, 4)
    assert u[0, 0].tolist() == [0.0, 0.5, 1.0, 1.0] and u[0, :, 0].tolist() == [0.0, 1.0, 2.0, 2.0] and u[0, 1, 1] == 1.5 and M.max() == 3.0
    assert R.bound(8, 1, 1.0, 2.0) == (np.expm1(2 * 16 * R.U) + 9 * R.U + R.EPS_EXP) * 2.0
    x = np.array([1.0, 1.00390625, -2.5, 65504.0, 1e-3], np.float32)
    assert np.array_equal(R.stored(x, "f16"), x.astype(np.float16).astype(np.float32))
    assert R.stored(np.array([1.00390625], np.float32), "bf16")[0] == 1.0 and R.stored(np.array([1.01171875], np.float32), "bf16")[0] == 1.015625


@pytest.mark.parametrize("seed", R.MASK_SEEDS)
def test_share_of_pixels_the_mask_test_excludes(seed):
    """tests/test_gpu_propagate.py::test_mask_case_against_the_float64_chain runs the kernels on R.mask_case(seed) for R.MASK_SEEDS and
    compares the masks with R.mask_reference everywhere except where the reference's fused value lies within the bound of the
    threshold.  Both sides come from the float64 reference alone, so the share it excludes is computed here, on the same inputs and
    plan: at most 1 % of any mask, known before any GPU run; the masks are neither empty nor full.  (The segmenter test on the tiny
    model's own taps and sigm has inputs that exist only on the device; it asserts the same cap itself.)"""
    s = R.MASK_SHAPE
    feat, sigm = R.mask_case(seed)
    plan = HU.propagation_plan(range(s["frames"]), [0, 4], 2)
    assert sorted(plan) == [1, 2, 3]
    res = R.mask_reference(feat, sigm, plan, s["radius"], s["temperature"], s["alpha"], s["threshold"])
    for f, (ref, lim, mask, unsure) in res.items():
        print("seed %d frame %d: %.4f %% of the pixels within the bound of the threshold, foreground %.3f" % (seed, f, 100 * unsure.mean(), mask.mean()))
        assert unsure.mean() <= 0.01 and 0.05 < mask.mean() < 0.95


# ---- FrameSegmenter(propagate=) without a device ---------------------------------------------------------------------------------------
def test_check_propagate_options():
    m = TS.FakeModel()
    assert SG.check_propagate(m, None, None) is None
    d = SG.check_propagate(m, {}, None)
    assert (d.level, d.radius, d.temperature, d.alpha, d.num_propagate, d.bank, d.results) == ("c4", 12, 0.07, 0.5, 2, 128, 512)
    assert SG.check_propagate(m, {}, "c5").level == "c5" and SG.check_propagate(m, {"level": "c4"}, "c5").level == "c4"

    class Opt:
        radius, alpha = -1, 0.0
    d = SG.check_propagate(m, Opt(), None)
    assert d.radius == -1 and d.alpha == 0.0 and d.bank == 128
    for bad in ({"level": "c3"}, {"level": "c6"}, {"temperature": 0}, {"temperature": 1e-9}, {"temperature": float("nan")}, {"alpha": 1.5}, {"alpha": -0.1},
                {"num_propagate": -1}, {"bank": 0}, {"results": 0}, {"radius": 1.5}, {"window": 3}, 7, "c4"):
        with pytest.raises(ValueError, match="propagate"):
            SG.check_propagate(m, bad, None)


def test_propagate_needs_a_run_and_no_dcrf():
    with pytest.raises(ValueError, match="dcrf"):
        SG.FrameSegmenter(TS.FakeModel(), dcrf=True, propagate={}, _stage=TS.FakeStage(3))
    seg = SG.FrameSegmenter(TS.FakeModel(), _stage=TS.FakeStage(3, check_reuse=False))
    with pytest.raises(RuntimeError, match="propagate="):
        next(iter(seg.propagate({0: [0]})))
    # with propagate=None the stage is called as before: the older fake stage knows no `propagate` argument
    n = sum(1 for _ in seg.run(TS._frames(5), TS._exprs()))
    assert n == 15


class PropagatingStage(TS.FakeStage):
    """FakeStage that knows the fifth call shape of segment() and propagate_batch(): the 'propagated mask' of (e, f) is filled with
    100 + 10 * e + f."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.banked, self.batches = [], []

    def segment(self, token, e, descs, nbytes, slot, propagate=None):
        super().segment(token, e, descs, nbytes, slot)
        assert propagate is not None
        self.banked.append((e, propagate[0], len(descs), propagate[1]))

    def propagate_batch(self, e, frames, sources, F, descs, nbytes, slot, jf=None, clean=None):
        assert nbytes <= self.reserved and jf is None and clean is None and len(frames) == len(descs) == len(sources)
        self.batches.append((e, list(frames), [list(s) for s in sources], F, slot))
        for f, d in zip(frames, descs):
            self.bufs[slot][d.offset: d.offset + d.h * d.w] = 100 + 10 * e + f


@pytest.mark.parametrize("n,depth,ready", [(11, 2, True), (6, 1, False)])
def test_frame_segmenter_propagate_plumbing(n, depth, ready):
    """run() yields what it yields without the option and hands the stage (first frame, F) with every segment call; propagate() plans
    per expression, batches of B ascending frames with their pivots nearest first, and yields exactly the plan's (e, f) at each
    frame's own out size; an oversize video raises before any work."""
    B = 4
    frames, exprs = TS._frames(n), TS._exprs()
    st0 = TS.FakeStage(depth + 1, ready=ready, check_reuse=False)
    plain = [(e, f, mk.copy()) for e, f, mk in SG.FrameSegmenter(TS.FakeModel(B=B), depth=depth, _stage=st0).run(frames, exprs)]
    st = PropagatingStage(depth + 1, ready=ready, check_reuse=False)
    seg = SG.FrameSegmenter(TS.FakeModel(B=B), depth=depth, propagate={"num_propagate": 2}, _stage=st)
    got = [(e, f, mk.copy()) for e, f, mk in seg.run(iter(frames), exprs, seq="v")]
    assert len(got) == len(plain) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    assert [x for x in st.log if x[0] == "segment"] == [x for x in st0.log if x[0] == "segment"]
    assert st.banked == [(e, b[0], len(set(b)), n) for b in SG.plan_batches(n, B) for e in range(3)]
    pivots = {0: [1], 1: [0, n - 1], 2: list(range(n))}
    out = [(e, f, mk.copy()) for e, f, mk in seg.propagate(pivots)]
    plans = {e: HU.propagation_plan(range(n), pivots[e], 2, 4) for e in range(3)}
    assert plans[2] == {} and [x[:2] for x in out] == [(e, f) for e in range(3) for f in sorted(plans[e])]
    for e, f, mk in out:
        h, w = frames[f].shape[:2]
        assert mk.shape == (h // 2, w // 2) and np.all(mk == 100 + 10 * e + f)
    want = []
    for e in range(3):
        todo = sorted(plans[e])
        want += [(e, todo[s: s + B], [plans[e][f] for f in todo[s: s + B]], n) for s in range(0, len(todo), B)]
    assert [b[:4] for b in st.batches] == want and all(0 <= b[4] <= depth for b in st.batches)
    # a PivotLog under the run's sequence keys gives the same plan as its pivots
    log = HU.PivotLog()
    rng = np.random.default_rng(n)
    for e in range(3):
        for f in range(n):
            log.add(("v", e), f, rng.uniform(0, 1, 5), 1.0, (1, 2))
    st.batches.clear()
    out2 = [x[:2] for x in seg.propagate(log)]
    assert out2 == [(e, f) for e in range(3) for f in sorted(HU.propagation_plan(range(n), log.pivots(("v", e), 2), 2, 4))]
    with pytest.raises(KeyError):
        next(seg.propagate(log, seq="other"))
    for opt in ({"bank": n - 1}, {"results": 3 * n - 1}):
        st2 = PropagatingStage(depth + 1)
        with pytest.raises(ValueError, match="exceed the banks"):
            next(SG.FrameSegmenter(TS.FakeModel(B=B), propagate=opt, _stage=st2).run(frames, exprs))
        assert st2.log == []
