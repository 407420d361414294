"""CPU tests of J / F scoring: hand-worked answers of the NumPy restatement (tests/jf_ref.py), hostutil.jf_radius / jf_from_counts / JFEval,
cmpc_mask_jf's export, workspace size and argument validation (before anything is launched: the library loads without a GPU, and the
fake pointers would fault if anything ran), and the segmenters' ground-truth plumbing driven through fake device stages."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import jf_ref as R
from tests import test_clip_segment_host as TC
from tests import test_segment_host as TS

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")


def _jf(pred, gt, r):
    return HU.jf_from_counts(R.counts(pred, gt, r))


# ---- the restatement, by hand --------------------------------------------------------------------------------------------------------
def test_bmap_small_shapes_by_hand():
    assert R.bmap(np.ones((1, 1))).tolist() == [[False]] and R.bmap(np.zeros((1, 1))).tolist() == [[False]]
    # 1 x w: the last row rule seg ^ e, then the last column seg ^ s = seg, then the corner 0
    assert R.bmap(np.array([[0, 1, 1, 0, 1]])).astype(int).tolist() == [[1, 0, 1, 1, 0]]
    assert R.bmap(np.array([[1, 1, 1]])).astype(int).tolist() == [[0, 0, 0]]
    # h x 1: every row is the last column: seg ^ s, the last pixel 0
    assert R.bmap(np.array([[0], [1], [1], [0], [1]])).astype(int).tolist() == [[1], [0], [1], [1], [0]]
    # 2 x 2: [0, 0] by the general rule, [0, 1] by the column rule, [1, 0] by the row rule, [1, 1] = 0
    assert R.bmap(np.array([[1, 0], [0, 0]])).astype(int).tolist() == [[1, 0], [0, 0]]
    assert R.bmap(np.array([[0, 0], [0, 1]])).astype(int).tolist() == [[1, 1], [1, 0]]
    assert R.bmap(np.array([[0, 1], [0, 0]])).astype(int).tolist() == [[1, 1], [0, 0]]
    assert R.bmap(np.array([[1, 1], [1, 1]])).astype(int).tolist() == [[0, 0], [0, 0]]
    # a 2 x 2 square inside 5 x 5: the boundary sits on the square's top-left side, one pixel out, and on its last row and column
    seg = np.zeros((5, 5), int)
    seg[2:4, 2:4] = 1
    assert R.bmap(seg).astype(int).tolist() == [[0, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 0, 1, 0], [0, 1, 1, 1, 0], [0, 0, 0, 0, 0]]


def test_dilate_is_the_disc():
    b = np.zeros((9, 9), bool)
    b[4, 4] = True
    d = R.dilate(b, 2)
    yy, xx = np.mgrid[0:9, 0:9]
    assert np.array_equal(d, (yy - 4) ** 2 + (xx - 4) ** 2 <= 4) and d.sum() == 13
    b[:] = False
    b[0, 0] = True                                              # nothing enters from outside, nothing wraps around
    assert R.dilate(b, 3).sum() == 11 and not R.dilate(b, 3)[-1].any() and not R.dilate(b, 3)[:, -1].any()
    assert R.dilate(np.ones((1, 1), bool), 128).tolist() == [[True]]


def test_known_answers():
    rng = np.random.default_rng(0)
    m = rng.random((20, 30)) < 0.5
    assert _jf(m, m, 1) == (1.0, 1.0)                                       # identical masks
    e = np.zeros((20, 30), bool)
    assert R.counts(e, e, 2).tolist() == [0] * 6 and _jf(e, e, 2) == (1.0, 1.0)          # both empty
    sq = np.zeros((20, 30), bool)
    sq[5:12, 6:15] = True
    c = R.counts(e, sq, 2)                                                   # empty prediction: P = 1, R = 0, F = 0
    assert c[2] == 0 and c[3] > 0 and c[0] == 0 and c[1] == 63 and HU.jf_from_counts(c) == (0.0, 0.0)
    c = R.counts(sq, e, 2)                                                   # empty ground truth: P = 0, R = 1, F = 0
    assert HU.jf_from_counts(c) == (0.0, 0.0)
    sh = np.roll(sq, 1, axis=1)                                              # the square one pixel to the east
    c = R.counts(sh, sq, 1)
    assert c[0] == 7 * 8 and c[1] == 7 * 10 and c[2] == c[3] == c[4] == c[5] and c[2] > 0
    assert HU.jf_from_counts(c) == (0.8, 1.0)
    far = np.roll(sq, 15, axis=1)                                            # fifteen pixels east: no boundary pixel within radius 2
    assert HU.jf_from_counts(R.counts(far, sq, 2))[1] == 0.0
    # the counters by hand on 1 x 5: bmap(pred) = 10110 -> n_pred 3; bmap(gt) = 01000 -> n_gt 1; radius 1 matches pixels 0 and 2
    c = R.counts(np.array([[0, 1, 1, 0, 1]]), np.array([[0, 0, 1, 1, 1]]), 1)
    assert c.tolist() == [2, 4, 3, 1, 2, 1]
    assert HU.jf_from_counts(c) == (0.5, 2 * (2 / 3) * 1.0 / (2 / 3 + 1.0))
    assert HU.jf_from_counts([0, 5, 4, 4, 0, 0]) == (0.0, 0.0)              # P + R = 0


def test_jf_radius():
    assert HU.jf_radius(720, 1280) == 12 and HU.jf_radius(33, 129) == 2 and HU.jf_radius(360, 640) == 6 and HU.jf_radius(1, 1) == 1
    assert HU.jf_radius(720, 1280, 3) == 3 and HU.jf_radius(5, 5, 1) == 1 and HU.jf_radius(5, 5, 2.0) == 2      # >= 1 passes through
    assert isinstance(HU.jf_radius(480, 640), int) and HU.jf_radius(480, 640) == 7                                # 0.008 * 800 = 6.4
    assert HU.jf_radius(300, 400, 0.01) == 5                                                                      # exactly 5.0: no round-up
    for bad in ((0, 5, 0.008), (5, 5, 0.0), (5, 5, 2.5), (5, 5, -1)):
        with pytest.raises(ValueError):
            HU.jf_radius(*bad)


def _counts_for(J, F):
    """Counts whose scores are exactly J = a / 10 and F = P = R = b / 10."""
    return [int(round(J * 10)), 10, 10, 10, int(round(F * 10)), int(round(F * 10))]


def test_jfeval_by_hand():
    assert HU.jf_decay_bins(5) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert HU.jf_decay_bins(4) == [(0, 1), (1, 2), (2, 2), (2, 3)]          # linspace(1, 4, 5) = 1, 1.75, 2.5, 3.25, 4 -> 1, 2, 3, 3, 4
    assert HU.jf_decay_bins(1) == [(0, 0)] * 4
    ev = HU.JFEval()
    Ja, Fa = [0.9, 0.7, 0.6, 0.4, 0.2], [1.0, 0.8, 0.5, 0.5, 0.3]
    for f in (3, 0, 4, 1, 2):                                                # any order: the statistics take frames in frame order
        ev.add("a", 10 * f, _counts_for(Ja[f], Fa[f]))
    Jb, Fb = [0.2, 0.6, 0.8, 1.0], [0.1, 0.1, 0.7, 0.9]
    for f in range(4):
        ev.add(("b", 1), f, _counts_for(Jb[f], Fb[f]))
    res = ev.result()
    a, b = res["per_sequence"]["a"], res["per_sequence"][("b", 1)]
    assert a["frames"] == 5 and b["frames"] == 4 and res["sequences"] == 2 and res["frames"] == 9
    assert a["J_mean"] == pytest.approx(0.56) and a["J_recall"] == 3 / 5 and a["J_decay"] == pytest.approx((0.9 + 0.7) / 2 - (0.4 + 0.2) / 2)
    assert a["F_mean"] == pytest.approx(0.62) and a["F_recall"] == 2 / 5 and a["F_decay"] == pytest.approx(0.9 - 0.4)
    assert b["J_mean"] == pytest.approx(0.65) and b["J_recall"] == 3 / 4 and b["J_decay"] == pytest.approx(0.4 - 0.9)
    assert b["F_mean"] == pytest.approx(0.45) and b["F_recall"] == 2 / 4 and b["F_decay"] == pytest.approx(0.1 - 0.8)
    for k in HU.JF_KEYS:
        assert res[k] == pytest.approx((a[k] + b[k]) / 2)
    assert res["J&F"] == (res["J_mean"] + res["F_mean"]) / 2 == pytest.approx((0.605 + 0.535) / 2)
    with pytest.raises(ValueError, match="already"):
        ev.add("a", 0, _counts_for(1, 1))
    with pytest.raises(ValueError):
        HU.JFEval().result()
    one = HU.JFEval()
    one.add(0, 7, [3, 4, 0, 0, 0, 0])
    r1 = one.result()
    assert (r1["J_mean"], r1["F_mean"], r1["J_decay"], r1["J_recall"], r1["J&F"]) == (0.75, 1.0, 0.0, 1.0, 0.875)


# ---- the C entry: exported, bound, sized and validated without a GPU ---------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("cmpc_mask_jf", "cmpc_mask_jf_workspace"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.cmpc_abi_version() == L.ABI_VERSION == 4            # additive: two new symbols
    assert L.JF_MAX_RADIUS == 128 and ctypes.sizeof(L.JfDesc) == 32 and EV.JF_COUNTS == 6


def _descs(items):
    return (L.JfDesc * len(items))(*[L.JfDesc(*it, 0) for it in items])


def test_workspace_size_formula():
    lib = L.load()
    shapes = [(1, 1), (1, 64), (1, 65), (70, 1), (7, 128), (33, 129), (720, 1280)]
    out = ctypes.c_int64(-1)
    for h, w in shapes:
        assert lib.cmpc_mask_jf_workspace(_descs([(0, 0, h, w, 1)]), 1, ctypes.byref(out)) == 0
        assert out.value == 8 * 2 * h * -(-w // 64), (h, w)
    d = _descs([(0, 0, h, w, 3) for h, w in shapes])
    assert lib.cmpc_mask_jf_workspace(d, len(shapes), ctypes.byref(out)) == 0
    assert out.value == sum(8 * 2 * h * -(-w // 64) for h, w in shapes) == EV.jf_workspace(d, len(shapes))
    plan = EV.JfPlan(shapes, [0] * 7, gts=[np.zeros(s, np.uint8) for s in shapes])
    assert plan.ws_bytes == out.value and [d.r for d in plan.descs] == [HU.jf_radius(h, w) for h, w in shapes]
    assert [o.offset for o in plan.gt_offs] == [0, 16, 80, 160, 240, 1136, 5408] and plan.gt_bytes == 5408 + 720 * 1280
    for bad, word in ((dict(B=0), b"outside"), (dict(B=33), b"outside"), (dict(d=None), b"NULL"), (dict(out=None), b"NULL")):
        kw = dict(d=d, B=7, out=ctypes.byref(out))
        kw.update(bad)
        assert lib.cmpc_mask_jf_workspace(kw["d"], kw["B"], kw["out"]) == -1
        assert b"mask_jf_workspace" in lib.cmpc_last_error() and word in lib.cmpc_last_error()
    assert lib.cmpc_mask_jf_workspace(_descs([(0, 0, 0, 5, 1)]), 1, ctypes.byref(out)) == -1 and b"empty" in lib.cmpc_last_error()
    assert lib.cmpc_mask_jf_workspace(_descs([(0, 0, 5, 5, 129)]), 1, ctypes.byref(out)) == -1 and b"radius" in lib.cmpc_last_error()


def test_mask_jf_rejects_invalid_arguments_before_launch():
    """The pointers are fake (8 is aligned, and nothing else): had a kernel been launched or a pointer been followed, the process would fault."""
    lib = L.load()
    good = [(0, 0, 10, 20, 2), (208, 200, 7, 65, 1)]
    need = 8 * 2 * (10 * 1 + 7 * 2)

    def call(items=good, B=None, pred=8, pb=208 + 455, gt=8, gb=200 + 455, counts=8, ws=8, wb=need, descs=True):
        d = _descs(items) if descs else None
        return lib.cmpc_mask_jf(pred, pb, gt, gb, d, len(items) if B is None else B, counts, ws, wb, None)

    def bad(word, **kw):
        assert call(**kw) == -1, kw
        msg = lib.cmpc_last_error()
        assert b"mask_jf" in msg and word in msg, (kw, msg)

    for k in ("pred", "gt", "counts", "ws"):
        bad(b"NULL", **{k: None})
    bad(b"NULL", descs=False)
    for B in (0, -1, L.EVAL_MAX_BATCH + 1):
        bad(b"outside 1..32", B=B, items=good * 17)
    bad(b"sample 1: empty", items=[good[0], (208, 200, 0, 65, 1)])
    bad(b"sample 0: empty", items=[(0, 0, 10, -3, 2), good[1]])
    for r in (0, -1, L.JF_MAX_RADIUS + 1):
        bad(b"sample 1: radius", items=[good[0], (208, 200, 7, 65, r)])
    bad(b"workspace", items=[good[0], (208, 200, 7, 65, L.JF_MAX_RADIUS)], wb=0)      # 128 itself passes the radius check
    bad(b"sample 1: prediction", pb=208 + 454)
    bad(b"sample 1: ground truth", gb=200 + 454)
    bad(b"sample 0: prediction", items=[(-16, 0, 10, 20, 2), good[1]])
    bad(b"sample 0: ground truth", items=[(0, 700, 10, 20, 2), good[1]])
    bad(b"workspace", wb=need - 1)
    bad(b"workspace", wb=0)
    bad(b"aligned", ws=12)
    bad(b"aligned", counts=4)
    with pytest.raises(L.CmpcError, match="mask_jf"):
        L.call("cmpc_mask_jf", 8, 10, 8, 10, _descs([(0, 0, 4, 4, 1)]), 1, 8, 8, 8 * 2 * 4, None)
    with pytest.raises(ValueError):
        EV.mask_jf([np.zeros((4, 4))], [])
    with pytest.raises(ValueError, match="radius"):
        EV.JfPlan([(4, 4)], [0], gts=[np.zeros((4, 4), np.uint8)], bound_th=200)


# ---- the segmenters' ground-truth plumbing, through fake stages -------------------------------------------------------------------------
def _gt_for(e, f, size):
    g = np.zeros(size, np.uint8)
    g[: 1 + (e + f) % size[0], : 1 + (3 * e + f) % size[1]] = 1 + e
    return g


class ScoringFrameStage(TS.FakeStage):
    """FakeStage whose segment() also 'scores': the counts of jf_ref on the mask it wrote and the plan's ground truths, at the plan's
    place in the slot."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.plans = []

    def segment(self, token, e, descs, nbytes, slot, jf=None):
        super().segment(token, e, descs, nbytes, slot)
        self.plans.append((e, jf))
        if jf is not None:
            assert SG.scored_bytes(nbytes, jf.n) <= self.reserved and jf.counts_off % 8 == 0 and jf.counts_off >= nbytes
            _fake_score(self.bufs[slot], self.bufs[slot], jf)


def _fake_score(src, dst, jf):
    out = dst[jf.counts_off: jf.counts_off + 48 * jf.n].view(np.int64).reshape(jf.n, 6)
    for k, d in enumerate(jf.descs):
        pred = src[d.pred_off: d.pred_off + d.h * d.w].reshape(d.h, d.w)
        assert jf.gts[k].shape == (d.h, d.w) and jf.gts[k].dtype == np.uint8 and jf.gt_offs[k].offset == d.gt_off
        out[k] = R.counts(pred, jf.gts[k], d.r)


@pytest.mark.parametrize("n,depth,ready", [(7, 2, True), (5, 1, False), (4, 3, True)])
def test_frame_segmenter_ground_truth_plumbing(n, depth, ready):
    B = 4
    frames, exprs = TS._frames(n), TS._exprs()
    plain = [(e, f, mk.copy()) for e, f, mk in SG.FrameSegmenter(TS.FakeModel(B=B), depth=depth, _stage=TS.FakeStage(depth + 1, ready=ready, check_reuse=False)).run(frames, exprs)]
    calls = []

    def gt(e, f):
        calls.append((e, f))
        if f % 2:
            return None                                          # every other frame is not annotated
        h, w = frames[f].shape[:2]
        g = _gt_for(e, f, (h // 2, w // 2))
        return (np.repeat((g * 40)[..., None], 3, 2), (40 * (1 + e), 0, 0)) if e == 1 else g       # an (annotation, key) pair, or a mask

    st = ScoringFrameStage(depth + 1, ready=ready, check_reuse=False)
    seg = SG.FrameSegmenter(TS.FakeModel(B=B), depth=depth, _stage=st)
    assert seg.jf is None
    got = [(e, f, mk.copy()) for e, f, mk in seg.run(iter(frames), exprs, ground_truth=gt, seq="vid")]
    assert len(got) == len(plain) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    want_order = [(e, f) for b in SG.plan_batches(n, B) for e in range(3) for f in sorted(set(b))]
    assert calls == want_order                                   # once per pair (pads never), in enqueue order
    want = HU.JFEval()
    for e, f, mk in got:
        if f % 2 == 0:
            h, w = mk.shape
            want.add(("vid", e), f, R.counts(mk, _gt_for(e, f, (h, w)), HU.jf_radius(h, w)))
    assert seg.jf.result() == want.result() and seg.jf.result()["frames"] == 3 * ((n + 1) // 2)
    # a batch without an annotated frame enqueues no scoring at all
    assert all((jf is None) == (not any(f % 2 == 0 for f in fr)) for (e, jf), fr in zip(st.plans, [x[2] for x in st.log if x[0] == "segment"]))
    # a caller's JFEval is used and kept; a wrong shape names the pair
    mine = HU.JFEval()
    list(seg.run(frames, exprs, ground_truth=gt, jf=mine, seq=1))
    assert seg.jf is mine and set(mine.seqs) == {(1, 0), (1, 1), (1, 2)}
    with pytest.raises(ValueError, match=r"expression 0, frame 0.*\(5, 5\)"):
        list(seg.run(frames, exprs, ground_truth=lambda e, f: np.zeros((5, 5), np.uint8)))
    with pytest.raises(ValueError, match="expression 2, frame 0"):
        list(seg.run(frames, exprs, ground_truth=lambda e, f: np.zeros((5, 5, 3), np.uint8) if e == 2 else None))


class ScoringClipStage(TC.FakeStage):
    def finish(self, f, slot, nbytes, jf=None):
        super().finish(f, slot, nbytes)
        self.log.append(("jf", f, None if jf is None else list(jf.idx)))
        if jf is not None:
            assert SG.scored_bytes(nbytes, jf.n) <= self.reserved and jf.counts_off % 8 == 0 and jf.counts_off >= nbytes
            _fake_score(self.dev, self.bufs[slot], jf)


def _drain(st, gen):
    out = []
    for e, f, mk in gen:
        out.append((e, f, mk.copy()))
        st.consumed.add((e, f))
    return out


@pytest.mark.parametrize("n,E,depth,ready", [(11, 3, 2, True), (6, 1, 1, False), (23, 2, 3, True)])
def test_clip_segmenter_ground_truth_plumbing(n, E, depth, ready):
    frames, exprs = list(TC._frames(n)), TC._exprs(E)
    st0 = TC.FakeStage(32, depth + 1, n, ready=ready)
    plain = _drain(st0, SG.ClipSegmenter(TC.FakeModel(), depth=depth, _stage=st0).run(frames, exprs))
    calls = []

    def gt(e, f):
        calls.append((e, f))
        if f % 2 or (e == 1 and f == 4):                         # every other frame, and one expression absent from one frame
            return None
        return _gt_for(e, f, frames[f].shape[:2])

    st = ScoringClipStage(32, depth + 1, n, ready=ready)
    seg = SG.ClipSegmenter(TC.FakeModel(), depth=depth, _stage=st)
    got = _drain(st, seg.run(iter(frames), exprs, ground_truth=gt, seq="v"))
    assert len(got) == len(plain) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    assert calls == [(e, f) for f in range(n) for e in range(E)]
    want = HU.JFEval()
    for e, f, mk in got:
        if not (f % 2 or (e == 1 and f == 4)):
            want.add(("v", e), f, R.counts(mk, _gt_for(e, f, mk.shape), HU.jf_radius(*mk.shape)))
    assert seg.jf.result() == want.result()
    assert [x[1:] for x in st.log if x[0] == "jf"] == [(f, None if f % 2 else [e for e in range(E) if not (e == 1 and f == 4)]) for f in range(n)]
    with pytest.raises(ValueError, match=r"expression 0, frame 0"):
        list(SG.ClipSegmenter(TC.FakeModel(), _stage=ScoringClipStage(32, 3, n)).run(frames, exprs, ground_truth=lambda e, f: np.zeros((2, 2))))
