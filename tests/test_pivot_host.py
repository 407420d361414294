"""CPU tests of the pivot-frame step: hostutil.find_pivot_frames by hand, against tests/pivot_ref.py and by its two properties,
hostutil.PivotLog, the argument validation of cmpc_mask_pool / cmpc_level_agree (before anything is launched: the library loads without a
GPU, and the fake pointers would fault if anything ran) and the segmenters' describe= plumbing driven through fake device stages."""
import importlib
import math

import numpy as np
import pytest

from tests import pivot_ref as R
from tests import test_clip_segment_host as TC
from tests import test_jf_host as TJ
from tests import test_segment_host as TS

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")


# ---- find_pivot_frames -----------------------------------------------------------------------------------------------------------------
def test_find_pivot_frames_by_hand():
    one = [[3.0, 4.0]]
    assert HU.find_pivot_frames(one) == [0] and HU.find_pivot_frames(one, 0, True) == [0]
    # F <= p: whatever is tried first blocks everything
    d = [[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    # S sums to (1.707, 2.414, 1.707): first = 1; similarities to it (0.707, 1, 0.707): ascending, ties by index -> 0, 2, 1
    assert HU.find_pivot_frames(d, 5) == [0] and HU.find_pivot_frames(d, 5, True) == [1]
    assert HU.find_pivot_frames(d, 1) == [0, 2] and HU.find_pivot_frames(d, 1, True) == [1]
    assert HU.find_pivot_frames(d, 0) == [0, 2, 1] and HU.find_pivot_frames(d, 0, True) == [1, 0, 2]
    # identical rows: every similarity is exactly 1, first = 0 (first occurrence), ties keep the frame order in both directions
    same = [[1.0, 0.0]] * 7
    assert HU.find_pivot_frames(same, 2) == [0, 3, 6] == HU.find_pivot_frames(same, 2, True)
    assert HU.find_pivot_frames(same, 3) == [0, 4] and HU.find_pivot_frames(same, 0) == list(range(7))
    # a zero row stays zero: similarity 0 to everything, itself included -- as written it is the LEAST similar frame and tried first
    z = [[2.0, 0.0], [0.0, 0.0], [5.0, 0.0]]
    assert HU.find_pivot_frames(z, 0) == [1, 0, 2] and HU.find_pivot_frames(z, 0, True) == [0, 2, 1]
    assert HU.find_pivot_frames(z, 1) == [1] and HU.find_pivot_frames(z, 1, True) == [0, 2]
    assert HU.find_pivot_frames(np.zeros((4, 3)), 1) == [0, 2]
    # as written the most dissimilar frame comes first and `first` last: the column sums are (2.96, 3.10, 3.20, 1.35), first = 2, and
    # the similarities to it (0.970, 0.991, 1, 0.243)
    d = [[1.0, 0.0], [0.9, 0.1], [0.8, 0.2], [0.0, 1.0]]
    assert HU.find_pivot_frames(d, 0) == [3, 0, 1, 2] and HU.find_pivot_frames(d, 0, True) == [2, 1, 0, 3]
    assert all(isinstance(f, int) for f in HU.find_pivot_frames(d, 0))
    for bad in (np.zeros(3), np.zeros((0, 4)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            HU.find_pivot_frames(bad)
    with pytest.raises(ValueError):
        HU.find_pivot_frames(d, -1)


def _random_descriptors(rng, F):
    d = rng.uniform(0.0, 1.0, (F, int(rng.integers(1, 9)))) * (rng.uniform(0, 1, (F, 1)) < 0.85)        # non-negative, some zero rows
    if F > 2 and rng.uniform() < 0.3:
        d[int(rng.integers(0, F))] = d[0]                                                                   # and some repeated ones
    return d


def test_find_pivot_frames_against_the_restatement_and_its_properties():
    """2000 random cases, F in 1..39, p in 0..3, zero rows included: the result equals tests/pivot_ref.py's in both orders, no two pivots
    lie within num_propagate of each other and every frame lies within num_propagate of a pivot."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        F, p = int(rng.integers(1, 40)), int(rng.integers(0, 4))
        d = _random_descriptors(rng, F)
        for nearest in (False, True):
            got = HU.find_pivot_frames(d, p, nearest)
            assert got == R.find_pivot_frames(d, p, nearest), (F, p, nearest)
            assert len(set(got)) == len(got) and all(0 <= f < F for f in got)
            s = sorted(got)
            assert all(b - a > p for a, b in zip(s, s[1:])), (F, p, got)
            assert all(min(abs(f - g) for g in got) <= p for f in range(F)), (F, p, got)


def test_consistency_and_pivot_log():
    assert HU.consistency(3, 4) == 0.75 and HU.consistency(0, 5) == 0.0 and math.isnan(HU.consistency(0, 0))
    log = HU.PivotLog()
    rows = {5: [1.0, 0.0], 2: [0.0, 1.0], 9: [1.0, 0.1], 7: [0.9, 0.0]}
    ius = {5: (1, 10), 2: (0, 0), 9: (3, 10), 7: (29, 100)}
    for f in (5, 2, 9, 7):                                         # any order of arrival
        log.add("a", f, np.array(rows[f], np.float32), 2.5 * f, np.array(ius[f], np.int64))
    log.add(("v", 1), 0, [0.0, 0.0, 1.0], 0.0, (0, 3))
    assert len(log) == 5
    d, ids = log.descriptors("a")
    assert ids == [2, 5, 7, 9] and d.dtype == np.float32 and np.array_equal(d, np.array([rows[f] for f in ids], np.float32))
    assert log.areas("a").tolist() == [5.0, 12.5, 17.5, 22.5]
    c = log.consistencies("a")
    assert math.isnan(c[0]) and c[1:].tolist() == [0.1, 0.29, 0.3]
    # pivots are frame ids, not row indices
    assert log.pivots("a", 0) == [ids[i] for i in HU.find_pivot_frames(d, 0)] and set(log.pivots("a", 0)) == {2, 5, 7, 9}
    assert log.pivots("a", 1, nearest_first=True) == [ids[i] for i in HU.find_pivot_frames(d, 1, True)]
    assert log.meta(1) == {"a": log.pivots("a", 1), ("v", 1): [0]}
    # below 0.3, and never a NaN frame
    assert log.inconsistent() == [("a", 5), ("a", 7), (("v", 1), 0)]
    assert log.inconsistent(below=0.05) == [(("v", 1), 0)] and log.inconsistent(below=2.0) == [("a", 5), ("a", 7), ("a", 9), (("v", 1), 0)]
    with pytest.raises(ValueError, match="already holds"):
        log.add("a", 5, rows[5], 1.0, (1, 1))
    with pytest.raises(KeyError):
        log.descriptors("b")
    # the log keeps its own copy of a descriptor (the segmenters hand it views of a pinned slot)
    buf = np.ones(4, np.float32)
    log.add("c", 0, buf, 1.0, (1, 1))
    buf[:] = 7
    assert log.descriptors("c")[0].tolist() == [[1.0, 1.0, 1.0, 1.0]]


# ---- the entry points' argument checks -------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("cmpc_mask_pool", "cmpc_mask_pool_workspace", "cmpc_level_agree"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.cmpc_abi_version() == L.ABI_VERSION == 4            # additive: new symbols, no layout change
    assert L.POOL_MODES == {"soft": 0, "hard": 1} and L.POOL_CHUNK == 64
    assert EV.agree_logit(0.5) == 0.0 and EV.agree_logit(0.2) == float(np.float32(math.log(0.25)))
    for bad in (0.0, 1.0, -1, 2):
        with pytest.raises(ValueError):
            EV.agree_logit(bad)


def test_workspace_size_formula():
    for n, h, w, C in [(1, 1, 1, 8), (8, 40, 40, 1024), (32, 8, 8, 40), (3, 7, 9, 1000), (2, 8, 8, 64), (2, 5, 13, 16)]:
        chunks = -(-h * w // L.POOL_CHUNK)
        assert EV.pool_workspace(n, h, w, C) == n * chunks * (C + 8) * 4
    for bad in [(0, 4, 4, 8), (33, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (1, 4, 4, 12), (1, 2048, 2048, 8)]:
        with pytest.raises(L.CmpcError, match="mask_pool_workspace"):
            EV.pool_workspace(*bad)
    assert L.load().cmpc_mask_pool_workspace(1, 4, 4, 8, None) == -1


def _pool(lib, dt=0, feat=64, stride=None, score=64, sH=16, sW=24, n=2, h=4, w=6, C=16, mode=0, desc=64, area=64, ws=64, ws_bytes=None):
    stride = h * w * C if stride is None else stride
    ws_bytes = (1 << 20) if ws_bytes is None else ws_bytes
    return lib.cmpc_mask_pool(dt, feat, stride, score, sH, sW, n, h, w, C, mode, 0.5, desc, area, ws, ws_bytes, None)


def test_mask_pool_rejects_invalid_arguments_before_launch():
    """Every call passes fake pointers: had a kernel been launched (or a pointer been followed) the process would fault."""
    lib = L.load()

    def bad(word, **kw):
        assert _pool(lib, **kw) == -1, kw
        msg = lib.cmpc_last_error()
        assert b"mask_pool" in msg and word in msg, (kw, msg)
    for p in ("feat", "score", "desc", "area", "ws"):
        bad(b"NULL", **{p: None})
    for n in (0, -1, L.EVAL_MAX_BATCH + 1):
        bad(b"outside", n=n)
    for kw in (dict(h=0), dict(w=0), dict(C=0), dict(h=-3)):
        bad(b"empty", **kw)
    bad(b"positions", h=2048, w=2048, sH=2048, sW=2048)
    for C in (4, 12, 1001):
        bad(b"multiple of 8", C=C)
    for dt in (3, -1):
        bad(b"dtype", dt=dt)
    for mode in (2, -1):
        bad(b"mode", mode=mode)
    for kw in (dict(sH=18), dict(sW=25), dict(sH=2), dict(sW=3), dict(sH=0), dict(sW=-6)):
        bad(b"not a multiple of the tap grid", **kw)
    for stride in (4 * 6 * 16 - 8, 4 * 6 * 16 + 4, -8, 0):
        bad(b"stride", stride=stride)
    need = EV.pool_workspace(2, 4, 6, 16)
    bad(b"workspace", ws_bytes=need - 1)
    bad(b"workspace", ws_bytes=0)
    for kw in (dict(feat=72), dict(ws=72), dict(score=66), dict(desc=66), dict(area=65)):
        bad(b"aligned", **kw)
    # nothing above went further than the checks; a valid set of arguments is not tried here (it would launch)


def test_level_agree_rejects_invalid_arguments_before_launch():
    lib = L.load()

    def call(a=64, b=64, n=2, h=5, w=7, t=0.0, counts=64):
        return lib.cmpc_level_agree(a, b, n, h, w, t, counts, None)
    for kw in (dict(a=None), dict(b=None), dict(counts=None)):
        assert call(**kw) == -1 and b"level_agree" in lib.cmpc_last_error() and b"NULL" in lib.cmpc_last_error()
    for n in (0, -2, L.EVAL_MAX_BATCH + 1):
        assert call(n=n) == -1 and b"outside" in lib.cmpc_last_error()
    for kw in (dict(h=0), dict(w=0), dict(w=-1)):
        assert call(**kw) == -1 and b"empty" in lib.cmpc_last_error()
    assert call(t=float("nan")) == -1 and b"NaN" in lib.cmpc_last_error()
    for kw in (dict(a=66), dict(b=65), dict(counts=68)):
        assert call(**kw) == -1 and b"aligned" in lib.cmpc_last_error()


def test_wrappers_reject_host_arrays_and_bad_options():
    with pytest.raises(ValueError):
        EV.mask_pool(np.zeros((1, 2, 2, 8), np.float32), np.zeros((1, 2, 2), np.float32))
    with pytest.raises(ValueError):
        EV.level_agree(np.zeros((1, 2, 2), np.float32), np.zeros((1, 2, 2), np.float32))
    with pytest.raises(ValueError):
        EV.check_pool_mode("mask")
    model = TS.FakeModel()
    for kw in (dict(describe="c2"), dict(describe="c6"), dict(describe=4), dict(describe_weights="mask"), dict(describe="c4", describe_weights=None)):
        with pytest.raises(ValueError, match="describe"):
            SG.FrameSegmenter(model, _stage=TS.FakeStage(3), **kw)
        with pytest.raises(ValueError, match="describe"):
            SG.ClipSegmenter(TC.FakeModel(), _stage=TC.FakeStage(32, 3, 4), **kw)
    v5 = TS.FakeModel()
    v5.v5 = True
    with pytest.raises(ValueError, match="c2"):
        SG.FrameSegmenter(v5, describe="c3", _stage=TS.FakeStage(3))
    assert SG.FrameSegmenter(v5, describe="c5", _stage=TS.FakeStage(3)).describe == "c5"
    assert SG.check_describe(model, None, "soft") is None and [SG.check_describe(model, k, "hard") for k in ("c3", "c4", "c5")] == [0, 1, 2]


def test_describe_plan_layout():
    for nbytes, scored, n, C in [(0, 0, 1, 8), (1001, 0, 4, 64), (1001, 3, 4, 64), (4096, 4, 4, 1024), (17, 1, 32, 24)]:
        p = SG.plan_describe(nbytes, scored, n, C)
        assert p.off == SG.scored_bytes(nbytes, scored) and p.off % 8 == 0 and p.off >= nbytes + 48 * scored
        assert (p.desc_off, p.area_off, p.end) == (p.off + 16 * n, p.off + 16 * n + 4 * n * C, p.off + 16 * n + 4 * n * C + 4 * n)
        host = np.zeros(p.end + 3, np.uint8)
        cnt, dsc, ar = SG.slot_describe(host, p)
        assert (cnt.shape, cnt.dtype, dsc.shape, dsc.dtype, ar.shape, ar.dtype) == ((n, 2), np.int64, (n, C), np.float32, (n,), np.float32)
        for part in (cnt, dsc, ar):
            part.view(np.uint8)[:] = 255
        assert not host[: p.off].any() and not host[p.end:].any() and host[p.off: p.end].all()       # the three parts tile the tail exactly
    with pytest.raises(ValueError):
        SG.DescribePlan(1, 8, 12)


# ---- the segmenters' plumbing, through fake stages ---------------------------------------------------------------------------------------
C_FAKE = 24


def _fake_values(e, f):
    """What the fake stages 'compute' for (expression e, frame f): counts, descriptor, area."""
    return (f + 1, 2 * f + e + 2), (100 * e + f + np.arange(C_FAKE) / 64).astype(np.float32), np.float32(e + f / 4)


def _fake_describe(buf, plan, row, e, f):
    cnt, dsc, ar = SG.slot_describe(buf, plan)
    cnt[row], dsc[row], ar[row] = _fake_values(e, f)


def _check_log(log, seq, n, E):
    assert len(log) == n * E and sorted(log.seqs) == [(seq, e) for e in range(E)]
    for e in range(E):
        d, ids = log.descriptors((seq, e))
        assert ids == list(range(n))
        for f in range(n):
            iu, want, area = _fake_values(e, f)
            assert np.array_equal(d[f], want) and log.areas((seq, e))[f] == area and log.consistencies((seq, e))[f] == iu[0] / iu[1]


class DescribingFrameStage(TS.FakeStage):
    """FakeStage whose segment() also 'scores' (as tests/test_jf_host.py's) and 'describes' into the plan's place in the slot."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.described = []

    def describe_channels(self):
        return C_FAKE

    def segment(self, token, e, descs, nbytes, slot, jf=None, describe=None):
        super().segment(token, e, descs, nbytes, slot)
        if jf is not None:
            TJ._fake_score(self.bufs[slot], self.bufs[slot], jf)
        assert describe is not None and describe.C == C_FAKE and describe.end <= self.reserved
        assert describe.off == SG.scored_bytes(nbytes, 0 if jf is None else jf.n) and describe.off >= nbytes     # behind masks and J / F counts
        frames = token[: len(descs)]
        assert describe.n == len(frames)                           # one row per real result: the pads of a short batch never
        self.described.append((e, list(frames), jf is not None))
        for i, f in enumerate(frames):
            _fake_describe(self.bufs[slot], describe, i, e, f)


@pytest.mark.parametrize("n,depth,ready", [(7, 2, True), (5, 1, False), (4, 3, True), (1, 2, True)])
@pytest.mark.parametrize("scored", [False, True])
def test_frame_segmenter_describe_plumbing(n, depth, ready, scored):
    B = 4
    frames, exprs = TS._frames(n), TS._exprs()
    st0 = TS.FakeStage(depth + 1, ready=ready, check_reuse=False)
    plain = [(e, f, mk.copy()) for e, f, mk in SG.FrameSegmenter(TS.FakeModel(B=B), depth=depth, _stage=st0).run(frames, exprs)]

    def gt(e, f):
        if f % 2:
            return None
        h, w = frames[f].shape[:2]
        return TJ._gt_for(e, f, (h // 2, w // 2))

    st = DescribingFrameStage(depth + 1, ready=ready)             # check_reuse: no slot is rewritten before its masks were handed out
    seg = SG.FrameSegmenter(TS.FakeModel(B=B), depth=depth, describe="c4", _stage=st)
    assert seg.pivots is None
    got = []
    for e, f, mk in seg.run(iter(frames), exprs, seq="vid", **(dict(ground_truth=gt) if scored else {})):
        assert (("vid", e), f) in [(s, fr) for s in seg.pivots.seqs for fr in seg.pivots.seqs[s]]        # logged before it is yielded
        got.append((e, f, mk.copy()))
        st.consumed.add((e, f))
    assert len(got) == len(plain) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    # one describe per real result, in enqueue order; slots are used exactly as without describing
    assert [(e, fr) for e, fr, _ in st.described] == [(e, sorted(set(b))) for b in SG.plan_batches(n, B) for e in range(3)]
    assert [x for x in st.log if x[0] == "segment"] == [x for x in st0.log if x[0] == "segment"]
    assert all(s == (scored and any(f % 2 == 0 for f in fr)) for _, fr, s in st.described)
    _check_log(seg.pivots, "vid", n, 3)
    if scored:
        want = HU.JFEval()
        for e, f, mk in got:
            if f % 2 == 0:
                want.add(("vid", e), f, TJ.R.counts(mk, TJ._gt_for(e, f, mk.shape), HU.jf_radius(*mk.shape)))
        assert seg.jf.result() == want.result()                    # the J / F counts are where they were
    else:
        assert seg.jf is None
    # a caller's log is used and kept
    mine = HU.PivotLog()
    st.holds, st.consumed = [None] * (depth + 1), set()
    for e, f, _ in seg.run(frames, exprs, seq=2, pivots=mine):
        st.consumed.add((e, f))
    assert seg.pivots is mine
    _check_log(mine, 2, n, 3)


class DescribingClipStage(TC.FakeStage):
    def describe_channels(self):
        return C_FAKE

    def head(self, f, e, descs, slot, describe=None):
        super().head(f, e, descs, slot)
        assert describe is not None and describe.n == self.E and describe.end <= self.reserved
        _fake_describe(self.dev, describe, e, e, f)
        self.log.append(("describe", f, e))

    def finish(self, f, slot, nbytes, jf=None, describe=None):
        super().finish(f, slot, nbytes)
        if jf is not None:
            TJ._fake_score(self.dev, self.bufs[slot], jf)
        assert describe.off == SG.scored_bytes(nbytes, 0 if jf is None else jf.n) and describe.off >= nbytes
        self.bufs[slot][describe.off: describe.end] = self.dev[describe.off: describe.end]


@pytest.mark.parametrize("n,E,depth,ready", [(11, 3, 2, True), (6, 1, 1, False), (23, 2, 3, True)])
@pytest.mark.parametrize("scored", [False, True])
def test_clip_segmenter_describe_plumbing(n, E, depth, ready, scored):
    frames, exprs = list(TC._frames(n)), TC._exprs(E)
    st0 = TC.FakeStage(32, depth + 1, n, ready=ready)
    plain = TJ._drain(st0, SG.ClipSegmenter(TC.FakeModel(), depth=depth, _stage=st0).run(frames, exprs))

    def gt(e, f):
        return None if f % 2 or (e == 1 and f == 4) else TJ._gt_for(e, f, frames[f].shape[:2])

    st = DescribingClipStage(32, depth + 1, n, ready=ready)
    seg = SG.ClipSegmenter(TC.FakeModel(), depth=depth, describe="c5", describe_weights="hard", _stage=st)
    got = TJ._drain(st, seg.run(iter(frames), exprs, seq="v", **(dict(ground_truth=gt) if scored else {})))
    assert len(got) == len(plain) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    assert [x[1:] for x in st.log if x[0] == "describe"] == [(f, e) for f in range(n) for e in range(E)]        # one per (frame, expression)
    keep = ("backbone", "gather", "head", "finish")
    assert [x for x in st.log if x[0] in keep] == [x for x in st0.log if x[0] in keep]                          # the same schedule and slots
    _check_log(seg.pivots, "v", n, E)
    assert seg.stats == {"frames": n, "backbone_passes": -(-n // TC.B), "gathers": n, "heads": n * E}
    if scored:
        want = HU.JFEval()
        for e, f, mk in got:
            if gt(e, f) is not None:
                want.add(("v", e), f, TJ.R.counts(mk, TJ._gt_for(e, f, mk.shape), HU.jf_radius(*mk.shape)))
        assert seg.jf.result() == want.result()
