"""CPU tests of the picture renderers: hand-worked answers of the NumPy restatement (tests/vis_ref.py), the colour tables of
visualize.py, and the export, workspace size and argument validation of cmpc_vis_overlay / cmpc_vis_heat / cmpc_vis_words (before
anything is launched: the library loads without a GPU, and the fake pointers would fault if anything ran)."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import vis_ref as R

L = importlib.import_module("cmpc-refseg_amd._lib")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
V = importlib.import_module("cmpc-refseg_amd.visualize")


# ---- the restatement, by hand --------------------------------------------------------------------------------------------------------
def test_overlays_by_hand():
    im = np.array([[[255, 254, 1], [0, 3, 200]], [[155, 10, 11], [156, 7, 9]]], np.uint8)
    mask = np.array([[1, 0], [255, 0]], np.uint8)
    # 255 / 2 + 100 = 227.5 -> 227; 155 / 2 + 100 = 177.5 -> 177; unmasked pixels are im >> 1
    assert R.overlay_pred(im, mask).tolist() == [[[227, 127, 0], [0, 1, 100]], [[177, 5, 5], [78, 3, 4]]]
    assert R.overlay_gt(mask).tolist() == [[[170, 0, 0], [0, 0, 170]], [[170, 0, 0], [0, 0, 170]]]
    grey = np.array([[9, 200, 255]], np.uint8)                              # 1 x 3, tiled to three channels
    assert R.overlay_pred(grey, np.array([[0, 2, 1]])).tolist() == [[[4, 4, 4], [200, 100, 100], [227, 127, 127]]]
    assert R.overlay_gt(np.array([[0, 2, 1]])).tolist() == [[[0, 0, 170], [170, 0, 0], [170, 0, 0]]]
    rng = np.random.default_rng(0)
    im, mask = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 2, (5, 7), dtype=np.uint8)
    want = im >> 1
    want[..., 0] += 100 * mask
    assert np.array_equal(R.overlay_pred(im, mask), want)                   # the shift form of ops_vis.hip, on every byte value
    assert R.overlay_pred(im, mask).dtype == np.uint8 and R.overlay_gt(mask).dtype == np.uint8


def test_index_rule_edges():
    v = np.array([0.0, 1.0, 0.5, 0.49999, -3.0, 7.0, 1.0 / 256, np.nextafter(1.0 / 256, 0)])
    assert R.index_of(v, 0.0, 1.0).tolist() == [0, 255, 128, 127, 0, 255, 1, 0]          # v == hi -> 255 (clipped 256), outside clips
    assert R.index_of(np.array([2.0, 2.0]), 2.0, 2.0).tolist() == [0, 0]                 # hi == lo -> 0
    assert R.index_of(np.array([-1.0, 0.0, 1.0]), -1.0, 1.0).tolist() == [0, 128, 255]
    idx, (lo, hi) = R.heat(np.array([[1.0, 3.0], [2.0, 5.0]], np.float32), 2, 2, vrange=None)   # identity size: the map itself
    assert (lo, hi) == (1.0, 5.0) and idx.tolist() == [[0, 128], [64, 255]]
    idx, rng_ = R.heat(np.full((3, 3), 0.25, np.float32), 3, 3, vrange=None)
    assert rng_ == (0.25, 0.25) and not idx.any()
    s = R.sigmoid32(np.array([0.0, 100.0, 1.0]))
    assert s.dtype == np.float32 and s[0] == 0.5 and s[1] == 1.0 and s[2] == np.float32(1) / (np.float32(1) + np.exp(np.float32(-1)))
    assert R.heat(np.zeros((2, 2), np.float32), 2, 2, sigmoid=True)[0].tolist() == [[128, 128], [128, 128]]


def test_word_sheet_by_hand():
    lut = V.gray_lut()
    # N = 1 x 2, ld = 3: panel 0 = (0, 1) -> indices (0, 255); panel 1 constant -> (0, 0); panel 2 not drawn (n_words = 2)
    g = np.array([[0.0, 5.0, 9.0], [1.0, 5.0, 8.0]], np.float32)
    sh = R.word_sheet(g, 2, (1, 2), 3, 1, 2, 1, lut)                        # zoom 1, cols 2, gap 1: 2 rows x 2 panels, 3 x 5 pixels
    W = 255
    assert sh[..., 0].tolist() == [[0, 255, W, 0, 0], [W, W, W, W, W], [W, W, W, W, W]] and np.array_equal(sh[..., 0], sh[..., 2])
    assert R.sheet_size(1, 2, 3, 1, 2, 1) == (3, 5) == V.sheet_size((1, 2), 3, 1, 2, 1)
    sh = R.word_sheet(g, 3, (1, 2), 3, 2, 1, 0, lut)                        # zoom 2, one column, no gap: 3 rows of 2 x 4 pixels
    assert sh.shape == (6, 4, 3) and sh[..., 1].tolist() == [[0, 0, W, W]] * 2 + [[0, 0, 0, 0]] * 2 + [[W, W, 0, 0]] * 2
    assert R.word_sheet(g, 0, (1, 2), 1, 4, 5, 2, lut).shape == (4, 8 * 5 + 2 * 4, 3)
    assert V.sheet_size((40, 40), 20) == (4 * 160 + 3 * 2, 5 * 160 + 4 * 2)


def test_colour_tables():
    jet, gray = V.jet_lut(), V.gray_lut()
    assert jet.shape == gray.shape == (256, 3) and jet.dtype == gray.dtype == np.uint8
    assert tuple(jet[0]) == (0, 0, 127) and tuple(jet[255]) == (127, 0, 0)
    assert jet[127][1] == 255 and jet[100][1] == 255                         # the green plateau
    assert gray[:, 0].tolist() == list(range(256)) and np.array_equal(gray[:, 0], gray[:, 1]) and np.array_equal(gray[:, 0], gray[:, 2])


def test_jet_table_equals_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    want = mpl.colormaps["jet"](np.arange(256), bytes=True)[:, :3]
    assert np.array_equal(V.jet_lut(), want)


# ---- the C entries: exported, bound, sized and validated without a GPU ----------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("cmpc_vis_overlay", "cmpc_vis_heat", "cmpc_vis_heat_workspace", "cmpc_vis_words"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.cmpc_abi_version() == L.ABI_VERSION == 4            # additive: new symbols only
    assert (L.VIS_PRED, L.VIS_GT, L.VIS_SIGMOID, L.VIS_AUTO) == (0, 1, 1, 2)


def _descs(items):
    """items: (offset, h, w, c) or (offset, h, w, c, rh, rw, top, left)."""
    return (L.EvalDesc * len(items))(*[L.EvalDesc(*(tuple(it) + (0,) * (9 - len(it)))) for it in items])


def _crop(off, H, W, h, w):
    return (off, h, w, 1) + tuple(HU.resize_and_crop_geometry(H, W, h, w))


def _fails(lib, rc, who, word):
    msg = lib.cmpc_last_error()
    assert rc == -1 and who in msg and word in msg, (rc, msg, word)


def test_overlay_rejects_invalid_arguments_before_launch():
    lib = L.load()
    fr = [(0, 4, 6, 3), (80, 5, 3, 1)]                             # 72 and 15 bytes
    mk = [(0, 4, 6, 1), (32, 5, 3, 1)]                             # 24 and 15 bytes
    ou = [(0, 4, 6, 3), (80, 5, 3, 3)]                             # 72 and 45 bytes

    def call(kind=L.VIS_PRED, frames=8, fb=95, fd=fr, masks=8, mb=47, md=mk, B=None, out=8, ob=125, od=ou):
        return lib.cmpc_vis_overlay(kind, frames, fb, _descs(fd) if fd is not None else None, masks, mb, _descs(md) if md is not None else None,
                                    len(md) if B is None and md is not None else (B or 0), out, ob, _descs(od) if od is not None else None, None)

    def bad(word, **kw):
        _fails(lib, call(**kw), b"vis_overlay", word)

    for k in ("frames", "fd", "masks", "md", "out", "od"):
        bad(b"NULL", **({k: None, "B": 2} if k == "md" else {k: None}))
    bad(b"NULL", kind=L.VIS_GT, masks=None)
    for B in (0, -1, L.EVAL_MAX_BATCH + 1):
        bad(b"outside 1..32", B=B, fd=fr * 17, md=mk * 17, od=ou * 17)
    for kind in (2, -1, 7):
        bad(b"kind", kind=kind)
    bad(b"sample 1: frame 5 x 4, mask 5 x 3", fd=[fr[0], (80, 5, 4, 1)])
    bad(b"sample 0: output 4 x 5, mask 4 x 6", od=[(0, 4, 5, 3), ou[1]])
    bad(b"sample 1: output", kind=L.VIS_GT, frames=None, fd=None, od=[ou[0], (80, 3, 5, 3)])
    bad(b"sample 0: empty", md=[(0, 0, 6, 1), mk[1]], fd=[(0, 0, 6, 3), fr[1]], od=[(0, 0, 6, 3), ou[1]])
    bad(b"sample 1: 2 channels", fd=[fr[0], (80, 5, 3, 2)])
    bad(b"sample 1: frame at offset", fb=94)
    bad(b"sample 1: mask at offset", mb=46)
    bad(b"sample 1: output at offset", ob=124)
    bad(b"sample 0: mask at offset", md=[(-16, 4, 6, 1), mk[1]])
    bad(b"sample 0: frame at offset", fd=[(30, 4, 6, 3), fr[1]])
    with pytest.raises(L.CmpcError, match="vis_overlay"):
        L.call("cmpc_vis_overlay", 5, 8, 10, _descs(fr), 8, 10, _descs(mk), 2, 8, 10, _descs(ou), None)
    with pytest.raises(ValueError, match="kind"):
        V.overlays([], [], kind="both")


def test_heat_workspace_and_invalid_arguments_before_launch():
    lib = L.load()
    out = ctypes.c_int64(-1)
    for B in (1, 5, 32):
        for flags, per in ((0, 0), (L.VIS_SIGMOID, 0), (L.VIS_AUTO, 16), (L.VIS_AUTO | L.VIS_SIGMOID, 16)):
            assert lib.cmpc_vis_heat_workspace(B, flags, ctypes.byref(out)) == 0 and out.value == per * B == V.heat_workspace(B, flags)
    _fails(lib, lib.cmpc_vis_heat_workspace(0, 0, ctypes.byref(out)), b"vis_heat_workspace", b"outside")
    _fails(lib, lib.cmpc_vis_heat_workspace(33, 0, ctypes.byref(out)), b"vis_heat_workspace", b"outside")
    _fails(lib, lib.cmpc_vis_heat_workspace(2, 4, ctypes.byref(out)), b"vis_heat_workspace", b"flags")
    _fails(lib, lib.cmpc_vis_heat_workspace(2, 0, None), b"vis_heat_workspace", b"NULL")

    H, W = 32, 32
    good = [_crop(0, H, W, 48, 64), _crop(48 * 64, H, W, 16, 12)]
    rgbd = [(0, 48, 64, 3), (48 * 64 * 3, 16, 12, 3)]
    ib, rb = 48 * 64 + 16 * 12, 3 * (48 * 64 + 16 * 12)

    def call(map_=8, B=None, H=H, W=W, d=good, flags=0, vmin=0.0, vmax=1.0, lut=8, idx=8, ib=ib, rgb=8, rb=rb, rd=rgbd, rng=8, ws=8, wb=32):
        return lib.cmpc_vis_heat(map_, len(d) if B is None and d is not None else (B or 0), H, W, _descs(d) if d is not None else None, flags,
                                 vmin, vmax, lut, idx, ib, rgb, rb, _descs(rd) if rd is not None else None, rng, ws, wb, None)

    def bad(word, **kw):
        _fails(lib, call(**kw), b"vis_heat", word)

    bad(b"NULL", map_=None)
    bad(b"NULL", d=None, B=2)
    bad(b"NULL", idx=None, rgb=None)
    bad(b"NULL", rd=None)
    for B in (0, -1, L.EVAL_MAX_BATCH + 1):
        bad(b"outside 1..32", B=B, d=good * 17, rd=rgbd * 17)
    bad(b"map size", H=0)
    bad(b"flags", flags=4)
    for vmin, vmax in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0)):
        bad(b"vmin", vmin=vmin, vmax=vmax)
    bad(b"LUT", lut=None)
    bad(b"sample 1: empty", d=[good[0], (0, 0, 5, 1, 1, 1, 0, 0)])
    bad(b"sample 0: geometry", d=[(0, 48, 64, 1, 64, 64, 8, 1), good[1]])
    bad(b"sample 1: shrink factor too large (Gaussian radius > 63)", H=640, W=640, d=[_crop(0, 640, 640, 48, 64), _crop(48 * 64, 640, 640, 16, 19)])
    bad(b"sample 1: index plane at offset", ib=ib - 1)
    bad(b"sample 1: RGB plane at offset", rb=rb - 1)
    bad(b"sample 0: RGB plane 48 x 63", rd=[(0, 48, 63, 3), rgbd[1]])
    bad(b"workspace", flags=L.VIS_AUTO, wb=31)
    bad(b"workspace", flags=L.VIS_AUTO, ws=None)
    bad(b"aligned", flags=L.VIS_AUTO, ws=12)
    bad(b"aligned", rng=4)
    # what AUTO refuses passes the checks without it up to the launch-free end: vmin >= vmax is not looked at with AUTO, a missing LUT
    # not without an RGB plane -- shown by the NEXT check failing instead
    bad(b"workspace", flags=L.VIS_AUTO, vmin=1.0, vmax=0.0, wb=0)
    bad(b"workspace", flags=L.VIS_AUTO, lut=None, rgb=None, rd=None, wb=0)
    with pytest.raises(L.CmpcError, match="vis_heat"):
        L.call("cmpc_vis_heat", 8, 1, 4, 4, _descs([_crop(0, 4, 4, 4, 4)]), 0, 1.0, 0.0, 8, 8, 16, None, 0, None, None, None, 0, None)
    # a radius of exactly 63 passes the radius check (and fails the next one)
    geo = _crop(0, 1300, 1300, 40, 40)
    assert int(4 * ((1300 / 40 - 1) / 2) + 0.5) == 63
    bad(b"index plane at offset", H=1300, W=1300, d=[geo], rd=[(0, 40, 40, 3)], ib=10)


def test_words_rejects_invalid_arguments_before_launch():
    lib = L.load()

    def call(gw=8, B=3, gh=4, gwd=5, ld=8, nw=(0, 3, 8), mw=8, zoom=3, cols=5, gap=2, lut=8, out=8, ob=None):
        sh, sw = V.sheet_size((gh, gwd), max(mw, 1), max(zoom, 1), max(cols, 1), max(gap, 0))
        n = (ctypes.c_int * len(nw))(*nw) if nw is not None else None
        return lib.cmpc_vis_words(gw, B, gh, gwd, ld, n, mw, zoom, cols, gap, lut, out, B * sh * sw * 3 if ob is None else ob, None)

    def bad(word, **kw):
        _fails(lib, call(**kw), b"vis_words", word)

    for k in ("gw", "nw", "lut", "out"):
        bad(b"NULL", **{k: None})
    for B in (0, -1, L.EVAL_MAX_BATCH + 1):
        bad(b"outside 1..32", B=B, nw=(1,) * 40)
    bad(b"grid", gh=0)
    bad(b"grid", ld=0)
    for mw in (0, 33):
        bad(b"max_words", mw=mw)
    bad(b"zoom", zoom=0)
    bad(b"zoom", cols=0)
    bad(b"zoom", gap=-1)
    bad(b"sample 2: n_words = 9", nw=(0, 3, 9), mw=16)                     # n_words > ld
    bad(b"sample 1: n_words = 4", nw=(0, 4, 3), mw=3)                      # n_words > max_words
    bad(b"sample 0: n_words = -1", nw=(-1, 3, 8))
    sh, sw = V.sheet_size((4, 5), 8, 3, 5, 2)
    bad(b"beyond the buffer", ob=3 * sh * sw * 3 - 1)
    bad(b"too large", zoom=1 << 14)
    with pytest.raises(L.CmpcError, match="vis_words"):
        L.call("cmpc_vis_words", 8, 1, 2, 2, 4, (ctypes.c_int * 1)(5), 8, 1, 1, 0, 8, 8, 1 << 20, None)
