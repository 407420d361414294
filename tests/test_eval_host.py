"""CPU tests of the evaluation layer (cmpc-refseg_amd/evaluate.py): hostutil.img_as_ubyte / end_padded, the packing planner, and
argument validation of cmpc_eval_prep / cmpc_eval_mask_iu before anything is launched (the library loads without a GPU)."""
import ctypes
import importlib

import numpy as np
import pytest

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
L = importlib.import_module("cmpc-refseg_amd._lib")

SIZES = [(480, 640), (333, 500), (240, 427), (100, 50), (320, 320), (50, 900)]


def test_img_as_ubyte_rounds_half_to_even_and_clips():
    x = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, -0.2, 0.0, 1.0, 254.5 / 255], dtype=np.float64)
    assert HU.img_as_ubyte(x).tolist() == [0, 2, 2, 0, 0, 255, 254]
    k = np.arange(256)
    assert np.array_equal(HU.img_as_ubyte(k / 255.0), k.astype(np.uint8))
    assert HU.img_as_ubyte(np.float32([0.2])).dtype == np.uint8
    with pytest.raises(ValueError):
        HU.img_as_ubyte(np.array([1.5]))
    with pytest.raises(ValueError):
        HU.img_as_ubyte(np.array([3], dtype=np.uint8))


def test_end_padded():
    T = 6
    rows = np.array([[0, 0, 0, 5, 7, 9], [1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 8]])
    ids, sl = HU.end_padded(rows)
    assert ids.dtype == np.int32 and sl.dtype == np.int32
    assert ids.tolist() == [[5, 7, 9, 0, 0, 0], [1, 2, 3, 4, 5, 6], [8, 0, 0, 0, 0, 0]]
    assert sl.tolist() == [3, T, 1]
    i1, s1 = HU.end_padded(rows[0])
    assert i1.tolist() == [5, 7, 9, 0, 0, 0] and int(s1) == 3
    # a pad id INSIDE the sentence is a word position, not padding
    i2, s2 = HU.end_padded(np.array([0, 4, 0, 6]))
    assert i2.tolist() == [4, 0, 6, 0] and int(s2) == 3
    vocab = {"<pad>": 0, "<unk>": 1, "a": 2, "dog": 3}
    front = HU.preprocess_sentence("a dog", vocab, T)
    assert tuple(x.tolist() if hasattr(x, "tolist") else x for x in HU.end_padded(np.array(front))) == \
        (HU.preprocess_sentence_lstm("a dog", vocab, T)[0], 2)
    with pytest.raises(ValueError):
        HU.end_padded(np.zeros((2, T), dtype=np.int64))
    with pytest.raises(ValueError):
        HU.end_padded(np.zeros((2, 2, 2), dtype=np.int64))


@pytest.mark.parametrize("HW", [320, 512])
def test_planner_matches_geometry(HW):
    shapes = [s + (3,) for s in SIZES] + [(240, 427)]
    d, nbytes = EV.plan_prep(shapes, HW, HW)
    off = 0
    for di, s in zip(d, shapes):
        c = s[2] if len(s) == 3 else 1
        assert (di.h, di.w, di.c) == (s[0], s[1], c)
        assert (di.rh, di.rw, di.top, di.left) == HU.resize_and_pad_geometry(s[0], s[1], HW, HW)
        assert di.offset == off and di.offset % 16 == 0
        off += -(-s[0] * s[1] * c // 16) * 16
    assert nbytes == off
    m, mbytes = EV.plan_masks(SIZES, HW, HW)
    for di, s in zip(m, SIZES):
        assert (di.rh, di.rw, di.top, di.left) == HU.resize_and_crop_geometry(HW, HW, s[0], s[1])
        assert di.offset % 16 == 0 and di.offset + s[0] * s[1] <= mbytes


def test_bad_inputs_raise_before_launch():
    with pytest.raises(ValueError):
        EV._images_u8([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError):
        EV._images_u8([np.zeros((4,), np.uint8)])
    with pytest.raises(ValueError):
        EV._images_u8([np.zeros((4, 4, 2), np.uint8)])
    with pytest.raises(ValueError):
        EV._images_u8([np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        EV._masks_u8([np.zeros((4,), np.uint8)])
    with pytest.raises(ValueError):
        EV.plan_prep([(4, 4, 3)] * (L.EVAL_MAX_BATCH + 1), 32, 32)
    with pytest.raises(ValueError):
        EV.plan_masks([], 32, 32)
    with pytest.raises(ValueError):
        EV.mask_iu(np.zeros((1, 4, 4), np.float32), [np.ones((4, 4))])


def _descs(shapes, HW, pad):
    return (EV.plan_prep if pad else EV.plan_masks)(shapes, HW, HW)


def _prep(lib, d, nbytes, B=None, H=32, src=1, proc=1, feed=1):
    return lib.cmpc_eval_prep(src, nbytes, d, len(d) if B is None else B, H, H, proc, feed, None)


def _mask(lib, d, nbytes, B=None, dt=0, H=32, m=1, gt=1, iu=1):
    return lib.cmpc_eval_mask_iu(m, dt, len(d) if B is None else B, H, H, 1e-9, gt, nbytes, d, iu, None, None)


def test_c_entry_points_reject_invalid_arguments():
    lib = L.load()
    d, n = _descs([(40, 30, 3), (20, 20, 1)], 32, True)
    # NULL pointers
    assert _prep(lib, d, n, src=None) == -1 and b"eval_prep" in lib.cmpc_last_error()
    assert _prep(lib, d, n, proc=None) == -1 and _prep(lib, d, n, feed=None) == -1
    assert lib.cmpc_eval_prep(1, n, None, 2, 32, 32, 1, 1, None) == -1
    # B <= 0, B above the per-launch maximum
    assert _prep(lib, d, n, B=0) == -1 and _prep(lib, d, n, B=-3) == -1
    big = (L.EvalDesc * (L.EVAL_MAX_BATCH + 1))(*([d[0]] * (L.EVAL_MAX_BATCH + 1)))
    assert _prep(lib, big, n) == -1 and b"outside" in lib.cmpc_last_error()
    # zero-sized / 1-D image, channels other than 1 or 3, wrong geometry, offset + size beyond the buffer
    for field, val in (("h", 0), ("w", 0), ("c", 2), ("c", 4), ("rh", d[0].rh + 1), ("top", d[0].top + 1), ("left", 5)):
        e = (L.EvalDesc * 2)(d[0], d[1])
        setattr(e[0], field, val)
        assert _prep(lib, e, n) == -1, field
    e = (L.EvalDesc * 2)(d[0], d[1])
    e[1].offset = n - 10
    assert _prep(lib, e, n) == -1 and b"beyond" in lib.cmpc_last_error()
    assert _prep(lib, d, n - 1) == -1
    # eval_mask_iu: the same checks, plus the map dtype and single-channel masks
    m, mn = _descs([(40, 30), (16, 50)], 32, False)
    assert _mask(lib, m, mn, m=None) == -1 and b"eval_mask_iu" in lib.cmpc_last_error()
    assert _mask(lib, m, mn, gt=None) == -1 and _mask(lib, m, mn, iu=None) == -1
    assert lib.cmpc_eval_mask_iu(1, 0, 2, 32, 32, 1e-9, 1, mn, None, 1, None, None) == -1
    assert _mask(lib, m, mn, dt=2) == -1 and b"dtype" in lib.cmpc_last_error()
    assert _mask(lib, m, mn, B=0) == -1 and _mask(lib, m, mn, B=L.EVAL_MAX_BATCH + 1) == -1
    for field, val in (("h", 0), ("c", 3), ("rw", m[0].rw - 1), ("left", m[0].left + 1)):
        e = (L.EvalDesc * 2)(m[0], m[1])
        setattr(e[0], field, val)
        assert _mask(lib, e, mn) == -1, field
    assert _mask(lib, m, mn - 1) == -1 and b"beyond" in lib.cmpc_last_error()
