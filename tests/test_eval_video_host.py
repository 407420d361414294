"""CPU tests of the video evaluation layer: hostutil.first_valid_idx against the driver's loop (trainval_video.py:191-197), the shared
front-padded -> end-padded helper, and VideoEvaluator.add()'s validation of a sample, which raises before anything touches a device."""
import importlib

import numpy as np
import pytest
import torch

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
MD = importlib.import_module("cmpc-refseg_amd.model")


def _driver_valid_idx(text):
    # trainval_video.py:191-197, verbatim in effect
    valid_idx = np.zeros([1], dtype=np.int32)
    for idx in range(text.shape[0]):
        if text[idx] != 0:
            valid_idx[0] = idx
            break
    return int(valid_idx[0])


def test_first_valid_idx_matches_driver_loop():
    rng = np.random.default_rng(0)
    T = 20
    rows = [np.zeros(T, np.int64), np.arange(1, T + 1), np.array([0] * (T - 1) + [7])]
    for _ in range(200):
        L = int(rng.integers(0, T + 1))
        r = np.zeros(T, np.int64)
        r[T - L:] = rng.integers(1, 100, L)
        rows.append(r)
    for r in rows:
        assert HU.first_valid_idx(r) == _driver_valid_idx(r)
        assert HU.first_valid_idx(r.astype(np.int32)) == _driver_valid_idx(r)
    assert HU.first_valid_idx(np.zeros(T, np.int32)) == 0          # all pad: the driver leaves 0
    with pytest.raises(ValueError):
        HU.first_valid_idx(np.zeros((2, T), np.int32))
    with pytest.raises(ValueError):
        HU.first_valid_idx(np.zeros(T, np.float32))


def test_video_words():
    T = 6
    we, sl = MD.video_words(np.array([[0, 0, 0, 5, 7, 9]]), np.array([[3]]), T)
    assert we.dtype == np.int32 and sl.dtype == np.int32
    assert we.tolist() == [[5, 7, 9, 0, 0, 0]] and sl.tolist() == [3]
    we, sl = MD.video_words(np.arange(1, 7), 0, T)
    assert we.tolist() == [[1, 2, 3, 4, 5, 6]] and sl.tolist() == [6]
    for words, vi in (([0, 0, 0, 5, 7, 9], 2), ([0, 0, 0, 5, 0, 9], 3), ([0] * 6, 0), ([0] * 6, 6)):
        with pytest.raises(ValueError):
            MD.video_words(np.array(words), vi, T)


class _Stub:
    """What VideoEvaluator reads of a model before it launches anything."""
    video, num_steps, H, W, frames, device, bb_stream = True, 6, 64, 64, 16, torch.device("cpu"), None


def _sample(rng, h=48, w=80, frames=16, L=3, T=6):
    text = np.zeros(T, np.int64)
    text[T - L:] = rng.integers(1, 50, L)
    clip = rng.integers(0, 256, (frames, h, w, 3), dtype=np.uint8)
    mask = np.zeros((h, w), bool)
    mask[h // 4: h // 2, w // 4: w // 2] = True
    return text, clip[8].copy(), clip, mask


def test_video_sample_checks():
    rng = np.random.default_rng(1)
    text, im, clip, mask = _sample(rng)
    we, sl, fr, key, m = EV.check_video_sample(0, text, im, clip, mask, 6, 16)
    assert we.tolist() == [[int(x) for x in text[3:]] + [0, 0, 0]] and sl.tolist() == [3]
    assert len(fr) == 5 and all(np.array_equal(f, clip[k]) for f, k in zip(fr, MD.FRAME_IDX))
    assert np.array_equal(key, im) and m.dtype == np.uint8 and np.array_equal(m, mask.astype(np.uint8))
    # a list of frames is accepted as well as one array
    assert all(np.array_equal(a, b) for a, b in zip(EV.check_video_sample(0, text, im, list(clip), mask, 6, 16)[2], fr))


def test_video_evaluator_add_rejects_invalid_samples():
    rng = np.random.default_rng(2)
    ev = EV.VideoEvaluator(_Stub())
    text, im, clip, mask = _sample(rng)
    ragged = list(clip)
    ragged[5] = np.zeros((40, 80, 3), np.uint8)
    interior = text.copy()
    interior[4] = 0
    cases = {
        "frames differ in size": (text, im, ragged, mask),
        "too few frames": (text, im, clip[:15], mask),
        "too many frames": (text, im, np.concatenate([clip, clip[:1]]), mask),
        "float frames": (text, im, clip.astype(np.float32), mask),
        "float key image": (text, im.astype(np.float32), clip, mask),
        "mask size": (text, im, clip, mask[:-1]),
        "all-pad sentence": (np.zeros(6, np.int64), im, clip, mask),
        "pad inside the sentence": (interior, im, clip, mask),
        "empty mask": (text, im, clip, np.zeros_like(mask)),
        "ids of the wrong length": (text[1:], im, clip, mask),
        "gray frames": (text, im, clip[..., 0], mask),
    }
    for name, args in cases.items():
        with pytest.raises(ValueError, match="sample 0"):
            ev.add(*args)
        assert ev.n == 0, name
    assert ev.n == 0


def test_video_evaluator_rejects_image_models():
    class Image(_Stub):
        video = False
    with pytest.raises(ValueError, match="video model"):
        EV.VideoEvaluator(Image())
    assert EV.VideoEvaluator(_Stub()).thresholds == (.5, .55, .6, .65, .7, .75, .8, .85, .9, .95)
