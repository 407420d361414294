"""The dense float64 reference of tests/resample_ref.py against hostutil's restatement on scipy.ndimage, over every case that
tests/test_gpu_resample_edges.py runs on the device: the GPU tests may assert only what the reference satisfies here.  Resampled values
agree to 1e-9 grey levels (a bound on float64 rounding, below), every host byte lies within half a level of the dense value, and every
binary decision (pad order 1 and order 0, crop) is identical.  The coverage guards check, through the restated tile selection, that
the case lists reach the LDS tile shapes they are there for.  Run with -s to see the per-case figures."""
import importlib

import numpy as np
import pytest

from tests import resample_ref as R

HU = importlib.import_module("cmpc-refseg_amd.hostutil")

# at most (2 * 63 + 1)^2 * 4 ~ 6.5e4 float64 operations per value, each off by at most 2^-53 * 255 grey levels: ~2e-9 if every rounding
# error pointed the same way.  A bound, not a measurement: the measured worst case is printed (about 1.4e-13).
MARGIN = 1e-9


@pytest.mark.parametrize("out", R.OUTS)
def test_values_and_bytes(out):
    worst = 0.0
    for h, w, c in R.prep_cases(out):
        im = R.image(h, w, c)
        host, dense = HU.resize_and_pad(im, *out), R.dense_pad(im, *out)
        assert host.shape == dense.shape
        dv = float(np.abs(255.0 * host - 255.0 * dense).max())
        db = float(np.abs(HU.img_as_ubyte(host).astype(np.float64) - 255.0 * dense).max())
        print("out %s source %s: host against dense %.3g levels, host bytes against dense %.6f" % (out, (h, w, c), dv, db))
        assert dv <= MARGIN, (out, (h, w, c), dv)
        assert db <= 0.5 + MARGIN, (out, (h, w, c), db)
        worst = max(worst, dv)
    print("out %s: worst host-against-dense discrepancy %.3g grey levels" % (out, worst))


def test_identity_is_the_source():
    im = R.image(23, 41, 3)
    assert np.array_equal(R.dense_pad(im, 23, 41) * 255.0, im.astype(np.float64))


@pytest.mark.parametrize("out", R.OUTS)
def test_target_decisions_equal(out):
    """resize_and_pad(mask) > 0 (order 1) and resize_and_pad_order0 against the dense reference, with no allowance; every mask's
    reference target is neither empty nor full over its resized rectangle (but for the listed exceptions)."""
    cases = R.target_cases(out)
    assert {"%dx%d" % s for s in R.sources(out)} <= {name.split()[0] for _, name, _ in cases}       # no source lost all its kinds
    for m, name, ref in cases:
        rh, rw, _, _ = HU.resize_and_pad_geometry(m.shape[0], m.shape[1], *out)
        n = int(ref.sum())
        if name.endswith("empty"):
            assert n == 0
        elif m.size > 4:
            assert 0 < n < rh * rw, (out, name, n, rh * rw)
        else:
            assert 0 < n <= rh * rw
        assert np.array_equal(HU.resize_and_pad(m, *out) > 0, ref), (out, name, "order 1")
        assert np.array_equal(HU.resize_and_pad_order0(m, *out), R.nearest_pad(m, *out)), (out, name, "order 0")
    # the order-0 targets are not all trivial either
    n0 = [int(R.nearest_pad(m, *out).sum()) for m, _, _ in cases]
    assert sum(0 < n < out[0] * out[1] for n in n0) > len(cases) // 3


# (map, size) whose outputs can only be all alike: radius 6 on 8 pixels (every output pixel sees the whole map); one column cut out of
# a one-row map
SATURATED = {((8, 8), (2, 2)), ((1, 5), (9, 1))}


@pytest.mark.parametrize("shape", R.MAPS)
def test_crop_decisions_equal(shape):
    groups = {}
    for kind, size, ref in R.crop_cases(shape):
        rh, rw, _, _ = HU.resize_and_crop_geometry(shape[0], shape[1], *size)
        assert max(R.radii(shape[0], shape[1], rh, rw)[2:]) <= R.MAXR
        m = R.binary_map(shape[0], shape[1], kind)
        for dt in (np.float32, np.uint8, bool):
            assert np.array_equal(HU.resize_and_crop(m.astype(dt), *size) > 0, ref), (shape, kind, size, dt)
        groups.setdefault(size, []).append(ref)
    for size, refs in groups.items():
        assert any(r.any() for r in refs) and any(not r.all() for r in refs), (shape, size)
        if size != (1, 1) and (shape, size) not in SATURATED:
            assert any(r.any() and not r.all() for r in refs), (shape, size)


# ---- coverage guards: the restated tile selection says the case lists reach what they are there for ----------------------------------
def test_prep_cases_reach_every_tile_shape():
    """The colour sources at (23, 41) reach all eight tile shapes of eval_prep_kernel, each by the source the case table names."""
    table = {}
    for h, w, c in R.prep_cases((23, 41)):
        t = R.tile_choice("prep", [(h, w, c or 1)], 23, 41)
        assert isinstance(t, tuple), ((h, w, c), t)
        table.setdefault((3 if c == 3 else 1, t), []).append((h, w))
    for (c, t), srcs in sorted(table.items(), key=lambda kv: (-kv[0][0], R.SHAPES.index(kv[0][1]))):
        print("eval_prep, %d channel(s), tile %s: %s" % (c, t, srcs))
    assert {t for c, t in table if c == 3} == set(R.SHAPES)
    for src, t in (((46, 82), (8, 32)), ((96, 96), (4, 32)), ((128, 128), (2, 32)), ((160, 160), (1, 32)), ((256, 256), (1, 16)),
                   ((320, 320), (1, 8)), ((40, 700), (1, 4)), ((50, 900), (1, 1))):
        assert src in table[(3, t)]
    assert R.BIG in table[(1, (1, 8))]
    # the neighbours of the tile-invariance test force what it says they force, whatever rides beside them
    assert R.tile_choice("prep", [(50, 900, 3), (1, 1, 3), (320, 320, 3)], 23, 41) == (1, 1)
    assert R.tile_choice("prep", [(96, 96, 3), (1, 1, 3), (46, 82, 3)], 23, 41) == (4, 32)
    assert R.tile_choice("target", [R.BIG + (1,), (5, 3, 1)], 23, 41) == (1, 4)
    assert R.tile_choice("target", [(50, 900, 1), (5, 3, 1)], 23, 41) == (1, 8)


def _scan(out):
    """Every tile shape plan_target can pick for one plain mask at output `out` with both radii within MAXR: a scan over source sizes."""
    sides = list(range(1, 64)) + list(range(64, 1500, 12))
    reach = {}
    for h in sides:
        for w in sides:
            t = R.tile_choice("target", [(h, w, 1)], out[0], out[1])
            if isinstance(t, tuple):
                reach.setdefault(t, (h, w))
    return reach


def test_target_cases_reach_every_reachable_tile_shape():
    """train_target_kernel's footprint is a quarter of a byte per pixel, so {1, 1} is out of reach under MAXR; the order-1 cases at
    (23, 41) reach all seven shapes that are not, and over all outputs and both orders nothing reachable is left out."""
    reach_all, have_all = set(), set()
    for out in R.OUTS:
        reach = _scan(out)
        have = {order: {R.tile_choice("target", [m.shape + (1,)], out[0], out[1], order) for m, _, _ in R.target_cases(out)} for order in (1, 0)}
        print("train_target at %s: reachable %s; order-1 cases %s; order-0 cases %s"
              % (out, sorted(reach, key=R.SHAPES.index), sorted(have[1], key=R.SHAPES.index), sorted(have[0], key=R.SHAPES.index)))
        assert all(isinstance(t, tuple) for t in have[1] | have[0])
        reach_all |= set(reach)
        have_all |= have[1] | have[0]
        if out == (23, 41):
            assert have[1] == set(reach) == set(R.SHAPES) - {(1, 1)}
    assert have_all == reach_all


def test_refusals_are_refusals():
    for src, why in R.REFUSALS:
        assert R.tile_choice("prep", [src], 23, 41) == why, src
    # the colour source is refused by its LDS footprint although its radii (61, 60) are within MAXR; the same source in grey fits
    rh, rw, _, _ = HU.resize_and_pad_geometry(720, 1280, 23, 41)
    assert R.radii(720, 1280, rh, rw)[2:] == (61, 60)
    assert R.tile_choice("prep", [(720, 1280, 1)], 23, 41) == (1, 8)
    # a refusal anywhere in the batch refuses the batch
    assert R.tile_choice("prep", [(5, 3, 3), (700, 40, 3)], 23, 41) == "radius"
    # the largest radius a square colour source gets through the LDS check with, at this output
    ok = [s for s in range(23, 1500) if isinstance(R.tile_choice("prep", [(s, s, 3)], 23, 41), tuple)]
    rmax = R.radii(ok[-1], ok[-1], 23, 23)[2]
    print("largest square colour source that fits at (23, 41): %d (radius %d)" % (ok[-1], rmax))
    assert 50 <= rmax < R.MAXR
