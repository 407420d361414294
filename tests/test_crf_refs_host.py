"""CPU companions of the DenseCRF edge tests (tests/test_gpu_crf_lattice_edges.py, tests/test_gpu_crf_exact_edges.py).  They pin the
windowed float64 reference of the exact path (tests/crf_exact_ref.py) to the oracle, pin the loop-free vertex numbering of the lattice
restatement to its dict version, and assert -- on the references alone -- the structural premise of every GPU case, so that a case cannot
silently stop exercising what it is for: key magnitudes next to the packing limits, the host bound's conservativeness, more than 256
scan chunks with a leader in the last one, the vertex-count extremes, the window radii, and at least 95 % sure pixels everywhere."""
import numpy as np
import pytest

from oracle import dense_crf_numpy as OC
from tests import crf_edge_cases as E
from tests import crf_exact_ref as X
from tests import crf_lattice_ref as R


# ---- the windowed reference of the exact path ----------------------------------------------------------------------------------------

def test_windowed_reference_without_window_is_the_oracle():
    for H, W, kw in ((20, 24, {}), (13, 37, dict(sxy_g=2.0, compat_g=1.5, sxy_b=9.0, srgb=6.0, compat_b=4.0, iters=3)), (9, 9, dict(iters=0))):
        p, rgb = E.disc(3, H, W)
        assert np.abs(X.dense_crf(p, rgb, window=False, **kw) - OC.dense_crf(p, rgb, **kw)).max() <= 1e-12


def test_windowed_reference_is_the_oracle_when_both_windows_cover_the_image():
    H, W = 20, 24
    kw = dict(sxy_g=6.0, sxy_b=20.0)                              # ceil(4 * 6) = 24 and ceil(4 * 20) = 80, both >= W - 1 = 23
    assert X.window_radius(H, W, kw["sxy_g"]) == X.window_radius(H, W, kw["sxy_b"]) == W - 1
    assert X.window_mask(H, W, W - 1).all()
    p, rgb = E.disc(4, H, W)
    assert np.abs(X.dense_crf(p, rgb, **kw) - OC.dense_crf(p, rgb, **kw)).max() <= 1e-12


def test_window_mask_and_radius():
    m = X.window_mask(3, 5, 1).reshape(3, 5, 3, 5)
    assert m[1, 2].sum() == 9 and m[0, 0].sum() == 4 and m[2, 4, 1, 3] and not m[2, 4, 0, 2] and not m[1, 0, 1, 2]
    assert np.array_equal(m.reshape(15, 15), m.reshape(15, 15).T)
    assert X.window_radius(320, 320, 3.0) == 12 and X.window_radius(320, 320, 20.0) == 80 and X.window_radius(37, 13, 20.0) == 36
    assert X.window_radius(600, 600, 127.75) == 511 and X.window_radius(600, 600, np.nextafter(np.float32(127.75), np.float32(200))) == 512


def test_windowed_reference_differs_from_the_oracle_only_by_the_truncated_tail():
    # What the exact kernel leaves out beyond 4 sigma.  Measured: at most 7.4e-6 under the default weights (2 x 512) and 3.5e-5 at
    # 40 x 45 with sxy_g 1 / sxy_b 4 and weak weights.  (The ~soft variants of the other shapes are left out to keep this test short.)
    names = [n for n in E.EXACT_ALL if E.truncated(n) and (not n.endswith("~soft") or n.startswith("window_"))]
    assert {"window_12x100", "window_40x45", "shape_33x65"} <= set(names)
    worst = {}
    for n in names:
        worst[n] = float(np.abs(E.exact_ref(n) - E.exact_oracle(n)).max())
        print("windowed vs dense oracle %-16s %.3e" % (n, worst[n]))
        assert worst[n] < 1e-4, (n, worst[n])
    assert min(worst[n] for n in ("table_512", "window_12x100", "window_40x45", "shape_33x65")) > 0      # the mask is really applied


def test_exact_case_premises(pkg):
    assert E.radii("table_300") == (12, 299)                      # the table's second trip of 256 entries
    w = np.exp(-0.5 * (np.arange(256, 300) / 120.0) ** 2)         # entries 256..299: 0.103 down to 0.045, far above the 2e-4 bar's reach
    assert w[0] >= 0.10 and w.min() >= 0.04
    assert E.radii("table_512") == (12, X.MAX_RADIUS) and E.exact_case("table_512").p.shape == (2, 512)      # the last slot
    assert X.window_radius(2, 514, 128.0) == X.MAX_RADIUS + 1
    lib = pkg._lib.load()
    fake = 256                                                    # never dereferenced: the call is refused before any launch
    assert lib.cmpc_dense_crf(fake, fake, 2, 514, 3.0, 3.0, 128.0, 3.0, 10.0, 5, fake, fake, None) == -1
    assert b"radius 512" in lib.cmpc_last_error()
    assert E.radii("window_12x100") == (12, 80) and E.radii("window_40x45") == (4, 16)                         # both inside the image
    for n, (H, W) in (("shape_1x1", (1, 1)), ("shape_1x29", (1, 29)), ("shape_31x1", (31, 1)), ("shape_33x65", (33, 65))):
        assert E.exact_case(n).p.shape == (H, W)
    assert 33 == 4 * 8 + 1 and 65 == 2 * 32 + 1                   # one row and one column past the kernel's 32 x 8 tile
    bits = E.exact_case("bits")
    assert set(np.unique(bits.rgb)) == {0, 255} and 0.5 / E.f32(0.57) ** 2 * 255 ** 2 * 1.4426950408889634 > 150   # exp2 underflows to 0


@pytest.mark.parametrize("name", E.EXACT_ALL)
def test_exact_cases_keep_95_percent_sure_pixels(name):
    assert E.sure_share(E.exact_ref(name)) >= E.SURE_SHARE, (name, E.sure_share(E.exact_ref(name)))


# ---- the lattice restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["key_bilateral", "key_gauss_1e-4", "uniform_rgb", "const255", "shape_18x19", "shape_1x1", "shape_2x1", "saturated",
                                  "small_3"])
def test_loop_free_numbering_equals_the_dict_numbering(name):
    c = E.lattice_case(name)
    kw = {k: v for k, v in c.kw.items() if k in ("sxy_g", "sxy_b", "srgb")}
    for a, b in zip(R.lattices(c.p.shape, c.rgb, **kw), R.lattices(c.p.shape, c.rgb, fast=True, **kw)):
        assert a.M == b.M and np.array_equal(a.off, b.off) and np.array_equal(a.nb, b.nb) and np.array_equal(a.w, b.w)


@pytest.mark.parametrize("name", E.LATTICE_ALL)
def test_lattice_cases_keep_95_percent_sure_pixels(name):
    assert E.sure_share(E.lattice_ref(name)) >= E.SURE_SHARE, (name, E.sure_share(E.lattice_ref(name)))


def _max_key(name, d):
    c = E.lattice_case(name)
    H, W = c.p.shape
    f = R.features(H, W, c.rgb, c.kw.get("sxy_b", 20.0), c.kw.get("srgb", 3.0)) if d == 5 else R.features(H, W, None, c.kw.get("sxy_g", 3.0))
    return int(np.abs(R.embed(f)[0]).max())


def test_key_range_premises():
    c = E.lattice_case("key_bilateral")
    assert c.p.shape == (12, 13) and set(np.unique(c.rgb)) == {0, 255}
    assert tuple(c.rgb[0, 0]) == (0, 0, 0) and tuple(c.rgb[-1, -1]) == (255, 255, 255)
    px = {tuple(v) for v in c.rgb.reshape(-1, 3)}
    assert (0, 0, 255) in px and (255, 0, 0) in px
    bound = E.bilateral_bound(12, 13, c.kw["sxy_b"], c.kw["srgb"])
    top = _max_key("key_bilateral", 5)
    print("bilateral key bound %.1f, largest |key| %d" % (bound, top))
    assert bound <= E.KEY_MAX[5] and 1900 <= top <= bound         # measured: 2015.7 and 1963
    for name, least in (("key_gauss_1e-3", 3e4), ("key_gauss_1e-4", 3e5)):
        g = E.lattice_case(name)
        top = _max_key(name, 2)
        print("%s largest |key| %d" % (name, top))
        assert least <= top <= E.gaussian_bound(12, 13, g.kw["sxy_g"]) <= E.KEY_MAX[2]


def test_host_key_bound_is_conservative():
    # Accepted parameters must never reach the device's out-of-range path: the real keys stay within the restated host bound.
    rng = np.random.default_rng(7)
    closest = 0.0
    for _ in range(200):
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        sxy, srgb = E.f32(rng.uniform(0.5, 30)), E.f32(np.exp(rng.uniform(np.log(0.57), np.log(30))))
        rgb = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        mid = rng.random((H, W, 3)) < 0.1
        rgb[mid] = rng.integers(0, 256, int(mid.sum()), dtype=np.uint8)
        kb = int(np.abs(R.embed(R.features(H, W, rgb, sxy, srgb))[0]).max())
        kg = int(np.abs(R.embed(R.features(H, W, None, sxy))[0]).max())
        bb, bg = E.bilateral_bound(H, W, sxy, srgb), E.gaussian_bound(H, W, sxy)
        assert kb <= bb and kg <= bg, (H, W, sxy, srgb, kb, bb, kg, bg)
        closest = max(closest, kb / bb)
    print("largest |key| / bound over the sweep: %.4f" % closest)


def test_bilateral_rejection_boundary_without_a_gpu(pkg):
    s = E.smallest_accepted_srgb()
    assert E.bilateral_bound(12, 13, 20.0, s) <= E.KEY_MAX[5] < E.bilateral_bound(12, 13, 20.0, 0.999 * s)
    assert E.bilateral_bound(12, 13, 20.0, 1.01 * s) <= E.KEY_MAX[5] < E.bilateral_bound(12, 13, 20.0, 0.99 * s)
    assert 0.55 < s < E.f32(0.57)                                 # the key-range case sits just inside
    lib = pkg._lib.load()
    fake = 256                                                    # never dereferenced: only the refused call is made here
    assert lib.cmpc_dense_crf_lattice(fake, fake, 1, 12, 13, 3.0, 3.0, 20.0, 0.99 * s, 10.0, 5, fake, fake, None) == -1
    assert b"12-bit" in lib.cmpc_last_error()


def test_vertex_count_premises():
    E5 = E.VH * E.VW * 6
    assert E.lattice_pair("uniform_rgb")[1].M >= 0.99 * E5        # measured: 4029 of 4032
    assert E.lattice_pair("const0")[1].M <= 64 and E.lattice_pair("const255")[1].M <= 64        # measured: 23 and 25
    assert E.lattice_case("const255").kw["srgb"] == E.f32(0.9) and (E.lattice_case("const255").rgb == 255).all()
    # the batch: one srgb for the three samples, and vertex counts two orders of magnitude apart within one call
    ms = [E.lattice_pair(n)[1].M for n in E.V_BATCH]
    assert len({E.lattice_case(n).kw["srgb"] for n in E.V_BATCH}) == 1 and ms[0] >= 0.99 * E5 and max(ms[1:]) <= 64, ms


@pytest.mark.parametrize("name,term", [("scan_d5", 1), ("scan_d2", 0)])
def test_scan_carry_premises(name, term):
    lat = E.lattice_pair(name)[term]
    entries = lat.N * (lat.d + 1)
    assert (entries, lat.d) == {"scan_d5": (263340, 5), "scan_d2": (262848, 2)}[name]
    assert -(-entries // E.CHUNK) > 256                           # the scan of the chunk counts takes its carry loop a second time
    first = np.unique(lat.off.reshape(-1), return_index=True)[1]  # first-appearance entry of every vertex: the device's "leader"
    late = int((first // E.CHUNK >= 256).sum())
    print("%s: M = %d, %d chunks, %d vertices led from chunk >= 256" % (name, lat.M, -(-entries // E.CHUNK), late))
    assert late >= 1 and E.lattice_case(name).kw["iters"] == 2
def test_boundary_shape_premises():
    ent = {n: (E.lattice_case(n).p.size * 3, E.lattice_case(n).p.size * 6) for n in E.SHAPES}
    assert ent["shape_11x31"][0] == 1023 and ent["shape_18x19"][0] == 1026 and ent["shape_10x17"][1] == 1020 and ent["shape_9x19"][1] == 1026
    assert [E.lattice_case(n).p.shape for n in E.SHAPES[4:]] == [(1, 1), (1, 2), (2, 1)]
    small = [E.lattice_case("small_%d" % b) for b in range(E.SMALL_B)]
    assert E.SMALL_B == 40 and all(c.p.shape == (5, 7) for c in small) and 5 * 7 * 6 < 256        # smaller than one block
    assert len({c.rgb.tobytes() for c in small}) == E.SMALL_B and len({c.p.tobytes() for c in small}) == E.SMALL_B


def test_unary_extreme_premises():
    for c, ref in ((E.lattice_case("saturated"), E.lattice_ref("saturated")), (E.exact_case("saturated"), E.exact_ref("saturated"))):
        assert c.p.shape == (9, 11) and set(np.unique(c.rgb)) == {0, 255}
        # float32 keeps 0, 1, 0.5 and 1e-8; 1 - 1e-8 rounds to 1: both of them take the 1e-30 clamp, on either side
        assert set(np.unique(c.p)) == {np.float32(0), np.float32(1e-8), np.float32(0.5), np.float32(1)}
        assert np.isfinite(ref).all() and 0 < ref.min() < 1e-30   # measured: 1.3e-33 for the lattice
    for it in (0, 5):
        c = E.all_tie(6, 7, it)
        for q in (R.dense_crf(c.p.astype(np.float64), c.rgb, **c.kw), X.dense_crf(c.p.astype(np.float64), c.rgb, **c.kw)):
            assert np.abs(q - 0.5).max() < 1e-12                  # no sure pixel by construction: the GPU tests assert the whole mask
