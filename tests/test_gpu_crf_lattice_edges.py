"""`cmpc_dense_crf_lattice` (csrc/ops_crf_lattice.hip) against the float64 restatement (tests/crf_lattice_ref.py) where the lattice can be
wrong without the feature's own tests noticing: keys next to the 12-bit and far into the 31-bit packing range, the second level of the
leader scan, nearly-all-distinct and nearly-all-shared vertices (alone and in one batch), entry counts around the 1024-entry chunk,
samples smaller than a block, a grid of 40 samples, and unary maps that hit the 1e-30 clamp or tie everywhere.

Every comparison asserts max |Q - ref| < 2e-4, the mask on the reference's sure pixels (|Q1 - Q0| > 1e-3) and sum_l Q = 1 to 1e-5
(tests/crf_edge_cases.py `check`).  tests/test_crf_refs_host.py asserts each case's premise on the CPU, and that at least 95 % of its
pixels are sure.  All parameters used here are accepted by the host bound: no test goes to the device's error path."""
import importlib

import numpy as np
import pytest

from tests import crf_edge_cases as E

CRF = importlib.import_module("cmpc-refseg_amd.crf")

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_sticky_device_error():
    """The lattice's device error word makes the NEXT call fail.  Spend that next call here, after every test, and blame the test that
    just ran: one broken case cannot cascade into unrelated tests."""
    yield
    import torch
    torch.cuda.synchronize()
    try:
        CRF.dense_crf_mask(np.full((2, 2), 0.5, np.float32), np.zeros((2, 2, 3), np.uint8), method="lattice", iters=0)
        torch.cuda.synchronize()
    except CRF._lib.CmpcError as e:
        pytest.fail("this test left the lattice's device error word set: %s" % e)


def _run(cases):
    """One batched call over cases of one size and one parameter set -> (Q [B, 2, H, W], masks [B, H, W]) as numpy."""
    import torch
    assert all(c.kw == cases[0].kw for c in cases)
    q, m = CRF.dense_crf_batch(np.stack([c.p for c in cases]), np.stack([c.rgb for c in cases]), method="lattice", want_q=True, **cases[0].kw)
    torch.cuda.synchronize()
    return q.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("name", E.LATTICE_SINGLE)
def test_lattice_edge_case_matches_restatement(name):
    """Measured max |Q - ref| per case: DESIGN.md section 13c."""
    q, m = _run([E.lattice_case(name)])
    E.check("lattice " + name, q[0], m[0], E.lattice_ref(name))


def test_lattice_accepts_srgb_just_inside_the_12_bit_bound():
    s = 1.01 * E.smallest_accepted_srgb()                         # the refusal 1 % below the boundary is asserted without a GPU
    c = E.lattice_case("key_bilateral")
    q, m = _run([E.Case(c.p, c.rgb, E.params(sxy_b=20.0, srgb=s))])
    assert np.isfinite(q).all() and m.max() <= 1


def test_lattice_batch_of_very_different_vertex_counts():
    """Uniform-random RGB (M = E), black and white (M ~ 25) in one call: the blur and links kernels bound their work by M[b]."""
    import torch
    cases = [E.lattice_case(n) for n in E.V_BATCH]
    q, m = _run(cases)
    for b, n in enumerate(E.V_BATCH):
        E.check("lattice batch3 " + n, q[b], m[b], E.lattice_ref(n))
        q1, m1 = _run([cases[b]])
        assert np.array_equal(q1[0], q[b]) and np.array_equal(m1[0], m[b]), n
    # the same through torch.equal on the device tensors, as the feature's own batch test compares
    sig = torch.tensor(np.stack([c.p for c in cases]), device="cuda:0")
    rgb = torch.tensor(np.stack([c.rgb for c in cases]), device="cuda:0")
    qb, mb = CRF.dense_crf_batch(sig, rgb, method="lattice", want_q=True, **cases[0].kw)
    for b in range(3):
        qs, ms = CRF.dense_crf_batch(sig[b: b + 1], rgb[b: b + 1], method="lattice", want_q=True, **cases[0].kw)
        assert torch.equal(qs[0], qb[b]) and torch.equal(ms[0], mb[b]), b


def test_lattice_batch_of_40_samples_smaller_than_a_block():
    names = ["small_%d" % b for b in range(E.SMALL_B)]
    q, m = _run([E.lattice_case(n) for n in names])
    worst = max(E.check("lattice batch40 " + n, q[b], m[b], E.lattice_ref(n)) for b, n in enumerate(names))
    print("crf-edge lattice batch40: worst of %d samples %.3e" % (E.SMALL_B, worst))


@pytest.mark.parametrize("iters", [0, 5])
@pytest.mark.parametrize("method", ["lattice", "exact"])
def test_all_tie_map_gives_label_0_and_equal_channels(method, iters):
    """p = 0.5 on a constant image: both labels run identical operations, so Q0 == Q1 bit for bit, and label 0 wins the tie everywhere.
    No pixel is sure here by construction, so the whole mask is asserted."""
    import torch
    c = E.all_tie(6, 7, iters)
    q, m = CRF.dense_crf_batch(c.p[None], c.rgb[None], method=method, want_q=True, **c.kw)
    torch.cuda.synchronize()
    q, m = q.cpu().numpy()[0], m.cpu().numpy()[0]
    assert np.array_equal(q[0], q[1]) and np.abs(q - 0.5).max() < 1e-6
    assert m.shape == (6, 7) and not m.any()
