"""`cmpc_dense_crf` (csrc/ops_crf.hip, the exact 4-sigma window) against the windowed float64 reference (tests/crf_exact_ref.py) at the
edges of its window table and tile: a radius beyond the table's first 256 entries, the last slot (511), bilateral and Gaussian windows
smaller than the image, 1 x N / N x 1 / 1 x 1 and one-past-the-32x8-tile shapes, colour distances that drive exp2 to exact zero, and a
unary map that takes the 1e-30 clamp.  The all-tie map runs in tests/test_gpu_crf_lattice_edges.py for both paths.

The reference truncates as the kernel documents, so none of the 2e-4 bar is spent on the 4-sigma tail.  Every comparison asserts
max |Q - ref| < 2e-4, the mask on the reference's sure pixels and sum_l Q = 1 to 1e-5 (tests/crf_edge_cases.py `check`);
tests/test_crf_refs_host.py asserts the radii, the refusal of radius 512 and the 95 % share of sure pixels on the CPU."""
import importlib

import numpy as np
import pytest

from tests import crf_edge_cases as E

CRF = importlib.import_module("cmpc-refseg_amd.crf")

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", E.EXACT_ALL)
def test_exact_edge_case_matches_windowed_reference(name):
    """Measured max |Q - ref| per case: DESIGN.md section 8."""
    import torch
    c = E.exact_case(name)
    q, m = CRF.dense_crf_batch(c.p[None], c.rgb[None], method="exact", want_q=True, **c.kw)
    torch.cuda.synchronize()
    E.check("exact " + name, q[0].cpu().numpy(), m[0].cpu().numpy(), E.exact_ref(name))
    # the two single-sample wrappers give the same bits as the batch wrapper's per-sample call
    assert torch.equal(CRF.dense_crf(c.p, c.rgb, **c.kw), q[0]) and torch.equal(CRF.dense_crf_mask(c.p, c.rgb, **c.kw), m[0])


def test_exact_batch_wrapper_equals_single_calls_with_q():
    import torch
    cases = [E.Case(*E.disc(20 + b, 19, 35), {}) for b in range(3)]
    sig = torch.tensor(np.stack([c.p for c in cases]), device="cuda:0")
    rgb = torch.tensor(np.stack([c.rgb for c in cases]), device="cuda:0")
    assert len({c.rgb.tobytes() for c in cases}) == 3
    q, m = CRF.dense_crf_batch(sig, rgb, method="exact", want_q=True)
    m_only = CRF.dense_crf_batch(sig, rgb, method="exact")
    torch.cuda.synchronize()
    assert q.shape == (3, 2, 19, 35) and torch.equal(m, m_only)
    for b in range(3):
        assert torch.equal(q[b], CRF.dense_crf(sig[b], rgb[b])) and torch.equal(m[b], CRF.dense_crf_mask(sig[b], rgb[b])), b
