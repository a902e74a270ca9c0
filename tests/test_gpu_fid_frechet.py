"""Device Frechet distance (eegan_fid_frechet / eegan_fid_dgemm, csrc/fid_sqrt.hip):
the fp64 MFMA GEMM against numpy, MeasureFID.device_frechet_distance against
the golden FIDs of the reference's script and against the host scipy path."""
import os

import numpy as np
import pytest
import torch

from _util import REPO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(REPO, 'tests', 'golden', 'fid.npz')
SHAPES = ((70, 90, 144), (400, 500, 272), (50, 400, 100))   # rank-deficient, full rank, mixed (D not a multiple of 16)


def _stats(N1, N2, D):
    """mu / sigma of fp32 ReLU-like features in which every feature fires in
    some sample, as pool_3 averages do (a feature dead in all samples zeroes a
    row of C1 C2 exactly; scipy's sqrtm then returns NaN and the host path
    moves to its eps branch, 1e-3 away)."""
    rs = np.random.RandomState(5)
    out = []
    for N in (N1, N2):
        a = np.maximum(rs.randn(N, D) * rs.rand(D) + 0.3 * rs.rand(D), 0).astype(np.float32).astype(np.float64)
        out += [a.mean(0), np.cov(a, rowvar=False)]
    return out


@pytest.mark.parametrize('D', [16, 48, 144, 272])
def test_dgemm_vs_numpy(gpu, D):
    """One MFMA block; a ragged wave tile; one 128 tile + remainder; two tiles
    + 16 with several K slabs.  Non-symmetric operands catch a transposed or
    permuted accumulator map; the gate is the dot-product rounding bound."""
    from eegan_hip._lib import ops
    from eegan_hip.tensor import stream
    rs = np.random.RandomState(D)
    A, B = rs.randn(D, D), rs.randn(D, D)
    alpha, beta = -0.5, 1.5
    a, b = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    c = torch.empty_like(a)
    ops.fid_dgemm(a.data_ptr(), b.data_ptr(), D, alpha, beta, c.data_ptr(), stream())
    ref = alpha * (A @ B) + beta * np.eye(D)
    bound = 2 * D * 2.0 ** -53 * (abs(alpha) * (np.abs(A) @ np.abs(B)) + abs(beta) * np.eye(D)) + 1e-300
    err = np.abs(c.cpu().numpy() - ref)
    print('dgemm D=%d max err / bound = %.3g' % (D, (err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('case,tol', [('c0', 1e-9), ('c1', 1e-9), ('sing', 1e-6)])
def test_golden_fid(gpu, case, tol):
    from metrics.FID.fid_score import MeasureFID
    g = np.load(GOLD)
    fid = MeasureFID.device_frechet_distance(*(g['%s/%s' % (case, k)] for k in ('mu1', 'sigma1', 'mu2', 'sigma2')),
                                             device=gpu)
    ref = float(g[case + '/fid'])
    print('golden %s: device %.17g reference %.17g' % (case, fid, ref))
    assert abs(fid - ref) <= tol * abs(ref)


@pytest.mark.parametrize('N1,N2,D', SHAPES)
def test_random_statistics_vs_host_path(gpu, N1, N2, D):
    from metrics.FID.fid_score import MeasureFID
    st = _stats(N1, N2, D)
    host = float(MeasureFID.calculate_frechet_distance(*st))
    out = MeasureFID._device_frechet(*st, device=gpu)
    print('N1=%d N2=%d D=%d: device %.17g host %.17g iterations %d' % (N1, N2, D, out[0], host, out[2]))
    assert abs(out[0] - host) <= 1e-6 * abs(host)
    assert out[2] < 64


def test_identical_statistics(gpu):
    from metrics.FID.fid_score import MeasureFID
    g = np.load(GOLD)
    mu, sigma = g['c1/mu1'], g['c1/sigma1']
    assert abs(MeasureFID.device_frechet_distance(mu, sigma, mu, sigma, device=gpu)) <= 1e-9 * np.trace(sigma)


def test_deterministic(gpu):
    from metrics.FID.fid_score import MeasureFID
    st = _stats(*SHAPES[0])
    a, b = (MeasureFID.device_frechet_distance(*st, device=gpu) for _ in range(2))
    assert a == b


def test_interface(gpu):
    from metrics.FID.fid_score import MeasureFID
    g = np.load(GOLD)
    d1 = MeasureFID.device_statistics(torch.from_numpy(g['c1/act1']).to(gpu), to_host=False)
    d2 = MeasureFID.device_statistics(torch.from_numpy(g['c1/act2']).to(gpu), to_host=False)
    assert all(t.is_cuda and t.dtype == torch.float64 for t in d1 + d2)
    h = [t.cpu().numpy() for t in d1 + d2]
    assert MeasureFID.device_frechet_distance(*d1, *d2) == MeasureFID.device_frechet_distance(*h, device=gpu)
    with pytest.raises(ValueError):
        MeasureFID.device_frechet_distance(h[0], h[1], g['c0/mu2'], g['c0/sigma2'], device=gpu)
