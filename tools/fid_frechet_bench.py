"""Device vs host Frechet distance at pool_3 size: MeasureFID.device_frechet_distance
(eegan_fid_frechet) against MeasureFID.calculate_frechet_distance (scipy sqrtm)
on the same statistics of N random ReLU features, in one process.

    python tools/fid_frechet_bench.py [--dims 2048] [--samples 5000] [--repeats 5] [--out FILE]

The device time is event-timed over whole calls (padding, C1 C2, the iteration
with its per-iteration readback, the final combination); the rate counts the
iteration's 3 GEMMs x 2 P^3 x iterations over that span, so it is a whole-call
figure, below the GEMM kernel's own rate.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'ee-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', type=int, default=2048)
    ap.add_argument('--samples', type=int, default=5000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('fid_frechet_bench needs a HIP device')
    from metrics.FID.fid_score import MeasureFID
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    D = a.dims
    st = []
    for _ in range(2):
        act = np.maximum(rs.randn(a.samples, D) * rs.rand(D) + 0.3 * rs.rand(D), 0).astype(np.float32)
        st += MeasureFID.device_statistics(torch.from_numpy(act).to(dev), to_host=False)
    out = MeasureFID._device_frechet(*st)   # warm-up: code objects, workspace
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.repeats + 1)]
    ev[0].record()
    for i in range(a.repeats):
        MeasureFID.device_frechet_distance(*st)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.repeats))
    host_in = [t.cpu().numpy() for t in st]
    t0 = time.perf_counter()
    host = float(MeasureFID.calculate_frechet_distance(*host_in))
    host_s = time.perf_counter() - t0
    P = -(-D // 128) * 128
    med = ms[len(ms) // 2]
    lines = ['D=%d N=%d padded P=%d repeats=%d' % (D, a.samples, P, a.repeats),
             'device_frechet_distance: median %.2f ms (min %.2f, max %.2f), %d iterations, eps pass %d'
             % (med, ms[0], ms[-1], out[2], out[3]),
             'whole-call fp64 rate: %.2f TFLOP/s (3 GEMMs x 2 P^3 x iterations / median)'
             % (3 * 2.0 * P ** 3 * out[2] / (med * 1e-3) / 1e12),
             'calculate_frechet_distance (scipy sqrtm, host): %.2f s' % host_s,
             'fid device %.17g host %.17g rel diff %.3g' % (out[0], host, abs(out[0] - host) / abs(host))]
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
