"""time of joint predictive draws (fp32):  python tools/sample_time.py [reps]

Three shapes users run: MAP / single task (1 component, m = 1000 candidates, S = 1024 draws), PACOH-SVGD (P = 10 particles,
m = 128, S = 4096), PACOH-VI Bayes (P = 100 posterior samples, m = 200, S = 1000).  Per shape: pacoh_mvn_factor, pacoh_mvn_sample and
a whole GaussianPredictive.sample() call (fresh object: factor + draws + grouping) against torch.linalg.cholesky + torch.matmul on
the same covariances (torch only here, as the yardstick: the product path has no torch fallback).  The transform's share of the fp32
MFMA peak counts the lower-triangle work only, 2 S m (m + 1) / 2 flops.

These are HIP-event times of back-to-back calls: they include the ctypes / torch dispatch of each call.  For kernel times, run one
shape and one part at a time under rocprofv3 --kernel-trace --stats, e.g.
    python tools/sample_time.py 20 --shape svgd --part transform      (pacoh_mvn_sample vs torch.matmul only)
    python tools/sample_time.py 20 --shape vi --part factor           (pacoh_mvn_factor vs torch.linalg.cholesky only)
and divide each kernel's total by the number of calls (reps + 3 warm-up)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meta_learning_pacoh_amd import _lib as L                         # noqa: E402
from meta_learning_pacoh_amd.distributions import GaussianPredictive  # noqa: E402

SHAPES = [('map', 1, 1000, 1024), ('svgd', 10, 128, 4096), ('vi', 100, 200, 1000)]     # (name, P, m, S)
PEAK_F32_TFLOPS = 157.3                                                # MI355X fp32 matrix peak (spec)


def timed(run, reps):
    for _ in range(3):
        run()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3                              # us


def covariances(P, m):
    g = torch.Generator().manual_seed(P * m)
    x = torch.rand(P, m, 1, generator=g) * 6 - 3
    K = torch.exp(-0.5 * (x - x.transpose(1, 2)) ** 2 / 0.5 ** 2) + 0.05 * torch.eye(m)
    return K.cuda()


def setup(P, m, S):
    cov = covariances(P, m)
    mu = torch.randn(P, m, device='cuda')
    eps = torch.randn(S, m, device='cuda')
    comp = torch.randint(P, (S,), device='cuda')
    order = torch.sort(comp, stable=True).indices.to(torch.int32)
    offsets = torch.zeros(P + 1, dtype=torch.int32, device='cuda')
    offsets[1:] = torch.cumsum(torch.bincount(comp, minlength=P), 0)
    o, off = (order, offsets) if P > 1 else (None, None)
    Lf, info = L.mvn_factor(cov)
    assert int((info < 0).sum()) == 0
    # torch yardstick of the transform: one (batched) matmul of each component's draws with the dense L^T -- mixtures as one
    # [P, max draws per component, m] x [P, m, m] product
    Lt = Lf.tril()
    n_max = int(torch.bincount(comp, minlength=P).max())
    eg = torch.zeros(P, n_max, m, device='cuda')
    if P > 1:
        mm = lambda: torch.matmul(eg, Lt.transpose(1, 2))          # noqa: E731
    else:
        mm = lambda: torch.matmul(eps, Lt[0].T)                    # noqa: E731
    return cov, mu, eps, o, off, Lf, info, mm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reps', nargs='?', type=int, default=20)
    ap.add_argument('--shape', choices=[s[0] for s in SHAPES], default=None, help='one shape only (default: all three)')
    ap.add_argument('--part', choices=['all', 'transform', 'factor'], default='all',
                    help='transform: pacoh_mvn_sample and torch.matmul only; factor: pacoh_mvn_factor and torch.linalg.cholesky only')
    a = ap.parse_args()
    reps = a.reps
    shapes = [s for s in SHAPES if a.shape in (None, s[0])]
    if a.part != 'all':
        for name, P, m, S in shapes:
            cov, mu, eps, o, off, Lf, info, mm = setup(P, m, S)
            torch.cuda.synchronize()
            if a.part == 'transform':
                t_ours = timed(lambda: L.mvn_sample(Lf, info, mu, eps, 0.1, 2.0, o, off), reps)
                t_torch = timed(mm, reps)
            else:
                t_ours = timed(lambda: L.mvn_factor(cov), reps)
                t_torch = timed(lambda: torch.linalg.cholesky(cov), reps)
            print('%-5s %s: ours %.1f us, torch %.1f us per call (HIP events; %d calls each incl. 3 warm-up)'
                  % (name, a.part, t_ours, t_torch, reps + 3))
        return
    print('%-5s %4s %5s %5s | %10s %10s %10s | %10s %10s %10s | %8s' % ('shape', 'P', 'm', 'S', 'factor us', 'sample us', 'sample() us',
                                                                         'torch chol', 'torch mm', 'torch sum', 'MFMA %'))
    for name, P, m, S in shapes:
        cov, mu, eps, o, off, Lf, info, mm = setup(P, m, S)
        t_factor = timed(lambda: L.mvn_factor(cov), reps)
        t_sample = timed(lambda: L.mvn_sample(Lf, info, mu, eps, 0.1, 2.0, o, off), reps)

        def whole():
            GaussianPredictive(mu, torch.ones_like(mu), cov, 0.1, 2.0, mixture=P > 1).sample((S,))
        t_whole = timed(whole, reps)
        t_chol = timed(lambda: torch.linalg.cholesky(cov), reps)
        t_mm = timed(mm, reps)
        flops = 2.0 * S * m * (m + 1) / 2
        share = flops / (t_sample * 1e-6) / (PEAK_F32_TFLOPS * 1e12) * 100
        print('%-5s %4d %5d %5d | %10.1f %10.1f %10.1f | %10.1f %10.1f %10.1f | %8.1f' % (name, P, m, S, t_factor, t_sample, t_whole, t_chol, t_mm,
                                                                                     t_chol + t_mm, share))
    print('(HIP-event call times, dispatch included; MFMA % over call time -- kernel times: --shape / --part under rocprofv3)')


if __name__ == '__main__':
    main()
