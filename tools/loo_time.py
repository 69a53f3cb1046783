"""time of the fused leave-one-out launch against what a user can compose without it:  python tools/loo_time.py [out] [--windows K]

Four shapes: fp32 20 480 problems of n = 64, f = 4 (BASELINE config #3's GP batch); fp32 5 120 problems of n = 128, f = 4 (config #4's);
fp64 2 560 problems of n = 128; and the reference launchers' regime, 20 problems of n = 20 (fp32).  Per shape:
  fused     L.gp_loo: one launch, nothing n x n leaves the CU
  composed  L.gp_lml_fwd(..., want_alpha=True, want_L=True), torch.cholesky_inverse(L).diagonal(), and the elementwise tail for
            mu_loo / var_loo / lpd -- the route without pacoh_gp_loo: it writes B n^2 factor entries to HBM and reads them back
Both produce the same three outputs; their largest difference is printed next to the times (the composed route in the same dtype).
Times are HIP events around `reps` back-to-back calls after a warm-up of the same calls, repeated over K windows that ALTERNATE the two
routes; reported: the median window and the min .. max spread, per call.  reps is chosen per shape so that a window of the faster route runs ~0.25 s.
Call times: they include the ctypes / torch dispatch of each call (several us: the n = 20 row is mostly that).
The table is written to `out` (default profiles/loo_time.txt)."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from meta_learning_pacoh_amd import _lib as L                         # noqa: E402

SHAPES = [  # name, dtype, tasks, P, n, f
    ('cfg3 fp32', torch.float32, 1024, 20, 64, 4),
    ('cfg4 fp32', torch.float32, 256, 20, 128, 4),
    ('fp64 n128', torch.float64, 128, 20, 128, 4),
    ('launcher', torch.float32, 2, 10, 20, 2),
]


def inputs(dtype, T, P, n, f):
    g = torch.Generator().manual_seed(T * n + f)
    z = (torch.randn(T * P, n, f, generator=g, dtype=torch.float64) * (1.5 / math.sqrt(f))).to(dtype).cuda()
    mean = (0.3 * torch.randn(T * P, n, generator=g, dtype=torch.float64)).to(dtype).cuda()
    y = torch.randn(T, n, generator=g, dtype=torch.float64).to(dtype).cuda()
    ls = (0.8 + 0.4 * torch.rand(P, f, generator=g, dtype=torch.float64)).to(dtype).cuda()
    os_ = (0.5 + torch.rand(P, generator=g, dtype=torch.float64)).to(dtype).cuda()
    noise = (0.05 + 0.1 * torch.rand(P, generator=g, dtype=torch.float64)).to(dtype).cuda()
    return z, mean, y, ls, os_, noise


def window(run, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3                              # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'loo_time.txt'))
    ap.add_argument('--windows', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loo_time.py needs a HIP device: nothing is measured without one')
    L.load_library()
    lines = ['# leave-one-out: the fused launch (L.gp_loo) against gp_lml_fwd(want_alpha, want_L) + torch.cholesky_inverse + elementwise tail.',
             '# python tools/loo_time.py: HIP-event call times in us (dispatch included), median of %d alternating windows [min .. max]; '
             'B = problems.' % a.windows,
             '%-10s %6s %4s %3s %5s | %28s | %28s | %6s | %9s' % ('shape', 'B', 'n', 'f', 'reps', 'fused us', 'composed us', 'ratio', 'max diff')]
    for name, dtype, T, P, n, f in SHAPES:
        z, mean, y, ls, os_, noise = inputs(dtype, T, P, n, f)
        B = T * P
        yb = y.repeat_interleave(P, 0)

        def fused():
            return L.gp_loo(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, B, P)

        def composed():
            _, alpha, Lf, _ = L.gp_lml_fwd(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, B, P, want_alpha=True, want_L=True)
            d = torch.cholesky_inverse(Lf).diagonal(dim1=-2, dim2=-1)
            e = alpha / d
            lpd = (-0.5 * (math.log(2 * math.pi) - torch.log(d) + alpha * e)).mean(1)
            return yb - e, 1.0 / d, lpd

        a1, a2 = fused(), composed()
        torch.cuda.synchronize()
        assert int(a1[3].abs().max()) == 0
        diff = max(float((a1[k] - a2[k]).abs().max()) for k in range(3))
        window(fused, 3), window(composed, 3)                         # warm-up of both routes (code objects, allocator)
        t0 = min(window(fused, 3), window(composed, 3))               # ... then the size of a window
        reps = max(5, min(5000, int(0.25e6 / max(t0, 1.0))))
        window(fused, reps), window(composed, reps)
        tf, tc = [], []
        for _ in range(a.windows):
            tf.append(window(fused, reps))
            tc.append(window(composed, reps))
        mf, mc = statistics.median(tf), statistics.median(tc)
        lines.append('%-10s %6d %4d %3d %5d | %9.1f [%7.1f .. %7.1f] | %9.1f [%7.1f .. %7.1f] | %6.2f | %9.1e'
                     % (name, B, n, f, reps, mf, min(tf), max(tf), mc, min(tc), max(tc), mf / mc, diff))
        print(lines[-1])
        sys.stdout.flush()
    lines.append('# ratio = fused / composed (below 1: the fused launch is faster)')
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:3]))


if __name__ == '__main__':
    main()
