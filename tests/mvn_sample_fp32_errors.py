"""Measure the fp32 error of the joint predictive draws (pacoh_mvn_factor + pacoh_mvn_sample) against the fp64 restatement, next to
plain torch fp32 (cholesky + matmul) on the same problems: the table behind FLOOR32 of test_gpu_mvn_sample.py.

    python tests/mvn_sample_fp32_errors.py [out.txt]

Per (m, B): the worst component error |y - y_ref| / (y_std sqrt(Sigma_ii)) over S in {1, 15, 16, 17, 1000}, of HIP and of torch, and
the worst ratio HIP / torch.  Needs a HIP device."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvn_sample_ref as R                                         # noqa: E402
import test_gpu_mvn_sample as T                                    # noqa: E402
from meta_learning_pacoh_amd import _lib as L                      # noqa: E402


def main():
    lines = ['%5s %3s | %10s %10s %8s | %s' % ('m', 'B', 'hip max', 'torch max', 'ratio', 'rungs')]
    worst_hip, worst_ratio = 0.0, 0.0
    for m in T.MS:
        for B in (1, 3, 20):
            cov = T.covariances(B, m, seed=1000 * m + B).float()
            cov64 = cov.double()
            Lf, info = L.mvn_factor(cov.cuda())
            rungs = info.cpu()
            Lref = R.factor_at(cov64, rungs, R.F32)
            g = torch.Generator().manual_seed(m + 7 * B)
            mu = torch.randn(B, m, generator=g, dtype=torch.float64).float()
            eh, et, ratio = 0.0, 0.0, 0.0
            for S in T.SS:
                eps = torch.randn(S, m, generator=g, dtype=torch.float64).float()
                comp = torch.randint(B, (S,), generator=g) if B > 1 else torch.zeros(S, dtype=torch.int64)
                order, offsets = R.group(comp, B)
                o, off = (order.int().cuda(), offsets.int().cuda()) if B > 1 else (None, None)
                y = L.mvn_sample(Lf, info, mu.cuda(), eps.cuda(), T.Y_MEAN, T.Y_STD, o, off).cpu().double()
                ref = R.sample_ref(Lref, mu.double(), eps.double(), comp, T.Y_MEAN, T.Y_STD)
                e_h = T.component_errors(y, ref, comp, cov64, B)
                e_t = T.component_errors(T.torch32_draws(cov64, rungs, mu, eps, comp), ref, comp, cov64, B)
                for a, b in zip(e_h, e_t):
                    eh, et = max(eh, a), max(et, b)
                    if b > 0:
                        ratio = max(ratio, a / b)
            worst_hip, worst_ratio = max(worst_hip, eh), max(worst_ratio, ratio)
            lines.append('%5d %3d | %10.3e %10.3e %8.2f | %s' % (m, B, eh, et, ratio, sorted(set(rungs.tolist()))))
    lines.append('worst HIP error %.3e, worst HIP / torch ratio %.2f' % (worst_hip, worst_ratio))
    text = '\n'.join(lines) + '\n'
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
