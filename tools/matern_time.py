"""time of the fused GP LML+gradient and predictive kernels per kernel family (fp32):  python tools/matern_time.py [reps]

Two shapes: 20 480 problems of n = 64 (f = 2, predictive m = 64) and 5 120 problems of n = 128 (f = 2, m = 128).  At each, ARD-RBF,
the three Matern families and cosine.  RBF and Matern run on the register-resident kernels (gp_reg.hip, gp_reg_matern.hip), cosine on
the general LDS-resident kernel (gp_small.hip): it stands for what a family costs off the register-resident path."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402

FAMILIES = [('rbf', L.KERNEL_RBF), ('matern12', L.KERNEL_MATERN12), ('matern32', L.KERNEL_MATERN32),
            ('matern52', L.KERNEL_MATERN52), ('cosine', L.KERNEL_COSINE)]
SHAPES = [(1024, 20, 64, 2), (256, 20, 128, 2)]          # (tasks, particles, n = m, f)


def timed(run, reps):
    for _ in range(3):
        run()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for T, P, n, f in SHAPES:
        B = T * P
        g = torch.Generator().manual_seed(0)
        z = torch.randn(B, n, f, generator=g).cuda()
        zt = torch.randn(B, n, f, generator=g).cuda()
        mean = (0.3 * torch.randn(B, n, generator=g)).cuda()
        mean_t = (0.3 * torch.randn(B, n, generator=g)).cuda()
        y = torch.randn(T, n, generator=g).cuda()
        ls = (torch.rand(P, f, generator=g) + 0.5).cuda()
        os_ = (torch.rand(P, generator=g) + 0.5).cuda()
        noise = (torch.rand(P, generator=g) * 0.3 + 0.1).cuda()
        res = {}
        for name, code in FAMILIES:
            fb = timed(lambda: L.gp_lml_fwdbwd(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, B, P, kernel=code), reps)
            pr = timed(lambda: L.gp_predict(z, 1, mean, L.MEAN_VECTOR, y, P, zt, 1, mean_t, ls, os_, noise, B, P, kernel=code), reps)
            res[name] = (fb, pr)
        print('%d problems, n = m = %d, f = %d' % (B, n, f))
        for name, (fb, pr) in res.items():
            print('  %-9s fwd+bwd %.4f ms (%.2fx rbf, cosine / it %.1fx)   predict %.4f ms (%.2fx rbf, cosine / it %.1fx)'
                  % (name, fb, fb / res['rbf'][0], res['cosine'][0] / fb, pr, pr / res['rbf'][1], res['cosine'][1] / pr))


if __name__ == '__main__':
    main()
