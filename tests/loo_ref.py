"""fp64 CPU reference of the leave-one-out predictive (include/pacoh_gp.h, pacoh_gp_loo), shared by tests/test_loo_host.py,
tests/test_gpu_loo.py and tests/loo_fp32_errors.py.
  brute(...)   really leaves each point out: the oracle's posterior predictive (oracle.gp_predict) conditioned on the other n - 1
               points, read at the left-out one; n = 1: the prior.  Independent of the closed form.
  closed(...)  the closed form the kernel evaluates (Rasmussen & Williams 5.4.2), in the dtype of its inputs:
               K = os k(Z,Z) + (noise + jitter) I,  alpha = K^-1 (y - m),  d = diag(K^-1)
               mu_loo = y - alpha / d,  var_loo = 1 / d,  lpd = mean_i log N(y_i; mu_loo_i, var_loo_i)
One problem per call: z [n,f], mean [n], y [n], lengthscale [f], outputscale and noise scalars."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref as MR                                 # noqa: E402
from oracle import pacoh_oracle as O                    # noqa: E402

F64 = torch.float64
FAMILIES = ('rbf', 'cos', 'm12', 'm32', 'm52')
CODE = {'rbf': 0, 'cos': 1, 'm12': 3, 'm32': 4, 'm52': 5}          # PACOH_KERNEL_*
NU = {'m12': 0.5, 'm32': 1.5, 'm52': 2.5}
LOG2PI = math.log(2.0 * math.pi)


def gram(z1, z2, lengthscale, outputscale, family):
    ls = lengthscale.reshape(1, -1)
    if family in NU:
        return MR.gram(z1, z2, ls, outputscale, NU[family])
    return O.gram_family(z1, z2, ls, outputscale, 'cos' if family == 'cos' else 'rbf')


def log_normal(y, mu, var):
    return -0.5 * (LOG2PI + torch.log(var) + (y - mu) ** 2 / var)


def brute(z, mean, y, lengthscale, outputscale, noise, family='rbf'):
    """-> mu_loo [n], var_loo [n], lpd (0-dim), all fp64: n posterior predictives on n - 1 points each"""
    z, mean, y, ls = z.to(F64), mean.to(F64), y.to(F64), lengthscale.to(F64).reshape(1, -1)
    os_, nz = float(outputscale), float(noise)
    n = z.shape[0]
    mu, var = torch.empty(n, dtype=F64), torch.empty(n, dtype=F64)
    saved = O.gram_family
    if family in NU:
        O.gram_family = MR.gram_family_for(NU[family])       # (gp_predict looks it up at call time, as tests/test_gpu_matern.py does)
    try:
        for i in range(n):
            if n == 1:
                mu[0], var[0] = mean[0], os_ * gram(z, z, ls, 1.0, family)[0, 0] + nz
                break
            keep = [j for j in range(n) if j != i]
            m_i, c_i = O.gp_predict(z[keep], mean[keep], y[keep], z[i:i + 1], mean[i:i + 1], ls, os_, nz,
                                    kernel='cos' if family == 'cos' else 'rbf')
            mu[i], var[i] = m_i[0], c_i[0, 0]
    finally:
        O.gram_family = saved
    return mu, var, log_normal(y, mu, var).mean()


def closed(z, mean, y, lengthscale, outputscale, noise, family='rbf', rung=0):
    """the three formulas in the dtype of z (fp64, or fp32 for the torch-fp32 yardstick); rung k >= 1: the jitter base 10^(k-1) of the
    ladder (base 1e-6 in fp32, 1e-8 in fp64) on the diagonal -> mu_loo [n], var_loo [n], lpd"""
    dt = z.dtype
    n = z.shape[0]
    jitter = 0.0 if rung == 0 else (1e-6 if dt == torch.float32 else 1e-8) * 10 ** (rung - 1)
    K = (torch.as_tensor(outputscale, dtype=dt) * gram(z, z, lengthscale.to(dt), 1.0, family)
         + (torch.as_tensor(noise, dtype=dt) + jitter) * torch.eye(n, dtype=dt))
    Lf = torch.linalg.cholesky(K)
    Kinv = torch.cholesky_inverse(Lf)
    alpha = Kinv @ (y - mean).to(dt)
    d = torch.diagonal(Kinv)
    mu, var = y.to(dt) - alpha / d, 1.0 / d
    return mu, var, log_normal(y.to(dt), mu, var).mean()


def errors(mu, var, lpd, ref):
    """(max_i |mu - mu_ref| / sqrt(var_ref), max_i |var - var_ref| / var_ref, |lpd - lpd_ref|) against ref = (mu, var, lpd) in fp64"""
    rm, rv, rl = ref
    mu, var = mu.double().cpu().reshape(-1), var.double().cpu().reshape(-1)
    e_mu = float(((mu - rm).abs() / rv.sqrt()).max()) if rm.numel() else 0.0
    e_var = float(((var - rv).abs() / rv).max()) if rm.numel() else 0.0
    return e_mu, e_var, abs(float(lpd) - float(rl))


def make_problem(n, f, family, seed, noise_ratio=0.03):
    """one well-posed problem: points of unit spread per lengthscale, noise / outputscale = noise_ratio.  The cosine kernel is positive
    definite for f = 1 only; its points stay within half a period"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, f, generator=g, dtype=F64) * (1.5 / math.sqrt(f))
    ls = 0.8 + 0.4 * torch.rand(f, generator=g, dtype=F64)
    if family == 'cos':
        assert f == 1
        z = torch.rand(n, 1, generator=g, dtype=F64) * 0.9
        ls = torch.full((1,), 2.0, dtype=F64)
    os_ = 0.5 + float(torch.rand((), generator=g, dtype=F64))
    y = torch.randn(n, generator=g, dtype=F64)
    mean = 0.3 * torch.randn(n, generator=g, dtype=F64)
    return z, mean, y, ls, os_, noise_ratio * os_
