"""CPU references of the conditioned GP posterior (include/pacoh_gp.h, pacoh_gp_condition / _cond_predict / _cond_append), shared by
tests/test_cond_host.py, tests/test_gpu_cond.py and tests/cond_fp32_errors.py.
  oracle_predict(...)  the fp64 reference: the oracle's posterior predictive (oracle.gp_predict) on the full context, as
                       tests/loo_ref.brute uses it.  Independent of the closed form below.
  direct(...)          the closed form the kernels keep, in the dtype of its inputs:  K = os k(Z,Z) + (noise + jitter) I = L L^T,
                       X = L^-1,  alpha = X^T X (y - m)
  predict(...)         mu = m* + K* alpha,  var = os + noise - |X k*|^2     (the jitter sits in the factor only)
  append(...)          the incremental (bordered) form, one point at a time, in plain torch: usable in fp32 on the CPU as the fp32
                       comparator of the append kernel
One problem per call: z [n,f], mean [n], y [n], lengthscale [f], outputscale and noise scalars."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref as LR                                    # noqa: E402
import matern_ref as MR                                 # noqa: E402
from oracle import pacoh_oracle as O                    # noqa: E402

F64 = torch.float64
FAMILIES, CODE, NU = LR.FAMILIES, LR.CODE, LR.NU
gram = LR.gram


def oracle_predict(z, mean, y, zt, mean_t, lengthscale, outputscale, noise, family='rbf'):
    """-> mu [m], var [m] in fp64 (observation noise included)"""
    z, mean, y, zt, mean_t = (t.to(F64) for t in (z, mean, y, zt, mean_t))
    ls = lengthscale.to(F64).reshape(1, -1)
    saved = O.gram_family
    if family in NU:
        O.gram_family = MR.gram_family_for(NU[family])
    try:
        mu, cov = O.gp_predict(z, mean, y, zt, mean_t, ls, float(outputscale), float(noise), kernel='cos' if family == 'cos' else 'rbf')
    finally:
        O.gram_family = saved
    return mu.reshape(-1), torch.diagonal(cov).clone()


def direct(z, mean, y, lengthscale, outputscale, noise, family='rbf', jitter=0.0):
    """-> X = chol(K + jitter I)^-1 [n,n] (lower triangular), alpha [n], in the dtype of z"""
    dt = z.dtype
    n = z.shape[0]
    K = (torch.as_tensor(outputscale, dtype=dt) * gram(z, z, lengthscale.to(dt), 1.0, family)
         + (torch.as_tensor(noise, dtype=dt) + jitter) * torch.eye(n, dtype=dt))
    Lf = torch.linalg.cholesky(K)
    X = torch.linalg.solve_triangular(Lf, torch.eye(n, dtype=dt), upper=False)
    return X, X.T @ (X @ (y - mean).to(dt))


def predict(X, alpha, z, zt, mean_t, lengthscale, outputscale, noise, family='rbf'):
    """-> mu [m], var [m] from the kept quantities, in the dtype of z"""
    dt = z.dtype
    Ks = torch.as_tensor(outputscale, dtype=dt) * gram(zt, z, lengthscale.to(dt), 1.0, family)          # [m,n]
    V = Ks @ X.T
    var = torch.as_tensor(outputscale, dtype=dt) + torch.as_tensor(noise, dtype=dt) - (V * V).sum(1)
    return mean_t.to(dt) + Ks @ alpha, var


def append(X, alpha, z, resid, z_new, resid_new, lengthscale, outputscale, noise, family='rbf', jitter=0.0):
    """the bordered update, point by point -> X [n+k,n+k], alpha [n+k], z [n+k,f], resid [n+k]; raises ValueError when s^2 <= 0"""
    dt = z.dtype
    os_, nz = torch.as_tensor(outputscale, dtype=dt), torch.as_tensor(noise, dtype=dt)
    for t in range(z_new.shape[0]):
        q = z.shape[0]
        zq = z_new[t:t + 1]
        k = os_ * gram(zq, z, lengthscale.to(dt), 1.0, family).reshape(-1)
        v = X @ k
        s2 = os_ + (nz + jitter) - (v * v).sum()
        if not bool(s2 > 0):
            raise ValueError('s^2 = %g' % float(s2))
        s = s2.sqrt()
        Xn = torch.zeros(q + 1, q + 1, dtype=dt)
        Xn[:q, :q] = X
        Xn[q, :q] = -(v @ X) / s
        Xn[q, q] = 1.0 / s
        resid = torch.cat([resid, resid_new[t:t + 1].to(dt)])
        u = Xn[q] @ resid
        alpha = torch.cat([alpha, torch.zeros(1, dtype=dt)]) + Xn[q] * u
        X, z = Xn, torch.cat([z, zq])
    return X, alpha, z, resid


def errors(mu, var, ref):
    """(max |mu - ref| / sqrt(var_ref), max |var - ref| / var_ref) against ref = (mu, var) in fp64"""
    rm, rv = ref
    mu, var = mu.double().cpu().reshape(-1), var.double().cpu().reshape(-1)
    return float(((mu - rm).abs() / rv.sqrt()).max()), float(((var - rv).abs() / rv).max())


def rel_max(a, ref):
    """max abs difference in units of the largest reference entry"""
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())
