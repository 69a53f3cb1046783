"""CPU references of the pathwise posterior function draws (include/pacoh_gp.h, pacoh_gp_path_fit / pacoh_gp_path_eval), shared by
tests/test_path_host.py, tests/test_gpu_path.py and tests/path_fp32_errors.py.  Plain torch, in the dtype of zs.
  frequencies(...)   omega [D,f] and phase [D] of a family from a seeded CPU generator (its own recipe, not the package's function)
  features(...)      Phi [rows,D] = sqrt(2 os / D) cos(u omega^T + phase)
  paths(...)         the draws through the KEPT X = L^-1:  v = X^T X (resid - Phi(zs) w - sqrt(noise + jitter) eps)
  paths_direct(...)  the same through torch.linalg.solve on K + jitter I, no X
  both ->            f [S,m] = mean_t + Phi(ut) w + os k(ut, zs) v      (the latent function, normalised space)
One problem per call: zs [n,f] the context ALREADY divided by the lengthscales, resid [n], zt [m,f] the raw test features, mean_t [m],
lengthscale [f], outputscale / noise / jitter scalars, omega [D,f], phase [D], w [S,D], eps [S,n]."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref as LR                                    # noqa: E402

F64 = torch.float64
FAMILIES = ('rbf', 'm12', 'm32', 'm52')
CODE, NU = LR.CODE, LR.NU


def frequencies(family, D, f, seed, dtype=F64):
    """RBF: omega ~ N(0, I_f).  Matern nu: omega = g / sqrt(u / 2 nu), g ~ N(0, I_f), u ~ chi^2(2 nu).  phase ~ U[0, 2 pi)"""
    g = torch.Generator().manual_seed(seed)
    omega = torch.randn(D, f, generator=g, dtype=F64)
    if family in NU:
        two_nu = int(round(2 * NU[family]))
        u = (torch.randn(D, two_nu, generator=g, dtype=F64) ** 2).sum(1)
        omega = omega / (u / two_nu).sqrt().unsqueeze(1)
    phase = 2.0 * math.pi * torch.rand(D, generator=g, dtype=F64)
    return omega.to(dtype), phase.to(dtype)


def features(u, omega, phase, outputscale):
    D = omega.shape[0]
    amp = (2.0 * torch.as_tensor(outputscale, dtype=u.dtype) / D).sqrt()
    return amp * torch.cos(u @ omega.T + phase)


def _gram_scaled(u1, u2, family):
    return LR.gram(u1, u2, torch.ones(u1.shape[1], dtype=u1.dtype), 1.0, family)


def _evaluate(v, zs, zt, mean_t, lengthscale, outputscale, family, omega, phase, w):
    dt = zs.dtype
    ut = zt.to(dt) / lengthscale.to(dt)
    os_ = torch.as_tensor(outputscale, dtype=dt)
    return (mean_t.to(dt).unsqueeze(1) + features(ut, omega, phase, outputscale) @ w.T + (os_ * _gram_scaled(ut, zs, family)) @ v.T).T


def _rhs(zs, resid, outputscale, noise, jitter, omega, phase, w, eps):
    dt = zs.dtype
    sd = (torch.as_tensor(noise, dtype=dt) + jitter).sqrt()
    return resid.to(dt) - w @ features(zs, omega, phase, outputscale).T - sd * eps          # [S,n]


def paths(X, zs, resid, zt, mean_t, lengthscale, outputscale, noise, jitter, family, omega, phase, w, eps):
    """-> f [S,m] through the kept X [n,n] (lower triangular rows of L^-1)"""
    R = _rhs(zs, resid, outputscale, noise, jitter, omega, phase, w, eps)
    v = (X.T @ (X @ R.T)).T
    return _evaluate(v, zs, zt, mean_t, lengthscale, outputscale, family, omega, phase, w)


def fit_direct(zs, resid, outputscale, noise, jitter, family, omega, phase, w, eps):
    """-> v [S,n] = (K + jitter I)^-1 R by a dense solve"""
    dt = zs.dtype
    n = zs.shape[0]
    K = (torch.as_tensor(outputscale, dtype=dt) * _gram_scaled(zs, zs, family)
         + (torch.as_tensor(noise, dtype=dt) + jitter) * torch.eye(n, dtype=dt))
    R = _rhs(zs, resid, outputscale, noise, jitter, omega, phase, w, eps)
    return torch.linalg.solve(K, R.T).T


def paths_direct(zs, resid, zt, mean_t, lengthscale, outputscale, noise, jitter, family, omega, phase, w, eps):
    """-> f [S,m] with no X"""
    v = fit_direct(zs, resid, outputscale, noise, jitter, family, omega, phase, w, eps)
    return _evaluate(v, zs, zt, mean_t, lengthscale, outputscale, family, omega, phase, w)
