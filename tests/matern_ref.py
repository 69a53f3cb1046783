"""fp64 torch restatement of the Matern kernel family (gpytorch.kernels.MaternKernel, nu = 1/2, 3/2, 5/2, ARD lengthscales), shared by
tests/test_matern_host.py (which pins it against scipy's general Matern formula and autograd) and tests/test_gpu_matern.py (which holds
the device kernels to it).  Written from the documented definition in include/pacoh_gp.h, independently of the device code."""
import math

import torch

NUS = (0.5, 1.5, 2.5)
CODE = {0.5: 3, 1.5: 4, 2.5: 5}           # PACOH_KERNEL_MATERN12 / 32 / 52


def matern_of_s(s, nu):
    """k / outputscale as a function of the scaled distance s >= 0"""
    if nu == 0.5:
        return torch.exp(-s)
    a = math.sqrt(2 * nu) * s
    if nu == 1.5:
        return (1 + a) * torch.exp(-a)
    return (1 + a + a * a / 3) * torch.exp(-a)


def kd_of_s(s, nu):
    """-(1/s) d(k/os)/ds, the weight of (u_i - u_j) in the gradient; nu = 1/2: 0 at s = 0 (gpytorch's clamped distance)"""
    if nu == 0.5:
        return torch.where(s > 0, torch.exp(-s) / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    a = math.sqrt(2 * nu) * s
    if nu == 1.5:
        return 3 * torch.exp(-a)
    return 5.0 / 3.0 * (1 + a) * torch.exp(-a)


def scaled_dist(z1, z2, lengthscale):
    """gpytorch's covar_dist on x / lengthscale: sqrt(clamp_min(|u_i - u_j|^2, 1e-30)), by direct differences"""
    a = (z1 / lengthscale).unsqueeze(-2)
    b = (z2 / lengthscale).unsqueeze(-3)
    return ((a - b) ** 2).sum(-1).clamp_min(1e-30).sqrt()


def gram(z1, z2, lengthscale, outputscale=1.0, nu=2.5):
    return outputscale * matern_of_s(scaled_dist(z1, z2, lengthscale), nu)


def gram_family_for(nu):
    """a drop-in for oracle.pacoh_oracle.gram_family that evaluates the Matern family whatever `kernel` says (the oracles look the
    function up at call time, so monkeypatching it turns their SE learners into Matern learners)"""
    def gram_family(z1, z2, lengthscale, outputscale=1.0, kernel='rbf'):
        return gram(z1, z2, lengthscale, outputscale, nu)
    return gram_family
