"""Posterior FUNCTION draws of a conditioned GP by pathwise conditioning (Matheron's rule on a random-Fourier-feature prior; Wilson et
al. 2020, "Efficiently sampling functions from Gaussian process posteriors"):

    paths = cond.sample_paths(16)                          # fit once: two triangular products with the stored L^-1
    f = paths(candidates)                                  # [P * 16, m]: one GEMM on the matrix cores, any m, no m x m covariance
    x_next = candidates[f[0].argmax()]                     # Thompson sampling

A draw is  f_s(x*) = m(x*) + sum_d phi_d(u*) w_sd + sum_i os k(u*, u_i) v_si  with u = z / lengthscale,
phi_d(u) = sqrt(2 os / D) cos(omega_d . u + phase_d)  and  v_s = (K + j I)^-1 (y - m - Phi(U) w_s - sqrt(noise + j) eps_s)
(csrc/gp_path.hip).  The prior part is approximate (D features: the RFF kernel error decays like 1 / sqrt(D)), the update is exact.
Families: RBF ('SE' and 'NN' features) and Matern nu = 1/2, 3/2, 5/2; the cosine family has no such spectral form."""
import math

import torch

from . import _lib as L

MATERN_2NU = {L.KERNEL_MATERN12: 1, L.KERNEL_MATERN32: 3, L.KERNEL_MATERN52: 5}


def draw_base(kernel, D, f, P, S, n, dtype, device='cpu', generator=None, like=None):
    """the random numbers behind S draws for each of P parameter rows on n context points -> (omega [D,f], phase [D], w [P,S,D],
    eps [P,S,n]).  Pure torch, any device.  The draws come from `generator` (None: the device's default one) in this fixed order, in
    `dtype`:  randn(D, f);  Matern only: c = randn(D, 2 nu), u = (c^2).sum(1), omega = g / sqrt(u / 2 nu);  2 pi rand(D);
    randn(P, S, D);  randn(P, S, n).
    like = an earlier base (omega, phase, w, eps_old [P,S,n_old]) with n_old <= n: omega, phase, w and the first n_old columns of eps
    are kept and ONLY randn(P, S, n - n_old) is drawn, so the new draws follow the same prior functions on a grown context."""
    L._path_family(kernel)
    if kernel != L.KERNEL_RBF and kernel not in MATERN_2NU:
        raise ValueError('unknown kernel family %r' % (kernel,))
    kw = dict(dtype=dtype, device=device, generator=generator)
    if like is not None:
        omega, phase, w, eps_old = like
        n_old = eps_old.shape[2]
        if tuple(omega.shape) != (D, f) or tuple(w.shape) != (P, S, D) or tuple(eps_old.shape) != (P, S, n_old) or n_old > n:
            raise ValueError('like= holds omega %s, w %s, eps %s: not a base of %d features x %d inputs, %d rows x %d draws on at most '
                             '%d points' % (tuple(omega.shape), tuple(w.shape), tuple(eps_old.shape), D, f, P, S, n))
        eps = torch.cat([eps_old.to(dtype), torch.randn(P, S, n - n_old, **kw)], dim=2) if n > n_old else eps_old.to(dtype)
        return omega, phase, w, eps.contiguous()
    omega = torch.randn(D, f, **kw)
    if kernel in MATERN_2NU:
        two_nu = MATERN_2NU[kernel]
        c = torch.randn(D, two_nu, **kw)
        u = (c * c).sum(1)
        omega = omega / torch.sqrt(u / two_nu).unsqueeze(1)
    phase = 2.0 * math.pi * torch.rand(D, **kw)
    w = torch.randn(P, S, D, **kw)
    eps = torch.randn(P, S, n, **kw)
    return omega, phase, w, eps


def check_base(base, D, f, P, S, n, dtype, device):
    """a caller's base= tuple against the shapes it must have -> the tuple (contiguous); no random number is drawn"""
    if not isinstance(base, (tuple, list)) or len(base) != 4:
        raise ValueError('base must be the tuple (omega [D,f], phase [D], w [P,S,D], eps [P,S,n])')
    omega, phase, w, eps = base
    want = ((D, f), (D,), (P, S, D), (P, S, n))
    for name, t, shape in zip(('omega', 'phase', 'w', 'eps'), base, want):
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise ValueError('base: %s must be %s, got %s' % (name, list(shape), list(t.shape) if torch.is_tensor(t) else type(t)))
        if t.dtype != dtype or t.device.type != torch.device(device).type:
            raise ValueError('base: %s must be %s on %s, got %s on %s' % (name, dtype, device, t.dtype, t.device))
    return tuple(t.contiguous() for t in base)


class PosteriorPaths:
    """returned by ConditionedGP.sample_paths().  A snapshot: it holds its own copy of the scaled context, the parameter rows, their
    hyper-parameters, the base and the fitted v, so later append() / meta_fit() calls do not change what it evaluates to, and two
    calls on the same inputs are bit-identical.
      paths(test_x)     -> tensor [P * num_paths, m] on the device, original units, component-major (rows p * num_paths .. of row p)
      paths.component   -> int tensor [P * num_paths]: the parameter row of each draw (SVGD / VI-Bayes: a stratified sample of the
                           equal-weight mixture, num_paths per row)
      paths.base        -> (omega [D,f], phase [D], w [P,S,D], eps [P,S,n]); pass as base= to reproduce, as like= to follow"""

    def __init__(self, engine, snap, norm_x, y_mean, y_std):
        self._engine, self._snap, self._norm_x = engine, snap, norm_x
        self._y_mean, self._y_std = float(y_mean), float(y_std)
        P, S = snap.w.shape[0], snap.w.shape[1]
        self.component = torch.arange(P, device=snap.w.device).repeat_interleave(S)

    @property
    def base(self):
        s = self._snap
        return s.omega, s.phase, s.w, s.eps

    @property
    def num_paths(self):
        return self._snap.w.shape[1]

    @property
    def n(self):
        """context points the draws are conditioned on"""
        return self._snap.n

    def __call__(self, test_x, observation_noise=False):
        """the draws at test_x [m,d] -> [P * num_paths, m] in original units (y_mean + y_std f); observation_noise adds
        y_std sqrt(noise_p) randn (torch's device generator) to the latent function values"""
        f = self._engine.cond_paths_eval(self._snap, self._norm_x(test_x))              # [P,S,m], normalised space
        P, S, m = f.shape
        out = (f * self._y_std + self._y_mean).reshape(P * S, m)
        if observation_noise:
            sd = self._y_std * torch.sqrt(self._snap.hypers[2]).reshape(P, 1).expand(P, S).reshape(P * S, 1)
            out = out + sd * torch.randn(P * S, m, dtype=out.dtype, device=out.device)
        return out
