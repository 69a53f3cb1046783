"""Posterior FUNCTION draws of a conditioned GP by pathwise conditioning (Matheron's rule on a random-Fourier-feature prior; Wilson et
al. 2020, "Efficiently sampling functions from Gaussian process posteriors"):

    paths = cond.sample_paths(16)                          # fit once: two triangular products with the stored L^-1
    f = paths(candidates)                                  # [P * 16, m]: one GEMM on the matrix cores, any m, no m x m covariance
    idx, value = paths.argmax(candidates)                  # Thompson sampling: each draw's best candidate, fused -- no [P * 16, m]
                                                           # tensor, pools of any size in constant device memory (argmin alike)

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


# ---- the selection rule of pacoh_gp_path_argmax as pure torch (no device work): the specification the tests pin -----------------------
def first_best(out, mask=None, largest=True):
    """the rule on a dense tensor out [..., m] -> (idx int64 [...], val [...]): among the eligible entries (mask [m] bool, True =
    eligible; None: all) that are not NaN, the greatest (largest) or smallest value; ties (==, so -0.0 ties with +0.0) go to the
    smaller index, whose own value is returned; nothing eligible: idx -1, val NaN"""
    m = out.shape[-1]
    ok = ~torch.isnan(out)
    if mask is not None:
        ok = ok & torch.as_tensor(mask, dtype=torch.bool, device=out.device)
    lose = float('-inf') if largest else float('inf')
    key = torch.where(ok, out, torch.full_like(out, lose))
    ext = (key.max(-1) if largest else key.min(-1)).values
    hit = ok & (out == ext.unsqueeze(-1))
    pos = torch.arange(m, device=out.device).expand(out.shape)
    idx = torch.where(hit, pos, torch.full_like(pos, m)).min(-1).values
    found = idx < m
    val = out.gather(-1, idx.clamp(max=m - 1).unsqueeze(-1)).squeeze(-1)
    return torch.where(found, idx, torch.full_like(idx, -1)), torch.where(found, val, torch.full_like(val, float('nan')))


def merge_best(val_a, idx_a, val_b, idx_b, largest=True):
    """two results of the rule on disjoint index sets (global indices; idx < 0: nothing) -> (idx, val) of their union: the better
    value, on a tie (==) the smaller index.  Commutative and associative, so chunks of a pool can be merged in any order"""
    b_ahead = (val_b > val_a) if largest else (val_b < val_a)
    b_ahead = b_ahead | ((val_b == val_a) & (idx_b < idx_a))
    take_b = (idx_b >= 0) & ((idx_a < 0) | b_ahead)
    return torch.where(take_b, idx_b, idx_a), torch.where(take_b, val_b, val_a)


def chunk_ranges(m, chunk):
    """[0, m) as consecutive ranges of at most `chunk` points -> [(lo, hi), ...]"""
    m, chunk = int(m), int(chunk)
    if m < 1 or chunk < 1:
        raise ValueError('need m >= 1 and chunk >= 1, got %d and %d' % (m, chunk))
    return [(lo, min(m, lo + chunk)) for lo in range(0, m, chunk)]


class PosteriorPaths:
    """returned by ConditionedGP.sample_paths().  A snapshot: it holds its own copy of the scaled context, the parameter rows, their
    hyper-parameters, the base and the fitted v, so later append() / meta_fit() calls do not change what it evaluates to, and two
    calls on the same inputs are bit-identical.
      paths(test_x)     -> tensor [P * num_paths, m] on the device, original units, component-major (rows p * num_paths .. of row p)
      paths.argmax(test_x) / paths.argmin(test_x) -> (idx int64 [P * num_paths], value [P * num_paths]): each draw's best point of
                           test_x and its value, fused on the device (csrc/gp_path.hip: pacoh_gp_path_argmax); paths(test_x) is
                           never formed, so test_x can be a pool of any size
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

    def _best(self, test_x, largest, mask, chunk):
        xn = self._norm_x(test_x)
        if mask is not None:
            mask = torch.as_tensor(mask, dtype=torch.bool).reshape(-1).to(xn.device).contiguous()
            if mask.shape[0] != xn.shape[0]:
                raise ValueError('mask must be [%d], got %s' % (xn.shape[0], tuple(mask.shape)))
        f, idx = self._engine.cond_paths_argmax(self._snap, xn, largest=largest, mask=mask, chunk=chunk)      # [P,S], normalised space
        return idx.reshape(-1), (f * self._y_std + self._y_mean).reshape(-1)

    def argmax(self, test_x, mask=None, chunk=None):
        """each draw's greatest point of test_x [m,d] -> (idx int64 [P * num_paths] on the device, component-major like paths(...);
        value [P * num_paths] = paths(test_x)[r, idx[r]] in original units).  It IS the first index among the exact maxima of the
        draw in normalised space (ties to the smaller index, NaN never wins), but paths(test_x) is never formed: the pool is streamed
        through the fused kernel in chunks of `chunk` candidates (None: 131 072), in constant device memory.
        mask: bool tensor or array [m], True = eligible (e.g. ~already_evaluated); a draw with no eligible point gives -1 / NaN."""
        return self._best(test_x, True, mask, chunk)

    def argmin(self, test_x, mask=None, chunk=None):
        """as argmax, for each draw's smallest point"""
        return self._best(test_x, False, mask, chunk)
