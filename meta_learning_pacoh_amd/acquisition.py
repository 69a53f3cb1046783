"""Analytic acquisition functions on the posterior predictive of an equal-weight mixture of P Gaussians per candidate, as pure torch:
the SPECIFICATION that the fused kernel (csrc/acq.hip: pacoh_mixture_acq) is held to, the way paths.first_best is for the argmax.

    values = mixture_acquisition(mu, var, 'ei', best=0.3)           # mu, var [T,P,m] in normalised space -> [T,m]
    idx, val = paths.first_best(values)                            # the selection rule is the argmax's: there is no second one

Kinds: 'ei' expected improvement, 'pi' probability of improvement, 'ucb' mean + sign beta std (sign = -1: the lower confidence
bound), 'mean', 'std'.  Everything here runs in NORMALISED space, in the dtype of mu, on any device; to_normalised / to_original
are the conversion to and from original units (y = y_mean + y_std y_n)."""
import math

import torch

KINDS = ('ei', 'pi', 'ucb', 'mean', 'std')          # the position is the `kind` code of pacoh_mixture_acq
SQRT2 = math.sqrt(2.0)
SQRT2PI = math.sqrt(2.0 * math.pi)


def kind_code(kind):
    if kind not in KINDS:
        raise ValueError('kind must be one of %s, got %r' % (', '.join(repr(k) for k in KINDS), kind))
    return KINDS.index(kind)


def mixture_acquisition(mu, var, kind, best=0.0, xi=0.0, beta=2.0, sign=1, noise=None):
    """mu, var [T,P,m] (P rows of an equal-weight mixture per task) -> values [T,m].  An explicit loop over the rows p = 0 .. P-1, every
    operation in the dtype of mu and in the order written here, so that an fp32 run is a fair comparator of the fp32 kernel.
    Per row: v_p = var_p - noise[p] if noise [P] is given (the latent function), then 0 where v_p < 0 (a NaN stays NaN).
    'mean' / 'std' / 'ucb': the mixture's moments by Welford's update, for k = p + 1
        delta = mu_p - M;  M += delta / k;  S += delta (mu_p - M);  V += (v_p - V) / k;      mean = M,  sd = sqrt(V + S / P)
      (GaussianPredictive.mean / .variance without their E[mu^2] - mean^2 cancellation);  'ucb' = M + (sign beta) sd.  'mean' never
      reads var, so only a NaN in mu shows in it.
    'ei' / 'pi': d = sign (mu_p - best) - xi,  s = sqrt(v_p);
        s > 0:  z = d / s,  Phi = 0.5 erfc(-z / sqrt 2),  phi = exp(-z^2 / 2) / sqrt(2 pi);   ei_p = max(s (z Phi + phi), 0),  pi_p = Phi
        s == 0: ei_p = max(d, 0),  pi_p = 1 if d > 0 else 0          (a NaN d or s gives NaN)
      value = (sum_p term_p) / P, summed in row order.  The clamp matters: for z << 0 the two terms cancel and -1e-40 must not beat 0.
    sign = +1 maximises the objective, -1 minimises it (improvement is best - mu)."""
    code = kind_code(kind)
    if mu.dim() != 3 or mu.shape != var.shape or mu.shape[1] < 1:
        raise ValueError('mu and var must both be [T,P,m], got %s and %s' % (tuple(mu.shape), tuple(var.shape)))
    if sign not in (1, -1):
        raise ValueError('sign must be +1 or -1, got %r' % (sign,))
    T, P, m = mu.shape
    if noise is not None and noise.numel() != P:
        raise ValueError('noise must be [%d], got %s' % (P, tuple(noise.shape)))
    zero = torch.zeros(T, m, dtype=mu.dtype, device=mu.device)
    nan = torch.full_like(zero, float('nan'))

    def latent(p):
        v = var[:, p] - noise.reshape(-1)[p] if noise is not None else var[:, p]
        return torch.where(v < 0, zero, v)

    if kind in ('mean', 'std', 'ucb'):
        M, S, V = zero.clone(), zero.clone(), zero.clone()
        for p in range(P):
            k = float(p + 1)
            delta = mu[:, p] - M
            M = M + delta / k
            S = S + delta * (mu[:, p] - M)
            V = V + (latent(p) - V) / k
        if kind == 'mean':
            return M
        sd = torch.sqrt(V + S / float(P))
        return sd if kind == 'std' else M + (float(sign) * float(beta)) * sd
    acc = zero.clone()
    one = torch.ones_like(zero)
    for p in range(P):
        d = float(sign) * (mu[:, p] - float(best)) - float(xi)
        s = torch.sqrt(latent(p))
        z = d / s
        Phi = 0.5 * torch.erfc(-z / SQRT2)
        if code == 0:
            phi = torch.exp(-(z * z) / 2.0) / SQRT2PI
            e = s * (z * Phi + phi)
            pos = torch.where(e < 0, zero, e)
            at0 = torch.where(d < 0, zero, d)
        else:
            pos = Phi
            at0 = torch.where(d > 0, one, torch.where(d == d, zero, d))
        acc = acc + torch.where(s > 0, pos, torch.where(s == 0, at0, nan))
    return acc / float(P)


def to_normalised(best_f, xi, y_mean, y_std):
    """the incumbent and the margin in original units -> (best_n, xi_n) in normalised space; beta needs no conversion"""
    return (float(best_f) - float(y_mean)) / float(y_std), float(xi) / float(y_std)


def to_original(values, kind, y_mean, y_std):
    """values of mixture_acquisition -> original units: 'mean' / 'ucb' are targets (y_std v + y_mean), 'std' / 'ei' are lengths on
    the target axis (y_std v), 'pi' is a probability (unchanged)"""
    kind_code(kind)
    if kind in ('mean', 'ucb'):
        return values * float(y_std) + float(y_mean)
    if kind in ('std', 'ei'):
        return values * float(y_std)
    return values
