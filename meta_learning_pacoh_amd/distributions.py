"""Predictive distribution objects returned by predict(..., return_density=True).

They play the role of AffineTransformedDistribution(MultivariateNormal) (meta_learn/models.py:15-43) and
EqualWeightedMixtureDist(batched=True) (models.py:74-140) in the reference: .mean, .stddev, .variance,
.log_prob (JOINT Gaussian log-density over all test points, per component), .cdf / .icdf (marginals), .marginal_log_prob (per-point
log-density of the marginals: what the leave-one-out predictive, which has no joint covariance, is scored with), and joint draws
.sample / .rsample (MultivariateNormal.rsample of the reference's single-Gaussian predictive).
The joint log-density runs the dense HIP Cholesky kernel on the predictive covariance; the draws factor it once per object
(pacoh_mvn_factor) and transform the standard normals on the matrix cores (pacoh_mvn_sample)."""
import math

import torch

from . import _lib as L
from .engine import NotPSDError

_NO_COV = 'predict(..., return_density=True) must be called to get the joint covariance'


class GaussianPredictive:
    """P Gaussian components over m test points, held in NORMALISED space with the affine
    un-normalisation y = y_mean + y_std * y_n applied on access.  P == 1 & mixture=False is the MAP case."""

    def __init__(self, mu_n, var_n, cov_n, y_mean, y_std, mixture):
        self._mu_n, self._var_n, self._cov_n = mu_n, var_n, cov_n        # [P,m], [P,m], [P,m,m]
        self.y_mean, self.y_std = float(y_mean), float(y_std)
        self.mixture = mixture
        self.num_dists = mu_n.shape[0]
        self._chol = None                    # (L [P,m,m], info [P]) of the first draw, reused by every later one

    # -- component moments in original units ------------------------------------------------------
    @property
    def _means(self):
        return self._mu_n * self.y_std + self.y_mean

    @property
    def _vars(self):
        return self._var_n * self.y_std ** 2

    @property
    def mean(self):
        m = self._means
        return m.mean(0) if self.mixture else m[0]

    @property
    def variance(self):
        if not self.mixture:
            return self._vars[0]
        means = self._means
        return ((means - means.mean(0)) ** 2).mean(0) + self._vars.mean(0)      # models.py:101-115

    @property
    def stddev(self):
        return torch.sqrt(self.variance)

    # -- densities --------------------------------------------------------------------------------
    def log_prob(self, value):
        """joint log-density of the m test targets (original units); mixture: logsumexp - log P"""
        if self._cov_n is None:
            raise RuntimeError(_NO_COV)
        value = torch.as_tensor(value, dtype=self._mu_n.dtype, device=self._mu_n.device).flatten()
        m = value.shape[0]
        resid = ((value - self.y_mean) / self.y_std).unsqueeze(0) - self._mu_n              # [P,m]
        logp, _, _ = L.mvn_logprob_dense(self._cov_n.clone(), resid.contiguous(), 1.0)
        logp = logp - m * math.log(self.y_std)
        if not self.mixture:
            return logp[0]
        return torch.logsumexp(logp, dim=0, keepdim=True) - math.log(self.num_dists)

    def marginal_log_prob(self, value):
        """per-point log-density [m] of the targets under the MARGINAL predictive of each point (original units); mixture:
        logsumexp over the components - log P.  Needs no covariance; elementwise torch, so it also works on CPU tensors"""
        value = torch.as_tensor(value, dtype=self._mu_n.dtype, device=self._mu_n.device).flatten()
        var = self._var_n
        z = ((value - self.y_mean) / self.y_std).unsqueeze(0) - self._mu_n                  # [P,m]
        logp = -0.5 * (z * z / var + torch.log(var) + math.log(2.0 * math.pi)) - math.log(self.y_std)
        if not self.mixture:
            return logp[0]
        return torch.logsumexp(logp, dim=0) - math.log(self.num_dists)

    def cdf(self, value):
        """marginal cdf per test point (mixture: mean over components, models.py:124-131)"""
        value = torch.as_tensor(value, dtype=self._mu_n.dtype, device=self._mu_n.device)
        return L.mixture_cdf(self._mu_n.contiguous(), self._var_n.contiguous(), value, self.y_mean, self.y_std)

    def icdf(self, quantile):
        """marginal quantiles per test point: Gaussian closed form for one component, the reference's bisection (models.py:136-140,
        util.py:9-42) for the mixture -- one kernel launch either way"""
        quantile = torch.as_tensor(quantile, dtype=self._mu_n.dtype, device=self._mu_n.device)
        return L.mixture_icdf(self._mu_n.contiguous(), self._var_n.contiguous(), quantile, self.y_mean, self.y_std,
                              closed_form=not self.mixture)

    def acquisition(self, kind, best_f=None, xi=0.0, beta=2.0, maximize=True):
        """the analytic acquisition function `kind` ('ei', 'pi', 'ucb', 'mean', 'std'; acquisition.py) at the m test points this
        object holds -> tensor [m] in original units, one fused launch.  Mixture: of the equal-weight mixture over the num_dists
        components; else of the single component.  The variance is the one held here, observation noise included.  best_f (original
        units) is the incumbent 'ei' / 'pi' improve on: required for them.  maximize=False: a smaller target is better."""
        from . import acquisition as A
        A.kind_code(kind)
        best_n, xi_n = 0.0, 0.0
        if kind in ('ei', 'pi'):
            if best_f is None:
                raise ValueError("best_f (the incumbent, in original units) is required for %r" % kind)
            best_n, xi_n = A.to_normalised(best_f, xi, self.y_mean, self.y_std)
        P = self.num_dists if self.mixture else 1
        sign = 1 if maximize else -1
        _, _, values = L.mixture_acq(self._mu_n[:P].contiguous(), self._var_n[:P].contiguous(), 1, P, kind, best_n, xi_n, float(beta),
                                     sign, want_values=True, largest=not (kind in ('mean', 'ucb') and sign == -1))
        return A.to_original(values[0], kind, self.y_mean, self.y_std)

    # -- joint draws ------------------------------------------------------------------------------
    def _factor(self):
        """the Cholesky factors of the P component covariances with gpytorch's jitter ladder, computed on the first draw (one host
        sync, to read which components failed) and kept; the covariance itself stays intact"""
        if self._chol is None:
            Lf, info = L.mvn_factor(self._cov_n)
            bad = torch.nonzero(info < 0).flatten().tolist()
            self._chol = (Lf, info, bad)
        Lf, info, bad = self._chol
        if bad:
            raise NotPSDError('predictive covariance of component %s is not positive definite even after adding jitter (%s)'
                              % (', '.join(str(c) for c in bad), '1e-6 .. 1e-4' if self._mu_n.dtype == torch.float32 else '1e-8 .. 1e-6'))
        return Lf, info

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """joint draws of the m test targets in original units, shape [*sample_shape, m]: y_mean + y_std (mu_c + L_c eps), L_c the
        jittered Cholesky factor of component c's predictive covariance (observation noise included, as likelihood(gp(x))).

        base_samples [*sample_shape, m]: the standard normals eps (then sample_shape is read from them, as gpytorch's
        MultivariateNormal.rsample does); otherwise eps are drawn on the device.  Draw order on the device generator, fixed:
        1. mixture only: the component of every draw, torch.randint(P, (S,));  2. eps = torch.randn(S, m).
        One component (mixture=False): every draw from component 0, as the reference.  Mixture: each draw picks a component uniformly
        and draws from it -- an extension, the reference's EqualWeightedMixtureDist (models.py:74-140) cannot sample.
        No autograd graph is built.  Raises engine.NotPSDError when a component is not positive definite after the jitter ladder."""
        if self._cov_n is None:
            raise RuntimeError(_NO_COV)
        mu_n = self._mu_n
        dev, dt = mu_n.device, mu_n.dtype
        m, P = mu_n.shape[1], self.num_dists
        with torch.no_grad():
            if base_samples is not None:
                base_samples = torch.as_tensor(base_samples, dtype=dt, device=dev)
                if base_samples.dim() < 1 or base_samples.shape[-1] != m:
                    raise RuntimeError('base_samples must have shape [*sample_shape, %d], got %s' % (m, tuple(base_samples.shape)))
                sample_shape = base_samples.shape[:-1]
            sample_shape = torch.Size(sample_shape)
            S = sample_shape.numel()
            if S == 0:
                return torch.empty(*sample_shape, m, dtype=dt, device=dev)
            Lf, info = self._factor()
            comp = torch.randint(P, (S,), device=dev) if self.mixture else None
            eps = (base_samples.reshape(S, m).contiguous() if base_samples is not None
                   else torch.randn(S, m, dtype=dt, device=dev))
            if comp is not None and P > 1:
                # (device-side grouping: a stable sort and the component boundaries in it -- no host sync)
                sorted_comp, order = torch.sort(comp, stable=True)
                order = order.to(torch.int32)
                offsets = torch.searchsorted(sorted_comp, torch.arange(P + 1, device=dev)).to(torch.int32)
                out = L.mvn_sample(Lf, info, mu_n.contiguous(), eps, self.y_mean, self.y_std, order, offsets)
            else:
                out = L.mvn_sample(Lf[:1], info[:1], mu_n[:1].contiguous(), eps, self.y_mean, self.y_std)
        return out.reshape(*sample_shape, m)

    def sample(self, sample_shape=torch.Size()):
        """the draws of rsample under torch.no_grad()"""
        with torch.no_grad():
            return self.rsample(sample_shape)
