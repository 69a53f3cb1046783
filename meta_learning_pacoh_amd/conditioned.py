"""A meta-learned GP conditioned ONCE on a task's context: predict as often as needed without refactoring, append points in O(n^2).

    cond = model.condition(context_x, context_y)          # Gram, jittered Cholesky and L^-1: once
    mean, std = cond.predict(candidates)                   # no factorisation: a Gram tile and a triangular GEMM on the matrix cores
    cond.append(x_new, y_new)                              # bordered update of the stored factor

What predict() of the learners recomputes on every call (csrc/gp_cond.hip keeps it: the rows of L^-1 and alpha) is what gpytorch
caches in its prediction strategy and updates in ExactGP.get_fantasy_model; the reference itself never reuses them.

Out of scope: the joint covariance (so no log_prob and no sample on this object: use predict(..., return_density=True) of the
learner), several tasks in one object, ragged contexts (n_valid), the single-task learner GPRegressionLearned, contexts beyond
_lib.gp_cond_max_n(dtype) points (there is no large-context path), and gradients."""
import numpy as np
import torch

from .distributions import GaussianPredictive
from .util import _handle_input_dimensionality


class ConditionedGP:
    """returned by RegressionModelMetaLearned.condition().  A snapshot: it holds its own copy of the parameter rows (MAP: the row;
    SVGD: the particles; VI: the mode, or the n_posterior_samples rows drawn at condition()) and of the normalisation statistics, so
    later meta_fit() calls do not change what it predicts."""

    def __init__(self, engine, state, mixture, x_mean, x_std, y_mean, y_std, dtype, device):
        self._engine, self._state, self._mixture = engine, state, mixture
        self._x_mean, self._x_std = np.array(x_mean, dtype=np.float64), np.array(x_std, dtype=np.float64)
        self._y_mean, self._y_std = np.array(y_mean, dtype=np.float64), np.array(y_std, dtype=np.float64)
        self._dtype, self._device = dtype, device

    @property
    def n(self):
        """context points conditioned on so far"""
        return self._state.n

    @property
    def capacity(self):
        """the most points this object can hold (append() beyond it raises)"""
        return self._state.cap

    def _to_device(self, arr):
        return torch.from_numpy(np.ascontiguousarray(arr.astype(np.float32))).to(self._dtype).to(self._device)

    def _norm_x(self, x):
        x = _handle_input_dimensionality(np.asarray(x))
        assert x.shape[1] == self._x_mean.shape[0]
        return self._to_device((x - self._x_mean) / self._x_std)

    def predict(self, test_x, return_density=False):
        """posterior predictive at test_x (observation noise included) -> (mean[m], std[m]) numpy in original units, or with
        return_density=True the GaussianPredictive (an equal-weighted mixture over the rows for SVGD and VI-Bayes).  That object has
        no joint covariance: .mean / .stddev / .cdf / .icdf / .marginal_log_prob work, .log_prob raises."""
        mu, var = self._engine.cond_predict(self._state, self._norm_x(test_x))
        dist = GaussianPredictive(mu, var, None, self._y_mean.reshape(-1)[0], self._y_std.reshape(-1)[0], mixture=self._mixture)
        if return_density:
            return dist
        return dist.mean.cpu().numpy(), dist.stddev.cpu().numpy()

    def confidence_intervals(self, test_x, confidence=0.9):
        """-> (ucb, lcb) of the predictive, as the learners' confidence_intervals"""
        dist = self.predict(test_x, return_density=True)
        alpha = (1 - confidence) / 2
        m = dist.mean.shape[0]
        ucb = dist.icdf(torch.ones(m) * (1 - alpha))
        lcb = dist.icdf(torch.ones(m) * alpha)
        return ucb.cpu(), lcb.cpu()

    def append(self, x, y):
        """add k >= 1 observed points in place -> self.  One launch and one host sync (the refusal flags); a row whose bordered
        update was refused (s^2 <= 0 in working precision) makes the object condition again on all n + k points from scratch, where
        the jitter ladder applies.  Growing past .capacity raises RuntimeError and changes nothing."""
        from .abstract import _raise_not_psd
        x, y = _handle_input_dimensionality(np.asarray(x), np.asarray(y))
        assert x.shape[1] == self._x_mean.shape[0] and y.shape[1] == 1 and x.shape[0] == y.shape[0]
        xn = self._to_device((x - self._x_mean) / self._x_std)
        yn = self._to_device(((y - self._y_mean) / self._y_std).flatten())
        fail = self._engine.cond_append(self._state, xn, yn)
        if bool(fail.any()):
            self._engine.cond_refit(self._state)
            _raise_not_psd(self._state.info)
        return self
