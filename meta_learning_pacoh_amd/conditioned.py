"""A meta-learned GP conditioned ONCE on a task's context: predict as often as needed without refactoring, append points in O(n^2).

    cond = model.condition(context_x, context_y)          # Gram, jittered Cholesky and L^-1: once
    mean, std = cond.predict(candidates)                   # no factorisation: a Gram tile and a triangular GEMM on the matrix cores
    cond.append(x_new, y_new)                              # bordered update of the stored factor
    paths = cond.sample_paths(16)                          # posterior function draws (paths.py): paths(candidates) -> [P * 16, m]
    idx, value = paths.argmax(candidates)                  # each draw's best candidate, fused: no [P * 16, m] tensor, any pool size
    idx, paths = cond.thompson(candidates, batch_size=4)   # a Thompson batch: 4 candidates, each the argmax of its own draw
    ei = cond.acquisition('ei', candidates)                # analytic acquisition ('ei', 'pi', 'ucb', 'mean', 'std') -> [m], original units
    idx, value = cond.acquire('ei', candidates, mask=free) # its best candidate, fused behind predict: no [P, m] values kept, any pool size

What predict() of the learners recomputes on every call (csrc/gp_cond.hip keeps it: the rows of L^-1 and alpha) is what gpytorch
caches in its prediction strategy and updates in ExactGP.get_fantasy_model; the reference itself never reuses them.

Out of scope: the joint covariance (so no log_prob on this object: use predict(..., return_density=True) of the learner; joint
DRAWS come from sample_paths(), which needs no covariance), the cosine kernel family in sample_paths(), several tasks in one object,
ragged contexts (n_valid), the single-task learner GPRegressionLearned, contexts beyond _lib.gp_cond_max_n(dtype) points (there is
no large-context path), gradients, and of the acquisition functions (acquisition.py): batch / q-acquisition and top-k, look-ahead
acquisition (knowledge gradient), a log-EI, and a per-task incumbent."""
import math

import numpy as np
import torch

from . import _lib as L
from . import acquisition as A
from .distributions import GaussianPredictive
from .paths import PosteriorPaths, check_base, draw_base
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

    def sample_paths(self, num_paths, num_features=1024, base=None, like=None):
        """num_paths posterior FUNCTION draws per parameter row by pathwise conditioning on num_features random Fourier features
        (paths.py) -> PosteriorPaths: paths(test_x) evaluates all of them at any number of points in one launch, without a joint
        covariance.  The fit costs two triangular products with the stored factor, once.
        base = (omega [D,f], phase [D], w [P,S,D], eps [P,S,n]) on the device: used as it is (shapes are checked, no random number is
        drawn).  like = an earlier PosteriorPaths of this object with the same num_paths and num_features: its omega, phase, w and
        eps columns are kept and eps is drawn only for the points appended since, so a loop follows the same prior functions as data
        arrive.  Otherwise the base comes from torch's device generator in the fixed order of paths.draw_base.
        The cosine kernel family raises NotImplementedError."""
        lay = self._engine.layout
        st = self._state
        P, S, D, f = st.theta.shape[0], int(num_paths), int(num_features), lay.feature_dim
        L._path_family(lay.kernel_code)
        if S < 1:
            raise ValueError('num_paths must be at least 1, got %d' % S)
        if D < L.PATH_MIN_FEATURES or D > L.PATH_MAX_FEATURES or D % 16:
            raise ValueError('num_features must be a multiple of 16 in [%d, %d], got %d' % (L.PATH_MIN_FEATURES, L.PATH_MAX_FEATURES, D))
        if base is not None and like is not None:
            raise ValueError('give base= or like=, not both')
        if base is not None:
            base = check_base(base, D, f, P, S, st.n, self._dtype, self._device)
        else:
            base = draw_base(lay.kernel_code, D, f, P, S, st.n, self._dtype, self._device,
                             like=None if like is None else like.base)
        snap = self._engine.cond_paths(st, base)
        return PosteriorPaths(self._engine, snap, self._norm_x, self._y_mean.reshape(-1)[0], self._y_std.reshape(-1)[0])

    def _acq(self, kind, candidates, best_f, xi, beta, maximize, observation_noise, mask, chunk, want_values):
        A.kind_code(kind)
        st = self._state
        xn = self._norm_x(candidates)
        if mask is not None:
            mask = torch.as_tensor(mask, dtype=torch.bool).reshape(-1).to(xn.device).contiguous()
            if mask.shape[0] != xn.shape[0]:
                raise ValueError('mask must be [%d], got %s' % (xn.shape[0], tuple(mask.shape)))
        y_mean, y_std = self._y_mean.reshape(-1)[0], self._y_std.reshape(-1)[0]
        best_n, xi_n = 0.0, 0.0
        if kind in ('ei', 'pi'):
            if best_f is None:                   # the best observed target of the context, already normalised (one host sync)
                seen = st.ctx_y[:st.n]
                best_n, xi_n = float(seen.max() if maximize else seen.min()), float(xi) / float(y_std)
            else:
                best_n, xi_n = A.to_normalised(best_f, xi, y_mean, y_std)
        val, idx, values = self._engine.cond_acq(st, xn, kind, best_n, xi_n, float(beta), 1 if maximize else -1,
                                                 not observation_noise, mask, chunk, want_values)
        return (idx[0], A.to_original(val[0], kind, y_mean, y_std),
                None if values is None else A.to_original(values, kind, y_mean, y_std))

    def acquisition(self, kind, candidates, best_f=None, xi=0.0, beta=2.0, maximize=True, observation_noise=False):
        """the analytic acquisition function `kind` at candidates [m,d] -> tensor [m] on the device, in original units: 'ei' expected
        improvement over best_f by more than xi, 'pi' its probability, 'ucb' mean + beta std (maximize=False: the lower confidence
        bound mean - beta std), 'mean', 'std'.  SVGD / VI-Bayes: of the equal-weight mixture over the rows ('ei' / 'pi': the mean of
        the rows' values; 'ucb' / 'mean' / 'std': the mixture's moments) -- acquisition.mixture_acquisition is the rule, one fused
        launch behind the predict launch computes it (csrc/acq.hip).
        best_f: the incumbent in original units (None: the best observed target of the conditioned context; only 'ei' / 'pi' read
        it).  maximize=False: a smaller target is better.  observation_noise=False (the default) scores the latent function, as BO
        libraries do; True scores the noisy target that predict() describes."""
        return self._acq(kind, candidates, best_f, xi, beta, maximize, observation_noise, None, None, True)[2]

    def acquire(self, kind, candidates, best_f=None, xi=0.0, beta=2.0, maximize=True, observation_noise=False, mask=None, chunk=None):
        """the best candidate by acquisition(...) -> (idx int64 scalar tensor on the device, value scalar tensor in original units):
        the greatest value ('mean' / 'ucb' with maximize=False: the smallest), ties to the smaller index, NaN never wins, idx -1 and
        value NaN when nothing is eligible.  The values are not kept: the pool is streamed in chunks of `chunk` candidates (None:
        131 072) through predict + the fused kernel, so it can be of any size.  mask: bool tensor or array [m], True = eligible."""
        idx, val, _ = self._acq(kind, candidates, best_f, xi, beta, maximize, observation_noise, mask, chunk, False)
        return idx, val

    def thompson(self, candidates, batch_size=1, num_features=1024, mask=None, chunk=None, like=None):
        """a batch of Thompson samples over a pool of candidates [m,d] -> (idx int64 [batch_size] on the device, paths).  With P
        parameter rows, S = ceil(batch_size / P) function draws per row are taken (sample_paths) and each draw's argmax over the
        eligible candidates found by the fused kernel (paths.argmax: any pool size); batch_size of the P S indices are returned,
        chosen by a random permutation from torch's device generator -- the stratified sample of the equal-weight mixture that
        paths.component documents.  idx is -1 where nothing was eligible; two draws may pick the same candidate.
        mask / chunk as paths.argmax; like = the PosteriorPaths of the previous round (the same batch_size and num_features) to follow
        the same prior functions after append().  The returned PosteriorPaths is what to pass as like= next round."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError('batch_size must be at least 1, got %d' % batch_size)
        P = self._state.theta.shape[0]
        paths = self.sample_paths(math.ceil(batch_size / P), num_features, like=like)
        idx, _ = paths.argmax(candidates, mask=mask, chunk=chunk)
        pick = torch.randperm(idx.shape[0], device=idx.device)[:batch_size]
        return idx[pick], paths
