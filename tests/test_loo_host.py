"""Leave-one-out predictive on the host side (no GPU): the two new C entry points (declared, exported, bound, argument validation
without a launch), the closed form of tests/loo_ref.py pinned against really leaving each point out, marginal_log_prob of
GaussianPredictive on CPU tensors, and the learners' loo / eval_loo interface."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref as R                                                # noqa: E402
from meta_learning_pacoh_amd import _lib                           # noqa: E402
from meta_learning_pacoh_amd.distributions import GaussianPredictive   # noqa: E402

EINVAL, ELIMIT, EDTYPE = -1, -2, -3
NEW = ('pacoh_gp_loo_max_n', 'pacoh_gp_loo')


@pytest.fixture(scope='module')
def lib():
    return _lib.load_library()


def test_new_symbols_are_declared_exported_and_bound(lib):
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pacoh_gp.h')) as fh:
        header = fh.read()
    for name in NEW:
        assert name + '(' in header
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert 'gpytorch.mlls.LeaveOneOutPseudoLikelihood' in header
    assert _lib.ABI_VERSION == 14 and lib.pacoh_abi_version() == 14


def test_size_limit_query(lib):
    for dt, tdt in ((0, torch.float32), (1, torch.float64)):
        limit = lib.pacoh_gp_loo_max_n(dt)
        assert limit >= 128
        assert limit >= lib.pacoh_gp_small_max_n(dt, 1)
        assert _lib.gp_loo_max_n(tdt) == limit
    assert lib.pacoh_gp_loo_max_n(5) == EDTYPE


def test_argument_validation_without_a_device(lib):
    fake, null = ctypes.c_void_p(4096), None
    ip = ctypes.cast(fake, _lib._ip)

    def call(z=fake, z_div=1, mean=fake, mode=_lib.MEAN_VECTOR, y=fake, y_div=3, ls=fake, os_=fake, noise=fake, nv=None,
             mu=fake, var=fake, lpd=fake, info=ip, B=6, P=3, n=16, f=2, dt=0):
        return lib.pacoh_gp_loo(z, z_div, mean, mode, y, y_div, ls, os_, noise, nv, mu, var, lpd, info, B, P, n, f, dt, null)

    assert call(z=null) == EINVAL
    assert call(y=null) == EINVAL
    assert call(ls=null) == EINVAL
    assert call(noise=null) == EINVAL
    assert call(mean=null) == EINVAL and call(mean=null, mode=_lib.MEAN_CONST) == EINVAL
    assert call(mu=null, var=null, lpd=null) == EINVAL             # nothing asked for
    assert call(B=0) == EINVAL and call(P=0) == EINVAL and call(n=0) == EINVAL and call(f=0) == EINVAL
    assert call(z_div=0) == EINVAL and call(y_div=0) == EINVAL
    assert call(n=4096) == ELIMIT
    for dt in (0, 1):
        assert call(n=lib.pacoh_gp_loo_max_n(dt) + 1, dt=dt) == ELIMIT
    assert call(f=17) == ELIMIT
    assert call(f=2 | (2 << _lib.KERNEL_SHIFT)) == ELIMIT           # family code 2 is unassigned
    assert call(dt=5) == EDTYPE
    assert call(dt=5, mu=null, var=null, lpd=null) == EDTYPE        # the dtype is looked at first, as in the other GP entry points


GRID = [(n, f, fam) for n in (1, 2, 9, 65, 128) for f in (1, 3, 16) for fam in R.FAMILIES if fam != 'cos' or f == 1]


@pytest.mark.parametrize('n,f,fam', GRID, ids=['n%d-f%d-%s' % c for c in GRID])
def test_closed_form_is_leaving_each_point_out(n, f, fam):
    pb = R.make_problem(n, f, fam, seed=100 * n + f)
    ref = R.brute(*pb, family=fam)
    mu, var, lpd = R.closed(*pb, family=fam)
    assert max(R.errors(mu, var, lpd, ref)) <= 1e-10


def test_closed_form_with_a_jitter_rung_is_that_of_the_jittered_matrix():
    z, mean, y, ls, os_, noise = R.make_problem(9, 2, 'rbf', seed=7)
    for rung, j in ((1, 1e-8), (3, 1e-6)):
        a = R.closed(z, mean, y, ls, os_, noise, rung=rung)
        b = R.closed(z, mean, y, ls, os_, noise + j)
        assert max(R.errors(a[0], a[1], a[2], b)) <= 1e-12


def test_marginal_log_prob_one_component_on_cpu():
    g = torch.Generator().manual_seed(0)
    m, y_mean, y_std = 11, 0.7, 2.5
    mu = torch.randn(1, m, generator=g, dtype=torch.float64)
    var = torch.rand(1, m, generator=g, dtype=torch.float64) + 0.1
    value = torch.randn(m, generator=g, dtype=torch.float64)
    dist = GaussianPredictive(mu, var, None, y_mean, y_std, mixture=False)
    want = torch.distributions.Normal(y_mean + y_std * mu[0], y_std * var[0].sqrt()).log_prob(value)
    got = dist.marginal_log_prob(value)
    assert got.shape == (m,)
    assert float((got - want).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError, match='return_density=True'):      # no joint covariance: the joint density still refuses
        dist.log_prob(value)


def test_marginal_log_prob_mixture_on_cpu():
    g = torch.Generator().manual_seed(1)
    P, m, y_mean, y_std = 4, 6, -1.0, 0.5
    mu = torch.randn(P, m, generator=g, dtype=torch.float64)
    var = torch.rand(P, m, generator=g, dtype=torch.float64) + 0.1
    value = torch.randn(m, generator=g, dtype=torch.float64)
    got = GaussianPredictive(mu, var, None, y_mean, y_std, mixture=True).marginal_log_prob(value.tolist())
    for i in range(m):
        dens = 0.0
        for p in range(P):
            s = y_std * math.sqrt(float(var[p, i]))
            dens += math.exp(-0.5 * ((float(value[i]) - (y_mean + y_std * float(mu[p, i]))) / s) ** 2) / (s * math.sqrt(2 * math.pi)) / P
        assert abs(float(got[i]) - math.log(dens)) <= 1e-12


def test_learners_have_the_loo_interface():
    from meta_learning_pacoh_amd import GPR_meta_mll, GPR_meta_svgd, GPR_meta_vi, GPR_mll
    from meta_learning_pacoh_amd.engine import GPEngine
    for cls in (GPR_meta_mll.GPRegressionMetaLearned, GPR_meta_svgd.GPRegressionMetaLearnedSVGD, GPR_meta_vi.GPRegressionMetaLearnedVI):
        assert callable(cls.loo) and callable(cls.eval_loo) and callable(cls.eval_loo_datasets)
    assert callable(GPR_mll.GPRegressionLearned.loo) and callable(GPR_mll.GPRegressionLearned.eval_loo)
    assert callable(GPEngine.loo_tasks)


def test_wrapper_validates_before_any_call():
    """shapes, dtypes and the size limit are refused in Python, before a device pointer is taken"""
    B, P, n, f = 6, 3, 8, 2
    z, y = torch.zeros(B, n, f), torch.zeros(2, n)
    ls, os_, noise = torch.ones(P, f), torch.ones(P), torch.ones(P)
    ok = dict(z=z, z_div=1, mean=None, mean_mode=_lib.MEAN_ZERO, y=y, y_div=P, lengthscale=ls, outputscale=os_, noise=noise, B=B, P=P)

    def call(**kw):
        return _lib.gp_loo(**dict(ok, **kw))

    with pytest.raises(ValueError, match='z must be'):
        call(z=z[:4])
    with pytest.raises(ValueError, match='y must be'):
        call(y=torch.zeros(2, n + 1))
    with pytest.raises(ValueError, match='y must be'):
        call(y=y[:1])
    with pytest.raises(ValueError, match='multiple of P'):
        call(B=5)
    with pytest.raises(ValueError, match='lengthscale'):
        call(lengthscale=torch.ones(P, f + 1))
    with pytest.raises(ValueError, match='mean must be'):
        call(mean_mode=_lib.MEAN_VECTOR, mean=torch.zeros(B, n - 1))
    with pytest.raises(ValueError, match='mean must be'):
        call(mean_mode=_lib.MEAN_CONST, mean=None)
    with pytest.raises(ValueError, match='n_valid'):
        call(n_valid=torch.zeros(2, dtype=torch.int64))
    limit = _lib.gp_loo_max_n(torch.float32)
    with pytest.raises(RuntimeError, match='limit of %d' % limit):
        call(z=torch.zeros(B, limit + 1, f), y=torch.zeros(2, limit + 1))
    with pytest.raises(RuntimeError, match='HIP device'):               # a well-formed call on CPU tensors: no CPU path
        call()
