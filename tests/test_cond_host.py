"""The conditioned GP posterior on the host side (no GPU): the four new C entry points (declared, exported, bound, argument validation
without a launch), the identities of tests/cond_ref.py in fp64 (incremental against direct, direct against the oracle's predictive),
and the public interface (RegressionModelMetaLearned.condition, ConditionedGP)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_ref as R                                               # noqa: E402
import loo_ref as LR                                               # noqa: E402
from meta_learning_pacoh_amd import _lib                           # noqa: E402

EINVAL, ELIMIT, EDTYPE = -1, -2, -3
NEW = ('pacoh_gp_cond_max_n', 'pacoh_gp_condition', 'pacoh_gp_cond_predict', 'pacoh_gp_cond_append')


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
    assert 'get_fantasy_model' in header
    assert _lib.ABI_VERSION == 14 and lib.pacoh_abi_version() == 14
    for name in ('gp_cond_max_n', 'gp_condition', 'gp_cond_predict', 'gp_cond_append'):
        assert callable(getattr(_lib, name))


def test_size_limit_query(lib):
    for dt, tdt in ((0, torch.float32), (1, torch.float64)):
        assert lib.pacoh_gp_cond_max_n(dt) == lib.pacoh_gp_loo_max_n(dt)
        assert _lib.gp_cond_max_n(tdt) == lib.pacoh_gp_loo_max_n(dt)
    assert lib.pacoh_gp_cond_max_n(5) == EDTYPE


def test_argument_validation_without_a_device(lib):
    fake, null = ctypes.c_void_p(4096), None

    def condition(z=fake, z_div=1, mean=fake, mode=_lib.MEAN_VECTOR, y=fake, y_div=3, ls=fake, os_=fake, noise=fake, zs=fake, resid=fake,
                  X=fake, alpha=fake, info=fake, B=6, P=3, n=16, cap=32, f=2, dt=0):
        return lib.pacoh_gp_condition(z, z_div, mean, mode, y, y_div, ls, os_, noise, zs, resid, X, alpha, info, B, P, n, cap, f, dt, null)

    def predict(zs=fake, X=fake, alpha=fake, info=fake, zt=fake, zt_div=1, mean=fake, mode=_lib.MEAN_VECTOR, ls=fake, os_=fake, noise=fake,
                mu=fake, var=fake, B=6, P=3, n=16, cap=32, m=5, f=2, dt=0):
        return lib.pacoh_gp_cond_predict(zs, X, alpha, info, zt, zt_div, mean, mode, ls, os_, noise, mu, var, B, P, n, cap, m, f, dt, null)

    def append(zs=fake, resid=fake, X=fake, alpha=fake, info=fake, zn=fake, zn_div=1, mean=fake, mode=_lib.MEAN_VECTOR, yn=fake, yn_div=3,
               ls=fake, os_=fake, noise=fake, fail=fake, B=6, P=3, n=16, cap=32, k=2, f=2, dt=0):
        return lib.pacoh_gp_cond_append(zs, resid, X, alpha, info, zn, zn_div, mean, mode, yn, yn_div, ls, os_, noise, fail,
                                        B, P, n, cap, k, f, dt, null)

    for name in ('z', 'y', 'ls', 'noise', 'zs', 'resid', 'X', 'alpha', 'info'):
        assert condition(**{name: null}) == EINVAL, name
    for name in ('zs', 'X', 'alpha', 'info', 'zt', 'ls', 'noise', 'mu'):
        assert predict(**{name: null}) == EINVAL, name
    for name in ('zs', 'resid', 'X', 'alpha', 'info', 'zn', 'yn', 'ls', 'noise', 'fail'):
        assert append(**{name: null}) == EINVAL, name
    for call in (condition, predict, append):
        assert call(mean=null) == EINVAL and call(mean=null, mode=_lib.MEAN_CONST) == EINVAL
        assert call(B=0) == EINVAL and call(P=0) == EINVAL and call(n=0) == EINVAL and call(f=0) == EINVAL
        assert call(n=33) == ELIMIT                                 # n > cap
        for dt in (0, 1):
            limit = lib.pacoh_gp_cond_max_n(dt)
            assert call(cap=limit + 1, dt=dt) == ELIMIT
            assert call(n=limit + 1, cap=limit + 1, dt=dt) == ELIMIT
        assert call(cap=4096) == ELIMIT
        assert call(f=17) == ELIMIT
        assert call(f=2 | (2 << _lib.KERNEL_SHIFT)) == ELIMIT       # family code 2 is unassigned
        assert call(dt=5) == EDTYPE
    assert condition(z_div=0) == EINVAL and condition(y_div=0) == EINVAL
    assert predict(zt_div=0) == EINVAL and predict(m=0) == EINVAL
    assert append(zn_div=0) == EINVAL and append(yn_div=0) == EINVAL and append(k=0) == EINVAL
    assert append(n=31, k=2) == ELIMIT and append(n=30, k=3) == ELIMIT     # n + k > cap


def test_wrappers_validate_before_any_call():
    """shapes, dtypes and the size limit are refused in Python, before a device pointer is taken"""
    B, P, n, f = 6, 3, 8, 2
    z, y = torch.zeros(B, n, f), torch.zeros(2, n)
    ls, os_, noise = torch.ones(P, f), torch.ones(P), torch.ones(P)
    ok = dict(z=z, z_div=1, mean=None, mean_mode=_lib.MEAN_ZERO, y=y, y_div=P, lengthscale=ls, outputscale=os_, noise=noise, B=B, P=P,
              capacity=16)

    def call(**kw):
        return _lib.gp_condition(**dict(ok, **kw))

    with pytest.raises(ValueError, match='z must be'):
        call(z=z[:4])
    with pytest.raises(ValueError, match='y must be'):
        call(y=torch.zeros(2, n + 1))
    with pytest.raises(ValueError, match='multiple of P'):
        call(B=5)
    with pytest.raises(ValueError, match='lengthscale'):
        call(lengthscale=torch.ones(P, f + 1))
    with pytest.raises(ValueError, match='mean must be'):
        call(mean_mode=_lib.MEAN_VECTOR, mean=torch.zeros(B, n - 1))
    limit = _lib.gp_cond_max_n(torch.float32)
    with pytest.raises(RuntimeError, match='limit of %d' % limit):
        call(capacity=limit + 1)
    with pytest.raises(RuntimeError, match='limit of %d' % limit):
        call(capacity=4)                                            # n > capacity
    with pytest.raises(RuntimeError, match='HIP device'):           # a well-formed call on CPU tensors: no CPU path
        call()
    state = _lib.gp_cond_alloc(B, 16, f, torch.float32, 'cpu')
    zt = torch.zeros(B, 5, f)
    with pytest.raises(ValueError, match='z_tst must be'):
        _lib.gp_cond_predict(state, n, zt[:, :, :1], 1, None, _lib.MEAN_ZERO, ls, os_, noise, B, P)
    with pytest.raises(ValueError, match='info must be'):
        _lib.gp_cond_predict(state[:4] + (state[4].long(),), n, zt, 1, None, _lib.MEAN_ZERO, ls, os_, noise, B, P)
    with pytest.raises(RuntimeError, match='HIP device'):
        _lib.gp_cond_predict(state, n, zt, 1, None, _lib.MEAN_ZERO, ls, os_, noise, B, P)
    with pytest.raises(ValueError, match='y_new must be'):
        _lib.gp_cond_append(state, n, zt, 1, None, _lib.MEAN_ZERO, torch.zeros(2, 4), P, ls, os_, noise, B, P)
    with pytest.raises(RuntimeError, match='limit of %d' % limit):
        _lib.gp_cond_append(state, 12, zt, 1, None, _lib.MEAN_ZERO, torch.zeros(2, 5), P, ls, os_, noise, B, P)     # 12 + 5 > 16
    with pytest.raises(RuntimeError, match='HIP device'):
        _lib.gp_cond_append(state, n, zt, 1, None, _lib.MEAN_ZERO, torch.zeros(2, 5), P, ls, os_, noise, B, P)


GRID = [(n, f, fam) for n in (1, 2, 9, 65, 128) for f in (1, 3, 16) for fam in R.FAMILIES if fam != 'cos' or f == 1]


def _test_points(pb, m, seed):
    z = pb[0]
    g = torch.Generator().manual_seed(seed)
    if z.shape[1] == 1 and float(z.min()) >= 0.0 and float(z.max()) <= 0.9:      # (the cosine problems: stay within half a period)
        zt = torch.rand(m, 1, generator=g, dtype=torch.float64) * 0.9
    else:
        zt = torch.randn(m, z.shape[1], generator=g, dtype=torch.float64) * float(z.std() if z.numel() > 1 else 1.0)
    return zt, 0.3 * torch.randn(m, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('n,f,fam', GRID, ids=['n%d-f%d-%s' % c for c in GRID])
def test_direct_form_is_the_oracles_predictive(n, f, fam):
    pb = LR.make_problem(n, f, fam, seed=100 * n + f)
    z, mean, y, ls, os_, noise = pb
    zt, mt = _test_points(pb, 7, seed=n + f)
    ref = R.oracle_predict(z, mean, y, zt, mt, ls, os_, noise, family=fam)
    X, alpha = R.direct(z, mean, y, ls, os_, noise, family=fam)
    mu, var = R.predict(X, alpha, z, zt, mt, ls, os_, noise, family=fam)
    assert max(R.errors(mu, var, ref)) <= 1e-10


@pytest.mark.parametrize('n0,k,f,fam', [(1, 1, 1, 'rbf'), (1, 7, 2, 'm32'), (8, 1, 4, 'm52'), (5, 20, 1, 'cos'), (30, 35, 5, 'm12'),
                                        (100, 28, 16, 'rbf')])
def test_incremental_form_is_the_direct_form(n0, k, f, fam):
    pb = LR.make_problem(n0 + k, f, fam, seed=7 * n0 + k)
    z, mean, y, ls, os_, noise = pb
    zt, mt = _test_points(pb, 7, seed=n0)
    X0, a0 = R.direct(z[:n0], mean[:n0], y[:n0], ls, os_, noise, family=fam)
    X1, a1, z1, r1 = R.append(X0, a0, z[:n0], (y - mean)[:n0], z[n0:], (y - mean)[n0:], ls, os_, noise, family=fam)
    X, alpha = R.direct(z, mean, y, ls, os_, noise, family=fam)
    assert torch.equal(z1, z) and torch.equal(r1, y - mean)
    assert R.rel_max(X1, X) <= 1e-10 and R.rel_max(a1, alpha) <= 1e-10
    ref = R.predict(X, alpha, z, zt, mt, ls, os_, noise, family=fam)
    assert max(R.errors(*R.predict(X1, a1, z1, zt, mt, ls, os_, noise, family=fam), ref)) <= 1e-10
    with pytest.raises(ValueError):                                  # a negative diagonal: the update refuses
        R.append(X0, a0, z[:n0], (y - mean)[:n0], z[n0:], (y - mean)[n0:], ls, os_, -2.0 * os_, family=fam)


def test_learners_have_the_condition_interface():
    import meta_learning_pacoh_amd as M
    from meta_learning_pacoh_amd import GPR_meta_mll, GPR_meta_svgd, GPR_meta_vi
    from meta_learning_pacoh_amd.abstract import RegressionModelMetaLearned
    from meta_learning_pacoh_amd.conditioned import ConditionedGP
    from meta_learning_pacoh_amd.engine import GPEngine
    assert M.ConditionedGP is ConditionedGP
    assert callable(RegressionModelMetaLearned.condition)
    for cls in (GPR_meta_mll.GPRegressionMetaLearned, GPR_meta_svgd.GPRegressionMetaLearnedSVGD, GPR_meta_vi.GPRegressionMetaLearnedVI):
        assert cls.condition is RegressionModelMetaLearned.condition
    for name in ('predict', 'confidence_intervals', 'append'):
        assert callable(getattr(ConditionedGP, name))
    assert isinstance(ConditionedGP.n, property) and isinstance(ConditionedGP.capacity, property)
    for name in ('condition', 'cond_predict', 'cond_append'):
        assert callable(getattr(GPEngine, name))
    assert 'Out of scope' in sys.modules[ConditionedGP.__module__].__doc__
