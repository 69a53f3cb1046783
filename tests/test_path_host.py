"""Pathwise posterior function draws on the host side (no GPU): the two new C entry points (declared, exported, bound, argument
validation without a launch), the Python wrappers' shape checks, the pinned order of the random draws (paths.draw_base), and the
reference tests/path_ref.py itself: its sample moments against the exact posterior (tests/cond_ref.oracle_predict) and, with a zero
base, its identity with the posterior mean of tests/cond_ref.predict."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_ref as R                                               # noqa: E402
import loo_ref as LR                                               # noqa: E402
import matern_ref as MR                                            # noqa: E402
import path_ref as PR                                              # noqa: E402
from meta_learning_pacoh_amd import _lib                           # noqa: E402
from meta_learning_pacoh_amd import paths as PP                    # noqa: E402

EINVAL, ELIMIT, EDTYPE = -1, -2, -3
NEW = ('pacoh_gp_path_fit', 'pacoh_gp_path_eval')
F64 = torch.float64


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
    assert 'Wilson et al. 2020' in header and 'sqrt(noise + j) eps_s' in header
    assert _lib.ABI_VERSION == 14 and lib.pacoh_abi_version() == 14
    for name in ('gp_path_fit', 'gp_path_eval'):
        assert callable(getattr(_lib, name))


def test_argument_validation_without_a_device(lib):
    fake, null = ctypes.c_void_p(4096), None

    def fit(zs=fake, resid=fake, X=fake, info=fake, os_=fake, noise=fake, omega=fake, phase=fake, w=fake, eps=fake, v=fake,
            B=6, P=3, n=16, cap=32, S=5, D=64, f=2, dt=0):
        return lib.pacoh_gp_path_fit(zs, resid, X, info, os_, noise, omega, phase, w, eps, v, B, P, n, cap, S, D, f, dt, null)

    def ev(zs=fake, v=fake, w=fake, info=fake, omega=fake, phase=fake, zt=fake, zt_div=1, mean=fake, mode=_lib.MEAN_VECTOR, ls=fake,
           os_=fake, out=fake, B=6, P=3, n=16, cap=32, S=5, D=64, m=7, f=2, dt=0):
        return lib.pacoh_gp_path_eval(zs, v, w, info, omega, phase, zt, zt_div, mean, mode, ls, os_, out, B, P, n, cap, S, D, m, f, dt, null)

    for name in ('zs', 'resid', 'X', 'info', 'noise', 'omega', 'phase', 'w', 'eps', 'v'):
        assert fit(**{name: null}) == EINVAL, name
    for name in ('zs', 'v', 'w', 'info', 'omega', 'phase', 'zt', 'ls', 'out'):
        assert ev(**{name: null}) == EINVAL, name
    assert ev(mean=null) == EINVAL and ev(mean=null, mode=_lib.MEAN_CONST) == EINVAL and ev(zt_div=0) == EINVAL
    for call in (fit, ev):
        assert call(dt=5) == EDTYPE
        assert call(dt=5, zs=null, n=99, D=8) == EDTYPE             # the dtype is looked at first
        assert call(B=0) == EINVAL and call(P=0) == EINVAL and call(f=0) == EINVAL
        assert call(n=33) == ELIMIT                                 # n > cap
        assert call(n=0) == ELIMIT
        for dt in (0, 1):
            limit = lib.pacoh_gp_cond_max_n(dt)
            assert call(cap=limit + 1, dt=dt) == ELIMIT
            assert call(n=limit + 1, cap=limit + 1, dt=dt) == ELIMIT
        assert call(cap=4096) == ELIMIT
        assert call(f=17) == ELIMIT
        assert call(f=2 | (2 << _lib.KERNEL_SHIFT)) == ELIMIT       # family code 2 is unassigned
        assert call(f=1 | (_lib.KERNEL_COSINE << _lib.KERNEL_SHIFT)) == ELIMIT
        for D in (8, 24, 16400, 0, -16):
            assert call(D=D) == ELIMIT, D
        assert call(S=0) == ELIMIT
    assert ev(m=0) == ELIMIT


def test_wrappers_validate_before_any_call():
    """shapes, dtypes and the limits are refused in Python, before a device pointer is taken"""
    B, P, n, f, S, D, m = 6, 3, 8, 2, 5, 32, 7
    state = _lib.gp_cond_alloc(B, 16, f, torch.float32, 'cpu')
    omega, phase, w, eps = torch.zeros(D, f), torch.zeros(D), torch.zeros(B, S, D), torch.zeros(B, S, n)
    ls, os_, noise = torch.ones(P, f), torch.ones(P), torch.ones(P)

    def fit(**kw):
        a = dict(state=state, n=n, omega=omega, phase=phase, w=w, eps=eps, outputscale=os_, noise=noise, B=B, P=P)
        a.update(kw)
        return _lib.gp_path_fit(**a)

    with pytest.raises(ValueError, match='omega must be'):
        fit(omega=torch.zeros(D, f + 1))
    with pytest.raises(ValueError, match='multiple of 16'):
        fit(omega=torch.zeros(24, f), phase=torch.zeros(24), w=torch.zeros(B, S, 24))
    with pytest.raises(ValueError, match='phase must be'):
        fit(phase=torch.zeros(D + 1))
    with pytest.raises(ValueError, match='w must be'):
        fit(w=torch.zeros(B + 1, S, D))
    with pytest.raises(ValueError, match='eps must be'):
        fit(eps=torch.zeros(B, S, n + 1))
    with pytest.raises(TypeError, match='mixed dtypes'):
        fit(w=w.double())
    with pytest.raises(ValueError, match='noise and outputscale'):
        fit(noise=torch.ones(P + 1))
    with pytest.raises(NotImplementedError, match='cosine'):
        fit(kernel=_lib.KERNEL_COSINE)
    limit = _lib.gp_cond_max_n(torch.float32)
    with pytest.raises(RuntimeError, match='limit of %d' % limit):
        fit(n=17, eps=torch.zeros(B, S, 17))                        # n > capacity
    with pytest.raises(RuntimeError, match='HIP device'):           # a well-formed call on CPU tensors: no CPU path
        fit()

    v, zt = torch.zeros(B, S, n), torch.zeros(B, m, f)

    def ev(**kw):
        a = dict(zs=state[0], n=n, v=v, omega=omega, phase=phase, w=w, info=state[4], z_tst=zt, zt_div=1, mean_tst=None,
                 mean_mode=_lib.MEAN_ZERO, lengthscale=ls, outputscale=os_, B=B, P=P)
        a.update(kw)
        return _lib.gp_path_eval(**a)

    with pytest.raises(ValueError, match='v must be'):
        ev(v=torch.zeros(B, S, n + 1))
    with pytest.raises(ValueError, match='info must be'):
        ev(info=state[4].long())
    with pytest.raises(ValueError, match='z_tst must be'):
        ev(z_tst=zt[:, :, :1])
    with pytest.raises(ValueError, match='lengthscale must be'):
        ev(lengthscale=torch.ones(P, f + 1))
    with pytest.raises(ValueError, match='mean must be'):
        ev(mean_mode=_lib.MEAN_VECTOR, mean_tst=torch.zeros(B, m + 1))
    with pytest.raises(NotImplementedError, match='cosine'):
        ev(kernel=_lib.KERNEL_COSINE)
    with pytest.raises(RuntimeError, match='HIP device'):
        ev()


@pytest.mark.parametrize('kernel,two_nu', [(_lib.KERNEL_RBF, 0), (_lib.KERNEL_MATERN12, 1), (_lib.KERNEL_MATERN32, 3),
                                           (_lib.KERNEL_MATERN52, 5)])
@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_draw_order_is_pinned(kernel, two_nu, dtype):
    """under a seeded CPU generator: randn(D,f); Matern: randn(D, 2 nu); 2 pi rand(D); randn(P,S,D); randn(P,S,n) -- value for value;
    like= keeps omega, phase, w and the old eps columns and draws only the new columns"""
    D, f, P, S, n = 32, 3, 2, 5, 7
    g = torch.Generator().manual_seed(99)
    omega, phase, w, eps = PP.draw_base(kernel, D, f, P, S, n, dtype, 'cpu', generator=g)
    h = torch.Generator().manual_seed(99)
    kw = dict(generator=h, dtype=dtype)
    g0 = torch.randn(D, f, **kw)
    if two_nu:
        c = torch.randn(D, two_nu, **kw)
        g0 = g0 / torch.sqrt((c * c).sum(1) / two_nu).unsqueeze(1)
    assert torch.equal(omega, g0)
    assert torch.equal(phase, 2.0 * math.pi * torch.rand(D, **kw))
    assert torch.equal(w, torch.randn(P, S, D, **kw))
    assert torch.equal(eps, torch.randn(P, S, n, **kw))
    for t in (omega, phase, w, eps):
        assert t.dtype == dtype
    assert float(phase.min()) >= 0.0 and float(phase.max()) < 2.0 * math.pi + 1e-6
    # like=: three more points
    o2, p2, w2, e2 = PP.draw_base(kernel, D, f, P, S, n + 3, dtype, 'cpu', generator=g, like=(omega, phase, w, eps))
    assert o2 is omega and p2 is phase and w2 is w
    assert torch.equal(e2[:, :, :n], eps) and torch.equal(e2[:, :, n:], torch.randn(P, S, 3, **kw))
    same = PP.draw_base(kernel, D, f, P, S, n, dtype, 'cpu', generator=g, like=(omega, phase, w, eps))
    assert torch.equal(same[3], eps)
    assert torch.equal(torch.randn(4, **kw), torch.randn(4, generator=g, dtype=dtype))      # ... and drew nothing for it
    with pytest.raises(ValueError, match='like='):
        PP.draw_base(kernel, D, f, P, S, n - 1, dtype, 'cpu', generator=g, like=(omega, phase, w, eps))
    with pytest.raises(ValueError, match='like='):
        PP.draw_base(kernel, D, f, P, S + 1, n, dtype, 'cpu', generator=g, like=(omega, phase, w, eps))


def test_draw_base_refuses_the_cosine_family_and_checks_a_given_base():
    with pytest.raises(NotImplementedError):
        PP.draw_base(_lib.KERNEL_COSINE, 32, 1, 1, 1, 4, F64)
    base = PP.draw_base(_lib.KERNEL_RBF, 32, 2, 3, 4, 5, F64, generator=torch.Generator().manual_seed(1))
    assert all(a is b or torch.equal(a, b) for a, b in zip(PP.check_base(base, 32, 2, 3, 4, 5, F64, 'cpu'), base))
    with pytest.raises(ValueError, match='eps must be'):
        PP.check_base(base, 32, 2, 3, 4, 6, F64, 'cpu')
    with pytest.raises(ValueError, match='w must be'):
        PP.check_base(base, 32, 2, 3, 5, 5, F64, 'cpu')
    with pytest.raises(ValueError, match='omega must be'):
        PP.check_base(base, 32, 2, 3, 4, 5, torch.float32, 'cpu')
    with pytest.raises(ValueError, match='base must be'):
        PP.check_base(base[:3], 32, 2, 3, 4, 5, F64, 'cpu')


def _latent_cov(z, mean, y, zt, mt, ls, os_, noise, fam):
    """the exact posterior of the LATENT function at zt from the oracle's joint predictive -> mu [m], cov [m,m]"""
    saved = R.O.gram_family
    if fam in LR.NU:
        R.O.gram_family = MR.gram_family_for(LR.NU[fam])
    try:
        mu, cov = R.O.gp_predict(z, mean, y, zt, mt, ls.reshape(1, -1), float(os_), float(noise), kernel='rbf')
    finally:
        R.O.gram_family = saved
    return mu.reshape(-1), cov - float(noise) * torch.eye(zt.shape[0], dtype=F64)


@pytest.mark.parametrize('fam', PR.FAMILIES)
def test_reference_draws_have_the_posterior_moments(fam):
    """fp64, f = 2, n = 20, m = 30, D = 2048, S = 20 000: the sample mean within 0.05 predictive std of the oracle's mean, the sample
    covariance within 0.15 of the largest latent posterior variance (measured with these seeds: <= 0.027 and <= 0.054; the bounds are those of the standard errors at S = 20 000 plus the RFF prior's
    kernel error at D = 2048, 0.065 - 0.072 of the outputscale)"""
    f, n, m, D, S = 2, 20, 30, 2048, 20000
    z, mean, y, ls, os_, noise = LR.make_problem(n, f, fam, seed=31)
    g = torch.Generator().manual_seed(5)
    zt = torch.randn(m, f, generator=g, dtype=F64) * float(z.std())
    mt = 0.3 * torch.randn(m, generator=g, dtype=F64)
    mu, var = R.oracle_predict(z, mean, y, zt, mt, ls, os_, noise, family=fam)
    mu_l, cov_l = _latent_cov(z, mean, y, zt, mt, ls, os_, noise, fam)
    assert float((mu_l - mu).abs().max()) <= 1e-12
    omega, phase = PR.frequencies(fam, D, f, seed=17)
    X, _ = R.direct(z, mean, y, ls, os_, noise, family=fam)
    s1, s2 = torch.zeros(m, dtype=F64), torch.zeros(m, m, dtype=F64)
    for _ in range(4):                                               # 4 x 5000 draws: the base of a chunk is 80 MB
        w = torch.randn(S // 4, D, generator=g, dtype=F64)
        eps = torch.randn(S // 4, n, generator=g, dtype=F64)
        fs = PR.paths(X, z / ls, y - mean, zt, mt, ls, os_, noise, 0.0, fam, omega, phase, w, eps)
        s1 += fs.sum(0)
        s2 += fs.T @ fs
    sm = s1 / S
    sc = (s2 - S * torch.outer(sm, sm)) / (S - 1)
    e_mean = float(((sm - mu).abs() / var.sqrt()).max())
    e_cov = float((sc - cov_l).abs().max() / torch.diagonal(cov_l).max())
    print('%s: sample mean off by %.3f predictive std, sample covariance by %.3f of the largest latent variance' % (fam, e_mean, e_cov))
    assert e_mean <= 0.05 and e_cov <= 0.15, (e_mean, e_cov)


@pytest.mark.parametrize('fam', PR.FAMILIES)
@pytest.mark.parametrize('n,f', [(1, 1), (9, 3), (65, 16)])
def test_zero_base_is_the_posterior_mean_and_the_two_forms_agree(fam, n, f):
    m, D, S = 11, 64, 3
    z, mean, y, ls, os_, noise = LR.make_problem(n, f, fam, seed=3 * n + f)
    g = torch.Generator().manual_seed(n)
    zt = torch.randn(m, f, generator=g, dtype=F64)
    mt = 0.3 * torch.randn(m, generator=g, dtype=F64)
    omega, phase = PR.frequencies(fam, D, f, seed=n + 1)
    X, alpha = R.direct(z, mean, y, ls, os_, noise, family=fam)
    mu, _ = R.predict(X, alpha, z, zt, mt, ls, os_, noise, family=fam)
    zero = PR.paths(X, z / ls, y - mean, zt, mt, ls, os_, noise, 0.0, fam, omega, phase, torch.zeros(S, D, dtype=F64),
                    torch.zeros(S, n, dtype=F64))
    assert zero.shape == (S, m) and float((zero - mu).abs().max()) <= 1e-12
    w, eps = torch.randn(S, D, generator=g, dtype=F64), torch.randn(S, n, generator=g, dtype=F64)
    a = PR.paths(X, z / ls, y - mean, zt, mt, ls, os_, noise, 0.0, fam, omega, phase, w, eps)
    b = PR.paths_direct(z / ls, y - mean, zt, mt, ls, os_, noise, 0.0, fam, omega, phase, w, eps)
    assert float((a - b).abs().max()) / math.sqrt(os_) <= 1e-11


def test_public_interface():
    import meta_learning_pacoh_amd as M
    from meta_learning_pacoh_amd.conditioned import ConditionedGP
    from meta_learning_pacoh_amd.engine import GPEngine
    assert M.PosteriorPaths is PP.PosteriorPaths
    assert callable(ConditionedGP.sample_paths)
    for name in ('cond_paths', 'cond_paths_eval'):
        assert callable(getattr(GPEngine, name))
    assert isinstance(PP.PosteriorPaths.base, property) and callable(PP.PosteriorPaths.__call__)
    assert 'sample_paths' in sys.modules[ConditionedGP.__module__].__doc__
