"""Analytic acquisition on the posterior predictive, on the host side (no GPU): the rule as pure torch
(meta_learning_pacoh_amd/acquisition.py: the specification tests/test_gpu_acq.py holds the kernel to) against quadrature and closed
forms in fp64, the unit conversions, the two C entry points (declared, exported, bound; every refusal without a launch; the workspace
query), and the argument errors of ConditionedGP.acquire / .acquisition / GaussianPredictive.acquisition on a stub engine."""
import ctypes
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from meta_learning_pacoh_amd import _lib                           # noqa: E402
from meta_learning_pacoh_amd import acquisition as A               # noqa: E402
from meta_learning_pacoh_amd.conditioned import ConditionedGP      # noqa: E402
from meta_learning_pacoh_amd.distributions import GaussianPredictive   # noqa: E402

EINVAL, ELIMIT, EDTYPE = -1, -2, -3
NEW = ('pacoh_mixture_acq_workspace_bytes', 'pacoh_mixture_acq')
F64 = torch.float64
NAN = float('nan')


def moments(T, P, m, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.5 * torch.randn(T, P, m, generator=g, dtype=F64), 1e-3 + (2.0 - 1e-3) * torch.rand(T, P, m, generator=g, dtype=F64)


# ------------------------------------------------------------------------------------------------------------ the spec in fp64
def quadrature_ei(mu, v, best, xi, sign, points=200001, width=12.0):
    """trapezoid rule of  int max(sign (y - best) - xi, 0) N(y; mu, v) dy  over mu +- width sd"""
    sd = math.sqrt(v)
    y = torch.linspace(mu - width * sd, mu + width * sd, points, dtype=F64)
    f = torch.clamp(sign * (y - best) - xi, min=0.0) * torch.exp(-0.5 * ((y - mu) / sd) ** 2) / (sd * math.sqrt(2.0 * math.pi))
    return float(torch.trapezoid(f, y))


@pytest.mark.parametrize('sign', [1, -1])
def test_single_gaussian_ei_is_the_integral_and_pi_the_tail(sign):
    mu, var = moments(1, 1, 20, seed=3)
    best, xi = 0.4, 0.05
    ei = A.mixture_acquisition(mu, var, 'ei', best=best, xi=xi, sign=sign)[0]
    pi = A.mixture_acquisition(mu, var, 'pi', best=best, xi=xi, sign=sign)[0]
    sd = torch.sqrt(var[0, 0])
    worst = 0.0
    for j in range(20):
        q = quadrature_ei(float(mu[0, 0, j]), float(var[0, 0, j]), best, xi, sign)
        worst = max(worst, abs(float(ei[j]) - q) / float(sd[j]))
    print('sign %+d: worst |ei - quadrature| / sd = %.2e' % (sign, worst))
    assert worst <= 1e-6
    cdf = torch.distributions.Normal(mu[0, 0], sd).cdf
    tail = 1.0 - cdf(torch.full_like(sd, best + xi)) if sign == 1 else cdf(torch.full_like(sd, best - xi))
    assert float((pi - tail).abs().max()) <= 1e-12


@pytest.mark.parametrize('kind', ['ei', 'pi'])
def test_mixture_improvement_is_the_mean_of_the_rows(kind):
    mu, var = moments(3, 7, 31, seed=5)
    whole = A.mixture_acquisition(mu, var, kind, best=0.9, xi=0.01)
    rows = torch.stack([A.mixture_acquisition(mu[:, p:p + 1], var[:, p:p + 1], kind, best=0.9, xi=0.01) for p in range(7)])
    assert float((whole - rows.mean(0)).abs().max()) <= 1e-14


@pytest.mark.parametrize('P', [1, 2, 20])
def test_moments_are_the_predictive_objects(P):
    mu, var = moments(1, P, 40, seed=7 + P)
    dist = GaussianPredictive(mu[0], var[0], None, 0, 1, True)
    mean = A.mixture_acquisition(mu, var, 'mean')[0]
    std = A.mixture_acquisition(mu, var, 'std')[0]
    assert float((mean - dist.mean).abs().max()) <= 1e-12 and float((std - dist.stddev).abs().max()) <= 1e-12
    for sign in (1, -1):
        ucb = A.mixture_acquisition(mu, var, 'ucb', beta=1.7, sign=sign)[0]
        assert torch.equal(ucb, mean + (sign * 1.7) * std)
    if P == 1:
        assert torch.equal(mean, mu[0, 0]) and torch.equal(std, torch.sqrt(var[0, 0]))


@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_maximise_is_minimise_of_the_mirrored_problem_bit_for_bit(dtype):
    mu, var = (t.to(dtype) for t in moments(2, 5, 33, seed=11))
    for kind in ('ei', 'pi', 'std'):
        a = A.mixture_acquisition(mu, var, kind, best=0.7, xi=0.02, sign=1)
        b = A.mixture_acquisition(-mu, var, kind, best=-0.7, xi=0.02, sign=-1)
        assert torch.equal(a, b), kind
    for kind in ('mean', 'ucb'):                 # the mirrored objective itself: the values change sign, nothing else
        a = A.mixture_acquisition(mu, var, kind, beta=1.3, sign=1)
        b = A.mixture_acquisition(-mu, var, kind, beta=1.3, sign=-1)
        assert torch.equal(a, -b), kind


def test_noise_is_taken_off_the_variance_and_clamped():
    mu, var = moments(2, 3, 17, seed=13)
    noise = torch.tensor([0.0005, 0.5, 3.0], dtype=F64)          # the last row's latent variance is negative everywhere: 0
    latent = torch.clamp(var - noise.reshape(1, 3, 1), min=0.0)
    assert float(latent[:, 2].max()) == 0.0 and float(latent[:, 1].min()) == 0.0 and float(latent[:, 1].max()) > 0.0
    for kind in A.KINDS:
        assert torch.equal(A.mixture_acquisition(mu, var, kind, best=0.2, noise=noise), A.mixture_acquisition(mu, latent, kind, best=0.2)), kind


def test_zero_variance_limits():
    mu = torch.tensor([[[0.5, 1.0, 1.5, 1.0]]], dtype=F64)
    var = torch.zeros_like(mu)
    assert A.mixture_acquisition(mu, var, 'ei', best=1.0)[0].tolist() == [0.0, 0.0, 0.5, 0.0]
    assert A.mixture_acquisition(mu, var, 'pi', best=1.0)[0].tolist() == [0.0, 0.0, 1.0, 0.0]
    assert A.mixture_acquisition(mu, var, 'ei', best=1.0, sign=-1)[0].tolist() == [0.5, 0.0, 0.0, 0.0]
    assert A.mixture_acquisition(mu, var, 'pi', best=1.0, sign=-1, xi=0.25)[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert A.mixture_acquisition(mu, var, 'std')[0].tolist() == [0.0] * 4
    # one row with and one without variance: the mean of the two rules
    mu2, var2 = torch.tensor([[[2.0], [2.0]]], dtype=F64), torch.tensor([[[0.0], [1.0]]], dtype=F64)
    one = A.mixture_acquisition(mu2[:, 1:], var2[:, 1:], 'ei', best=1.0)
    assert torch.equal(A.mixture_acquisition(mu2, var2, 'ei', best=1.0), (1.0 + one) / 2.0)


@pytest.mark.parametrize('kind', A.KINDS)
def test_a_nan_row_makes_the_point_nan(kind):
    mu, var = moments(2, 4, 9, seed=17)
    clean = A.mixture_acquisition(mu, var, kind, best=0.3)
    mu[1, 2, 4], var[1, 2, 4] = NAN, NAN
    mu[0, 0, 0] = NAN                                           # mu alone: every kind but 'std' of one row reads it ...
    var[0, 3, 8] = NAN                                          # ... var alone: every kind but 'mean' reads it
    out = A.mixture_acquisition(mu, var, kind, best=0.3)
    want = torch.zeros(2, 9, dtype=torch.bool)
    want[1, 4] = True
    want[0, 0] = True                                           # ('std' of a mixture reads mu through the spread of the means)
    want[0, 8] = kind != 'mean'
    assert torch.equal(torch.isnan(out), want)
    assert torch.equal(out[~want], clean[~want])


@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_far_tail_is_exactly_zero_never_negative(dtype):
    var = torch.full((1, 3, 64), 0.04, dtype=dtype)
    z = torch.linspace(-50.0, -5.0, 64, dtype=dtype)
    mu = (1.0 + 0.2 * z).reshape(1, 1, 64).expand(1, 3, 64).contiguous()
    ei = A.mixture_acquisition(mu, var, 'ei', best=1.0)[0]
    assert float(ei.min()) >= 0.0 and float(ei[0]) == 0.0 and not bool(torch.signbit(ei).any())
    assert float(A.mixture_acquisition(mu, var, 'pi', best=1.0)[0, 0]) == 0.0


def test_spec_refuses_bad_arguments():
    mu, var = moments(1, 2, 3, seed=1)
    with pytest.raises(ValueError, match='kind must be'):
        A.mixture_acquisition(mu, var, 'lcb')
    with pytest.raises(ValueError, match='sign must be'):
        A.mixture_acquisition(mu, var, 'ei', sign=0)
    with pytest.raises(ValueError, match=r'\[T,P,m\]'):
        A.mixture_acquisition(mu[0], var[0], 'ei')
    with pytest.raises(ValueError, match='noise must be'):
        A.mixture_acquisition(mu, var, 'ei', noise=torch.zeros(3, dtype=F64))


# ------------------------------------------------------------------------------------------------------------ unit conversions
def test_unit_conversions():
    y_mean, y_std = -3.5, 2.25
    best_n, xi_n = A.to_normalised(1.0, 0.5, y_mean, y_std)
    assert best_n == (1.0 - y_mean) / y_std and xi_n == 0.5 / y_std
    assert abs(best_n * y_std + y_mean - 1.0) <= 1e-15
    v = torch.tensor([0.0, 0.25, 1.5], dtype=F64)
    for kind in ('mean', 'ucb'):
        assert torch.equal(A.to_original(v, kind, y_mean, y_std), v * y_std + y_mean)
    for kind in ('std', 'ei'):
        assert torch.equal(A.to_original(v, kind, y_mean, y_std), v * y_std)
    assert torch.equal(A.to_original(v, 'pi', y_mean, y_std), v)
    with pytest.raises(ValueError):
        A.to_original(v, 'lcb', y_mean, y_std)
    # the conversions commute with the rule: scoring y = y_mean + y_std y_n in original units is scoring y_n with the converted scalars
    mu, var = moments(1, 3, 11, seed=19)
    mu_o, var_o = mu * y_std + y_mean, var * y_std ** 2
    for kind in A.KINDS:
        direct = A.mixture_acquisition(mu_o, var_o, kind, best=1.0, xi=0.5, beta=1.5)
        back = A.to_original(A.mixture_acquisition(mu, var, kind, best=best_n, xi=xi_n, beta=1.5), kind, y_mean, y_std)
        assert float((direct - back).abs().max()) <= 1e-12, kind


# ------------------------------------------------------------------------------------------------------------ the C entry points
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
    assert 'the reference has no acquisition function' in header
    for code, kind in enumerate(A.KINDS):
        assert '#define PACOH_ACQ_%s %d' % (kind.upper(), code) in header
    assert _lib.ABI_VERSION == 14 and lib.pacoh_abi_version() == 14
    assert callable(_lib.mixture_acq)


def test_argument_validation_without_a_device(lib):
    fake, null = ctypes.c_void_p(4096), None

    def acq(mu=fake, var=fake, noise=fake, mask=fake, values=fake, bv=fake, bi=fake, ws=fake, ws_bytes=None, kind=0, best=0.1, xi=0.0,
            beta=2.0, sign=1, T=3, P=4, m=300, idx_base=0, largest=1, first=1, strips=0, dt=0):
        if ws_bytes is None:
            ws_bytes = max(1, lib.pacoh_mixture_acq_workspace_bytes(T, m, strips, dt))
        return lib.pacoh_mixture_acq(mu, var, noise, mask, values, bv, bi, ws, ws_bytes, kind, best, xi, beta, sign, T, P, m, idx_base,
                                     largest, first, strips, dt, null)

    for name in ('mu', 'var', 'bv', 'bi', 'ws'):
        assert acq(**{name: null}) == EINVAL, name
    for kind in (-1, 5, 99):
        assert acq(kind=kind) == EINVAL
    for sign in (0, 2, -2):
        assert acq(sign=sign) == EINVAL
    assert acq(strips=-1, ws_bytes=1 << 20) == EINVAL and acq(idx_base=-1) == EINVAL
    for bad in (-1, 2):
        assert acq(largest=bad) == EINVAL and acq(first=bad) == EINVAL
    assert acq(T=0) == EINVAL and acq(P=0) == EINVAL and acq(m=0) == EINVAL and acq(m=-5) == EINVAL
    assert acq(T=65536, ws_bytes=1 << 24) == ELIMIT and acq(T=1 << 20, ws_bytes=1 << 26) == ELIMIT
    assert acq(dt=5) == EDTYPE
    assert acq(dt=5, mu=null, kind=9, strips=-1, T=1 << 20) == EDTYPE        # the dtype is looked at first
    for dt in (0, 1):
        for strips in (0, 1, 3):
            need = lib.pacoh_mixture_acq_workspace_bytes(3, 1000, strips, dt)
            assert need > 0
            assert acq(m=1000, strips=strips, dt=dt, ws_bytes=need - 1) == EINVAL
            assert acq(m=1000, strips=strips, dt=dt, ws_bytes=0) == EINVAL


def test_workspace_query(lib):
    q = lib.pacoh_mixture_acq_workspace_bytes
    for dt, size in ((0, 4), (1, 8)):
        assert q(1, 1, 0, dt) == 8 + size and q(1, 1, 1, dt) == 8 + size
        # a forced strip count, clamped to the number of 256-point blocks: exactly one (index, value) pair per (task, strip)
        assert q(3, 1000, 2, dt) == 3 * 2 * (8 + size)
        assert q(3, 1000, 9, dt) == 3 * 4 * (8 + size)
        assert q(3, 1000, 0, dt) == 3 * 4 * (8 + size)
        for strips in (0, 1, 2, 7):
            for m in (1, 257, 2373, 100000, 10 ** 7):
                last = 0
                for T in (1, 2, 3, 20, 64, 1000, 1024, 1025, 5000, 65535):
                    now = q(T, m, strips, dt)
                    assert now >= last and now > 0, (T, m, strips)
                    last = now
            for T in (1, 3, 700, 65535):
                last = 0
                for m in (1, 256, 257, 1000, 10 ** 5, 10 ** 7, 2 ** 31 - 1):
                    now = q(T, m, strips, dt)
                    assert now >= last and now > 0, (T, m, strips)
                    last = now
        for m in (1, 257, 2373, 100000):
            last = 0
            for strips in (1, 2, 3, 37, 38, 39, 5000):
                now = q(3, m, strips, dt)
                assert now >= last and now > 0, (m, strips)
                last = now
    assert q(1, 1, 0, 5) == 0 and q(0, 1, 0, 0) == 0 and q(65536, 1, 0, 0) == 0 and q(1, 0, 0, 0) == 0 and q(1, 1, -1, 0) == 0


def test_wrapper_validates_before_any_call():
    T, P, m = 2, 3, 7
    mu, var = torch.zeros(T * P, m), torch.ones(T * P, m)

    def acq(**kw):
        a = dict(mu=mu, var=var, T=T, P=P, kind='ei', best=0.0, xi=0.0, beta=2.0, sign=1)
        a.update(kw)
        return _lib.mixture_acq(**a)

    with pytest.raises(ValueError, match='kind must be'):
        acq(kind='lcb')
    with pytest.raises(ValueError, match='mu and var must both be'):
        acq(var=var[:, :5])
    with pytest.raises(ValueError, match='mu and var must both be'):
        acq(P=4)
    with pytest.raises(ValueError, match='one dtype'):
        acq(var=var.double())
    with pytest.raises(ValueError, match='sign must be'):
        acq(sign=0)
    with pytest.raises(ValueError, match='noise must be'):
        acq(noise=torch.zeros(P + 1))
    with pytest.raises(ValueError, match='noise must be'):
        acq(noise=torch.zeros(P, dtype=F64))
    with pytest.raises(ValueError, match='mask must be'):
        acq(mask=torch.ones(m + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='mask must be'):
        acq(mask=torch.ones(m))
    with pytest.raises(ValueError, match='must not be negative'):
        acq(strips=-1)
    with pytest.raises(ValueError, match='must not be negative'):
        acq(idx_base=-1)
    with pytest.raises(ValueError, match='first=False needs'):
        acq(first=False)
    with pytest.raises(ValueError, match='best_pair must be'):
        acq(first=False, best_pair=(torch.zeros(T), torch.zeros(T)))
    with pytest.raises(RuntimeError, match='HIP device'):           # a well-formed call on CPU tensors: no CPU path
        acq()


# ------------------------------------------------------------------------------------------------------------ the public objects
class StubEngine:
    """records what ConditionedGP hands to GPEngine.cond_acq and answers with fixed normalised values"""

    def __init__(self):
        self.calls = []

    def cond_acq(self, st, tst_x, kind, best_n, xi_n, beta, sign, latent, mask, chunk, want_values):
        self.calls.append(dict(m=tst_x.shape[0], kind=kind, best_n=best_n, xi_n=xi_n, beta=beta, sign=sign, latent=latent, mask=mask,
                               chunk=chunk, want_values=want_values))
        values = torch.arange(tst_x.shape[0], dtype=torch.float32) if want_values else None
        return torch.tensor([0.5]), torch.tensor([2]), values


def stub_cond():
    eng = StubEngine()
    st = SimpleNamespace(theta=torch.zeros(3, 4), n=4, cap=8, ctx_y=torch.tensor([0.25, -1.5, 2.0, 0.0, 99.0, 99.0, 99.0, 99.0]))
    return ConditionedGP(eng, st, True, [1.0], [2.0], [10.0], [4.0], torch.float32, 'cpu'), eng


def test_conditioned_gp_hands_normalised_scalars_to_the_engine():
    cond, eng = stub_cond()
    x = np.linspace(-1.0, 1.0, 5).reshape(-1, 1)
    idx, val = cond.acquire('ei', x, best_f=12.0, xi=0.4, mask=[True, False, True, True, True], chunk=3)
    c = eng.calls[-1]
    assert (c['m'], c['kind'], c['sign'], c['latent'], c['chunk'], c['want_values']) == (5, 'ei', 1, True, 3, False)
    assert c['best_n'] == (12.0 - 10.0) / 4.0 and c['xi_n'] == 0.4 / 4.0 and c['beta'] == 2.0
    assert c['mask'].dtype == torch.bool and c['mask'].tolist() == [True, False, True, True, True]
    assert int(idx) == 2 and idx.dim() == 0 and float(val) == 0.5 * 4.0           # 'ei' is a length on the target axis
    # best_f=None: the best OBSERVED target of the n points in use (normalised already), by the direction
    cond.acquire('pi', x)
    assert eng.calls[-1]['best_n'] == 2.0 and eng.calls[-1]['sign'] == 1
    _, val = cond.acquire('pi', x, maximize=False, observation_noise=True)
    assert eng.calls[-1]['best_n'] == -1.5 and eng.calls[-1]['sign'] == -1 and eng.calls[-1]['latent'] is False
    assert float(val) == 0.5                                                     # a probability: no units
    _, val = cond.acquire('ucb', x, beta=3.0, maximize=False)
    assert eng.calls[-1]['beta'] == 3.0 and float(val) == 0.5 * 4.0 + 10.0
    out = cond.acquisition('std', x)
    assert eng.calls[-1]['want_values'] and eng.calls[-1]['mask'] is None and eng.calls[-1]['chunk'] is None
    assert torch.equal(out, torch.arange(5, dtype=torch.float32) * 4.0)
    assert torch.equal(cond.acquisition('mean', x), torch.arange(5, dtype=torch.float32) * 4.0 + 10.0)


def test_conditioned_gp_argument_errors():
    cond, eng = stub_cond()
    x = np.zeros((5, 1))
    for call in (cond.acquire, cond.acquisition):
        with pytest.raises(ValueError, match='kind must be'):
            call('lcb', x)
        with pytest.raises(ValueError, match='kind must be'):
            call(0, x)
    with pytest.raises(ValueError, match=r'mask must be \[5\]'):
        cond.acquire('ei', x, mask=[True, False])
    assert eng.calls == []                                          # refused before the engine is asked


def test_gaussian_predictive_acquisition_argument_errors():
    dist = GaussianPredictive(torch.zeros(2, 5), torch.ones(2, 5), None, 0.0, 1.0, mixture=True)
    with pytest.raises(ValueError, match='kind must be'):
        dist.acquisition('lcb')
    for kind in ('ei', 'pi'):
        with pytest.raises(ValueError, match='best_f'):
            dist.acquisition(kind)
    with pytest.raises(RuntimeError, match='HIP device'):           # well-formed, on CPU tensors: no CPU path
        dist.acquisition('ucb')


def test_public_interface():
    from meta_learning_pacoh_amd import engine as E
    assert callable(E.GPEngine.cond_acq)
    for name in ('acquisition', 'acquire'):
        assert callable(getattr(ConditionedGP, name))
    doc = sys.modules[ConditionedGP.__module__].__doc__
    assert 'cond.acquire' in doc and 'cond.acquisition' in doc
