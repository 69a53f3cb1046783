"""Joint predictive draws on the host side (no GPU): the two new C entry points (exported, bound, argument validation without a launch),
the sample / rsample interface of GaussianPredictive, and the fp64 restatement of tests/mvn_sample_ref.py pinned against numpy / scipy."""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.linalg
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvn_sample_ref as R                                         # noqa: E402
from meta_learning_pacoh_amd import _lib                           # noqa: E402
from meta_learning_pacoh_amd.distributions import GaussianPredictive   # noqa: E402

EINVAL, ELIMIT, EDTYPE = -1, -2, -3
NEW = ('pacoh_mvn_factor_workspace_bytes', 'pacoh_mvn_factor', 'pacoh_mvn_sample')


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
    assert _lib.ABI_VERSION == 14 and lib.pacoh_abi_version() == 14


def test_factor_workspace_query(lib):
    for B, m, dt in ((1, 1, 0), (3, 17, 0), (20, 1000, 1), (100, 200, 0)):
        a, b = lib.pacoh_mvn_factor_workspace_bytes(B, m, dt), lib.pacoh_mvn_factor_workspace_bytes(B, m, dt)
        es = 8 if dt else 4
        assert a == b >= B * m * es + B * es
    assert lib.pacoh_mvn_factor_workspace_bytes(3, 17, 5) == 0
    assert lib.pacoh_mvn_factor_workspace_bytes(0, 17, 0) == 0
    assert lib.pacoh_mvn_factor_workspace_bytes(3, 0, 0) == 0


def test_factor_argument_validation(lib):
    fake, null = ctypes.c_void_p(4096), None
    info = ctypes.cast(fake, _lib._ip)
    assert lib.pacoh_mvn_factor(null, fake, info, fake, 2, 8, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, null, info, fake, 2, 8, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, fake, None, fake, 2, 8, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, fake, info, null, 2, 8, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, fake, info, fake, 0, 8, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, fake, info, fake, -1, 8, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, fake, info, fake, 2, 0, 0, null) == EINVAL
    assert lib.pacoh_mvn_factor(fake, fake, info, fake, 2, 8, 2, null) == EDTYPE
    assert lib.pacoh_mvn_factor(fake, fake, info, fake, 2, 70000, 0, null) == ELIMIT
    assert lib.pacoh_mvn_factor(fake, fake, info, fake, 2, 60000, 1, null) == ELIMIT     # no dense Cholesky for this size: nothing enqueued


def test_sample_argument_validation(lib):
    fake, null = ctypes.c_void_p(4096), None
    ip = ctypes.cast(fake, _lib._ip)

    def call(Lp=fake, info=ip, mu=fake, eps=fake, order=ip, offsets=ip, out=fake, B=3, m=8, S=16, dt=0):
        return lib.pacoh_mvn_sample(Lp, info, mu, eps, order, offsets, out, 0.0, 1.0, B, m, S, dt, null)

    assert call(Lp=null) == EINVAL
    assert call(info=None) == EINVAL
    assert call(mu=null) == EINVAL
    assert call(eps=null) == EINVAL
    assert call(out=null) == EINVAL
    assert call(B=0) == EINVAL and call(B=-2) == EINVAL
    assert call(m=0) == EINVAL and call(m=-1) == EINVAL
    assert call(S=-1) == EINVAL
    assert call(dt=7) == EDTYPE
    assert call(order=None, offsets=None) == EINVAL                # B > 1 needs the grouping
    assert call(offsets=None) == EINVAL and call(order=None) == EINVAL
    assert call(B=1, order=None, offsets=None, m=70000 * 64) == ELIMIT
    assert call(S=0) == 0                                          # nothing to draw: no launch


def test_gaussian_predictive_has_sampling():
    assert callable(GaussianPredictive.sample) and callable(GaussianPredictive.rsample)
    mu = torch.zeros(1, 5, dtype=torch.float64)
    g = GaussianPredictive(mu, torch.ones(1, 5, dtype=torch.float64), None, 0.0, 1.0, mixture=False)
    with pytest.raises(RuntimeError, match='return_density=True'):
        g.sample((3,))
    with pytest.raises(RuntimeError, match='return_density=True'):
        g.rsample((3,))
    cov = torch.eye(5, dtype=torch.float64)[None]
    g = GaussianPredictive(mu, torch.ones(1, 5, dtype=torch.float64), cov, 0.0, 1.0, mixture=False)
    e = g.sample((0, 4))                                            # S = 0: empty, nothing launched
    assert e.shape == (0, 4, 5)


def _spd(m, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(m, m + 3, generator=g, dtype=dtype)
    return X @ X.T / (m + 3) + 0.1 * torch.eye(m, dtype=dtype)


def crafted(dtype, m=6):
    """[4,m,m]: healthy | rank-deficient PSD block [[1,1],[1,1]] (rung 1) | eigenvalue -3 base (rung 2) | indefinite (fails)"""
    base = R.JITTER_BASE[dtype]
    A = torch.stack([_spd(m, s) for s in range(4)])
    for b, blk in ((1, [[1.0, 1.0], [1.0, 1.0]]), (2, [[1.0, 1.0 + 3 * base], [1.0 + 3 * base, 1.0]]), (3, [[1.0, 0.0], [0.0, -1.0]])):
        A[b, :2, :] = 0
        A[b, :, :2] = 0
        A[b, :2, :2] = torch.tensor(blk, dtype=torch.float64)
    if dtype == R.F32:
        A = A.float().double()                                      # what an fp32 covariance holds
    return A


@pytest.mark.parametrize('dtype', [R.F32, R.F64])
def test_ladder_rungs_of_crafted_covariances(dtype):
    A = crafted(dtype)
    rungs, Ls = R.factor_ref(A, dtype)
    assert rungs.tolist() == [0, 1, 2, -1]
    for b in range(3):
        j = R.rung_jitter(int(rungs[b]), dtype)
        Aj = A[b].numpy() + j * np.eye(A.shape[-1])
        np.testing.assert_allclose(Ls[b].numpy() @ Ls[b].numpy().T, Aj, rtol=0, atol=1e-12)
        np.testing.assert_allclose(Ls[b].numpy(), scipy.linalg.cholesky(Aj, lower=True), rtol=0, atol=1e-9)
        # scipy agrees that the rung before would not do (for the rung-2 case: an eigenvalue below -j)
        if rungs[b] > 0:
            jprev = R.rung_jitter(int(rungs[b]) - 1, dtype)
            assert np.linalg.eigvalsh(A[b].numpy() + jprev * np.eye(A.shape[-1])).min() <= 1e-15
    assert torch.isnan(Ls[3]).all()
    # the mirrored lower triangle is what is factored: garbage in the upper triangle changes nothing
    Ag = A.clone()
    Ag[0] += torch.triu(torch.full_like(Ag[0], 7.0), 1)
    r2, L2 = R.factor_ref(Ag, dtype)
    assert r2.tolist() == rungs.tolist() and torch.equal(L2[0], Ls[0])


def test_factor_is_llt_of_jittered_covariance():
    for m in (1, 2, 17, 64):
        A = _spd(m, m)[None]
        rungs, Ls = R.factor_ref(A, R.F64)
        assert rungs.tolist() == [0]
        np.testing.assert_allclose((Ls[0] @ Ls[0].T).numpy(), A[0].numpy(), rtol=0, atol=1e-12)
        assert torch.equal(Ls[0], torch.tril(Ls[0]))
    A = _spd(5, 1)[None]
    L2 = R.factor_at(A, torch.tensor([3]), R.F32)
    np.testing.assert_allclose((L2[0] @ L2[0].T).numpy(), A[0].numpy() + 1e-4 * np.eye(5), rtol=0, atol=1e-12)


def test_grouping_and_transform_against_numpy():
    g = torch.Generator().manual_seed(3)
    P, m, S = 4, 7, 50
    Ls = torch.stack([torch.linalg.cholesky(_spd(m, 10 + c)) for c in range(P)])
    mu = torch.randn(P, m, generator=g, dtype=torch.float64)
    eps = torch.randn(S, m, generator=g, dtype=torch.float64)
    comp = torch.randint(P, (S,), generator=g)
    order, offsets = R.group(comp, P)
    np.testing.assert_array_equal(order.numpy(), np.argsort(comp.numpy(), kind='stable'))
    np.testing.assert_array_equal(np.diff(offsets.numpy()), np.bincount(comp.numpy(), minlength=P))
    out = R.sample_ref(Ls, mu, eps, comp, y_mean=1.5, y_std=2.0)
    c, e = comp.numpy(), eps.numpy()
    want = 1.5 + 2.0 * (mu.numpy()[c] + np.einsum('sij,sj->si', Ls.numpy()[c], e))
    np.testing.assert_allclose(out.numpy(), want, rtol=0, atol=1e-12)


def test_reference_draws_have_the_predictive_moments():
    """sample mean and covariance of the restated draws against the Gaussian they come from (statistical, fixed seed)"""
    g = torch.Generator().manual_seed(5)
    m, S = 6, 200000
    Sigma = _spd(m, 99)
    Ls = torch.linalg.cholesky(Sigma)[None]
    mu = torch.randn(1, m, generator=g, dtype=torch.float64)
    eps = torch.randn(S, m, generator=g, dtype=torch.float64)
    y = R.sample_ref(Ls, mu, eps, y_mean=-0.5, y_std=3.0).numpy()
    cov = 9.0 * Sigma.numpy()
    se_mean = np.sqrt(np.diag(cov) / S)
    assert np.all(np.abs(y.mean(0) - (-0.5 + 3.0 * mu[0].numpy())) < 6 * se_mean)
    emp = np.cov(y, rowvar=False)
    se_cov = np.sqrt((cov ** 2 + np.outer(np.diag(cov), np.diag(cov))) / S)      # Var of a Gaussian sample covariance entry
    assert np.all(np.abs(emp - cov) < 6 * se_cov)


def test_wrappers_validate_shapes_before_any_call():
    """the C side cannot see shapes: the ctypes wrappers refuse mismatched tensors (checked before any device pointer is taken)"""
    B, m, S = 3, 8, 10
    Lf, mu, eps = torch.zeros(B, m, m), torch.zeros(B, m), torch.zeros(S, m)
    info = torch.zeros(B, dtype=torch.int32)
    order, offsets = torch.zeros(S, dtype=torch.int32), torch.zeros(B + 1, dtype=torch.int32)
    with pytest.raises(ValueError, match='cov'):
        _lib.mvn_factor(torch.zeros(B, m, m + 1))
    with pytest.raises(ValueError, match='Lf'):
        _lib.mvn_sample(Lf[:2], info, mu, eps, order=order, offsets=offsets)
    with pytest.raises(ValueError, match='Lf'):
        _lib.mvn_sample(torch.zeros(B, m + 1, m + 1), info, mu, eps, order=order, offsets=offsets)
    with pytest.raises(ValueError, match='info'):
        _lib.mvn_sample(Lf, info[:2], mu, eps, order=order, offsets=offsets)
    with pytest.raises(ValueError, match='info'):
        _lib.mvn_sample(Lf, info.long(), mu, eps, order=order, offsets=offsets)
    with pytest.raises(ValueError, match='eps'):
        _lib.mvn_sample(Lf, info, mu, torch.zeros(S, m + 1), order=order, offsets=offsets)
    with pytest.raises(ValueError, match='order'):
        _lib.mvn_sample(Lf, info, mu, eps)
    with pytest.raises(ValueError, match='order'):
        _lib.mvn_sample(Lf, info, mu, eps, order=order[:5], offsets=offsets)
    with pytest.raises(ValueError, match='order'):
        _lib.mvn_sample(Lf, info, mu, eps, order=order, offsets=offsets[:B])
