"""Joint draws from the posterior predictive on the MI355X: pacoh_mvn_factor (the dense Cholesky with gpytorch's jitter ladder, input
intact) and pacoh_mvn_sample (Y = E L^T on the matrix cores, grouped by component), against the fp64 restatement of
tests/mvn_sample_ref.py, and GaussianPredictive.sample / rsample on the predictive of every learner."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvn_sample_ref as R                                         # noqa: E402

pytestmark = pytest.mark.gpu

# fp32 floor of the per-component error |y - y_ref| / (y_std sqrt(Sigma_ii)) (profiles/mvn_sample_fp32_errors.txt)
FLOOR32 = 2e-5
BAR64 = 1e-10
Y_MEAN, Y_STD = 0.25, 1.5


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


def dev():
    return torch.device('cuda')


def covariances(B, m, seed):
    """B predictive-like covariances (fp64, CPU): RBF Gram of m points + observation noise, per-component scales"""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(B, m, m, dtype=torch.float64)
    for b in range(B):
        x = torch.rand(m, 1, generator=g, dtype=torch.float64) * 6 - 3
        ls = 0.3 + float(torch.rand(1, generator=g))
        os_ = 0.5 + float(torch.rand(1, generator=g))
        out[b] = os_ * torch.exp(-0.5 * (x - x.T) ** 2 / ls ** 2) + (0.02 + 0.05 * float(torch.rand(1, generator=g))) * torch.eye(m, dtype=torch.float64)
    return out


def grouping(comp, B):
    order, offsets = R.group(comp, B)
    if B == 1:
        return None, None
    return order.to(torch.int32).to(dev()), offsets.to(torch.int32).to(dev())


def component_errors(y, ref, comp, cov, B):
    """per component: max over its draws and points of |y - ref| / (y_std sqrt(Sigma_ii)); NaN-free components only"""
    sd = torch.sqrt(torch.diagonal(cov, dim1=-2, dim2=-1)) * Y_STD                 # [B,m]
    errs = []
    for c in range(B):
        rows = (comp == c).nonzero().flatten()
        if rows.numel() == 0:
            errs.append(0.0)
            continue
        errs.append(float(((y[rows] - ref[rows]).abs() / sd[c]).max()))
    return errs


def torch32_draws(cov64, rungs, mu, eps, comp):
    """plain torch fp32: cholesky of the fp32 covariance at the same rung + matmul, in fp32"""
    S, m = eps.shape
    out = torch.empty(S, m, dtype=torch.float32)
    for c in range(cov64.shape[0]):
        rows = (comp == c).nonzero().flatten()
        if rows.numel() == 0:
            continue
        A = R.symmetrise(cov64[c]).float() + float(R.rung_jitter(int(rungs[c]), R.F32)) * torch.eye(m)
        Lc = torch.linalg.cholesky(A)
        out[rows] = Y_MEAN + Y_STD * (mu[c].float() + eps[rows].float() @ Lc.T)
    return out.double()


MS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 256, 509, 512, 1000, 1024]
SS = [1, 15, 16, 17, 1000]


@pytest.mark.parametrize('dtype', [R.F32, R.F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('B', [1, 3, 20])
@pytest.mark.parametrize('m', MS)
def test_draws_exact_with_base_samples(L, m, B, dtype):
    tdt = torch.float32 if dtype == R.F32 else torch.float64
    cov = covariances(B, m, seed=1000 * m + B).to(tdt)                        # what the kernel sees ...
    cov64 = cov.double()                                                      # ... and the oracle, exactly
    cov_d = cov.to(dev())
    Lf, info = L.mvn_factor(cov_d)
    rungs = info.cpu()
    assert (rungs >= 0).all() and (rungs <= 3).all(), rungs
    Lref = R.factor_at(cov64, rungs, dtype)
    g = torch.Generator().manual_seed(m + 7 * B)
    mu = torch.randn(B, m, generator=g, dtype=torch.float64).to(tdt)
    for S in SS:
        eps = torch.randn(S, m, generator=g, dtype=torch.float64).to(tdt)
        comp = torch.randint(B, (S,), generator=g) if B > 1 else torch.zeros(S, dtype=torch.int64)
        order, offsets = grouping(comp, B)
        y = L.mvn_sample(Lf, info, mu.to(dev()), eps.to(dev()), Y_MEAN, Y_STD, order, offsets).cpu().double()
        ref = R.sample_ref(Lref, mu.double(), eps.double(), comp, Y_MEAN, Y_STD)
        assert torch.isfinite(y).all()
        e_hip = component_errors(y, ref, comp, cov64, B)
        if dtype == R.F64:
            assert max(e_hip) <= BAR64, (S, e_hip)
        else:
            e_t = component_errors(torch32_draws(cov64, rungs, mu, eps, comp), ref, comp, cov64, B)
            for c in range(B):
                assert e_hip[c] <= max(40 * e_t[c], FLOOR32), (S, c, e_hip[c], e_t[c])


def _spd(m, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(m, m + 3, generator=g, dtype=torch.float64)
    return X @ X.T / (m + 3) + 0.1 * torch.eye(m, dtype=torch.float64)


def crafted(dtype, m):
    """[5,m,m]: healthy | rank-deficient PSD block (rung 1) | eigenvalue -3 base (rung 2) | indefinite (exhausts the ladder) | healthy"""
    base = R.JITTER_BASE[dtype]
    A = torch.stack([_spd(m, 50 + s) for s in range(5)])
    for b, blk in ((1, [[1.0, 1.0], [1.0, 1.0]]), (2, [[1.0, 1.0 + 3 * base], [1.0 + 3 * base, 1.0]]), (3, [[1.0, 0.0], [0.0, -1.0]])):
        A[b, :2, :] = 0
        A[b, :, :2] = 0
        A[b, :2, :2] = torch.tensor(blk, dtype=torch.float64)
    return A


@pytest.mark.parametrize('dtype', [R.F32, R.F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('m', [6, 128])
def test_jitter_ladder_in_one_launch(L, m, dtype):
    from meta_learning_pacoh_amd.distributions import GaussianPredictive
    from meta_learning_pacoh_amd.engine import NotPSDError
    tdt = torch.float32 if dtype == R.F32 else torch.float64
    cov = crafted(dtype, m).to(tdt)
    rungs_ref, _ = R.factor_ref(cov.double(), dtype)
    assert rungs_ref.tolist() == [0, 1, 2, -1, 0]
    Lf, info = L.mvn_factor(cov.to(dev()))
    assert info.cpu().tolist()[:3] + info.cpu().tolist()[4:] == [0, 1, 2, 0] and int(info[3]) < 0
    g = torch.Generator().manual_seed(m)
    B, S = 5, 40
    mu = torch.randn(B, m, generator=g, dtype=torch.float64).to(tdt).to(dev())
    eps = torch.randn(S, m, generator=g, dtype=torch.float64).to(tdt).to(dev())
    comp = torch.arange(S) % B
    order, offsets = grouping(comp, B)
    y = L.mvn_sample(Lf, info, mu, eps, Y_MEAN, Y_STD, order, offsets).cpu()
    assert torch.isnan(y[comp == 3]).all()
    assert torch.isfinite(y[comp != 3]).all()
    bar = BAR64 if dtype == R.F64 else 1e-4
    ref = R.sample_ref(R.factor_at(cov.double(), info.cpu(), dtype), mu.cpu().double(), eps.cpu().double(), comp, Y_MEAN, Y_STD)
    for c in (0, 1, 2, 4):
        assert float((y[comp == c].double() - ref[comp == c]).abs().max()) <= bar * Y_STD * 10
    # the healthy components are bitwise those of a launch without the bad ones
    keep = [0, 4]
    Lh, ih = L.mvn_factor(cov[keep].contiguous().to(dev()))
    assert torch.equal(Lh[0].tril(), Lf[0].tril()) and torch.equal(Lh[1].tril(), Lf[4].tril())
    rows = torch.cat([(comp == c).nonzero().flatten() for c in keep])
    comp_h = torch.cat([torch.full(((comp == c).sum(),), k) for k, c in enumerate(keep)])
    oh, offh = grouping(comp_h, 2)
    yh = L.mvn_sample(Lh, ih, mu[keep].contiguous(), eps[rows.to(dev())].contiguous(), Y_MEAN, Y_STD, oh, offh).cpu()
    assert torch.equal(yh, y[rows])
    # the predictive object raises where gpytorch's psd_safe_cholesky does, naming the component
    gp = GaussianPredictive(mu, torch.ones_like(mu), cov.to(dev()), Y_MEAN, Y_STD, mixture=True)
    with pytest.raises(NotPSDError, match='component 3'):
        gp.sample((8,))


def _predictive(mixture, P=4, m=24, dtype=torch.float32, seed=0):
    from meta_learning_pacoh_amd.distributions import GaussianPredictive
    cov = covariances(P, m, seed).to(dtype).to(dev())
    g = torch.Generator().manual_seed(seed + 1)
    mu = torch.randn(P, m, generator=g, dtype=torch.float64).to(dtype).to(dev())
    var = torch.diagonal(cov, dim1=-2, dim2=-1).contiguous()
    return GaussianPredictive(mu, var, cov, 0.7, 2.0, mixture=mixture)


@pytest.mark.parametrize('mixture', [False, True])
def test_input_intact_and_factor_cached(L, mixture):
    gp = _predictive(mixture)
    cov0 = gp._cov_n.clone()
    Lf, info = L.mvn_factor(gp._cov_n)
    torch.cuda.synchronize()
    assert torch.equal(gp._cov_n, cov0)
    value = gp.mean + 0.1
    lp0 = gp.log_prob(value)
    base = torch.randn(3, 5, gp._mu_n.shape[1], device=dev())
    a = gp.rsample(base_samples=base)
    chol = gp._chol
    b = gp.rsample(base_samples=base)
    assert gp._chol is chol                                         # factored once, on the first draw
    assert a.shape == (3, 5, gp._mu_n.shape[1])
    if not mixture:
        assert torch.equal(a, b)
        assert torch.equal(chol[0][0].tril(), Lf[0].tril())
    lp1 = gp.log_prob(value)
    assert torch.equal(lp0, lp1) and torch.equal(gp._cov_n, cov0)
    assert gp.sample((2, 3)).shape == (2, 3, gp._mu_n.shape[1])
    assert gp.sample(torch.Size()).shape == (gp._mu_n.shape[1],)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_mixture_replays_documented_draw_order(L, dtype):
    P, m = 5, 33
    gp = _predictive(True, P=P, m=m, dtype=dtype, seed=3)
    shape = (40, 25)
    S = 40 * 25
    torch.cuda.manual_seed(123)
    y = gp.sample(shape).reshape(S, m)
    torch.cuda.manual_seed(123)
    comp = torch.randint(P, (S,), device=dev())
    eps = torch.randn(S, m, dtype=dtype, device=dev())
    counts = torch.bincount(comp, minlength=P)
    assert (counts > 0).all()
    Lf, info = gp._chol[0], gp._chol[1]
    seen = torch.zeros(P, dtype=torch.int64)
    for c in range(P):
        rows = (comp == c).nonzero().flatten()
        yc = L.mvn_sample(Lf[c:c + 1].contiguous(), info[c:c + 1].contiguous(), gp._mu_n[c:c + 1].contiguous(), eps[rows].contiguous(),
                          gp.y_mean, gp.y_std)
        assert torch.equal(yc, y[rows])                           # every draw is its component's transform of its eps
        seen[c] = rows.numel()
    assert seen.tolist() == counts.cpu().tolist()
    ref = R.sample_ref(R.factor_at(gp._cov_n.cpu().double(), info.cpu(), R.F32 if dtype == torch.float32 else R.F64),
                       gp._mu_n.cpu().double(), eps.cpu().double(), comp.cpu(), gp.y_mean, gp.y_std)
    tol = 1e-9 if dtype == torch.float64 else 1e-3
    assert float((y.cpu().double() - ref).abs().max()) < tol


# ------------------------------------------------------------------------------------------ learners
def _tasks():
    from oracle import pacoh_oracle as O
    return O.sinusoid_tasks_nd(4, 40, 1, seed0=31)


def _moments_ok(pred, y, mixture):
    S = y.shape[0]
    y = y.double()
    mean, var = pred.mean.double(), pred.variance.double()
    if mixture:
        mus, vs = pred._means.double(), pred._vars.double()
        d = mus - mean
        mu4 = (d ** 4 + 6 * d ** 2 * vs + 3 * vs ** 2).mean(0)     # fourth central moment of the equal-weight mixture
    else:
        mu4 = 3 * var ** 2
    se_mean = torch.sqrt(var / S)
    se_var = torch.sqrt((mu4 - var ** 2) / S + 2 * var ** 2 / S ** 2)
    assert bool(((y.mean(0) - mean).abs() <= 6 * se_mean).all()), float(((y.mean(0) - mean).abs() / se_mean).max())
    assert bool(((y.var(0) - var).abs() <= 6 * se_var).all()), float(((y.var(0) - var).abs() / se_var).max())


def _learner_predictives():
    import meta_learning_pacoh_amd as M
    tasks = _tasks()
    (cx, cy), (tx, _) = tasks[0], tasks[1]
    tx = tx[:20]
    out = []
    model = M.GPRegressionMetaLearned(tasks, num_iter_fit=5, random_seed=30)
    out.append(('map', model.predict(cx, cy, tx, return_density=True), False))
    gp = M.GPRegressionLearned(cx, cy, learning_mode='both', covar_module='SE', mean_module='constant', random_seed=30)
    out.append(('single', gp.predict(tx, return_density=True), False))
    svgd = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=5, random_seed=1, num_iter_fit=3)
    out.append(('svgd', svgd.predict(cx, cy, tx, return_density=True), True))
    vi = M.GPRegressionMetaLearnedVI(tasks, svi_batch_size=2, random_seed=9)
    out.append(('vi-bayes', vi.predict(cx, cy, tx, n_posterior_samples=10, return_density=True), True))
    out.append(('vi-map', vi.predict(cx, cy, tx, mode='MAP', return_density=True), False))
    return out


def test_learner_predictives_sample():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    for name, pred, mixture in _learner_predictives():
        assert pred.mixture == mixture, name
        y = pred.sample((4096,))
        assert y.shape == (4096, 20), name
        assert torch.isfinite(y).all(), name
        assert pred.rsample((2, 3)).shape == (2, 3, 20), name
        _moments_ok(pred, y, mixture)


def test_single_component_sample_covariance():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    import meta_learning_pacoh_amd as M
    tasks = _tasks()
    (cx, cy), (tx, _) = tasks[0], tasks[1]
    model = M.GPRegressionMetaLearned(tasks, num_iter_fit=5, random_seed=30)
    pred = model.predict(cx, cy, tx[:32], return_density=True)
    torch.cuda.manual_seed(5)
    S = 200000
    y = pred.sample((S,)).double()
    cov = pred._cov_n[0].double() * pred.y_std ** 2
    emp = torch.cov(y.T)
    dg = torch.diagonal(cov)
    se = torch.sqrt((cov ** 2 + dg[:, None] * dg[None, :]) / S)
    assert bool(((emp - cov).abs() <= 6 * se).all()), float(((emp - cov).abs() / se).max())
    assert bool(((y.mean(0) - pred.mean.double()).abs() <= 6 * torch.sqrt(dg / S)).all())
