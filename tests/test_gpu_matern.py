"""The Matern kernel family (nu = 1/2, 3/2, 5/2) on the device: the Gram entry point, the LML with its five gradients and the posterior
predictive on the register-resident kernels (fp32, n <= 128, f <= 4: every block count), the general LDS-resident kernel (f = 5, 16;
fp64) and the dense path (n = 200, 512), against an fp64 torch restatement with autograd (tests/matern_ref.py); the learners with a
MaternKernel object against the fp64 oracles.

fp32 bars are per problem and measured: the HIP error of a quantity may not exceed ERR_FACTOR times the error torch's own fp32
evaluation of the same expression makes, worst over a few point orders (plus a small floor) -- the method of
tests/test_gpu_fp32_accuracy.py, restated here."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref as MR                                 # noqa: E402
from oracle import pacoh_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

ERR_FACTOR = 10.0        # HIP fp32 error <= this x torch fp32's worst error over the point orders ...
ERR_FLOOR = 2e-5         # ... or this relative error, whichever is larger
N_ORDERS = 3
FP64_BAR = 1e-9
LOG_2PI = math.log(2 * math.pi)


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    import meta_learning_pacoh_amd as m
    return m


# ---- the fp64 / fp32 torch restatement of one problem ----------------------------------------------------------------------------------
def ref_lml(z, m, y, ls, os_, noise, nu):
    """-> (lml, d_z, d_m, d_ls, d_os, d_noise) of one problem by autograd (os_ None: unit outputscale, d_os None)"""
    z, m, ls, noise = [t.clone().requires_grad_(True) for t in (z, m, ls, noise)]
    osv = os_.clone().requires_grad_(True) if os_ is not None else None
    n = z.shape[0]
    K = (osv if osv is not None else 1.0) * MR.gram(z, z, ls, 1.0, nu) + noise * torch.eye(n, dtype=z.dtype)
    Lc = torch.linalg.cholesky(K)
    r = (y - m).unsqueeze(-1)
    alpha = torch.cholesky_solve(r, Lc)
    lml = -0.5 * ((r * alpha).sum() + 2.0 * torch.log(torch.diagonal(Lc)).sum() + n * LOG_2PI) / n
    ins = [z, m, ls, noise] + ([osv] if osv is not None else [])
    g = torch.autograd.grad(lml, ins)
    return lml.detach(), g[0], g[1], g[2], (g[4] if osv is not None else None), g[3]


def ref_predict(zc, mc, yc, zt, mt, ls, os_, noise, nu):
    osv = os_ if os_ is not None else 1.0
    n, m = zc.shape[0], zt.shape[0]
    Kxx = osv * MR.gram(zc, zc, ls, 1.0, nu) + noise * torch.eye(n, dtype=zc.dtype)
    Kxs = osv * MR.gram(zc, zt, ls, 1.0, nu)
    Kss = osv * MR.gram(zt, zt, ls, 1.0, nu)
    Lc = torch.linalg.cholesky(Kxx)
    alpha = torch.cholesky_solve((yc - mc).unsqueeze(-1), Lc)
    mu = mt + (Kxs.T @ alpha).squeeze(-1)
    V = torch.linalg.solve_triangular(Lc, Kxs, upper=False)
    cov = Kss - V.T @ V + noise * torch.eye(m, dtype=zc.dtype)
    return mu, torch.diagonal(cov).clone(), cov


def rel(a, b):
    """max-abs error of a against b, relative to max |b| (per quantity of one problem)"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
class Batch:
    """T tasks x P particles = B problems; inputs per problem (z_div = 1) or per task (z_div = P); y per task"""

    def __init__(self, T, P, n, f, mean_mode, shared, with_os, ragged, dtype, seed, dup=False, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        self.T, self.P, self.n, self.f, self.B = T, P, n, f, T * P
        self.mean_mode, self.dtype = mean_mode, dtype
        self.z_div = P if shared else 1
        self.z = scale * torch.randn(self.B // self.z_div, n, f, generator=g, dtype=torch.float64)
        if dup:                                              # coincident points: every odd row repeats the row before it
            self.z[:, 1::2] = self.z[:, 0:n - 1:2][:, :self.z[:, 1::2].shape[1]]
        self.y = torch.randn(T, n, generator=g, dtype=torch.float64)
        self.ls = torch.rand(P, f, generator=g, dtype=torch.float64) * 1.0 + 0.5
        self.os = (torch.rand(P, generator=g, dtype=torch.float64) + 0.5) if with_os else None
        self.noise = torch.rand(P, generator=g, dtype=torch.float64) * 0.3 + 0.1
        self.mean = {0: None, 1: 0.3 * torch.randn(self.B, n, generator=g, dtype=torch.float64),
                     2: 0.3 * torch.randn(P, generator=g, dtype=torch.float64)}[mean_mode]
        self.nv = None
        if ragged:
            self.nv = torch.randint(max(1, n // 2), n + 1, (T,), generator=g, dtype=torch.int32)
            self.nv[0] = n
            if T > 1:
                self.nv[1] = max(1, n - 7) if n > 1 else 1
        self.zt = torch.randn(self.B // self.z_div, max(3, n // 2 + 5), f, generator=g, dtype=torch.float64)
        self.mt = {0: None, 1: 0.3 * torch.randn(self.B, self.zt.shape[1], generator=g, dtype=torch.float64), 2: self.mean}[mean_mode]

    def dev(self, t):
        return None if t is None else t.to(self.dtype).cuda()

    def problem(self, b, dtype=torch.float64):
        """the problem's own valid inputs: (z, m, y, ls, os, noise, zt, mt), cast to dtype"""
        p, t = b % self.P, b // self.P
        nv = self.n if self.nv is None else int(self.nv[t])
        z = self.z[b // self.z_div, :nv]
        if self.mean_mode == 1:
            m, mt = self.mean[b, :nv], self.mt[b]
        elif self.mean_mode == 2:
            m, mt = self.mean[p].expand(nv), self.mean[p].expand(self.zt.shape[1])
        else:
            m, mt = torch.zeros(nv, dtype=torch.float64), torch.zeros(self.zt.shape[1], dtype=torch.float64)
        c = lambda v: None if v is None else v.to(dtype)
        return (c(z), c(m.clone()), c(self.y[t, :nv]), c(self.ls[p]), c(self.os[p] if self.os is not None else None), c(self.noise[p]),
                c(self.zt[b // self.z_div]), c(mt.clone())), nv

    def run_lml(self, L, code):
        return L.gp_lml_fwdbwd(self.dev(self.z), self.z_div, self.dev(self.mean), self.mean_mode, self.dev(self.y), self.P, self.dev(self.ls),
                               self.dev(self.os), self.dev(self.noise), self.B, self.P,
                               n_valid=None if self.nv is None else self.nv.cuda(), kernel=code)

    def run_predict(self, L, code):
        return L.gp_predict(self.dev(self.z), self.z_div, self.dev(self.mean), self.mean_mode, self.dev(self.y), self.P, self.dev(self.zt),
                            self.z_div, self.dev(self.mt), self.dev(self.ls), self.dev(self.os), self.dev(self.noise), self.B, self.P,
                            n_valid=None if self.nv is None else self.nv.cuda(), want_cov=True, kernel=code)


def _lml_quantities(out, bt, b, nv):
    """the device outputs of problem b, restricted to its valid rows: (lml, d_z, d_m, d_ls, d_os, d_noise)"""
    lml, d_z, d_mean, d_ls, d_os, d_noise = [None if t is None else t.double().cpu() for t in out[:6]]
    if bt.mean_mode == 1:
        dm = d_mean[b, :nv]
    elif bt.mean_mode == 2:
        dm = d_mean[b]
    else:
        dm = None
    return [lml[b], d_z[b, :nv], dm, d_ls[b], None if d_os is None else d_os[b], d_noise[b]]


def _ref_quantities(bt, b, nu, dtype=torch.float64, perm=None):
    (z, m, y, ls, os_, noise, _, _), nv = bt.problem(b, dtype)
    if perm is not None:
        z, m, y = z[perm], m[perm], y[perm]
    lml, dz, dm, dls, dos, dnz = ref_lml(z, m, y, ls, os_, noise, nu)
    if perm is not None:
        inv = torch.argsort(perm)
        dz, dm = dz[inv], dm[inv]
    if bt.mean_mode == 2:
        dm = dm.sum()
    elif bt.mean_mode == 0:
        dm = None
    return [lml, dz, dm, dls, dos, dnz], nv


NAMES = ('lml', 'd_z', 'd_mean', 'd_ls', 'd_os', 'd_noise')


def check_lml(L, bt, nu, fp64_bar=FP64_BAR):
    out = bt.run_lml(L, MR.CODE[nu])
    info = out[6].cpu()
    assert (info == 0).all(), info
    assert out[1].shape == (bt.B, bt.n, bt.f)
    worst = {}
    for b in range(bt.B):
        ref, nv = _ref_quantities(bt, b, nu)
        got = _lml_quantities(out, bt, b, nv)
        if bt.dtype == torch.float64:
            bars = [fp64_bar] * 6
        else:
            g = torch.Generator().manual_seed(100 + b)
            orders = [None] + [torch.randperm(nv, generator=g) for _ in range(N_ORDERS - 1)]
            errs = [0.0] * 6
            for perm in orders:
                r32, _ = _ref_quantities(bt, b, nu, torch.float32, perm)
                errs = [max(e, rel(q32, q64)) if q64 is not None else 0.0 for e, q32, q64 in zip(errs, r32, ref)]
            bars = [max(ERR_FACTOR * e, ERR_FLOOR) for e in errs]
        for name, g_, r_, bar in zip(NAMES, got, ref, bars):
            if r_ is None:
                continue
            assert g_ is not None and torch.isfinite(g_).all(), (name, b)
            e = rel(g_, r_)
            worst[name] = max(worst.get(name, 0.0), e / bar)
            assert e <= bar, '%s of problem %d: rel err %.3g > bar %.3g (nu %g, n %d, nv %d, f %d, %s)' % (
                name, b, e, bar, nu, bt.n, nv, bt.f, bt.dtype)
        # rows past the problem's n_valid come back as 0
        if nv < bt.n:
            assert (out[1][b, nv:] == 0).all()
    return worst


def check_predict(L, bt, nu):
    mu, var, cov, info = bt.run_predict(L, MR.CODE[nu])
    assert (info.cpu() == 0).all()
    mu, var, cov = mu.double().cpu(), var.double().cpu(), cov.double().cpu()
    for b in range(bt.B):
        (z, m, y, ls, os_, noise, zt, mt), nv = bt.problem(b)
        r = ref_predict(z, m, y, zt, mt, ls, os_, noise, nu)
        if bt.dtype == torch.float64:
            bars = [FP64_BAR] * 3
        else:
            g = torch.Generator().manual_seed(200 + b)
            errs = [0.0] * 3
            for k in range(N_ORDERS):
                perm = torch.arange(nv) if k == 0 else torch.randperm(nv, generator=g)
                (z3, m3, y3, ls3, os3, nz3, zt3, mt3), _ = bt.problem(b, torch.float32)
                r32 = ref_predict(z3[perm], m3[perm], y3[perm], zt3, mt3, ls3, os3, nz3, nu)
                errs = [max(e, rel(a, c)) for e, a, c in zip(errs, r32, r)]
            bars = [max(ERR_FACTOR * e, ERR_FLOOR) for e in errs]
        for name, g_, r_, bar in zip(('mu', 'var', 'cov'), (mu[b], var[b], cov[b]), r, bars):
            e = rel(g_, r_)
            assert e <= bar, '%s of problem %d: rel err %.3g > bar %.3g (nu %g, n %d, nv %d, f %d, %s)' % (
                name, b, e, bar, nu, bt.n, nv, bt.f, bt.dtype)


# ---- the Gram entry point ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_gram(L, nu, dtype):
    g = torch.Generator().manual_seed(5)
    B, P, n, m, f = 6, 3, 23, 17, 3
    z1 = torch.randn(B, n, f, generator=g, dtype=torch.float64)
    z2 = torch.randn(B, m, f, generator=g, dtype=torch.float64)
    ls = torch.rand(P, f, generator=g, dtype=torch.float64) + 0.5
    os_ = torch.rand(P, generator=g, dtype=torch.float64) + 0.5
    noise = torch.rand(P, generator=g, dtype=torch.float64) * 0.1 + 0.1
    d = lambda t: t.to(dtype).cuda()
    K = L.gram_rbf_ard(d(z1), 1, d(z2), 1, d(ls), d(os_), d(noise), 0, B, P, kernel=MR.CODE[nu]).double().cpu()
    Ks = L.gram_rbf_ard(d(z1), 1, d(z1), 1, d(ls), d(os_), d(noise), 1, B, P, kernel=MR.CODE[nu]).double().cpu()
    tol = 2e-6 if dtype == torch.float32 else 1e-13
    for b in range(B):
        p = b % P
        ref = MR.gram(z1[b], z2[b], ls[p], os_[p], nu)
        assert rel(K[b], ref) < tol
        refs = MR.gram(z1[b], z1[b], ls[p], os_[p], nu) + noise[p] * torch.eye(n, dtype=torch.float64)
        assert rel(Ks[b], refs) < tol


# ---- the register-resident kernels: every block count, f = 1..4 -------------------------------------------------------------------------
REG_N = [1, 15, 16, 17, 33, 48, 64, 65, 96, 128]


@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('n', REG_N)
def test_lml_register_kernel_fp32(L, nu, n):
    for f in (1, 2, 3, 4):
        k = REG_N.index(n) * 4 + f
        bt = Batch(T=3, P=2, n=n, f=f, mean_mode=k % 3, shared=bool(k % 2), with_os=(k // 2) % 2 == 0, ragged=n > 1 and k % 4 != 1,
                   dtype=torch.float32, seed=1000 + 31 * k + int(10 * nu))
        check_lml(L, bt, nu)


@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('n', [1, 17, 64, 65, 128])
def test_predict_register_kernel_fp32(L, nu, n):
    for f in (1, 2, 3, 4):
        k = n + f
        bt = Batch(T=2, P=2, n=n, f=f, mean_mode=k % 3, shared=bool(k % 2), with_os=f != 3, ragged=n > 1 and f % 2 == 0,
                   dtype=torch.float32, seed=2000 + 7 * k + int(10 * nu))
        check_predict(L, bt, nu)


@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('n', [1, 17, 64, 128])
def test_lml_and_predict_fp64(L, nu, n):
    for f in (1, 3):
        k = n + f
        bt = Batch(T=2, P=2, n=n, f=f, mean_mode=k % 3, shared=bool(k % 2), with_os=f == 1, ragged=n > 1,
                   dtype=torch.float64, seed=3000 + k + int(10 * nu))
        check_lml(L, bt, nu)
        check_predict(L, bt, nu)


# ---- the general kernel (f > 4) and the dense path (n > 128) --------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('f', [5, 16])
def test_general_kernel(L, nu, dtype, f):
    bt = Batch(T=2, P=2, n=40, f=f, mean_mode=f % 3, shared=f == 5, with_os=True, ragged=True, dtype=dtype, seed=4000 + f, scale=2.0)
    check_lml(L, bt, nu)
    check_predict(L, bt, nu)


@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('n', [200, 512])
def test_dense_path_fp64(L, nu, n):
    bt = Batch(T=2, P=1, n=n, f=2, mean_mode=1, shared=False, with_os=True, ragged=True, dtype=torch.float64, seed=5000 + n, scale=2.0)
    check_lml(L, bt, nu, fp64_bar=FP64_BAR)
    check_predict(L, bt, nu)


@pytest.mark.parametrize('nu', MR.NUS)
def test_dense_path_fp32(L, nu):
    bt = Batch(T=2, P=1, n=200, f=2, mean_mode=2, shared=False, with_os=True, ragged=False, dtype=torch.float32, seed=5500, scale=2.0)
    check_lml(L, bt, nu)


# ---- coincident inputs, jitter ladder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('n', [24, 64, 100])
def test_duplicate_inputs_nu_half(L, dtype, n):
    """nu = 1/2 is not differentiable at s = 0: coincident points contribute no gradient (gpytorch's clamped distance) -- finite, and
    equal to the clamp form of the restatement"""
    bt = Batch(T=2, P=2, n=n, f=2, mean_mode=1, shared=True, with_os=True, ragged=False, dtype=dtype, seed=6000 + n, dup=True)
    out = bt.run_lml(L, MR.CODE[0.5])
    for t in out[:6]:
        if t is not None:
            assert torch.isfinite(t).all()
    check_lml(L, bt, 0.5)


@pytest.mark.parametrize('nu', MR.NUS)
@pytest.mark.parametrize('dtype, n', [(torch.float32, 20), (torch.float32, 64), (torch.float32, 128), (torch.float32, 40 + 100),
                                      (torch.float64, 30)])
def test_jitter_ladder_leaves_healthy_problems_bitwise(L, nu, dtype, n):
    """a problem whose matrix is singular (duplicate points, noise 1e-12) sits beside healthy ones: it takes the jitter ladder
    (info > 0) or fails (-1, NaN), the healthy problems' outputs are bitwise those of a batch without it"""
    f, P = 2, 4
    g = torch.Generator().manual_seed(7000 + n)
    z = torch.randn(P, n, f, generator=g, dtype=torch.float64)
    z[0, 1::2] = z[0, 0:n - 1:2]
    y = torch.randn(1, n, generator=g, dtype=torch.float64)
    ls = torch.rand(P, f, generator=g, dtype=torch.float64) + 0.5
    noise = torch.rand(P, generator=g, dtype=torch.float64) * 0.3 + 0.1
    noise[0] = 1e-12 if dtype == torch.float32 else -1e-9          # (fp64 factors K + 1e-12 I of duplicates without a failure; -1e-9 fails, the first rung fixes it)
    d = lambda t: t.to(dtype).cuda()
    code = MR.CODE[nu]
    full = L.gp_lml_fwdbwd(d(z), 1, None, L.MEAN_ZERO, d(y), P, d(ls), None, d(noise), P, P, kernel=code)
    info = full[6].cpu()
    assert int(info[0]) != 0 and (info[1:] == 0).all(), info
    # the healthy problems alone: the same three as problems 1..3 of a batch whose problem 0 is healthy too
    z2, noise2 = z.clone(), noise.clone()
    z2[0] = torch.randn(n, f, generator=g, dtype=torch.float64)
    noise2[0] = 0.2
    ref = L.gp_lml_fwdbwd(d(z2), 1, None, L.MEAN_ZERO, d(y), P, d(ls), None, d(noise2), P, P, kernel=code)
    for a, b in zip(full[:6], ref[:6]):
        if a is not None:
            assert torch.equal(a[1:], b[1:])
    if int(info[0]) > 0:
        for t in full[:6]:
            if t is not None:
                assert torch.isfinite(t[0]).all()


def test_unknown_family_codes_refused(L):
    lib = L.load_library()
    z = torch.randn(2, 8, 2).cuda()
    y = torch.randn(2, 8).cuda()
    ls, noise = torch.ones(1, 2).cuda(), torch.full((1,), 0.1).cuda()
    for code in (2, 6):
        with pytest.raises(Exception):
            L.gp_lml_fwdbwd(z, 1, None, L.MEAN_ZERO, y, 1, ls, None, noise, 2, 1, kernel=code)
    # the task-fused entry points stay ARD-RBF only: they refuse the Matern codes, the learners fall back to the multi-launch step
    h = L._hidden_arr([32, 32])
    for code in (L.KERNEL_MATERN12, L.KERNEL_MATERN32, L.KERNEL_MATERN52):
        assert lib.pacoh_svgd_task_workspace_bytes(2534, 10, 20, 1, 2, L.MEAN_VECTOR, h, 2, 1, h, 2, L._kf(2, code), 0, L.F32) == 0


# ---- learners --------------------------------------------------------------------------------------------------------------------------------------
class _MaternKernel:
    """stand-in for gpytorch.kernels.MaternKernel(nu, ard_num_dims): recognised by class name (modules.py)"""

    def __init__(self, nu, dims=1, raw=0.0):
        self.nu = nu
        self.raw_lengthscale = torch.nn.Parameter(torch.full((1, dims), raw))


_MaternKernel.__name__ = 'MaternKernel'


class _ScaleKernel:
    def __init__(self, base, raw=0.0):
        self.base_kernel, self.raw_outputscale = base, torch.nn.Parameter(torch.tensor(raw))


_ScaleKernel.__name__ = 'ScaleKernel'


@pytest.mark.parametrize('nu', MR.NUS)
def test_single_task_learner_matches_oracle(M, nu, monkeypatch):
    monkeypatch.setattr(O, 'gram_family', MR.gram_family_for(nu))
    rs = np.random.RandomState(31)
    x = rs.uniform(-2, 2, size=(40, 2))
    y = np.sin(2.5 * x[:, :1]) + 0.2 * x[:, 1:] + 0.05 * rs.randn(40, 1)
    kw = dict(mean_module='constant', num_iter_fit=1, lr=1e-2, random_seed=4)
    m = M.GPRegressionLearned(x, y, learning_mode='learn_kernel', covar_module=_ScaleKernel(_MaternKernel(nu, 2)), **kw)
    assert m.layout.kernel_code == MR.CODE[nu] and m.layout.blocks['lengthscale_raw'] == 2
    o = O.SingleTaskOracle(x, y, learning_mode='learn_kernel', covar_module='SE', dtype=torch.float64, **kw)
    losses = [m.fit(verbose=False, n_iter=1) for _ in range(6)]
    ref = [rec[1] for rec in o.fit(n_iter=6, log_period=1)]
    for a, b in zip(losses, ref):
        assert abs(a - b) < 2e-4 * max(1.0, abs(b)), (losses, ref)
    lo, hi = m.layout.slices['lengthscale_raw']
    got = m.theta[0, lo:hi].cpu().double()
    want = o.raw_lengthscale.detach().reshape(-1)
    assert float((got - want).abs().max()) < 2e-3
    assert abs(float(m.theta[0, m.layout.slices['outputscale_raw'][0]]) - float(o.raw_outputscale.detach())) < 2e-3
    mean, std = m.predict(x[:7])
    assert np.isfinite(mean).all() and (np.asarray(std) > 0).all()
    ll, rmse, calib = m.eval(x, y)
    assert np.isfinite(ll) and np.isfinite(rmse)


@pytest.mark.parametrize('nu', MR.NUS)
def test_meta_learner_matches_oracle_and_unties_lengthscales(M, nu, monkeypatch):
    monkeypatch.setattr(O, 'gram_family', MR.gram_family_for(nu))
    rs = np.random.RandomState(8)
    tasks = []
    for _ in range(6):
        x = rs.uniform(-1, 1, size=(11, 2))
        tasks.append((x, np.sin(3 * x[:, :1]) + 0.1 * rs.randn(11, 1)))      # depends on the first input only
    m = M.GPRegressionMetaLearned(tasks, mean_module='constant', covar_module=_ScaleKernel(_MaternKernel(nu, 2)), task_batch_size=6,
                                  lr_params=5e-3, random_seed=2)
    assert m.layout.blocks['lengthscale_raw'] == 2 and m.layout.kernel_code == MR.CODE[nu]
    o = O.MapOracle(tasks, mean_module='constant', covar_module='SE', task_batch_size=6, lr_params=5e-3, random_seed=2, dtype=torch.float64)
    m.meta_fit(verbose=False, n_iter=8)
    o.meta_fit(n_iter=8)
    lay = m.layout
    got = m.theta[0].cpu().double()
    lo, hi = lay.slices['lengthscale_raw']
    want_ls = o.raw_lengthscale.detach().reshape(-1)
    assert float((got[lo:hi] - want_ls).abs().max()) < 5e-4, (got[lo:hi], want_ls)
    assert abs(float(got[lay.slices['outputscale_raw'][0]]) - float(o.raw_outputscale.detach())) < 5e-4
    assert abs(float(got[lay.slices['noise_raw'][0]]) - float(o.raw_noise.detach().reshape(-1)[0])) < 5e-4
    # ARD: the two lengthscales move apart (a tied scale would keep them equal)
    assert abs(float(got[lo] - got[lo + 1])) > 1e-3 and abs(float(want_ls[0] - want_ls[1])) > 1e-3
    mean, std = m.predict(*tasks[0], tasks[1][0])
    assert np.isfinite(mean).all() and (std > 0).all()
    ll, rmse, calib = m.eval(*tasks[0], tasks[1][0], tasks[1][1])
    assert np.isfinite(ll) and np.isfinite(rmse)
    ucb, lcb = m.confidence_intervals(*tasks[0], tasks[1][0])
    assert torch.isfinite(ucb).all() and torch.isfinite(lcb).all() and (ucb > lcb).all()
