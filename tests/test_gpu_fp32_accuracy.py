"""The fp32 small-context GP kernels (n <= 128 register- and LDS-resident MFMA kernels, the fp32 LDS-resident general kernel, the
register-resident marginal predictive) against the fp64 oracle, PROBLEM BY PROBLEM, with bars set by what plain torch fp32 loses on
the same expression: for every problem b and output q

    err_hip(b, q) <= max(R * err_torch32(b, q), A[q])      (and <= 1e-3 in the benign row)

err_hip: the HIP fp32 result against the fp64 oracle; err_torch32: the oracle expression evaluated in fp32 on the CPU (autograd for
the gradients) against the same fp64 oracle, the WORST over NORD orders of the problem's context points.  The order changes nothing in
exact arithmetic and every rounding in fp32, so the spread of torch's error over the orders is what fp32 can lose on that problem --
its conditioning, measured -- where one evaluation is a single draw from it (a gradient that is a difference of two large sums, e.g.
d_noise = (|alpha|^2 - tr K^-1) / 2n at outputscale 50, loses 1e-5 in one order and 1e-3 in another).  Both start from the SAME
fp32-rounded inputs, so input rounding is not kernel error.
Per-problem errors (measure(), shared with tests/small_fp32_errors.py):
  LML                     |h - r| / max(|r|, 1)
  d_z[b], d_mean[b],      ||h - r|| / max(||r||, 1e-3 ||(d_ls, d_os, d_noise)_ref[b]||)   -- norm over the problem's own entries, no
  d_ls[b], d_os[b],          sum over tasks and no norm over the batch; the floor (a thousandth of that problem's hyper-gradient)
  d_noise[b]                 keeps gradients that are ~0 (short lengthscales: d_z ~ exp(-400)) from dividing by ~0
  mu[b], var[b], alpha[b], L[b]   ||h - r|| / max(||r||, 1e-3 sqrt(len))
Every launch holds six parameter rows in six regimes (ROWS), so every problem has neighbours in other regimes, and the batches mix
tasks of different valid sizes, shared and per-problem inputs, the three mean modes and per-problem weights of the LML."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacoh_oracle as O

DEV = 'cuda'
F64 = torch.float64
NORD = 8                               # orders of the context points torch fp32 is evaluated in (the first: as given)
BENIGN_CAP = 1e-3                      # no bar above this in the benign row

ROWS = [  # the parameter rows of every launch: name, lengthscale, outputscale, noise
    ('benign', 1.0, 1.0, 0.3),
    ('floor', 1.0, 1.0, 1e-3),         # the MAP noise floor
    ('long', 8.0, 1.0, 1e-2),          # long lengthscale: K close to rank one
    ('short', 0.05, 1.0, 0.3),         # short lengthscale: K ~ os I
    ('big_os', 1.0, 50.0, 0.3),
    ('tiny_os', 1.0, 1e-2, 1e-4),      # tiny outputscale with small noise
]

# Bars, from profiles/small_fp32_errors.txt (tests/small_fp32_errors.py on an MI355X).  Measured worst HIP errors, benign row: LML 3.6e-7,
# d_z 6.1e-6, d_mean 9.0e-6, d_ls 1.6e-4, d_os 4.0e-4, d_noise 2.6e-4, mu 7.8e-6, var 4.8e-7, alpha 1.4e-6, L 4.4e-7.  Against torch fp32's
# worst over the NORD point orders every HIP error is within 9.2x (d_z of a short-lengthscale problem, 3.6e-5), except a few entries
# that are tiny in absolute terms (one-point tasks, exact zeros): the worst of them beyond 10x torch is LML 1.7e-7, d_z 2.1e-6,
# d_mean 1.2e-7, d_ls 1.3e-6, d_os / d_noise 3.2e-7, alpha 8.6e-8 -- the floors A are 4x those.  R = 40 is 4.3x the worst ratio.
# The tightest entry is the benign row's d_os of 4.0e-4 (a problem whose d_os is ~0: measured against 1e-3 of its hyper-gradient;
# torch fp32 itself reaches 2.9e-4 over 200 point orders), 2.5x under BENIGN_CAP.  What this resolves: one problem (17-point kernel,
# 15 valid points, outputscale 50) loses 1.0e-3 on d_noise where torch in the given order loses 7.8e-6 -- but d_noise is there the
# difference of |alpha|^2 and tr K^-1, which cancel 300-fold, and torch's error over the point orders reaches 1.4e-3.
R = 40.0
A = dict(lml=1e-6, d_z=1e-5, d_mean=5e-7, d_ls=1e-5, d_os=2e-6, d_noise=2e-6, mu=1e-7, var=1e-7, alpha=5e-7, L=1e-7)


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


# ---------------------------------------------------------------------------------------------------------------------- problems
class Problem:
    """T tasks x the six ROWS, b = t * P + p; every input already rounded to fp32 (the fp64 oracle starts from the same values)"""

    def __init__(self, n, f, T, shared_z, mean, weighted, ragged, seed, with_os=True, m=0):
        P = len(ROWS)
        B = T * P
        g = torch.Generator().manual_seed(seed)
        q = lambda t: t.float()
        self.n, self.f, self.T, self.P, self.B, self.m, self.mean_mode = n, f, T, P, B, m, mean
        self.z_div = P if shared_z else 1
        self.z = q(1.5 / math.sqrt(f) * torch.randn(T if shared_z else B, n, f, generator=g, dtype=F64))
        self.y = q(torch.randn(T, n, generator=g, dtype=F64))
        base = torch.tensor([r[1] for r in ROWS], dtype=F64).unsqueeze(1)
        self.ls = q(base * (0.8 + 0.4 * torch.rand(P, f, generator=g, dtype=F64)))
        self.os = q(torch.tensor([r[2] for r in ROWS], dtype=F64)) if with_os else None
        self.noise = q(torch.tensor([r[3] for r in ROWS], dtype=F64))
        self.mean = {'zero': None, 'vector': q(0.3 * torch.randn(B, n, generator=g, dtype=F64)),
                     'const': q(0.3 * torch.randn(P, generator=g, dtype=F64))}[mean]
        self.gl = q(torch.rand(B, generator=g, dtype=F64) + 0.5) if weighted else None
        edges = [n, 1, 15, 16, 17, n - 1]                    # a full task first, then the sizes where the block masks go wrong
        self.sizes = [min(n, max(1, edges[t % 6])) for t in range(T)] if ragged else [n] * T
        self.ragged = ragged
        if m:                                                 # the predictive: test points per problem (or per task), test-point mean
            self.zt = q(1.5 / math.sqrt(f) * torch.randn(T if shared_z else B, m, f, generator=g, dtype=F64))
            self.mt = q(0.3 * torch.randn(B, m, generator=g, dtype=F64)) if mean == 'vector' else self.mean

    def perm(self, k):
        """[B, n] point order k of every problem: a permutation of its valid points (identity for k = 0 and beyond nv)"""
        pp = torch.arange(self.n).repeat(self.B, 1)
        if k:
            g = torch.Generator().manual_seed(1000 * k + self.n)
            for b in range(self.B):
                pp[b, :self.nv(b)] = torch.randperm(self.nv(b), generator=g)
        return pp

    def row(self, b):
        return ROWS[b % self.P][0]

    def nv(self, b):
        return self.sizes[b // self.P]

    # per-problem (b-indexed) copies of the inputs
    def per_problem(self):
        B, P = self.B, self.P
        t = torch.arange(B) // P
        p = torch.arange(B) % P
        z = self.z[t] if self.z_div == P else self.z
        mean = {'zero': torch.zeros(B, self.n), 'vector': self.mean,
                'const': None if self.mean is None else self.mean[p]}[self.mean_mode]
        os_ = self.os[p] if self.os is not None else torch.ones(B)
        gl = self.gl if self.gl is not None else torch.ones(B)
        return z, mean, self.y[t], self.ls[p], os_, self.noise[p], gl

    def groups(self):
        """problems grouped by valid size: the CPU oracle runs batched over each group"""
        sz = torch.tensor([self.nv(b) for b in range(self.B)])
        return [(int(s), (sz == s).nonzero().squeeze(1)) for s in torch.unique(sz)]

    def dev_args(self, L):
        d = lambda t: None if t is None else t.to(DEV)
        mode = {'zero': L.MEAN_ZERO, 'vector': L.MEAN_VECTOR, 'const': L.MEAN_CONST}[self.mean_mode]
        nv = d(torch.tensor(self.sizes, dtype=torch.int32)) if self.ragged else None
        return d(self.z), self.z_div, d(self.mean), mode, d(self.y), self.P, d(self.ls), d(self.os), d(self.noise), self.B, self.P, nv


def _gram(z, ls, os_, noise, dtype):
    n = z.shape[-2]
    return os_.reshape(-1, 1, 1) * O.gram_rbf_ard(z, z, ls.unsqueeze(1)) + noise.reshape(-1, 1, 1) * torch.eye(n, dtype=dtype)


def _no_jitter(z, ls, os_, noise, dtype):
    # the oracle's psd_safe_cholesky adds its jitter to the WHOLE batch when one matrix fails: none may here
    assert int(torch.linalg.cholesky_ex(_gram(z, ls, os_, noise, dtype))[1].abs().max()) == 0, 'the oracle needed jitter in %s' % dtype


def _take(t, pp):
    """rows pp[k] of t[k] (t: [k, s] or [k, s, f])"""
    return t.gather(1, pp if t.dim() == 2 else pp.unsqueeze(-1).expand(-1, -1, t.shape[-1]))


def oracle_lml_grads(pb, dtype, grads=True, order=0):
    """LML and per-problem gradients of the oracle (O.gp_mll, autograd) in `dtype`, one batched evaluation per valid size, with the
    context points in order `order` (Problem.perm); the gradients come back in the given order"""
    B, n, f = pb.B, pb.n, pb.f
    z, mean, y, ls, os_, noise, gl = pb.per_problem()
    perm = pb.perm(order)
    out = dict(lml=torch.zeros(B, dtype=F64), d_z=torch.zeros(B, n, f, dtype=F64), d_ls=torch.zeros(B, f, dtype=F64),
               d_os=torch.zeros(B, dtype=F64), d_noise=torch.zeros(B, dtype=F64),
               d_mean=torch.zeros(B, n, dtype=F64) if pb.mean_mode == 'vector' else torch.zeros(B, dtype=F64))
    for s, idx in pb.groups():
        leaf = lambda t: t.to(dtype).clone().requires_grad_(grads)
        pp = perm[idx, :s]
        zz, lsl, osl, nzl = leaf(z[idx, :s]), leaf(ls[idx]), leaf(os_[idx]), leaf(noise[idx])
        zp = _take(zz, pp)
        _no_jitter(zp.detach(), lsl.detach(), osl.detach(), nzl.detach(), dtype)
        if pb.mean_mode == 'vector':
            ml = leaf(mean[idx, :s])
            mv = _take(ml, pp)
        elif pb.mean_mode == 'const':
            ml = leaf(mean[idx])
            mv = ml.unsqueeze(1).expand(-1, s)
        else:
            ml, mv = None, torch.zeros(len(idx), s, dtype=dtype)
        v = O.gp_mll(zp, mv, _take(y[idx, :s], pp).to(dtype), lsl.unsqueeze(1), osl, nzl)
        out['lml'][idx] = v.detach().double()
        if not grads:
            continue
        (v * gl[idx].to(dtype)).sum().backward()
        out['d_z'][idx, :s] = zz.grad.double()
        out['d_ls'][idx], out['d_os'][idx], out['d_noise'][idx] = lsl.grad.double(), osl.grad.double(), nzl.grad.double()
        if pb.mean_mode == 'vector':
            out['d_mean'][idx, :s] = ml.grad.double()
        elif pb.mean_mode == 'const':
            out['d_mean'][idx] = ml.grad.double()
    return out


def oracle_chol(pb, dtype, order=0):
    """LML, Cholesky factor and alpha = K^-1 (y - mean) per problem in `dtype` (the outputs of the general kernel's forward), context
    points in order `order`; alpha comes back in the given order, the factor (which depends on the order) only for order 0"""
    B, n = pb.B, pb.n
    z, mean, y, ls, os_, noise, _ = pb.per_problem()
    mean = mean if pb.mean_mode == 'vector' else (mean.unsqueeze(1).expand(B, n) if pb.mean_mode == 'const' else torch.zeros(B, n))
    perm = pb.perm(order)
    out = dict(lml=torch.zeros(B, dtype=F64), alpha=torch.zeros(B, n, dtype=F64), L=torch.zeros(B, n, n, dtype=F64) if order == 0 else None)
    for s, idx in pb.groups():
        pp = perm[idx, :s]
        zz = _take(z[idx, :s], pp).to(dtype)
        lsl, osl, nzl = (t.to(dtype) for t in (ls[idx], os_[idx], noise[idx]))
        _no_jitter(zz, lsl, osl, nzl, dtype)
        mm, yy = _take(mean[idx, :s], pp).to(dtype), _take(y[idx, :s], pp).to(dtype)
        Lf = torch.linalg.cholesky(_gram(zz, lsl, osl, nzl, dtype))
        if order == 0:
            out['L'][idx, :s, :s] = Lf.double()
        ap = torch.cholesky_solve((yy - mm).unsqueeze(-1), Lf).squeeze(-1).double()
        out['alpha'][idx, :s] = torch.zeros(len(idx), s, dtype=F64).scatter(1, pp, ap)
        out['lml'][idx] = O.gp_mll(zz, mm, yy, lsl.unsqueeze(1), osl, nzl).double()
    return out


def oracle_predict(pb, dtype, order=0):
    """posterior mean and variance at the test points per problem in `dtype`, context points in order `order`"""
    B, m = pb.B, pb.m
    perm = pb.perm(order)
    z, mean, y, ls, os_, noise, _ = pb.per_problem()
    t = torch.arange(B) // pb.P
    zt = pb.zt[t] if pb.z_div == pb.P else pb.zt
    if pb.mean_mode == 'vector':
        mc, mt = mean, pb.mt
    elif pb.mean_mode == 'const':
        mc, mt = mean.unsqueeze(1).expand(B, pb.n), mean.unsqueeze(1).expand(B, m)
    else:
        mc, mt = torch.zeros(B, pb.n), torch.zeros(B, m)
    out = dict(mu=torch.zeros(B, m, dtype=F64), var=torch.zeros(B, m, dtype=F64))
    for s, idx in pb.groups():
        pp = perm[idx, :s]
        zz = _take(z[idx, :s], pp).to(dtype)
        lsl, osl, nzl = (t_.to(dtype) for t_ in (ls[idx], os_[idx], noise[idx]))
        _no_jitter(zz, lsl, osl, nzl, dtype)
        mu, cov = O.gp_predict(zz, _take(mc[idx, :s], pp).to(dtype), _take(y[idx, :s], pp).to(dtype), zt[idx].to(dtype), mt[idx].to(dtype),
                               lsl.unsqueeze(1), osl, nzl)
        out['mu'][idx], out['var'][idx] = mu.double(), torch.diagonal(cov, dim1=-2, dim2=-1).double()
    return out


# ---------------------------------------------------------------------------------------------------------------------- errors
def _per_problem(h, r, floor):
    B = r.shape[0]
    d = (h.double().cpu().reshape(B, -1) - r.reshape(B, -1)).norm(dim=1)
    return d / torch.maximum(r.reshape(B, -1).norm(dim=1), floor)


def _worst(errs):
    return torch.stack(errs).max(0).values


def _grad_errors(out, ref, cpus, names):
    """{q: (err_hip[B], err_torch32[B])} of the gradient outputs `names` (floor: 1e-3 x the problem's hyper-gradient); cpus: the torch
    fp32 results in the NORD orders"""
    hyper = torch.cat([ref['d_ls'], ref['d_os'].unsqueeze(1), ref['d_noise'].unsqueeze(1)], 1).norm(dim=1)
    floor = 1e-3 * hyper
    return {q: (_per_problem(out[q], ref[q], floor), _worst([_per_problem(c[q], ref[q], floor) for c in cpus])) for q in names}


def _lml_errors(h, ref, cpus):
    den = ref.abs().clamp_min(1.0)
    return (h.double().cpu() - ref).abs() / den, _worst([(c - ref).abs() / den for c in cpus])


def _vec_errors(h, ref, cpus, floor):
    return _per_problem(h, ref, floor), _worst([_per_problem(c, ref, floor) for c in cpus])


def measure(L, kind, pb):
    """run one case: the HIP launch(es), the fp64 oracle and the torch fp32 evaluation -> {quantity: (err_hip[B], err_torch32[B])}.
    kind: 'lml' (gp_lml_fwd, then gp_lml_fwdbwd), 'small' (gp_lml_fwd with alpha and L: the general kernel), 'predict'.
    Asserts what is exact on the way: clean Cholesky everywhere, padded rows of d_z / d_mean exactly 0, no d_os without outputscale."""
    args = pb.dev_args(L)
    errs = {}
    if kind == 'predict':
        mt = None if pb.mt is None else pb.mt.to(DEV)
        mu, var, cov, info = L.gp_predict(*args[:6], pb.zt.to(DEV), pb.z_div, mt, *args[6:11], n_valid=args[11])
        assert cov is None and int(info.abs().max()) == 0
        ref, cpus = oracle_predict(pb, F64), [oracle_predict(pb, torch.float32, k) for k in range(NORD)]
        for q, h in (('mu', mu), ('var', var)):
            floor = torch.full((pb.B,), 1e-3 * math.sqrt(pb.m), dtype=F64)
            errs[q] = _vec_errors(h, ref[q], [c[q] for c in cpus], floor)
        return errs
    if kind == 'small':
        assert pb.n <= L.gp_small_max_n(torch.float32, False)
        lml, alpha, Lf, info = L.gp_lml_fwd(*args[:11], n_valid=args[11], want_alpha=True, want_L=True)
        assert int(info.abs().max()) == 0
        ref, cpus = oracle_chol(pb, F64), [oracle_chol(pb, torch.float32, k) for k in range(NORD)]
        errs['lml'] = _lml_errors(lml, ref['lml'], [c['lml'] for c in cpus])
        alpha, Lf = alpha.cpu().double(), Lf.cpu().double()
        for b in range(pb.B):                                  # (what the kernel leaves beyond a ragged task's rows is not part of the contract)
            s = pb.nv(b)
            alpha[b, s:] = 0.0
            Lf[b, s:] = 0.0
            Lf[b, :, s:] = 0.0
        for q, h in (('alpha', alpha), ('L', Lf)):
            floor = torch.full((pb.B,), 1e-3 * math.sqrt(pb.n), dtype=F64)
            errs[q] = _vec_errors(h, ref[q], [c[q] for c in (cpus if q == 'alpha' else cpus[:1])], floor)   # (the factor: order 0)
        return errs
    lml_f, _, _, info_f = L.gp_lml_fwd(*args[:11], n_valid=args[11])
    out = L.gp_lml_fwdbwd(*args[:11], n_valid=args[11], g_lml=None if pb.gl is None else pb.gl.to(DEV), want_dz=True)
    lml, d_z, d_mean, d_ls, d_os, d_noise, info = out
    assert int(info_f.abs().max()) == 0 and int(info.abs().max()) == 0
    if pb.os is None:
        assert d_os is None                                    # (gp_reg_kernel<NB, 2, true, false> does not form it)
    assert (d_mean is None) == (pb.mean_mode == 'zero')
    for b in range(pb.B):                                      # padded rows: exactly zero
        s = pb.nv(b)
        assert float(d_z[b, s:].abs().sum()) == 0.0
        if pb.mean_mode == 'vector':
            assert float(d_mean[b, s:].abs().sum()) == 0.0
    ref, cpus = oracle_lml_grads(pb, F64), [oracle_lml_grads(pb, torch.float32, order=k) for k in range(NORD)]
    errs['lml_fwd'] = _lml_errors(lml_f, ref['lml'], [c['lml'] for c in cpus])
    errs['lml'] = _lml_errors(lml, ref['lml'], [c['lml'] for c in cpus])
    got = dict(d_z=d_z, d_ls=d_ls, d_noise=d_noise)
    names = ['d_z', 'd_ls', 'd_noise']
    if d_mean is not None:
        got['d_mean'] = d_mean
        names.insert(1, 'd_mean')
    if d_os is not None:
        got['d_os'] = d_os
        names.insert(-1, 'd_os')
    errs.update(_grad_errors(got, ref, cpus, names))
    return errs


def bars(errs_torch, q):
    """the bar of every problem: max(R x torch fp32's error, A[q]), at most BENIGN_CAP in the benign row"""
    bar = torch.clamp_min(R * errs_torch, A['lml' if q == 'lml_fwd' else q])
    benign = torch.tensor([ROWS[b % len(ROWS)][0] == 'benign' for b in range(len(bar))])
    return torch.where(benign, bar.clamp_max(BENIGN_CAP), bar)


def check(errs, tag):
    bad = []
    for q, (eh, ec) in errs.items():
        bar = bars(ec, q)
        for b in (eh > bar).nonzero().squeeze(1).tolist():
            bad.append('%s b=%d (%s): hip %.2e torch32 %.2e bar %.2e' % (q, b, ROWS[b % len(ROWS)][0], eh[b], ec[b], bar[b]))
    assert not bad, '%s\n  ' % (tag,) + '\n  '.join(bad[:20])


# ---------------------------------------------------------------------------------------------------------------------- cases
REG = [  # n, f, T, shared z, mean mode, g_lml weights, ragged   -- gp_reg_kernel<NB, FP, false> (gp_lml_fwd) and <NB, FP, true> (fwdbwd)
    (1, 1, 3, False, 'zero', False, False),        # <1, 2>: one point
    (1, 3, 3, True, 'const', True, False),         # <1, 4>
    (8, 2, 6, False, 'vector', True, True),        # <1, 2>, ragged (8, 1, 8, 8, 8, 7)
    (8, 4, 3, True, 'zero', False, False),         # <1, 4>
    (16, 1, 6, True, 'const', False, True),        # <1, 2>: one full block, ragged (16, 1, 15, 16, 16, 15)
    (16, 4, 3, False, 'vector', True, False),      # <1, 4>
    (17, 2, 3, False, 'const', True, False),       # <2, 2>: one row in the second block
    (17, 3, 6, False, 'zero', False, True),        # <2, 4>, ragged (17, 1, 15, 16, 17, 16)
    (33, 1, 3, True, 'vector', False, False),      # <3, 2>
    (33, 4, 6, False, 'const', True, True),        # <3, 4>, ragged
    (48, 2, 6, False, 'zero', True, True),         # <3, 2>: three full blocks, ragged
    (48, 3, 3, True, 'vector', False, False),      # <3, 4>
    (49, 2, 3, False, 'vector', False, False),     # <4, 2>
    (49, 4, 6, True, 'zero', True, True),          # <4, 4>, ragged
    (64, 1, 6, False, 'const', False, True),       # <4, 2>: cfg #3's context size, ragged
    (64, 4, 3, False, 'vector', True, False),      # <4, 4>
    (65, 2, 6, True, 'vector', True, True),        # <6, 2>: five blocks padded to six, ragged
    (65, 3, 3, False, 'zero', False, False),       # <6, 4>
    (80, 1, 3, False, 'const', True, False),       # <6, 2>
    (80, 4, 6, False, 'vector', False, True),      # <6, 4>, ragged
    (96, 2, 3, False, 'zero', False, False),       # <6, 2>: six full blocks
    (96, 3, 6, True, 'const', True, True),         # <6, 4>, ragged
    (97, 1, 6, False, 'vector', False, True),      # <8, 2>: seven blocks padded to eight, ragged
    (97, 4, 3, True, 'zero', True, False),         # <8, 4>
    (112, 2, 3, True, 'const', False, False),      # <8, 2>
    (112, 3, 6, False, 'vector', True, True),      # <8, 4>, ragged
    (113, 2, 6, False, 'zero', True, True),        # <8, 2>: one row in the eighth block, ragged
    (113, 4, 3, False, 'const', False, False),     # <8, 4>
    (128, 2, 3, False, 'vector', True, False),     # <8, 2>: cfg #4's context size
    (128, 4, 6, True, 'vector', False, True),      # <8, 4>, ragged
    (128, 2, 17, False, 'vector', True, True),     # <8, 2>, B = 102
    (64, 4, 17, True, 'const', False, True),       # <4, 4>, B = 102
    (33, 1, 17, False, 'zero', True, False),       # <3, 2>, B = 102
]
NO_OS = [  # outputscale None: gp_reg_kernel<NB, 2, true, false> (fwdbwd) and <NB, 2, false> with os = 1 (gp_lml_fwd)
    (64, 2, 6, False, 'vector', True, True),       # <4, 2, true, false>, ragged
    (49, 1, 3, True, 'zero', False, False),        # <4, 2, true, false>: 49 of 64 rows
    (128, 2, 17, False, 'const', True, True),      # <8, 2, true, false>, B = 102, ragged
    (100, 1, 3, True, 'vector', False, False),     # <8, 2, true, false>: 100 of 128 rows
]
MFMA = [  # f > 4: the LDS-resident gp_mfma_kernel<NB, NW, FP, false / true> (NW = 1 up to NB = 4, then 2)
    (9, 5, 3, False, 'vector', True, False),       # NB 1, FP 8
    (16, 16, 6, True, 'zero', False, True),        # NB 1, FP 16, ragged
    (20, 8, 6, False, 'const', False, True),       # NB 2, FP 8, ragged
    (32, 9, 3, False, 'vector', True, False),      # NB 2, FP 16
    (40, 16, 3, True, 'vector', False, False),     # NB 3, FP 16
    (48, 5, 6, False, 'zero', True, True),         # NB 3, FP 8, ragged
    (50, 8, 3, False, 'const', True, False),       # NB 4, FP 8
    (64, 9, 6, False, 'vector', False, True),      # NB 4, FP 16, ragged
    (65, 5, 6, True, 'vector', True, True),        # NB 5, FP 8, ragged
    (80, 16, 3, False, 'zero', False, False),      # NB 5, FP 16
    (90, 9, 3, False, 'const', True, False),       # NB 6, FP 16
    (96, 8, 6, False, 'vector', False, True),      # NB 6, FP 8, ragged
    (100, 16, 6, False, 'vector', True, True),     # NB 7, FP 16, ragged
    (112, 5, 3, True, 'const', False, False),      # NB 7, FP 8
    (113, 9, 3, False, 'zero', True, False),       # NB 8, FP 16
    (128, 8, 6, False, 'vector', True, True),      # NB 8, FP 8, ragged
    (128, 16, 17, False, 'vector', True, True),    # NB 8, FP 16, B = 102
]
SMALL = [  # gp_lml_fwd with alpha and L: the general kernel gp_small_kernel<float, FP, MODE_FWD> (group size pow2 >= n)
    (5, 2, 3, False, 'vector', False, False),      # FP 2, eight-lane groups
    (30, 4, 6, True, 'const', False, True),        # FP 4, ragged
    (64, 8, 3, False, 'zero', False, False),       # FP 8
    (100, 16, 6, False, 'vector', False, True),    # FP 16, 128-lane groups, ragged
    (150, 3, 3, False, 'const', False, False),     # FP 4, n > 128 (256-lane groups)
    (128, 2, 17, False, 'vector', False, True),    # FP 2, B = 102, ragged
]
PRED = [  # n, f, T, shared inputs, mean mode, m, ragged  -- gp_reg_predict_kernel<NB, FP>
    (1, 1, 3, False, 'zero', 5, False),            # <1, 2>: one context point
    (16, 3, 6, True, 'vector', 37, True),          # <1, 4>, ragged
    (17, 2, 6, False, 'const', 16, True),          # <2, 2>, ragged
    (20, 4, 3, False, 'vector', 1, False),         # <2, 4>: one test point
    (40, 1, 3, True, 'zero', 20, False),           # <3, 2>
    (33, 4, 6, False, 'vector', 37, True),         # <3, 4>, ragged
    (64, 2, 6, False, 'const', 37, True),          # <4, 2>, ragged
    (49, 3, 3, True, 'vector', 17, False),         # <4, 4>
    (65, 1, 6, False, 'vector', 40, True),         # <6, 2>, ragged
    (96, 4, 3, False, 'zero', 33, False),          # <6, 4>
    (100, 2, 6, True, 'const', 16, True),          # <8, 2>, ragged
    (128, 4, 3, False, 'vector', 37, False),       # <8, 4>
    (128, 2, 17, False, 'vector', 37, True),       # <8, 2>, B = 102, ragged
]


def make(kind, case, i):
    if kind == 'predict':
        n, f, T, shared, mean, m, ragged = case
        return Problem(n, f, T, shared, mean, False, ragged, seed=9000 + i, m=m)
    n, f, T, shared, mean, weighted, ragged = case
    seed = {'lml': 1000, 'no_os': 3000, 'mfma': 5000, 'small': 7000}[kind] + i
    return Problem(n, f, T, shared, mean, weighted, ragged, seed=seed, with_os=kind != 'no_os')


ALL = ([('lml', c, i) for i, c in enumerate(REG)] + [('no_os', c, i) for i, c in enumerate(NO_OS)] +
       [('mfma', c, i) for i, c in enumerate(MFMA)] + [('small', c, i) for i, c in enumerate(SMALL)] +
       [('predict', c, i) for i, c in enumerate(PRED)])


@pytest.mark.parametrize('kind,case,i', ALL, ids=['%s-%d-n%d-f%d' % (k, i, c[0], c[1]) for k, c, i in ALL])
def test_fp32_per_problem_error_against_torch_fp32(L, kind, case, i):
    pb = make(kind, case, i)
    errs = measure(L, {'no_os': 'lml', 'mfma': 'lml'}.get(kind, kind), pb)
    check(errs, (kind, case))


# ---------------------------------------------------------------------------------------------------------------------- jitter ladder
LADDER_ROWS = [  # name, lengthscale, outputscale, noise
    ('healthy', 1.0, 1.0, 0.3),
    ('ladder', 1.0, 2.0 ** -6, 5e-10),   # identical points: the fp32 matrix is os 1 1^T exactly, a zero pivot until the jitter
    ('failed', 1.0, 1.0, -1.0),          # K - I: indefinite on every rung
    ('healthy', 0.7, 2.0, 0.05),
]
LADDER_BAR = 2e-2                        # the laddered problem against the oracle at noise + jitter (condition ~ os / jitter ~ 1.6e4):
                                         # measured <= 4.5e-3 (LML, d_noise; profiles/small_fp32_errors.txt, rows `ladder`)


def ladder_launch(L, n, T, with_bad):
    f = 2
    rows = LADDER_ROWS if with_bad else [LADDER_ROWS[0], LADDER_ROWS[3]]
    P = len(rows)
    g = torch.Generator().manual_seed(n)
    z = 1.5 / math.sqrt(f) * torch.randn(T, len(LADDER_ROWS), n, f, generator=g, dtype=F64)
    z[:, 1] = z[:, 1, :1]                                    # the laddered row: n copies of one point
    mean = 0.3 * torch.randn(T, len(LADDER_ROWS), n, generator=g, dtype=F64)
    gl = torch.rand(T, len(LADDER_ROWS), generator=g, dtype=F64) + 0.5
    y = torch.randn(T, n, generator=g, dtype=F64)
    keep = [0, 1, 2, 3] if with_bad else [0, 3]
    z, mean, gl = (t[:, keep].reshape(T * P, *t.shape[2:]).float() for t in (z, mean, gl))
    ls = torch.tensor([[r[1]] * f for r in rows]).float()
    os_ = torch.tensor([r[2] for r in rows]).float()
    noise = torch.tensor([r[3] for r in rows]).float()
    args = [t.to(DEV) for t in (z, mean, y.float(), ls, os_, noise, gl)]
    out = L.gp_lml_fwdbwd(args[0], 1, args[1], L.MEAN_VECTOR, args[2], P, args[3], args[4], args[5], T * P, P, g_lml=args[6])
    return [o.cpu() for o in out], (z, mean, y.float(), ls, os_, noise, gl)


def ladder_errors(out, inputs, b, jitter):
    """per-output error of laddered problem b against the fp64 oracle at noise + jitter (rules of measure())"""
    z, mean, y, ls, os_, noise, gl = inputs
    P = len(LADDER_ROWS)
    p, t = b % P, b // P
    lv = [z[b].double().requires_grad_(True), mean[b].double().requires_grad_(True), ls[p].double().requires_grad_(True),
          os_[p].double().requires_grad_(True), noise[p].double().requires_grad_(True)]
    v = O.gp_mll(lv[0], lv[1], y[t].double(), lv[2], lv[3], lv[4] + jitter)
    (v * float(gl[b])).backward()
    ref = dict(lml=v.detach(), d_z=lv[0].grad, d_mean=lv[1].grad, d_ls=lv[2].grad, d_os=lv[3].grad, d_noise=lv[4].grad)
    floor = 1e-3 * float(torch.cat([lv[2].grad, lv[3].grad.reshape(1), lv[4].grad.reshape(1)]).norm())
    errs = dict(lml=abs(float(out[0][b]) - float(ref['lml'])) / max(abs(float(ref['lml'])), 1.0))
    for k, q in zip((1, 2, 3, 4, 5), ('d_z', 'd_mean', 'd_ls', 'd_os', 'd_noise')):
        errs[q] = float((out[k][b].double() - ref[q]).norm()) / max(float(ref[q].norm()), floor)
    return errs


@pytest.mark.parametrize('n', [32, 64, 96, 128])           # gp_reg_kernel<2 / 4 / 6 / 8, 2, true>
def test_jitter_ladder_per_problem(L, n):
    """one launch holding a problem that needs a rung of the jitter ladder, one that fails every rung and healthy neighbours: the healthy
    problems are bit for bit what a launch without the bad ones gives (one wave per problem), the laddered one matches the oracle at
    noise + 1e-6 10^(info - 1), the failed one reports info = -1 and NaN outputs -- and only that one"""
    T, P = 3, len(LADDER_ROWS)
    out, inputs = ladder_launch(L, n, T, True)
    ref_out, _ = ladder_launch(L, n, T, False)
    info = out[6]
    for t in range(T):
        for p, (name, *_rest) in enumerate(LADDER_ROWS):
            b = t * P + p
            vals = [out[0][b], out[1][b], out[2][b], out[3][b], out[4][b], out[5][b]]
            if name == 'failed':
                assert int(info[b]) == -1
                assert all(bool(torch.isnan(v).all()) for v in vals), b
                continue
            assert all(bool(torch.isfinite(v).all()) for v in vals), b
            if name == 'ladder':
                assert 1 <= int(info[b]) <= 3
                errs = ladder_errors(out, inputs, b, 1e-6 * 10 ** (int(info[b]) - 1))
                assert max(errs.values()) < LADDER_BAR, (b, errs)
                continue
            assert int(info[b]) == 0
            b2 = t * 2 + (0 if p == 0 else 1)
            for k in range(7):
                assert torch.equal(out[k][b], ref_out[k][b2]), (b, k)
