"""Large-n GP path (every n x n matrix materialised in HBM: gram -> MFMA-panel Cholesky -> triangular inverse -> batched MFMA
GEMM -> gradient contractions; csrc/dense_gp.hip) against the CPU oracle: same checks as the LDS-resident kernels, at sizes
beyond their limit and -- with the routing forced -- at small sizes where both device paths must agree."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacoh_oracle as O
from tests.test_gpu_kernels import make_problem, maxrel, oracle_mll, relerr

DEV = 'cuda:0'
TOL = {torch.float32: 2e-3, torch.float64: 1e-9}


@pytest.fixture()
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.FORCE_DENSE = True
    yield _lib
    _lib.FORCE_DENSE = False


CASES = [
    (2, 2, 64, 2, True),       # small: both device paths exist
    (3, 2, 47, 3, False),      # odd n, shared inputs (SE kernel on x)
    (2, 2, 200, 3, True),      # beyond the LDS-resident limit
    (1, 2, 300, 2, True),
    (2, 1, 512, 8, False),     # cfg #5 shape
    (1, 1, 33, 16, True),      # max feature dim, one row past a panel
]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('case', CASES)
def test_dense_lml_fwdbwd(L, dtype, case):
    T, P, n, f, pez = case
    z, mean, y, ls, os_, noise = make_problem(T, P, n, f, dtype, seed=7 * n + f, per_eval_z=pez, noise_lo=0.0)
    gl = torch.rand(T * P, dtype=dtype) + 0.5
    leaves = [t.double().clone().requires_grad_(True) for t in (z, mean, ls, os_, noise)]
    ref = oracle_mll(leaves[0], leaves[1], y.double(), leaves[2], leaves[3], leaves[4], T, P, pez)
    (ref * gl.double()).sum().backward()
    out = L.gp_lml_fwdbwd(z.to(DEV), 1 if pez else P, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV),
                          os_.to(DEV), noise.to(DEV), T * P, P, g_lml=gl.to(DEV), want_dz=pez)
    lml, d_z, d_mean, d_ls, d_os, d_noise, info = out
    assert int(info.abs().max()) == 0
    assert maxrel(lml, ref) < TOL[dtype]
    gtol = 1e-2 if dtype == torch.float32 else 1e-7
    if pez:
        assert relerr(d_z, leaves[0].grad) < gtol
    assert relerr(d_mean, leaves[1].grad) < gtol
    assert relerr(d_ls.reshape(T, P, f).sum(0), leaves[2].grad) < gtol
    assert relerr(d_os.reshape(T, P).sum(0), leaves[3].grad) < gtol
    assert relerr(d_noise.reshape(T, P).sum(0), leaves[4].grad) < gtol
    # forward-only entry point gives the same value
    lml2, _, _, info2 = L.gp_lml_fwd(z.to(DEV), 1 if pez else P, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV),
                                     os_.to(DEV), noise.to(DEV), T * P, P)
    assert torch.equal(lml2, lml) and int(info2.abs().max()) == 0


# VERDICT r4 (weak #2 / next #2): the sizes the README promises beyond the ones tested so far -- odd n and n mod 4 != 0 at every
# dtype, everything between 513 and ~1000 in fp32 incl. n = 784, the reference's largest training context
# (experiments/data_sim.py:563, MNIST).  LML and ALL gradients against the oracle's fp64 autograd; which kernel generation factors a
# size (left-looking: 97 <= n <= 512 with 16-byte rows; right-looking otherwise) is the dispatcher's business -- both must be right.
BIG = [(torch.float32, n) for n in (129, 255, 513, 640, 784, 1000)] + [(torch.float64, n) for n in (129, 255, 511, 640, 1000)]


@pytest.mark.parametrize('dtype,n', BIG)
def test_dense_lml_fwdbwd_at_odd_and_large_contexts(L, dtype, n):
    T, P, f = 1, 2, 3
    z, mean, y, ls, os_, noise = make_problem(T, P, n, f, dtype, seed=3 * n + 1, per_eval_z=True, noise_lo=0.05)
    gl = torch.rand(T * P, dtype=dtype) + 0.5
    leaves = [t.double().clone().requires_grad_(True) for t in (z, mean, ls, os_, noise)]
    ref = oracle_mll(leaves[0], leaves[1], y.double(), leaves[2], leaves[3], leaves[4], T, P, True)
    (ref * gl.double()).sum().backward()
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV), os_.to(DEV), noise.to(DEV), T * P, P,
                          g_lml=gl.to(DEV), want_dz=True)
    lml, d_z, d_mean, d_ls, d_os, d_noise, info = out
    assert int(info.abs().max()) == 0
    # fp32 bars (north star: 1e-2 rel).  Measured on these very problems, norm-wise against the fp64 oracle (tests/dense_fp32_errors.py ->
    # profiles/r06_dense_fp32_errors.txt): LML <= 6e-7, every gradient <= 1.5e-5 at n = 129 ... 1000 -- within 1-12x of what plain torch
    # fp32 autograd on the CPU loses on the same expression (<= 6e-6).  Asserted with a margin of ~20x on the worst measured entry
    assert maxrel(lml, ref) < (1e-4 if dtype == torch.float32 else 1e-9)
    gtol = 5e-4 if dtype == torch.float32 else 1e-7
    assert relerr(d_z, leaves[0].grad) < gtol and relerr(d_mean, leaves[1].grad) < gtol
    assert relerr(d_ls.reshape(T, P, f).sum(0), leaves[2].grad) < gtol
    assert relerr(d_os.reshape(T, P).sum(0), leaves[3].grad) < gtol and relerr(d_noise.reshape(T, P).sum(0), leaves[4].grad) < gtol
    lml2, _, _, info2 = L.gp_lml_fwd(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV), os_.to(DEV), noise.to(DEV), T * P, P)
    assert torch.equal(lml2, lml) and int(info2.abs().max()) == 0


def test_dense_predict_at_the_mnist_context_size(L):
    """posterior predictive at n = 784 context / 50 test points, fp32 (the reference's MNIST tasks): mean, variance, covariance"""
    T, P, n, m, f = 1, 2, 784, 50, 2
    z, mean, y, ls, os_, noise = make_problem(T, P, n, f, torch.float32, seed=11, noise_lo=0.05)
    g = torch.Generator().manual_seed(3)
    zt = torch.randn(T * P, m, f, generator=g)
    mt = 0.2 * torch.randn(T * P, m, generator=g)
    mu, var, cov, info = L.gp_predict(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, zt.to(DEV), 1, mt.to(DEV),
                                      ls.to(DEV), os_.to(DEV), noise.to(DEV), T * P, P, want_cov=True)
    B = T * P
    rm, rc = O.gp_predict(z.double(), mean.double(), y.unsqueeze(1).expand(T, P, n).reshape(B, n).double(), zt.double(), mt.double(),
                          ls.unsqueeze(0).expand(T, P, f).reshape(B, 1, f).double(), os_.unsqueeze(0).expand(T, P).reshape(B).double(),
                          noise.unsqueeze(0).expand(T, P).reshape(B).double())
    assert int(info.abs().max()) == 0 and relerr(mu, rm) < 1e-2 and relerr(cov, rc) < 1e-2


def test_dense_matches_lds_resident_kernels(L):
    """same inputs through both device paths (fp32, headline shape n=64, f=2)"""
    T, P, n, f = 4, 3, 64, 2
    z, mean, y, ls, os_, noise = [t.to(DEV) for t in make_problem(T, P, n, f, torch.float32, seed=1)]
    dense = L.gp_lml_fwdbwd(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, T * P, P)
    L.FORCE_DENSE = False
    small = L.gp_lml_fwdbwd(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, T * P, P)
    for a, b in zip(dense[:6], small[:6]):
        assert relerr(a, b) < 2e-3


def test_dense_const_and_zero_mean(L):
    T, P, n, f = 3, 2, 150, 2
    z, _, y, ls, os_, noise = make_problem(T, P, n, f, torch.float64, seed=11)
    c = torch.tensor([0.3, -0.7], dtype=torch.float64, requires_grad=True)
    ref = oracle_mll(z, c.unsqueeze(0).expand(T, P).reshape(-1, 1).expand(-1, n), y, ls, os_, noise, T, P)
    ref.sum().backward()
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, c.detach().to(DEV), L.MEAN_CONST, y.to(DEV), P, ls.to(DEV), os_.to(DEV),
                          noise.to(DEV), T * P, P)
    assert maxrel(out[0], ref) < 1e-9 and relerr(out[2].reshape(T, P).sum(0), c.grad) < 1e-8
    one = torch.ones(P, dtype=torch.float64)
    ref0 = oracle_mll(z, torch.zeros(T * P, n, dtype=torch.float64), y, ls, one, noise, T, P)
    out0 = L.gp_lml_fwdbwd(z.to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), P, ls.to(DEV), None, noise.to(DEV), T * P, P)
    assert maxrel(out0[0], ref0) < 1e-9 and out0[2] is None and out0[4] is None


def test_dense_ragged_n_valid(L):
    T, P, n, f = 4, 2, 140, 2
    sizes = [140, 5, 77, 1]
    z, mean, y, ls, os_, noise = make_problem(T, P, n, f, torch.float64, seed=5)
    nv = torch.tensor(sizes, dtype=torch.int32)
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV), os_.to(DEV),
                          noise.to(DEV), T * P, P, n_valid=nv.to(DEV))
    lml, d_z, d_mean, d_ls, d_os, d_noise, info = [o.cpu() for o in out]
    for t in range(T):
        s = sizes[t]
        for p in range(P):
            b = t * P + p
            zz = z[b, :s].clone().requires_grad_(True)
            mm = mean[b, :s].clone().requires_grad_(True)
            hy = [h.clone().requires_grad_(True) for h in (ls[p], os_[p], noise[p])]
            ref = O.gp_mll(zz, mm, y[t, :s], hy[0], hy[1], hy[2])
            ref.backward()
            assert abs(float(lml[b] - ref)) < 1e-9 * max(1, abs(float(ref)))
            assert relerr(d_z[b, :s], zz.grad) < 1e-7 and float(d_z[b, s:].abs().sum()) == 0
            assert relerr(d_mean[b, :s], mm.grad) < 1e-7 and float(d_mean[b, s:].abs().sum()) == 0
            assert relerr(d_ls[b], hy[0].grad) < 1e-7
            assert relerr(d_os[b], hy[1].grad) < 1e-7 and relerr(d_noise[b], hy[2].grad) < 1e-7


def test_dense_jitter_ladder(L):
    """identical points + ~zero noise: the fp32 factorisation fails, the retry launches re-build only that problem with
    gpytorch's psd_safe_cholesky jitter and report the attempt in info[]"""
    n, f = 160, 2
    gen = torch.Generator().manual_seed(21)
    z = torch.zeros(2, n, f, dtype=torch.float32)           # one task, two hyper-parameter sets: b = p
    z[1] = torch.randn(n, f, generator=gen)
    y = torch.randn(1, n, dtype=torch.float32, generator=gen)
    ls = torch.ones(2, f, dtype=torch.float32)
    noise = torch.tensor([1e-12, 0.3], dtype=torch.float32)
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 2, ls.to(DEV), None, noise.to(DEV), 2, 2)
    lml, info = out[0].cpu(), out[-1].cpu()
    assert int(info[0]) >= 1 and int(info[1]) == 0
    assert bool(torch.isfinite(lml).all()) and bool(torch.isfinite(out[3]).all())
    # the healthy problem is untouched by the retries
    ref1 = O.gp_mll(z[1].double(), torch.zeros(n, dtype=torch.float64), y[0].double(), ls[1].double(),
                    torch.tensor(1.0, dtype=torch.float64), noise[1].double())
    assert abs(float(lml[1]) - float(ref1)) < 1e-3 * abs(float(ref1))
    jit = 1e-6 * 10 ** (int(info[0]) - 1)
    K = torch.ones(n, n, dtype=torch.float64) + (1e-12 + jit) * torch.eye(n, dtype=torch.float64)
    ref0 = torch.distributions.MultivariateNormal(torch.zeros(n, dtype=torch.float64), K).log_prob(y[0].double()) / n
    assert abs(float(lml[0]) - float(ref0)) < 0.2 * abs(float(ref0))     # fp32 at condition ~1e8: loose by nature


@pytest.mark.parametrize('ragged', [False, True])
def test_dense_jitter_ladder_fp64_all_rungs_in_one_launch(L, ragged):
    """fp64, n = 200 (the left-looking kernel's sizes: the ladder's three rungs are ONE launch there -- a failed problem's workgroup
    rebuilds its own matrix with the jitter and factors it again): identical points with noise 1e-20 fail, succeed with jitter 1e-8
    and report attempt 1; the healthy problem beside it is untouched; with ragged tasks the padded rows stay identity rows"""
    n, f = 200, 3
    gen = torch.Generator().manual_seed(5)
    z = torch.zeros(2, n, f, dtype=torch.float64)
    z[1] = torch.randn(n, f, generator=gen, dtype=torch.float64)
    y = torch.randn(1, n, dtype=torch.float64, generator=gen)
    ls = torch.ones(2, f, dtype=torch.float64)
    noise = torch.tensor([1e-20, 0.3], dtype=torch.float64)
    nv = 170 if ragged else n
    n_valid = torch.tensor([nv], dtype=torch.int32, device=DEV) if ragged else None
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 2, ls.to(DEV), None, noise.to(DEV), 2, 2, n_valid=n_valid)
    lml, info = out[0].cpu(), out[-1].cpu()
    assert info.tolist() == [1, 0]
    assert bool(torch.isfinite(lml).all()) and all(bool(torch.isfinite(o).all()) for o in out[1:-1] if o is not None)
    ref1 = O.gp_mll(z[1, :nv], torch.zeros(nv, dtype=torch.float64), y[0, :nv], ls[1], torch.tensor(1.0, dtype=torch.float64), noise[1])
    assert abs(float(lml[1]) - float(ref1)) < 1e-9 * abs(float(ref1))
    K = torch.ones(nv, nv, dtype=torch.float64) + (1e-20 + 1e-8) * torch.eye(nv, dtype=torch.float64)
    ref0 = torch.distributions.MultivariateNormal(torch.zeros(nv, dtype=torch.float64), K).log_prob(y[0, :nv]) / nv
    assert abs(float(lml[0]) - float(ref0)) < 1e-4 * abs(float(ref0))      # (condition number 2e10: the factorisation itself is the error)


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('n,dtype', [(640, torch.float32), (1000, torch.float32), (640, torch.float64), (904, torch.float64)])
def test_dense_two_level_path_ladder_and_healthy_neighbours(L, n, dtype, ragged):
    """512 < n <= 1024, fp32 (round 5): rung 0 of the ladder is the two-level factorisation + inverse on the left-looking kernels and
    the tiled GEMM; a problem either sub-factorisation rejects takes the later rungs on the right-looking kernel and its inverse
    through the late mask; in fp64 no right-looking kernel takes these sizes (a call with gradients returned PACOH_ELIMIT above
    n ~ 520 until round 5) and the later rungs are two-level too, on the problems still marked failed.  Identical points with a
    negative noise term are indefinite until the jitter exceeds |noise|: -5e-6 (fp64: -5e-8) needs rung 2, -1e-2 fails every rung.
    info = [2, -1, 0, 0]; the healthy problems (one with the failing ones in its launch, one alone) agree bit for bit and with the
    oracle; gradients finite where info >= 0, NaN for the failure"""
    f = 3
    f64 = dtype == torch.float64
    gen = torch.Generator().manual_seed(n)
    z = torch.zeros(4, n, f, dtype=dtype)
    z[2] = torch.randn(n, f, generator=gen, dtype=dtype)
    z[3] = z[2]
    y = torch.randn(1, n, generator=gen, dtype=dtype)
    ls = torch.ones(4, f, dtype=dtype)
    jit2 = 1e-7 if f64 else 1e-5
    noise = torch.tensor([-0.5 * jit2, -1e-2, 0.3, 0.3], dtype=dtype)
    nv = n - 77 if ragged else n
    n_valid = torch.tensor([nv], dtype=torch.int32, device=DEV) if ragged else None
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 4, ls.to(DEV), None, noise.to(DEV), 4, 4, n_valid=n_valid, want_dz=True)
    lml, info = out[0].cpu(), out[-1].cpu()
    assert info.tolist() == [2, -1, 0, 0]
    grads = [o.cpu() for o in out[1:-1] if o is not None]
    for b in (0, 2, 3):
        assert bool(torch.isfinite(lml[b])) and all(bool(torch.isfinite(gr[b]).all()) for gr in grads), b
    assert bool(torch.isnan(lml[1]))
    assert torch.equal(lml[2], lml[3]) and all(torch.equal(gr[2], gr[3]) for gr in grads)
    leaves = [z[2, :nv].double().clone().requires_grad_(True), ls[2].double().clone().requires_grad_(True), noise[2].double().clone().requires_grad_(True)]
    ref = O.gp_mll(leaves[0], torch.zeros(nv, dtype=torch.float64), y[0, :nv].double(), leaves[1], torch.tensor(1.0, dtype=torch.float64), leaves[2])
    ref.backward()
    assert abs(float(lml[2]) - float(ref)) < (1e-9 if f64 else 1e-4) * abs(float(ref))
    d_z, d_ls, d_noise = out[1].cpu(), out[3].cpu(), out[5].cpu()
    gtol = 1e-7 if f64 else 1e-3                     # (fp32: profiles/r06_dense_fp32_errors.txt, rows `ladder`)
    assert relerr(d_z[2, :nv], leaves[0].grad) < gtol and relerr(d_ls[2], leaves[1].grad) < gtol and relerr(d_noise[2], leaves[2].grad) < gtol
    alone = L.gp_lml_fwdbwd(z[3:].to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 1, ls[3:].to(DEV), None, noise[3:].to(DEV), 1, 1, n_valid=n_valid, want_dz=True)
    assert torch.equal(alone[0].cpu()[0], lml[3])
    fwd = L.gp_lml_fwd(z.to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 4, ls.to(DEV), None, noise.to(DEV), 4, 4, n_valid=n_valid)
    assert fwd[-1].cpu().tolist() == [2, -1, 0, 0] and torch.equal(fwd[0].cpu()[2:], lml[2:])
    # the jittered rank-one problem: log-density of 1 1^T + (noise + jitter) I (ill-conditioned by construction: the factorisation is the error)
    K = torch.ones(nv, nv, dtype=torch.float64) + (float(noise[0]) + jit2) * torch.eye(nv, dtype=torch.float64)
    ref0 = torch.distributions.MultivariateNormal(torch.zeros(nv, dtype=torch.float64), K).log_prob(y[0, :nv].double()) / nv
    assert abs(float(lml[0]) - float(ref0)) < (1e-3 if f64 else 0.2) * abs(float(ref0))


@pytest.mark.parametrize('dtype,n,B', [(torch.float32, 1024, 1), (torch.float64, 1024, 2), (torch.float32, 516, 9), (torch.float64, 514, 3)])
def test_two_level_path_edges(L, dtype, n, B):
    """the ends of the two-level range: n = 1024 (two sub-blocks of 512), n = 514 / 516 (the smallest second sub-block the split
    produces: 194 / 196 rows), batches of 1 / 2 / 3 / 9 problems (the tiled GEMM deals workgroups to the XCDs in groups of eight
    problems: the remainder path) -- LML and the gradients the call returns against the oracle, forward-only bit-equal"""
    f, P = 2, 1
    z, mean, y, ls, os_, noise = make_problem(B, P, n, f, dtype, seed=n + B, per_eval_z=True, noise_lo=0.05)
    leaves = [t.double().clone().requires_grad_(True) for t in (z, mean, ls, os_, noise)]
    ref = oracle_mll(leaves[0], leaves[1], y.double(), leaves[2], leaves[3], leaves[4], B, P, True)
    ref.sum().backward()
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV), os_.to(DEV), noise.to(DEV), B * P, P, want_dz=True)
    lml, d_z, d_mean, d_ls, d_os, d_noise, info = out
    assert int(info.abs().max()) == 0
    # (fp32, measured: LML <= 1.4e-7, gradients <= 6.2e-5 -- d_ls at n = 1024, where torch fp32 itself is at 5.5e-6;
    #  profiles/r06_dense_fp32_errors.txt, rows `edge`)
    assert maxrel(lml, ref) < (1e-4 if dtype == torch.float32 else 1e-9)
    gtol = 1e-3 if dtype == torch.float32 else 1e-7
    assert relerr(d_z, leaves[0].grad) < gtol and relerr(d_mean, leaves[1].grad) < gtol
    assert relerr(d_ls.reshape(B, P, f).sum(0), leaves[2].grad) < gtol
    assert relerr(d_os.reshape(B, P).sum(0), leaves[3].grad) < gtol and relerr(d_noise.reshape(B, P).sum(0), leaves[4].grad) < gtol
    lml2, _, _, info2 = L.gp_lml_fwd(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, ls.to(DEV), os_.to(DEV), noise.to(DEV), B * P, P)
    assert torch.equal(lml2, lml) and int(info2.abs().max()) == 0


def test_two_level_path_is_what_ran(L):
    """PACOH_CHOL_BLOCKED=0 PACOH_TRTRI_BLOCKED=0 select the right-looking kernels at n = 640 fp32: the two runs must agree to rounding
    AND differ in the last bits, or the switch (and with it the claim that the two-level path ran in the tests above) is dead.  (The
    tiled GEMM has no such test: it accumulates k in the order of the kernel it replaces and returns the same bits --
    profiles/r05_dense_big_n.txt shows it by name.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, sys; sys.path.insert(0, '.'); from meta_learning_pacoh_amd import _lib as L\n"
            "g = torch.Generator().manual_seed(5)\n"
            "n = 640; z = torch.randn(2, n, 3, generator=g).cuda(); y = torch.randn(1, n, generator=g).cuda()\n"
            "ls = torch.ones(2, 3).cuda(); nz = torch.tensor([0.3, 0.2]).cuda()\n"
            "out = L.gp_lml_fwdbwd(z, 1, None, L.MEAN_ZERO, y, 2, ls, None, nz, 2, 2, want_dz=True); torch.cuda.synchronize()\n"
            "print(repr(float(out[0][0])), repr(float(out[1][1, 17, 2])), repr(float(out[3][0, 1])))\n")
    outs = []
    for env in (dict(os.environ), dict(os.environ, PACOH_CHOL_BLOCKED='0', PACOH_TRTRI_BLOCKED='0')):
        res = subprocess.run([sys.executable, '-c', code], cwd=root, env=env, capture_output=True, text=True, check=True)
        outs.append([float(v) for v in res.stdout.split()])
    a, b = outs
    assert all(abs(x - y) <= 2e-3 * max(abs(y), 1e-3) for x, y in zip(a, b)), (a, b)
    assert a != b, a


@pytest.mark.parametrize('ragged', [False, True])
def test_dense_jitter_ladder_fp64_every_rung_and_the_failure_exit(L, ragged):
    """the fused ladder (chol_ll_retry_kernel: up to three more factorisations inside ONE launch, the matrix rebuilt in the
    workgroup before each) beyond its first rung: identical points with a NEGATIVE noise term make K = 1 1^T + (noise +
    jitter) I indefinite until the jitter exceeds |noise| -- -5e-8 needs rung 2 (1e-7), -5e-7 rung 3 (1e-6), -1e-3 fails every rung:
    info = [2, 3, -1, 0], NaN outputs for the failure only, the second and third executions of the factorisation body give the
    log-density of the jittered matrix, and the healthy problem in the same launch equals a launch of its own bit for bit"""
    n, f = 200, 3
    gen = torch.Generator().manual_seed(9)
    z = torch.zeros(4, n, f, dtype=torch.float64)
    z[3] = torch.randn(n, f, generator=gen, dtype=torch.float64)
    y = torch.randn(1, n, dtype=torch.float64, generator=gen)
    ls = torch.ones(4, f, dtype=torch.float64)
    noise = torch.tensor([-5e-8, -5e-7, -1e-3, 0.3], dtype=torch.float64)
    nv = 170 if ragged else n
    n_valid = torch.tensor([nv], dtype=torch.int32, device=DEV) if ragged else None
    out = L.gp_lml_fwdbwd(z.to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 4, ls.to(DEV), None, noise.to(DEV), 4, 4, n_valid=n_valid)
    lml, info = out[0].cpu(), out[-1].cpu()
    assert info.tolist() == [2, 3, -1, 0]
    grads = [o.cpu() for o in out[1:-1] if o is not None]
    for b in (0, 1, 3):
        assert bool(torch.isfinite(lml[b])) and all(bool(torch.isfinite(gr[b]).all()) for gr in grads)
    assert bool(torch.isnan(lml[2]))
    for gr in grads:                                         # (per-point outputs: NaN on the task's own rows, 0 on padded ones)
        row = gr[2][:nv] if gr.dim() >= 2 and gr.shape[1] == n else gr[2]
        assert bool(torch.isnan(row).all())
    for b, jit in ((0, 1e-7), (1, 1e-6)):
        K = torch.ones(nv, nv, dtype=torch.float64) + (float(noise[b]) + jit) * torch.eye(nv, dtype=torch.float64)
        ref = torch.distributions.MultivariateNormal(torch.zeros(nv, dtype=torch.float64), K).log_prob(y[0, :nv]) / nv
        assert abs(float(lml[b]) - float(ref)) < 1e-4 * abs(float(ref)), (b, float(lml[b]), float(ref))
    alone = L.gp_lml_fwdbwd(z[3:].to(DEV), 1, None, L.MEAN_ZERO, y.to(DEV), 1, ls[3:].to(DEV), None, noise[3:].to(DEV), 1, 1, n_valid=n_valid)
    assert torch.equal(alone[0].cpu()[0], lml[3])
    for a_, o_ in zip(alone[1:-1], out[1:-1]):
        assert (a_ is None and o_ is None) or torch.equal(a_.cpu()[0], o_.cpu()[3])


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('case', [(2, 2, 64, 130, 4), (1, 2, 200, 50, 2), (1, 1, 300, 7, 3),
                                  # m >= 96: V = Z K_xs and cov = K_ss - V^T V on the LDS-tiled GEMM (round 5) -- aligned rows (16-byte
                                  # staging loads), misaligned rows and ragged tile edges (scalar staging), more than one tile each way
                                  (1, 2, 384, 128, 4), (1, 1, 333, 257, 2), (1, 2, 200, 130, 3),
                                  # 512 < n <= 1024: the two-level factorisation + inverse (fp64 had no path with an inverse here)
                                  (1, 2, 640, 100, 3), (1, 1, 904, 40, 2)])
def test_dense_predict(L, dtype, case):
    T, P, n, m, f = case
    B = T * P
    z, mean, y, ls, os_, noise = make_problem(T, P, n, f, dtype, seed=m, noise_lo=0.0)
    g = torch.Generator().manual_seed(99)
    zt = torch.randn(B, m, f, generator=g, dtype=dtype)
    mt = 0.2 * torch.randn(B, m, generator=g, dtype=dtype)
    mu, var, cov, info = L.gp_predict(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, zt.to(DEV), 1, mt.to(DEV),
                                      ls.to(DEV), os_.to(DEV), noise.to(DEV), B, P, want_cov=True)
    yy = y.unsqueeze(1).expand(T, P, n).reshape(B, n).double()
    lsb = ls.unsqueeze(0).expand(T, P, f).reshape(B, 1, f).double()
    osb = os_.unsqueeze(0).expand(T, P).reshape(B).double()
    nb = noise.unsqueeze(0).expand(T, P).reshape(B).double()
    rm, rc = O.gp_predict(z.double(), mean.double(), yy, zt.double(), mt.double(), lsb, osb, nb)
    tol = 5e-3 if dtype == torch.float32 else 1e-8
    assert int(info.abs().max()) == 0
    assert relerr(mu, rm) < tol
    assert relerr(var, torch.diagonal(rc, dim1=-2, dim2=-1)) < tol
    assert relerr(cov, rc) < tol
    mu2, var2, cov2, _ = L.gp_predict(z.to(DEV), 1, mean.to(DEV), L.MEAN_VECTOR, y.to(DEV), P, zt.to(DEV), 1, mt.to(DEV),
                                      ls.to(DEV), os_.to(DEV), noise.to(DEV), B, P, want_cov=False)
    assert cov2 is None and torch.equal(mu2, mu) and torch.equal(var2, var)


def test_dense_path_slabs_match_single_pass(L):
    """meta-batches whose O(B n^2) scratch exceeds the budget are processed in slabs of whole tasks: same results"""
    T, P, n, f = 5, 3, 150, 2
    z, mean, y, ls, os_, noise = [t.to(DEV) for t in make_problem(T, P, n, f, torch.float64, seed=3)]
    nv = torch.tensor([150, 40, 150, 7, 99], dtype=torch.int32, device=DEV)
    gl = (torch.rand(T * P, dtype=torch.float64) + 0.5).to(DEV)
    full = L.gp_lml_fwdbwd(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, T * P, P, n_valid=nv, g_lml=gl)
    budget = L.DENSE_WS_BYTES
    try:
        L.DENSE_WS_BYTES = 2 * L.load_library().pacoh_gp_lml_dense_workspace_bytes(P, n, f, L.F64, 1) + 1     # two tasks per slab
        slabs = L.gp_lml_fwdbwd(z, 1, mean, L.MEAN_VECTOR, y, P, ls, os_, noise, T * P, P, n_valid=nv, g_lml=gl)
        shared = L.gp_lml_fwdbwd(z[::P].contiguous(), P, None, L.MEAN_ZERO, y, P, ls, os_, noise, T * P, P, want_dz=False)
        L.DENSE_WS_BYTES = budget
        shared_full = L.gp_lml_fwdbwd(z[::P].contiguous(), P, None, L.MEAN_ZERO, y, P, ls, os_, noise, T * P, P, want_dz=False)
    finally:
        L.DENSE_WS_BYTES = budget
    for a, b in zip(full, slabs):
        assert torch.equal(a, b)
    for a, b in zip(shared_full, shared):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_dense_path_budget_with_inputs_shared_by_the_whole_batch(L, monkeypatch, dtype):
    """a batch the entry point cannot cut into slabs of whole tasks (z_div = y_div = B: one input set for every problem) gets the whole
    workspace even when it is over DENSE_WS_BYTES -- a capped buffer is PACOH_EINVAL there: same results as without the budget, and
    the oracle's"""
    T, P, n, f = 3, 2, 129, 2
    B = T * P
    z, mean, y, ls, os_, noise = make_problem(T, P, n, f, dtype, seed=129, noise_lo=0.05)
    z, y = z[:1].contiguous(), y[:1].contiguous()
    gl = torch.rand(B, dtype=dtype) + 0.5
    d = [t.to(DEV) for t in (z, mean, y, ls, os_, noise, gl)]
    call = lambda: L.gp_lml_fwdbwd(d[0], B, d[1], L.MEAN_VECTOR, d[2], B, d[3], d[4], d[5], B, P, g_lml=d[6])
    full = call()
    need = L.load_library().pacoh_gp_lml_dense_workspace_bytes(B, n, f, L.dtype_code(z), 1)
    monkeypatch.setattr(L, 'DENSE_WS_BYTES', need // 4)
    capped = call()
    for a, b in zip(full, capped):
        assert (a is None and b is None) or torch.equal(a, b)
    lml, d_z, d_mean, d_ls, d_os, d_noise, info = capped
    assert int(info.abs().max()) == 0
    leaves = [t.double().clone().requires_grad_(True) for t in (z[0].expand(B, n, f), mean, ls, os_, noise)]
    ref = oracle_mll(leaves[0], leaves[1], y[0].double().expand(T, n), leaves[2], leaves[3], leaves[4], T, P, True)
    (ref * gl.double()).sum().backward()
    tol_l, tol_g = (1e-4, 5e-4) if dtype == torch.float32 else (1e-9, 1e-7)
    assert maxrel(lml, ref) < tol_l
    assert relerr(d_z, leaves[0].grad) < tol_g and relerr(d_mean, leaves[1].grad) < tol_g
    assert relerr(d_ls.reshape(T, P, f).sum(0), leaves[2].grad) < tol_g
    assert relerr(d_os.reshape(T, P).sum(0), leaves[3].grad) < tol_g and relerr(d_noise.reshape(T, P).sum(0), leaves[4].grad) < tol_g


@pytest.mark.parametrize('dtype,n', [(torch.float32, 509), (torch.float64, 255), (torch.float32, 641)])
def test_raw_c_abi_call_pads_and_slabs_by_itself(L, dtype, n):
    """a host that binds pacoh_gp_lml_dense directly gets what the Python binding gives -- a
    context size with misaligned rows is run as a ragged batch of the next aligned size INSIDE the call (left-looking kernels:
    profiles/r06_raw_abi_n509_kernels.txt shows them by name), and a workspace that holds fewer problems than the batch makes the call
    loop over slabs of whole tasks.  Raw ctypes call, no helper of _lib in between; against the oracle and bit-equal across slab sizes"""
    import ctypes
    lib = L.load_library()
    T, P, f = 3, 2, 3
    B = T * P
    code = L.F32 if dtype == torch.float32 else L.F64
    z, mean, y, ls, os_, noise = [t.to(DEV) for t in make_problem(T, P, n, f, dtype, seed=n, per_eval_z=True, noise_lo=0.05)]
    nv = torch.tensor([n, n - 30, n], dtype=torch.int32, device=DEV)

    def call(ws_bytes):
        out = dict(lml=torch.empty(B, dtype=dtype, device=DEV), d_z=torch.full((B, n, f), float('nan'), dtype=dtype, device=DEV),
                   d_mean=torch.full((B, n), float('nan'), dtype=dtype, device=DEV), d_ls=torch.empty(B, f, dtype=dtype, device=DEV),
                   d_os=torch.empty(B, dtype=dtype, device=DEV), d_noise=torch.empty(B, dtype=dtype, device=DEV),
                   info=torch.empty(B, dtype=torch.int32, device=DEV))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = lib.pacoh_gp_lml_dense(p(z), 1, p(mean), L.MEAN_VECTOR, p(y), P, p(ls), p(os_), p(noise), p(nv), None, p(out['lml']), p(out['d_z']),
                                    p(out['d_mean']), p(out['d_ls']), p(out['d_os']), p(out['d_noise']), p(out['info']), p(ws), ws_bytes,
                                    B, P, n, f, code, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, out
    need_all = lib.pacoh_gp_lml_dense_workspace_bytes(B, n, f, code, 1)
    need_one = lib.pacoh_gp_lml_dense_workspace_bytes(P, n, f, code, 1)
    assert 0 < need_one < need_all
    rc, whole = call(need_all)
    assert rc == 0 and int(whole['info'].abs().max()) == 0
    rc1, one_task = call(need_one)                       # three slabs
    rc2, two_tasks = call(2 * need_one)                  # two slabs (2 + 1 tasks)
    assert rc1 == 0 and rc2 == 0
    for k in whole:
        assert torch.equal(whole[k], one_task[k]) and torch.equal(whole[k], two_tasks[k]), k
    assert call(need_one - 1)[0] == -1                   # PACOH_EINVAL: not even one task fits
    # the oracle on the ragged tasks (rows >= n_valid are ignored: their gradients are exact zeros)
    tol_l, tol_g = (1e-4, 1e-3) if dtype == torch.float32 else (1e-9, 1e-7)
    for t in range(T):
        m_ = int(nv[t])
        for p_ in range(P):
            b = t * P + p_
            lv = [z[b, :m_].double().cpu().requires_grad_(True), mean[b, :m_].double().cpu().requires_grad_(True)]
            ref = O.gp_mll(lv[0], lv[1], y[t, :m_].double().cpu(), ls[p_].double().cpu(), os_[p_].double().cpu(), noise[p_].double().cpu())
            ref.backward()
            assert abs(float(whole['lml'][b]) - float(ref)) < tol_l * abs(float(ref))
            assert relerr(whole['d_z'][b, :m_], lv[0].grad) < tol_g and relerr(whole['d_mean'][b, :m_], lv[1].grad) < tol_g
            assert float(whole['d_z'][b, m_:].abs().max() if m_ < n else 0.0) == 0.0
