"""Pathwise posterior function draws (csrc/gp_path.hip: pacoh_gp_path_fit / pacoh_gp_path_eval) and what is built on them, on the GPU.

Batches: tests/test_gpu_cond.make_case / Dev (3 parameter rows, noise ratios 0.02 / 0.05 / 0.3, the rotating z_div / zt_div / mean
modes), conditioned with L.gp_condition.  Error per problem, in normalised space,
  e = max_{s,t} |out - ref| / sqrt(os_p),     ref = tests/path_ref.paths_direct in fp64 on the same inputs and base.
fp64: e <= 1e-10, the bar of tests/test_gpu_cond.py.  The two fp64 forms of tests/path_ref.py (through the kept X, through a dense
  solve) are compared on every case of this module as well and must agree to 1e-11: the bar is not taken from the kernels.
fp32: the rule of tests/test_gpu_fp32_accuracy.py,  e_hip <= max(R e_torch32, A),  R = 40,  e_torch32 = tests/path_ref.paths in torch
  fp32 on the CPU on the same fp32-rounded inputs, the worst over NORD = 8 orders of the context points.  The floor A follows that
  module's rule from profiles/path_fp32_errors.txt (tests/path_fp32_errors.py, which shares measure() below).
Learners: model.condition().sample_paths() through the public API."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_ref as R                                               # noqa: E402
import path_ref as PR                                              # noqa: E402
import test_gpu_cond as TC                                         # noqa: E402  (make_case / Dev / build_learner / LEARNER_BAR)
import test_gpu_loo as TL                                          # noqa: E402
import test_gpu_fp32_accuracy as FA                                # noqa: E402  (R / NORD: the fp32 yardstick's own)

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
BAR64, BAR_REF = 1e-10, 1e-11
NORD, R40 = FA.NORD, FA.R
NS = (1, 2, 15, 16, 17, 63, 64, 65, 128, 'limit')
MS = (1, 15, 16, 17, 64, 65, 200)                       # the test-tile (64) and MFMA-tile (16) edges
SS = (1, 15, 16, 17, 33, 65)                            # the draw-tile (16), fit-group (16) and eval-group (64) edges
DS = (16, 48, 1024)                                     # one slab, a partial chunk of 64 columns, many chunks
FS = (1, 4, 5, 16)
FAMS = PR.FAMILIES
APPENDS = ((7, 2), (64, 1), (100, 28), ('limit-1', 1))
N_SWEEP = 12                                            # every value of every axis above appears at least once in 12 rotations
N_SPECS = N_SWEEP + len(APPENDS) + 1

# fp32 floor, from profiles/path_fp32_errors.txt (tests/path_fp32_errors.py on an MI355X) by the rule of
# tests/test_gpu_fp32_accuracy.py: 4x the worst HIP error among the problems beyond 10x torch fp32, 0 if there is none.  No problem
# is beyond 10x torch: no floor.  Measured: worst ratio hip / torch32 6.3, so R = 40 has a factor 6 in hand; worst HIP error 1.5e-3
# (the planted frequency of norm 3e4, where the fp32 argument of the cosine is itself off by 1e-3 radians and torch loses 2.5e-3);
# without it 3.0e-4.  Learner rows: 7e-7 .. 1.6e-6 on both sides.
A32 = 0.0


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


# ---------------------------------------------------------------------------------------------------------------------- cases
class Spec:
    """one case: condition on n0 points with capacity cap, append k, S draws on D features, m test points"""

    def __init__(self, tag, n0, k, cap, m, S, D, f, fam, case_no, planted=False):
        self.tag, self.n0, self.k, self.cap, self.m, self.S, self.D, self.f, self.fam = tag, n0, k, cap, m, S, D, f, fam
        self.case_no, self.planted, self.n = case_no, planted, n0 + k

    def build(self, fp32):
        """-> (TC.Case, base) in fp64, rounded to fp32 first when the launch is fp32"""
        case = TC.make_case(self.n, self.f, self.fam, self.case_no, self.m, fp32=fp32, T=3 if self.n <= 65 else 1)
        q = (lambda t: t.float().double()) if fp32 else (lambda t: t)
        omega, phase = PR.frequencies(self.fam, self.D, self.f, seed=7000 + self.case_no)
        if self.planted:                                # a Cauchy-tail frequency: arguments of 1e4 .. 1e5 radians
            d = torch.arange(1, self.f + 1, dtype=F64)
            omega[3] = 3.0e4 * d / d.norm()
        g = torch.Generator().manual_seed(8000 + self.case_no)
        w = torch.randn(case.b.B, self.S, self.D, generator=g, dtype=F64)
        eps = torch.randn(case.b.B, self.S, self.n, generator=g, dtype=F64)
        return case, tuple(q(t) for t in (omega, phase, w, eps))


def specs(limit):
    out = []
    for ci in range(N_SWEEP):
        n = NS[ci % len(NS)]
        n = limit if n == 'limit' else n
        m, S, D = MS[ci % len(MS)], SS[ci % len(SS)], DS[(ci + ci // 3) % len(DS)]
        f, fam = FS[ci % len(FS)], FAMS[(ci + ci // 4) % len(FAMS)]
        cap = (n, min(limit, n + 5), limit)[ci % 3]
        out.append(Spec('n=%d m=%d S=%d D=%d f=%d %s cap=%d' % (n, m, S, D, f, fam, cap), n, 0, cap, m, S, D, f, fam, 2000 + ci))
    for i, (n0, k) in enumerate(APPENDS):
        n0 = limit - 1 if n0 == 'limit-1' else n0
        cap = (min(limit, n0 + k + 6), limit)[i % 2]
        f, fam, S, D = (2, 16, 4, 5)[i], FAMS[i], (5, 20, 16, 3)[i], (48, 64, 256, 32)[i]
        out.append(Spec('append n0=%d k=%d S=%d D=%d f=%d %s cap=%d' % (n0, k, S, D, f, fam, cap), n0, k, cap, 33, S, D, f, fam, 2100 + i))
    out.append(Spec('planted |omega| = 3e4, m12', 20, 0, 24, 40, 6, 48, 3, 'm12', 2200, planted=True))
    assert len(out) == N_SPECS
    sp = out[:N_SWEEP]                                   # every value of every axis at least once
    assert {s.n0 for s in sp} == {limit if n == 'limit' else n for n in NS}
    assert {s.m for s in sp} == set(MS) and {s.S for s in sp} == set(SS) and {s.D for s in sp} == set(DS)
    assert {s.f for s in sp} == set(FS) and {s.fam for s in sp} == set(FAMS)
    return out


def launch(L, spec, case, base, dtype, noise=None):
    """condition (+ append) + fit + eval -> (v [B,S,n], out [B,S,m], info [B]) on the CPU"""
    dev = TC.Dev(L, case, dtype, noise=noise)
    state = dev.condition(spec.n0, spec.cap)
    if spec.k:
        assert int(dev.append(state, spec.n0, spec.k).abs().sum()) == 0
    omega, phase, w, eps = (t.to(dtype).to(DEV).contiguous() for t in base)
    b = case.b
    v = L.gp_path_fit(state, spec.n, omega, phase, w, eps, dev.os, dev.noise, b.B, b.P, kernel=dev.kernel)
    out = L.gp_path_eval(state[0], spec.n, v, omega, phase, w, state[4], dev.zt, case.zt_div, dev.mt, dev.mode, dev.ls, dev.os, b.B, b.P,
                         kernel=dev.kernel)
    assert tuple(v.shape) == (b.B, spec.S, spec.n) and tuple(out.shape) == (b.B, spec.S, spec.m)
    return v.cpu(), out.cpu(), state[4].cpu()


def problem_inputs(case, b, base):
    """problem b in fp64 -> the arguments of PR.paths_direct after zs / resid"""
    z, mean, y, ls, os_, noise = case.b.problem(b)
    zt, mt = case.test_points(b)
    omega, phase, w, eps = base
    return z, mean, y, (zt, mt, ls, os_, noise, 0.0, case.b.family, omega, phase, w[b]), eps[b]


def reference(case, b, base):
    z, mean, y, args, eps = problem_inputs(case, b, base)
    return PR.paths_direct(z / args[2], y - mean, *args, eps)


def err(out, ref, os_):
    return float((out.double() - ref).abs().max()) / math.sqrt(os_)


# ---------------------------------------------------------------------------------------------------------------------- fp64
@pytest.mark.parametrize('ci', range(N_SPECS))
def test_fp64_against_the_direct_reference(L, ci):
    spec = specs(TC.limit_of(L, F64))[ci]
    case, base = spec.build(False)
    v, out, info = launch(L, spec, case, base, F64)
    assert int(info.abs().max()) == 0
    worst = worst_ref = 0.0
    for b in range(case.b.B):
        z, mean, y, args, eps = problem_inputs(case, b, base)
        ls, os_, noise = args[2], args[3], args[4]
        ref = PR.paths_direct(z / ls, y - mean, *args, eps)
        X, _ = R.direct(z, mean, y, ls, os_, noise, family=case.b.family)
        e_ref = err(PR.paths(X, z / ls, y - mean, *args, eps), ref, os_)
        assert e_ref <= BAR_REF, ('the two fp64 reference forms disagree', spec.tag, b, e_ref)
        vref = PR.fit_direct(z / ls, y - mean, os_, noise, 0.0, case.b.family, base[0], base[1], base[2][b], eps)
        e_v = float((v[b] - vref).abs().max() / vref.abs().max())
        e = err(out[b], ref, os_)
        worst, worst_ref = max(worst, e), max(worst_ref, e_ref)
        print('%s b=%d e %.2e (v %.2e; reference forms %.2e)' % (spec.tag, b, e, e_v, e_ref))
        assert e <= BAR64, (spec.tag, b, e)
    print('%s worst %.2e, reference forms %.2e' % (spec.tag, worst, worst_ref))


@pytest.mark.parametrize('dtype', [F64, F32])
def test_failed_row_among_good_neighbours(L, dtype):
    """the second parameter row's noise is 10 below: its Cholesky fails on every rung (info = -1), its v and out are NaN, and its
    neighbours are bit for bit what a clean run gives (S = 17: two fit groups; m = 65: two test tiles)"""
    limit = TC.limit_of(L, dtype)
    spec = Spec('failed row', 9, 0, 12, 65, 17, 48, 2, 'rbf', 2300)
    case, base = spec.build(dtype == F32)
    good = launch(L, spec, case, base, dtype)
    bad_noise = case.b.noise.clone()
    bad_noise[1] -= 10.0
    bad = launch(L, spec, case, base, dtype, noise=bad_noise)
    assert limit >= spec.cap
    for b in range(case.b.B):
        if b % TC.P3 == 1:
            assert int(bad[2][b]) == -1 and bool(torch.isnan(bad[0][b]).all()) and bool(torch.isnan(bad[1][b]).all())
        else:
            assert int(bad[2][b]) == 0
            assert torch.equal(bad[0][b], good[0][b]) and torch.equal(bad[1][b], good[1][b]), b
            assert bool(torch.isfinite(good[1][b]).all())


# ---------------------------------------------------------------------------------------------------------------------- fp32
def _orders(s):
    for k in range(NORD):
        yield torch.arange(s) if k == 0 else torch.randperm(s, generator=torch.Generator().manual_seed(1000 * k + s))


def torch32_error(case, b, base, ref):
    """e of tests/path_ref.paths in torch fp32 on the CPU (X from tests/cond_ref.direct in fp32), the worst over NORD orders of the
    context points"""
    z, mean, y, args, eps = problem_inputs(case, b, base)
    zt, mt, ls, os_, noise, _, fam, omega, phase, w = args
    worst = 0.0
    for p in _orders(z.shape[0]):
        z0, m0, y0 = z[p].float(), mean[p].float(), y[p].float()
        X, _ = R.direct(z0, m0, y0, ls.float(), os_, noise, family=fam)
        out = PR.paths(X, z0 / ls.float(), y0 - m0, zt.float(), mt.float(), ls.float(), os_, noise, 0.0, fam, omega.float(),
                       phase.float(), w.float(), eps[:, p].float())
        worst = max(worst, err(out, ref, os_))
    return worst


def measure(L, spec):
    """one fp32 condition (+ append) + fit + eval -> [(e of HIP, e of torch fp32)] per problem; asserts clean Choleskys on the way"""
    case, base = spec.build(True)
    v, out, info = launch(L, spec, case, base, F32)
    assert int(info.abs().max()) == 0
    rows = []
    for b in range(case.b.B):
        ref = reference(case, b, base)
        rows.append((err(out[b], ref, case.b.problem(b)[4]), torch32_error(case, b, base, ref)))
    return rows


@pytest.mark.parametrize('ci', range(N_SPECS))
def test_fp32_per_problem_error_against_torch_fp32(L, ci):
    assert A32 is not None, 'the floor A32 has not been set from profiles/path_fp32_errors.txt'
    spec = specs(TC.limit_of(L, F32))[ci]
    bad = []
    for b, (h, c) in enumerate(measure(L, spec)):
        bar = max(R40 * c, A32)
        print('%s b=%d hip %.2e torch32 %.2e bar %.2e' % (spec.tag, b, h, c, bar))
        if not h <= bar:
            bad.append('b=%d: hip %.2e torch32 %.2e bar %.2e' % (b, h, c, bar))
    assert not bad, '%s\n  ' % spec.tag + '\n  '.join(bad[:20])


# ---------------------------------------------------------------------------------------------------------------------- limits
def test_refused_calls_launch_nothing(L):
    """every PACOH_ELIMIT / PACOH_EINVAL of the C entry points leaves v / out (zero-filled before) untouched"""
    for dtype in (F32, F64):
        limit = TC.limit_of(L, dtype)
        B, P, f, n, cap, S, D, m = 2, 1, 2, 4, 6, 3, 32, 5
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)
        one = torch.ones(1, dtype=dtype, device=DEV)
        state = L.gp_condition(z(B, n, f), 1, None, L.MEAN_ZERO, z(B, n), 1, one.reshape(1, 1).expand(1, f).contiguous(), one, one, B, P,
                               capacity=cap)
        zs, resid, X, alpha, info = state
        omega, phase, w, eps, v, out, zt, ls = z(D, f), z(D), z(B, S, D), z(B, S, n), z(B, S, n), z(B, S, m), z(B, m, f), z(1, f) + 1
        lib, p, code, st = L.load_library(), L._ptr, L.dtype_code(zs), L._stream()

        def fit(n=n, cap=cap, S=S, D=D, kf=f, v_=v, B=B):
            return lib.pacoh_gp_path_fit(p(zs), p(resid), p(X), p(info), p(one), p(one), p(omega), p(phase), p(w), p(eps),
                                         None if v_ is None else p(v_), B, P, n, cap, S, D, kf, code, st)

        def ev(n=n, cap=cap, S=S, D=D, m=m, kf=f, zt_=zt, zt_div=1, B=B):
            return lib.pacoh_gp_path_eval(p(zs), p(v), p(w), p(info), p(omega), p(phase), None if zt_ is None else p(zt_), zt_div, None,
                                          L.MEAN_ZERO, p(ls), p(one), p(out), B, P, n, cap, S, D, m, kf, code, st)

        for call in (fit, ev):
            assert call(n=cap + 1) == -2 and call(cap=limit + 1) == -2 and call(n=0) == -2
            assert call(kf=17) == -2 and call(kf=f | (2 << L.KERNEL_SHIFT)) == -2 and call(kf=f | (L.KERNEL_COSINE << L.KERNEL_SHIFT)) == -2
            assert call(D=8) == -2 and call(D=24) == -2 and call(D=16400) == -2 and call(S=0) == -2
            assert call(B=0) == -1
        assert ev(m=0) == -2 and ev(zt_=None) == -1 and ev(zt_div=0) == -1 and fit(v_=None) == -1
        torch.cuda.synchronize()
        assert float(v.abs().sum()) == 0.0 and float(out.abs().sum()) == 0.0
        assert fit() == 0 and ev() == 0                              # ... and the well-formed calls run
        torch.cuda.synchronize()
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------------------------- learners
FAMILY_OF = {0: 'rbf', 3: 'm12', 4: 'm32', 5: 'm52'}


def _tx():
    return np.linspace(-3.5, 3.5, 23).reshape(-1, 1)


def _condition(kind):
    model, kw = TC.build_learner(kind)
    cx, cy = TL.tiny_tasks()[1]
    torch.manual_seed(4321)
    return model, model.condition(cx[:4], cy[:4], **kw), cx, cy


def learner_errors(cond, paths, tx):
    """paths(tx) against tests/path_ref.paths_direct on the state pulled to the CPU -> [(e of HIP, e of torch fp32)] per parameter
    row; the test features and means are the engine's own (code this feature does not touch)"""
    snap, eng = paths._snap, cond._engine
    P, S, n, m = snap.w.shape[0], snap.w.shape[1], snap.n, tx.shape[0]
    fam = FAMILY_OF[eng.layout.kernel_code]
    zt, zt_div, mt, mode = eng._features(snap.theta, cond._norm_x(tx).unsqueeze(0).contiguous(), 1, m)
    zt, mt = zt.cpu().double(), None if mt is None else mt.cpu().double()
    zs = snap.zs.cpu().double()
    # the residuals are not part of the snapshot: they are those of the first n points of the state the draws were fitted on
    resid = cond._state.bufs[1][:, :n].cpu().double()
    ls, os_, noise = (None if h is None else h.cpu().double() for h in snap.hypers)
    info = snap.info.cpu()
    omega, phase, w, eps = (t.cpu().double() for t in paths.base)
    y_mean, y_std = float(cond._y_mean.reshape(-1)[0]), float(cond._y_std.reshape(-1)[0])
    out = ((paths(tx).cpu().double() - y_mean) / y_std).view(P, S, m)
    rows = []
    for p in range(P):
        rung = int(info[p])
        jit = 0.0 if rung == 0 else 1e-6 * 10 ** (rung - 1)
        o = 1.0 if os_ is None else float(os_[p])
        mp = torch.zeros(m, dtype=F64) if mode == 0 else (mt.reshape(P, m)[p] if mode == 1 else mt.reshape(-1)[p].expand(m))
        ztp = zt[p // zt_div]
        args = (ztp, mp, ls[p], o, float(noise[p]), jit, fam, omega, phase, w[p])
        ref = PR.paths_direct(zs[p], resid[p], *args, eps[p])
        worst = 0.0
        for q in _orders(n):
            a32 = tuple(t.float() if torch.is_tensor(t) else t for t in args)
            worst = max(worst, err(PR.paths_direct(zs[p][q].float(), resid[p][q].float(), *a32, eps[p][:, q].float()), ref, o))
        rows.append((err(out[p], ref, o), worst))
    return rows


@pytest.mark.parametrize('kind', TC.KINDS)
def test_learners_zero_base_is_the_posterior_mean(L, kind):
    """with w = 0 and eps = 0 every path is the posterior mean of its parameter row: against cond_predict (code this feature does not
    touch), per component, in units of the predictive std, at the bar of tests/test_gpu_cond.py"""
    model, cond, cx, cy = _condition(kind)
    tx = _tx()
    P, f, S, D = cond._state.theta.shape[0], model.engine.layout.feature_dim, 3, 64
    omega, phase = PR.frequencies('rbf', D, f, seed=1)
    d = lambda t: t.to(model.dtype).to(DEV)
    base = (d(omega), d(phase), torch.zeros(P, S, D, dtype=model.dtype, device=DEV), torch.zeros(P, S, cond.n, dtype=model.dtype, device=DEV))
    paths = cond.sample_paths(S, D, base=base)
    out = paths(tx)
    assert tuple(out.shape) == (P * S, len(tx)) and out.is_cuda
    assert torch.equal(paths.component.cpu(), torch.arange(P).repeat_interleave(S))
    mu, var = cond._engine.cond_predict(cond._state, cond._norm_x(tx))
    y_mean, y_std = float(cond._y_mean.reshape(-1)[0]), float(cond._y_std.reshape(-1)[0])
    diff = ((out.view(P, S, -1) - (mu * y_std + y_mean).unsqueeze(1)).abs() / (var.sqrt() * y_std).unsqueeze(1)).max()
    print(kind, 'zero-base paths vs cond_predict: %.2e predictive std' % float(diff))
    assert float(diff) <= TC.LEARNER_BAR
    if kind == 'map':                                    # a single row: the public mean is that row's
        assert float(np.max(np.abs(out[0].cpu().numpy() - cond.predict(tx)[0]) / cond.predict(tx)[1])) <= TC.LEARNER_BAR
    for wrong in (base[:3], (base[0], base[1], base[2], base[3][:, :, :-1]), (base[0], base[1], base[2][:, :2], base[3])):
        with pytest.raises(ValueError):
            cond.sample_paths(S, D, base=wrong)


@pytest.mark.parametrize('kind', TC.KINDS)
def test_learners_seeded_paths_snapshot_and_like(L, kind):
    assert A32 is not None, 'the floor A32 has not been set from profiles/path_fp32_errors.txt'
    model, cond, cx, cy = _condition(kind)
    tx = _tx()
    P, S, D = cond._state.theta.shape[0], 5, 128
    torch.manual_seed(77)
    paths = cond.sample_paths(S, D)
    torch.manual_seed(77)
    twin = cond.sample_paths(S, D)                       # the same generator state: the same base, bit for bit
    for a, b in zip(paths.base, twin.base):
        assert torch.equal(a, b)
    assert [tuple(t.shape) for t in paths.base] == [(D, model.engine.layout.feature_dim), (D,), (P, S, D), (P, S, 4)]
    first = paths(tx)
    assert tuple(first.shape) == (P * S, len(tx)) and tuple(paths.component.shape) == (P * S,)
    assert torch.equal(first, paths(tx)) and torch.equal(first, twin(tx))
    assert paths.num_paths == S and paths.n == 4
    noisy = paths(tx, observation_noise=True)
    assert noisy.shape == first.shape and not torch.equal(noisy, first) and bool(torch.isfinite(noisy).all())
    for p, (h, c) in enumerate(learner_errors(cond, paths, tx)):
        print('%s row %d: hip %.2e torch32 %.2e' % (kind, p, h, c))
        assert h <= max(R40 * c, A32), (kind, p, h, c)
    # a snapshot: one more meta-iteration and a later append change nothing
    model.meta_fit(verbose=False, log_period=1000, n_iter=1)
    cond.append(cx[4:], cy[4:])
    assert cond.n == 6 and paths.n == 4
    assert torch.equal(first, paths(tx))
    # like=: the same prior functions on the grown context
    torch.manual_seed(5)
    grown = cond.sample_paths(S, D, like=paths)
    for a, b in zip(grown.base[:3], paths.base[:3]):
        assert torch.equal(a, b)
    assert tuple(grown.base[3].shape) == (P, S, 6) and torch.equal(grown.base[3][:, :, :4], paths.base[3])
    torch.manual_seed(5)
    assert torch.equal(grown.base[3][:, :, 4:], torch.randn(P, S, 2, dtype=model.dtype, device=DEV))
    assert grown.n == 6 and not torch.equal(grown(tx), first)
    for p, (h, c) in enumerate(learner_errors(cond, grown, tx)):
        print('%s grown row %d: hip %.2e torch32 %.2e' % (kind, p, h, c))
        assert h <= max(R40 * c, A32), (kind, p, h, c)
    with pytest.raises(ValueError):
        cond.sample_paths(S + 1, D, like=paths)
    with pytest.raises(ValueError):
        cond.sample_paths(S, 24)
    with pytest.raises(ValueError):
        cond.sample_paths(0, D)


def test_cosine_kernel_learner_raises_not_implemented(L):
    import meta_learning_pacoh_amd as M

    class CosineKernel:
        def __init__(self, raw=0.0):
            self.raw_period_length = torch.nn.Parameter(torch.full((1, 1), raw))

    class ScaleKernel:
        def __init__(self, base, raw=0.0):
            self.base_kernel, self.raw_outputscale = base, torch.nn.Parameter(torch.tensor(raw))

    tasks = TL.tiny_tasks()
    m = M.GPRegressionMetaLearned(tasks, mean_module='constant', covar_module=ScaleKernel(CosineKernel(2.0), -3.0), task_batch_size=2,
                                  random_seed=2)
    cond = m.condition(*tasks[0])
    mean, std = cond.predict(_tx())
    assert np.isfinite(mean).all()
    with pytest.raises(NotImplementedError, match='cosine'):
        cond.sample_paths(4)
