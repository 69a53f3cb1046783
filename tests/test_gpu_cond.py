"""The conditioned GP posterior (csrc/gp_cond.hip: pacoh_gp_condition / pacoh_gp_cond_predict / pacoh_gp_cond_append) and what is built
on it, on the GPU.

fp64: every problem against tests/cond_ref.oracle_predict (the oracle's posterior predictive on the full context) at 1e-10 on
  e_mu = max_s |mu_s - ref_s| / sqrt(var_ref_s),   e_var = max_s |var_s - ref_s| / var_ref_s,
the kept X = L^-1 and alpha against tests/cond_ref.direct at 1e-10 of the largest reference entry, and against L.gp_predict on the same
inputs.  That bar is not taken from the kernels: the incremental form against the direct one in fp64 on the CPU (up to 188 successive
appends, all four exponential families, f in {1,2,4,5,16}, noise ratios 0.02 - 0.3) is off by at most 2.8e-12 (e_mu), 6.6e-14
(e_var), 8e-14 / 5e-14 of the largest entry (alpha / X).
fp32: the same two errors per problem held the way tests/test_gpu_fp32_accuracy.py holds the other fp32 kernels,
  err_hip <= max(R err_torch32, A),   R = 40 the project's value,
err_torch32 the same closed form (predict) or the incremental form (append) of tests/cond_ref.py in torch fp32 on the CPU on the SAME
fp32-rounded inputs, the worst over NORD = 8 orders of the context points, against the fp64 reference.  The floors A follow that
module's rule from profiles/cond_fp32_errors.txt (tests/cond_fp32_errors.py, which shares measure() below).
Learners: condition().predict() / .append() / .confidence_intervals() against predict() / confidence_intervals() of the learner
through the public API; both sides are fp32."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_ref as R                                               # noqa: E402
import test_gpu_loo as TL                                          # noqa: E402  (make_batch / combos / _duplicated: the LOO generator)
import test_gpu_fp32_accuracy as FA                                # noqa: E402  (R / NORD: the fp32 yardstick's own)

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
BAR64 = 1e-10
P3 = TL.P3
NS = (1, 2, 7, 8, 9, 31, 33, 63, 64, 65, 127, 128, 'limit')
FS = (1, 4, 5, 16)
MS = (1, 15, 16, 17, 64, 65, 200)                       # the test-tile (64) and MFMA-tile (16) edges
APPENDS = ((1, 1), (1, 7), (7, 2), (8, 1), (15, 2), (16, 1), (31, 2), (63, 2), (64, 1), (100, 28), (127, 1), ('limit-1', 1))
NORD, R40 = FA.NORD, FA.R

# fp32 floors, from profiles/cond_fp32_errors.txt (tests/cond_fp32_errors.py on an MI355X) by the rule of tests/test_gpu_fp32_accuracy.py:
# 4x the worst HIP error among the problems beyond 10x torch fp32.  No problem of any of the four outputs is beyond 10x torch (p = predict
# after condition, a = predict after condition + append): no floor.  Measured: worst ratio hip / torch32 9.5 (var after condition; mu 3.1,
# after append 1.6 / 1.3), so R = 40 has a factor 4 in hand; worst HIP errors mu 2.5e-3 (in units of the predictive std), var 2.6e-5.
A32 = dict(p_mu=0.0, p_var=0.0, a_mu=0.0, a_var=0.0)
# learners: 4x the worst difference profiles/cond_fp32_errors.txt records for the four cases below (5.0e-6 of a predictive std: the
# confidence bounds of the VI mixture after append; means and stds differ by at most 8.4e-7), far below the cap of 1e-3
LEARNER_BAR = 2.0e-5


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


def limit_of(L, dtype):
    return L.gp_cond_max_n(dtype)


# ---------------------------------------------------------------------------------------------------------------------- batches
class Case:
    """a TL.Batch (T tasks x P3 rows, n context points) with m test points: zt [B / zt_div, m, f], test mean per the batch's mode"""

    def __init__(self, batch, m, zt_div, seed, fp32=False):
        self.b, self.m, self.zt_div = batch, m, zt_div
        g = torch.Generator().manual_seed(90000 + seed)
        q = (lambda t: t.float().double()) if fp32 else (lambda t: t)
        rows = batch.B // zt_div
        if batch.family == 'cos':
            zt = torch.rand(rows, m, 1, generator=g, dtype=F64) * 0.9
        else:
            zt = torch.randn(rows, m, batch.f, generator=g, dtype=F64) * (1.5 / np.sqrt(batch.f))
        self.zt = q(zt)
        self.mt = q(0.3 * torch.randn(batch.B, m, generator=g, dtype=F64)) if batch.mean_mode == 'vector' else batch.mean

    def test_points(self, b):
        """-> zt [m,f], mean_t [m] of problem b"""
        if self.b.mean_mode == 'vector':
            mt = self.mt[b]
        elif self.b.mean_mode == 'const':
            mt = self.mt[b % self.b.P].expand(self.m)
        else:
            mt = torch.zeros(self.m, dtype=F64)
        return self.zt[b // self.zt_div], mt

    def reference(self, b, n=None):
        """fp64 oracle predictive of problem b conditioned on its first n points -> (mu, var)"""
        z, mean, y, ls, os_, noise = self.b.problem(b)
        n = z.shape[0] if n is None else n
        zt, mt = self.test_points(b)
        return R.oracle_predict(z[:n], mean[:n], y[:n], zt, mt, ls, os_, noise, family=self.b.family)


class Dev:
    """the case's tensors on the device in one dtype, and the three launches"""

    def __init__(self, L, case, dtype, noise=None):
        b = case.b
        d = lambda t: None if t is None else t.to(dtype).to(DEV).contiguous()
        self.L, self.case, self.dtype = L, case, dtype
        self.z, self.mean, self.y, self.ls, self.os = d(b.z), d(b.mean), d(b.y), d(b.ls), d(b.os)
        self.noise = d(b.noise if noise is None else noise)
        self.zt, self.mt = d(case.zt), d(case.mt)
        self.mode = {'zero': L.MEAN_ZERO, 'vector': L.MEAN_VECTOR, 'const': L.MEAN_CONST}[b.mean_mode]
        self.kernel = R.CODE[b.family]

    def _ctx(self, lo, hi):
        b = self.case.b
        mean = self.mean[:, lo:hi].contiguous() if b.mean_mode == 'vector' else self.mean
        return self.z[:, lo:hi].contiguous(), mean, self.y[:, lo:hi].contiguous()

    def condition(self, n, cap=None, state=None, noise=None):
        b = self.case.b
        z, mean, y = self._ctx(0, n)
        return self.L.gp_condition(z, b.z_div, mean, self.mode, y, b.y_div, self.ls, self.os, self.noise if noise is None else noise,
                                   b.B, b.P, capacity=cap, state=state, kernel=self.kernel)

    def predict(self, state, n):
        b = self.case.b
        mu, var = self.L.gp_cond_predict(state, n, self.zt, self.case.zt_div, self.mt, self.mode, self.ls, self.os, self.noise, b.B, b.P,
                                         kernel=self.kernel)
        return mu.cpu(), var.cpu()

    def append(self, state, n0, k, noise=None):
        b = self.case.b
        z, mean, y = self._ctx(n0, n0 + k)
        return self.L.gp_cond_append(state, n0, z, b.z_div, mean, self.mode, y, b.y_div, self.ls, self.os,
                                     self.noise if noise is None else noise, b.B, b.P, kernel=self.kernel).cpu()

    def gp_predict(self):
        """L.gp_predict on the same inputs.  Its LDS-resident path does not take every f at the conditioned posterior's size limit
        (n = 132, f = 16 in fp64 is beyond its LDS plan), so beyond 128 points the comparator is its large-context path"""
        b = self.case.b
        saved = self.L.FORCE_DENSE
        self.L.FORCE_DENSE = saved or b.n > 128
        try:
            mu, var, _, info = self.L.gp_predict(self.z, b.z_div, self.mean, self.mode, self.y, b.y_div, self.zt, self.case.zt_div, self.mt,
                                                 self.ls, self.os, self.noise, b.B, b.P, kernel=self.kernel)
        finally:
            self.L.FORCE_DENSE = saved
        return mu.cpu(), var.cpu(), info.cpu()


def make_case(n, f, family, case_no, m, fp32=False, T=None, noise_ratio=(0.02, 0.05, 0.3)):
    """the case_no-th rotation of (z_div, zt_div, mean mode) (TL.combos) and of y_div"""
    z_div, zt_div, mean_mode = TL.combos(case_no)
    y_div = (P3, 1)[(case_no // 3) % 2]
    batch = TL.make_batch(n, f, family, TL.tasks_for(n) if T is None else T, z_div, y_div, mean_mode, seed=case_no, fp32=fp32,
                          noise_ratio=noise_ratio)
    return Case(batch, m, zt_div, case_no, fp32=fp32)


def clone_state(state):
    return tuple(t.clone() for t in state)


def state_cpu(state):
    return tuple(t.cpu() for t in state)


def check_state_against_direct(case, st, n, b, bar=BAR64, jitter=0.0):
    """rows < n of problem b's zs / resid / X / alpha against tests/cond_ref.direct in fp64 -> the four relative differences"""
    z, mean, y, ls, os_, noise = case.b.problem(b)
    X, alpha = R.direct(z[:n], mean[:n], y[:n], ls, os_, noise, family=case.b.family, jitter=jitter)
    zs, resid, Xs, al, _ = st
    e = (float((zs[b, :n].double() - z[:n] / ls).abs().max()), float((resid[b, :n].double() - (y - mean)[:n]).abs().max()),
         R.rel_max(Xs[b, :n, :n], X), R.rel_max(al[b, :n], alpha))
    assert max(e) <= bar, (b, n, e)
    return e


# ---------------------------------------------------------------------------------------------------------------------- fp64
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('f', FS)
def test_fp64_condition_and_predict(L, n, f):
    limit = limit_of(L, F64)
    ni = NS.index(n)
    n = limit if n == 'limit' else n
    worst = 0.0
    for k, fam in enumerate(TL.families_for(f)):
        case_no = ni * 20 + FS.index(f) * 5 + k
        case = make_case(n, f, fam, case_no, MS[case_no % len(MS)])
        cap = (n, min(limit, n + 5), limit)[case_no % 3]
        dev = Dev(L, case, F64)
        state = dev.condition(n, cap)
        mu, var = dev.predict(state, n)
        gmu, gvar, ginfo = dev.gp_predict()
        st = state_cpu(state)
        assert torch.equal(st[4], ginfo) and int(ginfo.abs().max()) == 0, (fam, st[4].tolist(), ginfo.tolist())
        for b in range(case.b.B):
            ref = case.reference(b)
            e = R.errors(mu[b], var[b], ref) + R.errors(mu[b], var[b], (gmu[b].double(), gvar[b].double()))
            worst = max(worst, *e)
            assert max(e) <= BAR64, (fam, case_no, cap, b, e)
            check_state_against_direct(case, st, n, b)
    print('n=%d f=%d worst error %.2e' % (n, f, worst))


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('n,k', [(7, 2), (33, 31), (100, 3)])
def test_state_discipline(L, dtype, n, k):
    """a sentinel outside rows [0, n) and zeros above the diagonal: after condition nothing above the diagonal and nothing at or behind
    row n has changed; after append of k points the same with n + k"""
    S = 7.5
    case = make_case(n + k, 4, 'rbf', 300 + n, 17, fp32=dtype == F32)
    dev = Dev(L, case, dtype)
    B, cap = case.b.B, n + k + 6
    state = L.gp_cond_alloc(B, cap, 4, dtype, DEV)
    for t in state[:4]:
        t.fill_(S)
    state[2].copy_(torch.tril(state[2]))

    def check(st, used):
        zs, resid, X, alpha, _ = state_cpu(st)
        assert bool((zs[:, used:] == S).all()) and bool((resid[:, used:] == S).all()) and bool((alpha[:, used:] == S).all())
        assert float(torch.triu(X, 1).abs().sum()) == 0.0
        assert bool((torch.tril(X)[:, used:] == torch.tril(torch.full_like(X, S))[:, used:]).all())
        assert bool((zs[:, :used] != S).any()) and bool(torch.isfinite(X).all())

    out = dev.condition(n, state=state)
    assert out[2].data_ptr() == state[2].data_ptr() and int(state[4].abs().max()) == 0
    check(state, n)
    fail = dev.append(state, n, k)
    assert int(fail.abs().sum()) == 0
    check(state, n + k)
    mu, var = dev.predict(state, n + k)
    # fp32 here only shows that the state is usable (its accuracy is the fp32 test's business): noise / outputscale >= 0.02, so
    # cond(K) <= (n + k) / 0.02 + 1 and a bar of 10 x cond x 2^-24, the form of the jitter test's bar (3.1e-3 at 103 points)
    bar = BAR64 if dtype == F64 else 10 * ((n + k) / 0.02 + 1) * 2.0 ** -24
    for b in range(B):
        assert max(R.errors(mu[b], var[b], case.reference(b))) <= bar, b


def _append_case(L, n0, k, idx, dtype=F64, fp32=False):
    fam = ('rbf', 'm12', 'm32', 'm52')[idx % 4]
    f = (2, 1, 4, 5, 16)[idx % 5]
    return make_case(n0 + k, f, fam, 400 + idx, 17, fp32=fp32, T=3 if n0 + k <= 65 else 1)


@pytest.mark.parametrize('n0,k', APPENDS, ids=['%s+%d' % c for c in APPENDS])
def test_fp64_append_against_condition_on_all_points(L, n0, k):
    limit = limit_of(L, F64)
    idx = APPENDS.index((n0, k))
    n0 = limit - 1 if n0 == 'limit-1' else n0
    n = n0 + k
    case = _append_case(L, n0, k, idx)
    dev = Dev(L, case, F64)
    cap = (n, limit)[idx % 2]
    full = dev.condition(n, cap)
    one_call = dev.condition(n0, cap)
    fail = dev.append(one_call, n0, k)
    k_calls = dev.condition(n0, cap)
    for t in range(k):
        fail = fail + dev.append(k_calls, n0 + t, 1)
    assert int(fail.abs().sum()) == 0
    outs = [(state_cpu(s), dev.predict(s, n)) for s in (full, one_call, k_calls)]
    fz, fr = outs[0][0][0], outs[0][0][1]
    worst = 0.0
    for b in range(case.b.B):
        ref = case.reference(b)
        for st, (mu, var) in outs:
            assert torch.equal(st[0][b, :n], fz[b, :n]) and torch.equal(st[1][b, :n], fr[b, :n])
            e = check_state_against_direct(case, st, n, b) + R.errors(mu[b], var[b], ref)
            worst = max(worst, *e)
            assert max(e) <= BAR64, (b, e)
    print('n0=%d k=%d worst error %.2e' % (n0, k, worst))


# ---------------------------------------------------------------------------------------------------------------------- fp32
def _orders(s, salt):
    for k in range(NORD):
        yield torch.arange(s) if k == 0 else torch.randperm(s, generator=torch.Generator().manual_seed(1000 * k + s + salt))


def torch32_errors(case, b, ref, n0, k):
    """(e_mu, e_var) of the torch-fp32 comparator on problem b, the worst over NORD orders of its points: k = 0 the closed form
    (cond_ref.direct + predict), k > 0 the closed form on the first n0 points followed by the incremental form (cond_ref.append)"""
    z, mean, y, ls, os_, noise = case.b.problem(b)
    zt, mt = case.test_points(b)
    fam = case.b.family
    worst = [0.0, 0.0]
    for p0, p1 in zip(_orders(n0, 0), _orders(k, 7) if k else [None] * NORD):
        z0, m0, y0 = z[:n0][p0].float(), mean[:n0][p0].float(), y[:n0][p0].float()
        X, alpha = R.direct(z0, m0, y0, ls.float(), os_, noise, family=fam)
        zz = z0
        if k:
            z1, r1 = z[n0:][p1].float(), (y[n0:][p1].float() - mean[n0:][p1].float())
            X, alpha, zz, _ = R.append(X, alpha, z0, y0 - m0, z1, r1, ls.float(), os_, noise, family=fam)
        mu, var = R.predict(X, alpha, zz, zt.float(), mt.float(), ls.float(), os_, noise, family=fam)
        worst = [max(a, c) for a, c in zip(worst, R.errors(mu, var, ref))]
    return worst


def measure(L, case, n0, k):
    """one fp32 condition(n0) [+ append(k)] + predict -> [(e_mu, e_var) of HIP, the same of torch fp32] per problem; asserts clean
    Choleskys and no refused update on the way"""
    dev = Dev(L, case, F32)
    state = dev.condition(n0, n0 + k)
    if k:
        assert int(dev.append(state, n0, k).abs().sum()) == 0
    assert int(state[4].abs().max()) == 0
    mu, var = dev.predict(state, n0 + k)
    rows = []
    for b in range(case.b.B):
        ref = case.reference(b)
        rows.append((R.errors(mu[b], var[b], ref), torch32_errors(case, b, ref, n0, k)))
    return rows


def cases32(L):
    """(tag, kind 'p' | 'a', build, n0, k): predict on n in (1, 2, 8, 33, 64, 128, limit) x every family; append on a subset of APPENDS"""
    limit = limit_of(L, F32)
    out = []
    for i, n in enumerate((1, 2, 8, 33, 64, 128, limit)):
        for j, fam in enumerate(R.FAMILIES):
            f = 1 if fam == 'cos' else FS[(i + j) % 4]
            no = 1000 + 5 * i + j
            out.append(('predict n=%d f=%d %s' % (n, f, fam), 'p',
                        lambda n=n, f=f, fam=fam, no=no: make_case(n, f, fam, no, MS[no % len(MS)], fp32=True), n, 0))
    for i, (n0, k) in enumerate(((1, 7), (8, 1), (31, 2), (64, 1), (100, 28), (limit - 1, 1))):
        out.append(('append n0=%d k=%d' % (n0, k), 'a', lambda n0=n0, k=k, i=i: _append_case(L, n0, k, i, fp32=True), n0, k))
    return out


N_CASES32 = 7 * 5 + 6


@pytest.mark.parametrize('ci', range(N_CASES32))
def test_fp32_per_problem_error_against_torch_fp32(L, ci):
    assert all(v is not None for v in A32.values()), 'the floors A32 have not been set from profiles/cond_fp32_errors.txt'
    cs = cases32(L)
    assert len(cs) == N_CASES32
    tag, kind, build, n0, k = cs[ci]
    bad = []
    for b, (eh, ec) in enumerate(measure(L, build(), n0, k)):
        for q, h, c in zip(('mu', 'var'), eh, ec):
            bar = max(R40 * c, A32[kind + '_' + q])
            print('%s b=%d %s hip %.2e torch32 %.2e bar %.2e' % (tag, b, q, h, c, bar))
            if h > bar:
                bad.append('%s b=%d: hip %.2e torch32 %.2e bar %.2e' % (q, b, h, c, bar))
    assert not bad, '%s\n  ' % tag + '\n  '.join(bad[:20])


# ---------------------------------------------------------------------------------------------------------------------- jitter, failures, limits
def test_jitter_rung_is_that_of_gp_predict(L):
    """the duplicated-points batch of tests/test_gpu_loo.py (fp32, outputscale 2^-6, noise 5e-10, n = 8): info in 1..3, mu / var against
    the fp64 closed form at noise + jitter IN THE FACTOR within that test's bar 10 x cond x 2^-24 (mu: the computed term K* alpha,
    relative to its largest entry), and info / mu / var agree with L.gp_predict on the same problems within the same bar"""
    n, os_ = 8, 2.0 ** -6
    batch, _ = TL._duplicated(L, n, os_, 5e-10)
    case = Case(batch, 17, 1, 555, fp32=True)
    dev = Dev(L, case, F32)
    state = dev.condition(n, n + 3)
    mu, var = dev.predict(state, n)
    gmu, gvar, ginfo = dev.gp_predict()
    info = state[4].cpu()
    assert torch.equal(info, ginfo)
    for b in range(batch.B):
        if b % P3 != 1:
            assert int(info[b]) == 0
            continue
        rung = int(info[b])
        assert 1 <= rung <= 3
        j = 1e-6 * 10 ** (rung - 1)
        z, mean, y, ls, o, noise = batch.problem(b)
        zt, mt = case.test_points(b)
        X, alpha = R.direct(z, mean, y, ls, o, noise, jitter=j)
        rm, rv = R.predict(X, alpha, z, zt, mt, ls, o, noise)
        scale = (rm - mt).abs().max()
        bar = 10 * (n * os_ + j) / j * 2.0 ** -24
        e = (float((mu[b].double() - rm).abs().max() / scale), float(((var[b].double() - rv).abs() / rv).max()),
             float((mu[b].double() - gmu[b].double()).abs().max() / scale), float(((var[b].double() - gvar[b].double()).abs() / rv).max()))
        print('rung %d errors vs closed form mu %.1e var %.1e, vs gp_predict mu %.1e var %.1e, bar %.1e' % ((rung,) + e + (bar,)))
        assert max(e) <= bar, (b, rung, e, bar)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_failed_problem_among_good_neighbours(L, dtype):
    """negative noise on row p = 1 at condition: info = -1, NaN alpha, NaN predictions for that problem only; append with a noise
    array whose entry 1 is -2 os (s^2 < 0: a numeric refusal): fail = 1 exactly there, those problems' rows < n as before; the
    neighbours are bit for bit what the launches give without it (n = 9: sixteen-lane groups, four problems share a wave)"""
    n, k = 9, 3
    case = make_case(n + k, 2, 'rbf', 77, 17, fp32=dtype == F32)
    B = case.b.B
    dev = Dev(L, case, dtype)
    good = dev.condition(n, n + k + 2)
    good_pred = dev.predict(good, n)
    bad_noise = dev.noise.clone()
    bad_noise[1] = -2.0
    bad = dev.condition(n, n + k + 2, noise=bad_noise)
    bad_pred = dev.predict(bad, n)
    gs, bs = state_cpu(good), state_cpu(bad)
    for b in range(B):
        if b % P3 == 1:
            assert int(bs[4][b]) == -1 and bool(torch.isnan(bs[3][b, :n]).all()) and float(bs[2][b].abs().sum()) == 0.0
            assert bool(torch.isnan(bad_pred[0][b]).all()) and bool(torch.isnan(bad_pred[1][b]).all())
        else:
            assert int(bs[4][b]) == 0
            for q in range(4):
                assert torch.equal(bs[q][b], gs[q][b]), (b, q)
            assert torch.equal(bad_pred[0][b], good_pred[0][b]) and torch.equal(bad_pred[1][b], good_pred[1][b])
    # append
    refuse = dev.noise.clone()
    refuse[1] = -2.0 * dev.os[1]
    tampered = clone_state(good)
    assert int(dev.append(good, n, k).abs().sum()) == 0
    fail = dev.append(tampered, n, k, noise=refuse)
    ts, after = state_cpu(tampered), state_cpu(good)
    for b in range(B):
        assert int(fail[b]) == (1 if b % P3 == 1 else 0)
        if b % P3 == 1:
            for q in range(4):
                assert torch.equal(ts[q][b, :n], gs[q][b, :n]), (b, q)
        else:
            for q in range(4):
                assert torch.equal(ts[q][b], after[q][b]), (b, q)


def test_beyond_the_limits_raises_and_launches_nothing(L):
    for dtype in (F32, F64):
        limit = limit_of(L, dtype)
        B, f, n = 2, 1, 4
        z = torch.zeros(B, n, f, dtype=dtype, device=DEV)
        y = torch.zeros(B, n, dtype=dtype, device=DEV)
        one = torch.ones(1, dtype=dtype, device=DEV)
        with pytest.raises(RuntimeError, match='limit of %d' % limit):
            L.gp_condition(z, 1, None, L.MEAN_ZERO, y, 1, one.reshape(1, 1), one, one, B, 1, capacity=limit + 1)
        state = L.gp_condition(z, 1, None, L.MEAN_ZERO, y, 1, one.reshape(1, 1), one, one, B, 1, capacity=n + 1)
        with pytest.raises(RuntimeError, match='limit of %d' % limit):
            L.gp_cond_append(state, n, z[:, :2].contiguous(), 1, None, L.MEAN_ZERO, y[:, :2].contiguous(), 1, one.reshape(1, 1), one, one, B, 1)
        torch.cuda.synchronize()
        before = state_cpu(state)
        lib, p = L.load_library(), L._ptr
        zs, resid, X, alpha, info = state
        fail = torch.zeros(B, dtype=torch.int32, device=DEV)
        out = torch.zeros(B, 2, dtype=dtype, device=DEV)
        kf, code = 1, L.dtype_code(z)
        # the C entry points themselves: PACOH_ELIMIT before anything is enqueued
        assert lib.pacoh_gp_condition(p(z), 1, None, L.MEAN_ZERO, p(y), 1, p(one), p(one), p(one), p(zs), p(resid), p(X), p(alpha), p(info),
                                      B, 1, n, limit + 1, kf, code, L._stream()) == -2
        assert lib.pacoh_gp_cond_predict(p(zs), p(X), p(alpha), p(info), p(z), 1, None, L.MEAN_ZERO, p(one), p(one), p(one), p(out), p(out),
                                         B, 1, n, limit + 1, 2, kf, code, L._stream()) == -2
        assert lib.pacoh_gp_cond_append(p(zs), p(resid), p(X), p(alpha), p(info), p(z), 1, None, L.MEAN_ZERO, p(y), 1, p(one), p(one),
                                        p(one), p(fail), B, 1, n, n + 1, 2, kf, code, L._stream()) == -2
        torch.cuda.synchronize()
        assert float(out.abs().sum()) == 0.0 and int(fail.abs().sum()) == 0
        for a, c in zip(before, state_cpu(state)):
            assert torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------------- learners
KINDS = ('map', 'svgd', 'vi-mode', 'vi-bayes')


def build_learner(kind):
    if kind == 'vi-bayes':
        return TL.build_learner('vi')[0], {'n_posterior_samples': 4}
    return TL.build_learner({'vi-mode': 'vi'}.get(kind, kind))


def learner_differences(kind):
    """-> (dict of the differences between condition().predict() / condition(first 3).append(rest).predict() / .confidence_intervals()
    and the learner's own predict() / confidence_intervals() on the same context, in units of the predictive std; model; kw)"""
    model, kw = build_learner(kind)
    tasks = TL.tiny_tasks()
    cx, cy = tasks[1]
    tx = np.linspace(-3.5, 3.5, 23).reshape(-1, 1)

    def seeded(fn):
        torch.manual_seed(4321)                  # VI 'Bayes' draws its rows per call: the same stream on both sides
        return fn()
    mean, std = seeded(lambda: model.predict(cx, cy, tx, **kw))
    ucb, lcb = seeded(lambda: model.confidence_intervals(cx, cy, tx, **kw))
    cond = seeded(lambda: model.condition(cx, cy, **kw))
    grown = seeded(lambda: model.condition(cx[:3], cy[:3], **kw)).append(cx[3:], cy[3:])
    assert cond.n == grown.n == cx.shape[0]
    out = {}
    for tag, c in (('cond', cond), ('append', grown)):
        m, s = c.predict(tx)
        u, l_ = c.confidence_intervals(tx)
        out[tag + '_mean'] = float(np.max(np.abs(m - mean) / std))
        out[tag + '_std'] = float(np.max(np.abs(s - std) / std))
        out[tag + '_ci'] = float(max(np.max(np.abs(u.numpy() - ucb.numpy()) / std), np.max(np.abs(l_.numpy() - lcb.numpy()) / std)))
    return out, model, kw, cond, tx


@pytest.mark.parametrize('kind', KINDS)
def test_learners_condition_is_predict(L, kind):
    assert LEARNER_BAR is not None and LEARNER_BAR <= 1e-3, 'LEARNER_BAR has not been set from profiles/cond_fp32_errors.txt'
    diffs, model, kw, cond, tx = learner_differences(kind)
    print(kind, diffs)
    for q, v in diffs.items():
        assert v <= LEARNER_BAR, (q, v, diffs)
    # a snapshot: one more meta-iteration does not change what the object predicts; two calls are bit-identical (VI-Bayes: no redraw)
    first = cond.predict(tx)
    model.meta_fit(verbose=False, log_period=1000, n_iter=1)
    again = cond.predict(tx)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    dist = cond.predict(tx, return_density=True)
    assert dist.mean.shape == (len(tx),) and float(dist.stddev.min()) > 0.0
    assert dist.marginal_log_prob(torch.zeros(len(tx))).shape == (len(tx),)
    with pytest.raises(RuntimeError, match='return_density=True'):
        dist.log_prob(torch.zeros(len(tx)))


def test_append_falls_back_to_conditioning_on_all_points(L, monkeypatch):
    """one refused problem (reported by a patched _lib.gp_cond_append): append() leaves a state bit-identical to condition() on all
    points; beyond the capacity it raises and changes nothing"""
    model, kw = build_learner('map')
    cx, cy = TL.tiny_tasks()[1]
    whole = model.condition(cx, cy)
    real = L.gp_cond_append

    def refusing(*a, **k):
        fail = real(*a, **k)
        fail[0] = 1
        return fail
    monkeypatch.setattr(L, 'gp_cond_append', refusing)
    grown = model.condition(cx[:3], cy[:3]).append(cx[3:], cy[3:])
    assert grown.n == whole.n == 6
    for a, b in zip(grown._state.bufs, whole._state.bufs):
        assert torch.equal(a, b)
    monkeypatch.setattr(L, 'gp_cond_append', real)
    small = model.condition(cx[:3], cy[:3], capacity=4)
    assert small.capacity == 4
    before = clone_state(small._state.bufs)
    with pytest.raises(RuntimeError, match='capacity of 4'):
        small.append(cx[3:], cy[3:])
    assert small.n == 3
    for a, b in zip(before, small._state.bufs):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match='limit of %d' % L.gp_cond_max_n(F32)):
        model.condition(cx, cy, capacity=L.gp_cond_max_n(F32) + 1)


def test_condition_raises_not_psd(L, monkeypatch):
    from meta_learning_pacoh_amd.engine import NotPSDError
    model, kw = build_learner('map')
    cx, cy = TL.tiny_tasks()[0]
    real = model.engine._hypers

    def broken(theta):
        ls, os_, noise = real(theta)
        return ls, os_, noise - 10.0
    monkeypatch.setattr(model.engine, '_hypers', broken)
    with pytest.raises(NotPSDError):
        model.condition(cx, cy)
