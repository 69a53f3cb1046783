"""Fused per-draw argmax / argmin of the posterior paths over a candidate pool (csrc/gp_path.hip: pacoh_gp_path_argmax), on the GPU.

The yardstick throughout is L.gp_path_eval of the same build on the same inputs -- merged code that tests/test_gpu_path.py holds to
the fp64 reference -- followed by the pure-torch rule paths.first_best (pinned on the CPU by tests/test_path_argmax_host.py).  The
fused kernel runs the SAME K loop, so no tolerance appears anywhere: indices are compared with torch.equal and values bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cond as TC                                         # noqa: E402  (make_case / Dev / build_learner)
import test_gpu_path as TP                                         # noqa: E402  (Spec / specs / N_SPECS)
from meta_learning_pacoh_amd import paths as PP                    # noqa: E402

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
DTYPES = [F64, F32]
TILE = 64


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


class Run:
    """one case conditioned and fitted on the device: .eval() is the yardstick, .best(...) the fused call on the same arguments"""

    def __init__(self, L, spec, case, base, dtype, noise=None):
        self.L, self.spec, self.case = L, spec, case
        self.dev = dev = TC.Dev(L, case, dtype, noise=noise)
        self.state = dev.condition(spec.n0, spec.cap)
        if spec.k:
            assert int(dev.append(self.state, spec.n0, spec.k).abs().sum()) == 0
        self.omega, self.phase, self.w, eps = (t.to(dtype).to(DEV).contiguous() for t in base)
        b = case.b
        self.v = L.gp_path_fit(self.state, spec.n, self.omega, self.phase, self.w, eps, dev.os, dev.noise, b.B, b.P, kernel=dev.kernel)
        self.zt, self.mt = dev.zt, dev.mt

    def _args(self, lo, hi):
        dev, b = self.dev, self.case.b
        whole = lo == 0 and hi == self.zt.shape[1]
        zt = self.zt if whole else self.zt[:, lo:hi].contiguous()
        mt = self.mt if (whole or dev.mode != self.L.MEAN_VECTOR) else self.mt[:, lo:hi].contiguous()
        return (self.state[0], self.spec.n, self.v, self.omega, self.phase, self.w, self.state[4], zt, self.case.zt_div, mt, dev.mode,
                dev.ls, dev.os, b.B, b.P)

    def eval(self):
        return self.L.gp_path_eval(*self._args(0, self.zt.shape[1]), kernel=self.dev.kernel)

    def best(self, lo=0, hi=None, **kw):
        """-> (idx [B,S], val [B,S]) of the candidates lo .. hi - 1 (global indices when idx_base=lo is passed)"""
        val, idx = self.L.gp_path_argmax(*self._args(lo, self.zt.shape[1] if hi is None else hi), kernel=self.dev.kernel, **kw)
        return idx, val


def same(got, want):
    """(idx, val) pairs: the same indices; where there is one, the same value BIT FOR BIT (so the sign of a zero); elsewhere NaN"""
    (gi, gv), (wi, wv) = got, want
    if gi.dtype != torch.int64 or not torch.equal(gi, wi):
        return False
    some = wi >= 0
    ints = torch.int32 if gv.dtype == F32 else torch.int64
    return bool(torch.equal(gv.view(ints)[some], wv.view(ints)[some]) and torch.isnan(gv[~some]).all() and torch.isnan(wv[~some]).all())


def check_against_eval(run, out, strips_list, mask=None):
    """every strip setting and both directions against first_best on gp_path_eval's output; val is out[b, s, idx] itself"""
    for largest in (True, False):
        want = PP.first_best(out, mask, largest)
        wi = want[0]
        picked = out.gather(2, wi.clamp(min=0).unsqueeze(2)).squeeze(2)
        assert same((wi, picked), want)                              # (the yardstick's value IS the entry of out)
        for strips in strips_list:
            got = run.best(largest=largest, strips=strips, mask=mask)
            assert same(got, want), (run.spec.tag, largest, strips)


# ------------------------------------------------------------------------------------------------------------------- 1. sweep
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('ci', range(TP.N_SPECS))
def test_sweep_against_eval_and_first_best(L, ci, dtype):
    spec = TP.specs(TC.limit_of(L, dtype))[ci]
    case, base = spec.build(dtype == F32)
    run = Run(L, spec, case, base, dtype)
    out = run.eval()
    assert bool(torch.isfinite(out).all())
    tiles = -(-spec.m // TILE)
    check_against_eval(run, out, (0, 1, 2, tiles))


# -------------------------------------------------------------------------------------------------------------- 2. many tiles
@pytest.mark.parametrize('dtype', DTYPES)
def test_many_tiles(L, dtype):
    spec = TP.Spec('many tiles', 20, 0, 24, TILE * 37 + 5, 17, 48, 4, 'rbf', 2404)
    case, base = spec.build(dtype == F32)
    run = Run(L, spec, case, base, dtype)
    check_against_eval(run, run.eval(), (1, 3, 38, 0))


# -------------------------------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case_no', [2500, 2504, 2508])             # the three mean modes
def test_ties_go_to_the_first_index(L, dtype, case_no):
    """70 points repeated three times: the copies sit at other tile and lane positions.  The rule stays "the first index among the
    exact extrema of gp_path_eval's output"; where gp_path_eval gives the copies the same bits, that index is below 70"""
    spec = TP.Spec('ties', 9, 0, 12, 210, 17, 48, 2, 'm32', case_no)
    case, base = spec.build(dtype == F32)
    case.zt = case.zt[:, :70].repeat(1, 3, 1).contiguous()
    if case.b.mean_mode == 'vector':
        case.mt = case.mt[:, :70].repeat(1, 3).contiguous()
    run = Run(L, spec, case, base, dtype)
    out = run.eval()
    check_against_eval(run, out, (0, 1, 2, 4))
    equal = torch.equal(out[:, :, :70], out[:, :, 70:140]) and torch.equal(out[:, :, :70], out[:, :, 140:])
    print('mean mode %s, %s: the three copies are %sbit-equal in gp_path_eval' % (case.b.mean_mode, dtype, '' if equal else 'NOT '))
    if equal:
        for largest in (True, False):
            idx, _ = run.best(largest=largest)
            assert bool(((idx >= 0) & (idx < 70)).all())


# -------------------------------------------------------------------------------------------------------------------- 4. mask
@pytest.mark.parametrize('dtype', DTYPES)
def test_mask(L, dtype):
    spec = TP.Spec('mask', 33, 0, 40, 200, 17, 48, 4, 'm52', 2600)
    case, base = spec.build(dtype == F32)
    run = Run(L, spec, case, base, dtype)
    out = run.eval()
    m = spec.m
    half = (torch.rand(m, generator=torch.Generator().manual_seed(5)) < 0.5).to(DEV)
    check_against_eval(run, out, (0, 1, 4), mask=half)
    check_against_eval(run, out, (0,), mask=half.to(torch.uint8))
    for largest in (True, False):                                    # the winners masked: the runner-up must win
        idx, val = run.best(largest=largest)
        rest = torch.ones(m, dtype=torch.bool, device=DEV)
        rest[idx.reshape(-1)] = False
        idx2, val2 = run.best(largest=largest, mask=rest)
        assert same((idx2, val2), PP.first_best(out, rest, largest))
        assert not bool((idx2 == idx).any())
        assert bool((val2 <= val).all() if largest else (val2 >= val).all())
    for k in (0, 63, 64, 199):                                       # one eligible point
        one = torch.zeros(m, dtype=torch.bool, device=DEV)
        one[k] = True
        for strips in (0, 4):
            idx, val = run.best(mask=one, strips=strips)
            assert bool((idx == k).all()) and torch.equal(val, out[:, :, k])
    none = torch.zeros(m, dtype=torch.bool, device=DEV)              # all masked
    for largest in (True, False):
        for strips in (0, 1, 4):
            idx, val = run.best(mask=none, largest=largest, strips=strips)
            assert bool((idx == -1).all()) and bool(torch.isnan(val).all())


# ------------------------------------------------------------------------------------------------------------------ 5. chunks
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case_no', [2704, 2708])                         # a mean vector, a constant mean
def test_chunks_in_any_order_equal_the_single_call(L, dtype, case_no):
    spec = TP.Spec('chunks', 17, 0, 20, 200, 17, 48, 5, 'm12', case_no)
    case, base = spec.build(dtype == F32)
    run = Run(L, spec, case, base, dtype)
    mask = (torch.rand(200, generator=torch.Generator().manual_seed(6)) < 0.7).to(DEV)
    ranges = ((0, 64), (64, 65), (65, 200))
    for largest in (True, False):
        for mk in (None, mask):
            whole = run.best(largest=largest, mask=mk)
            assert same(whole, PP.first_best(run.eval(), mk, largest))
            for order in (ranges, ranges[::-1]):
                best = None
                for j, (lo, hi) in enumerate(order):
                    val, idx = run.L.gp_path_argmax(*run._args(lo, hi), kernel=run.dev.kernel, largest=largest,
                                                    mask=None if mk is None else mk[lo:hi], idx_base=lo, first=j == 0, best=best)
                    best = (val, idx)
                assert same((best[1], best[0]), whole), (largest, mk is None, order)
    # a chunk with nothing eligible, first and last, leaves the other chunk's result
    none = torch.zeros(200, dtype=torch.bool, device=DEV)
    part = run.best(lo=64, hi=200, idx_base=64)
    val, idx = run.L.gp_path_argmax(*run._args(0, 64), kernel=run.dev.kernel, mask=none[:64])
    assert bool((idx == -1).all())
    val, idx = run.L.gp_path_argmax(*run._args(64, 200), kernel=run.dev.kernel, idx_base=64, first=False, best=(val, idx))
    assert same((idx, val), part)
    val, idx = run.L.gp_path_argmax(*run._args(0, 64), kernel=run.dev.kernel, mask=none[:64], first=False, best=(val, idx))
    assert same((idx, val), part)


# -------------------------------------------------------------------------------------------------------------- 6. failed row
@pytest.mark.parametrize('dtype', DTYPES)
def test_failed_row_among_good_neighbours(L, dtype):
    """the construction of tests/test_gpu_path.py: the second parameter row's noise is 10 below, its Cholesky fails on every rung
    (info = -1): -1 / NaN for that row, with and without a running best, and the neighbours bit for bit what a clean run gives
    (S = 17, m = 65: two test tiles)"""
    spec = TP.Spec('failed row', 9, 0, 12, 65, 17, 48, 2, 'rbf', 2300)
    case, base = spec.build(dtype == F32)
    good = Run(L, spec, case, base, dtype)
    bad_noise = case.b.noise.clone()
    bad_noise[1] -= 10.0
    bad = Run(L, spec, case, base, dtype, noise=bad_noise)
    info = bad.state[4].cpu()
    for largest in (True, False):
        for strips in (0, 1, 2):
            gi, gv = good.best(largest=largest, strips=strips)
            bi, bv = bad.best(largest=largest, strips=strips)
            # ... and with a finite pair already in best_*: a failed row still gives -1 / NaN
            pv, pi = torch.zeros_like(bv), torch.zeros_like(bi)
            bad.L.gp_path_argmax(*bad._args(0, 65), kernel=bad.dev.kernel, largest=largest, strips=strips, first=False, best=(pv, pi))
            for b in range(case.b.B):
                if b % TC.P3 == 1:
                    assert int(info[b]) == -1
                    for i, v in ((bi, bv), (pi, pv)):
                        assert bool((i[b] == -1).all()) and bool(torch.isnan(v[b]).all())
                else:
                    assert int(info[b]) == 0 and bool((gi[b] >= 0).all())
                    assert same((bi[b], bv[b]), (gi[b], gv[b])), b


# ----------------------------------------------------------------------------------------------------------- 7. refused calls
def test_refused_calls_launch_nothing(L):
    """every refusal of pacoh_gp_path_argmax leaves best_val / best_idx (a sentinel before) untouched"""
    for dtype in (F32, F64):
        limit = TC.limit_of(L, dtype)
        B, P, f, n, cap, S, D, m = 2, 1, 2, 4, 6, 3, 32, 70
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)
        one = torch.ones(1, dtype=dtype, device=DEV)
        state = L.gp_condition(z(B, n, f), 1, None, L.MEAN_ZERO, z(B, n), 1, one.reshape(1, 1).expand(1, f).contiguous(), one, one, B, P,
                               capacity=cap)
        zs, resid, X, alpha, info = state
        omega, phase, w, v, zt, ls = z(D, f), z(D), z(B, S, D), z(B, S, n), z(B, m, f), z(1, f) + 1
        bv = torch.full((B, S), -7.0, dtype=dtype, device=DEV)
        bi = torch.full((B, S), -7, dtype=torch.int64, device=DEV)
        lib, p, code, st = L.load_library(), L._ptr, L.dtype_code(zs), L._stream()
        need = lib.pacoh_gp_path_argmax_workspace_bytes(B, S, m, 2, code)
        ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=DEV)

        def am(n=n, cap=cap, S=S, D=D, m=m, kf=f, zt_=zt, zt_div=1, B=B, bv_=bv, bi_=bi, ws_=ws, ws_bytes=need, idx_base=0, largest=1,
               first=1, strips=2):
            q = lambda t: None if t is None else p(t)
            return lib.pacoh_gp_path_argmax(p(zs), p(v), p(w), p(info), p(omega), p(phase), q(zt_), zt_div, None, L.MEAN_ZERO, p(ls),
                                            p(one), None, q(bv_), q(bi_), q(ws_), ws_bytes, B, P, n, cap, S, D, m, kf, idx_base, largest,
                                            first, strips, code, st)

        assert am(n=cap + 1) == -2 and am(cap=limit + 1) == -2 and am(n=0) == -2
        assert am(kf=17) == -2 and am(kf=f | (2 << L.KERNEL_SHIFT)) == -2 and am(kf=f | (L.KERNEL_COSINE << L.KERNEL_SHIFT)) == -2
        assert am(D=8) == -2 and am(D=24) == -2 and am(D=16400) == -2 and am(S=0) == -2
        assert am(B=0) == -1 and am(m=0) == -2
        assert am(zt_=None) == -1 and am(zt_div=0) == -1 and am(bv_=None) == -1 and am(bi_=None) == -1 and am(ws_=None) == -1
        assert am(ws_bytes=need - 1) == -1 and am(ws_bytes=0) == -1
        assert am(strips=-1) == -1 and am(idx_base=-1) == -1
        assert am(largest=2) == -1 and am(largest=-1) == -1 and am(first=2) == -1 and am(first=-1) == -1
        torch.cuda.synchronize()
        assert bool((bv == -7.0).all()) and bool((bi == -7).all())
        assert am() == 0                                             # ... and the well-formed call runs
        torch.cuda.synchronize()
        assert bool(torch.isfinite(bv).all()) and bool((bi == 0).all())    # all inputs zero: every point ties, the first index wins


# ---------------------------------------------------------------------------------------------------------------- 8. learners
def _pool(m):
    return np.linspace(-3.5, 3.5, m).reshape(-1, 1)


@pytest.mark.parametrize('kind', TC.KINDS)
def test_learners_through_the_public_api(L, kind):
    model, cond, cx, cy = TP._condition(kind)
    m = 173
    tx = _pool(m)
    P, S, D = cond._state.theta.shape[0], 5, 128
    torch.manual_seed(31)
    paths = cond.sample_paths(S, D)
    out = paths(tx)                                                  # [P S, m], original units
    fn = cond._engine.cond_paths_eval(paths._snap, cond._norm_x(tx))                 # [P, S, m], normalised space
    mask = np.random.RandomState(3).rand(m) < 0.5
    for name, largest in (('argmax', True), ('argmin', False)):
        idx, val = getattr(paths, name)(tx)
        assert tuple(idx.shape) == (P * S,) and idx.dtype == torch.int64 and idx.is_cuda and tuple(val.shape) == (P * S,)
        ext = out.max(1).values if largest else out.min(1).values
        at = out.gather(1, idx.unsqueeze(1)).squeeze(1)
        assert torch.equal(at, ext) and torch.equal(val, at)         # out[r, idx[r]] == out[r].max(), and value is that entry
        # the first-index rule, in normalised space (the affine map to original units can merge two distinct values into one)
        wi, wv = PP.first_best(fn, None, largest)
        assert torch.equal(idx, wi.reshape(-1))
        assert torch.equal(val, (wv * paths._y_std + paths._y_mean).reshape(-1))
        # chunks
        for chunk in (50, 64, 172, 173, 1000):
            ci, cv = getattr(paths, name)(tx, chunk=chunk)
            assert torch.equal(ci, idx) and torch.equal(cv, val), (name, chunk)
        # mask: a numpy array and a device tensor
        wi, wv = PP.first_best(fn, torch.from_numpy(mask).to(DEV), largest)
        for mk in (mask, torch.from_numpy(mask), torch.from_numpy(mask).to(DEV)):
            for chunk in (None, 50):
                mi, mv = getattr(paths, name)(tx, mask=mk, chunk=chunk)
                assert torch.equal(mi, wi.reshape(-1)) and torch.equal(mv, (wv * paths._y_std + paths._y_mean).reshape(-1))
                assert bool(torch.from_numpy(mask).to(DEV)[mi].all())
        ni, nv = getattr(paths, name)(tx, mask=np.zeros(m, dtype=bool))
        assert bool((ni == -1).all()) and bool(torch.isnan(nv).all())
    with pytest.raises(ValueError):
        paths.argmax(tx, mask=mask[:-1])
    # Thompson sampling: batch_size indices, each some draw's argmax; the returned paths serve as like=
    torch.manual_seed(32)
    idx, tp = cond.thompson(tx, batch_size=5, num_features=D)
    assert tuple(idx.shape) == (5,) and idx.dtype == torch.int64 and idx.is_cuda
    assert isinstance(tp, PP.PosteriorPaths) and tp.num_paths == -(-5 // P)
    every, _ = tp.argmax(tx)
    assert tuple(every.shape) == (P * tp.num_paths,) and set(idx.tolist()) <= set(every.tolist())
    # ... WITHOUT replacement among the draws: the multiset of the 5 is contained in the multiset of all
    pool = sorted(every.tolist())
    for i in sorted(idx.tolist()):
        pool.remove(i)
    cond.append(tx[int(idx[0])].reshape(1, 1), np.zeros((1, 1)))
    idx2, tp2 = cond.thompson(tx, batch_size=5, num_features=D, like=tp)
    for a, b in zip(tp2.base[:3], tp.base[:3]):
        assert torch.equal(a, b)
    assert tp2.n == tp.n + 1 and tuple(idx2.shape) == (5,)
    evaluated = np.zeros(m, dtype=bool)
    evaluated[int(idx[0])] = True
    idx3, _ = cond.thompson(tx, batch_size=5, num_features=D, mask=~evaluated, like=tp2)
    assert int(idx[0]) not in idx3.tolist()
    with pytest.raises(ValueError):
        cond.thompson(tx, batch_size=0)


# ------------------------------------------------------------------------------------------------------ 9. no dense intermediate
def test_no_dense_intermediate(L):
    """m = 50 000 candidates, 16 draws for each of the three SVGD rows, chunk = 4096: the allocator's peak rises during paths.argmax
    by less than HALF of the P S m 4 bytes that paths(tx) alone would allocate for its result.  A condition, not a measurement."""
    model, cond, cx, cy = TP._condition('svgd')
    P, S, m = cond._state.theta.shape[0], 16, 50000
    assert P == 3
    tx = _pool(m)
    torch.manual_seed(33)
    paths = cond.sample_paths(S, 128)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, val = paths.argmax(tx, chunk=4096)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    dense = P * S * m * 4
    print('peak rise during paths.argmax: %d bytes; paths(tx) alone: %d bytes' % (rise, dense))
    assert rise < dense // 2, (rise, dense)
    assert tuple(idx.shape) == (P * S,) and bool(((idx >= 0) & (idx < m)).all()) and bool(torch.isfinite(val).all())
    # (the result itself, against the dense way at this size)
    fn = cond._engine.cond_paths_eval(paths._snap, cond._norm_x(tx))
    wi, wv = PP.first_best(fn, None, True)
    assert torch.equal(idx, wi.reshape(-1)) and torch.equal(val, (wv * paths._y_std + paths._y_mean).reshape(-1))
