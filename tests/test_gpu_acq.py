"""Analytic acquisition with a fused argmax (csrc/acq.hip: pacoh_mixture_acq) and what is built on it, on the GPU.

Values: against meta_learning_pacoh_amd/acquisition.py (mixture_acquisition, the specification) in fp64 on the CPU on the SAME inputs
rounded to the call's dtype, per task:
  'ei', 'ucb', 'mean', 'std':  max_s |h - r| / sd_mix_ref(s),  sd_mix_ref the fp64 mixture std, noise included;   'pi':  max_s |h - r|.
fp64 at BAR64 = 1e-10, tests/test_gpu_cond.py's bar for the moments this kernel consumes (the epilogue's own rounding is orders below).
fp32 the way tests/test_gpu_fp32_accuracy.py holds the other fp32 kernels:  err_hip <= max(R err_torch32, A),  R = 40 the project's
value, err_torch32 the same specification run in torch fp32 on the CPU against the fp64 run; the floors A follow that module's rule
from profiles/acq_fp32_errors.txt (tests/acq_fp32_errors.py, which shares cases() / measure() below).
Selection: exact -- the pair equals paths.first_best of the kernel's own values (torch.equal), with and without values, for every
strip count, under masks, ties, NaN rows and chunked merging; and the winner is right by the specification's measure.
Learners: cond.acquisition / cond.acquire / GaussianPredictive.acquisition through the public API."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cond as TC                                         # noqa: E402  (build_learner / KINDS of the learners)
import test_gpu_loo as TL                                          # noqa: E402  (tiny_tasks)
import test_gpu_fp32_accuracy as FA                                # noqa: E402  (R: the fp32 yardstick's own)
from meta_learning_pacoh_amd import acquisition as A               # noqa: E402
from meta_learning_pacoh_amd import paths as PP                    # noqa: E402

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
DTYPES = (F32, F64)
BAR64 = 1e-10
R40 = FA.R
BLOCK = 256
TS = (1, 3)
PS = (1, 2, 3, 20, 65)
MS = (1, 63, 64, 65, 255, 256, 257, 1000)              # the wave (64) and block (256) edges, several blocks
STRIPS = (0, 1, 2, 'blocks')
XI, BETA = 0.0078125, 2.0

# fp32 floors, from profiles/acq_fp32_errors.txt (tests/acq_fp32_errors.py on an MI355X) by the rule of tests/test_gpu_fp32_accuracy.py:
# 4x the worst HIP error among the tasks beyond 10x torch fp32.  No task of any kind is beyond 10x torch: no floor.  Measured: worst ratio
# hip / torch32 3.9 ('ei'; 'pi' 1.7, 'ucb' 1.1, 'mean' and 'std' 1.0: the Welford kinds are the same operations in the same order), so
# R = 40 has a factor 10 in hand; worst HIP errors 1.2e-6 ('ei'), 2.0e-6 ('ucb') of the mixture std, 1.4e-7 ('pi').
A32 = dict(ei=0.0, pi=0.0, ucb=0.0, mean=0.0, std=0.0)
# learners: 4x the worst difference profiles/acq_fp32_errors.txt records for the learner cases below (1.5e-6 of a predictive std: the
# learner's own density object, whose moments come from another predict kernel, against the conditioned object; the fused values
# against the rule on the same moments differ by at most 4.8e-7), far below the cap of 1e-3
LEARNER_BAR = 6.0e-6


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


# ------------------------------------------------------------------------------------------------------------------------ cases
class Case:
    """synthetic moments of T tasks x P rows at m candidates, rounded to `dtype` and kept in fp64 on the CPU: mu ~ 1.5 randn,
    var ~ U(1e-3, 2), noise[p] in (0, 1e-3] (latent variances stay positive) or None, best near the upper quartile of mu"""

    def __init__(self, T, P, m, dtype, seed, noise=True, sign=1, strips=0, tag=''):
        g = torch.Generator().manual_seed(70000 + seed)
        q = lambda t: t.to(dtype).double()
        self.T, self.P, self.m, self.dtype, self.sign, self.tag = T, P, m, dtype, sign, tag
        self.mu = q(1.5 * torch.randn(T, P, m, generator=g, dtype=F64))
        self.var = q(1e-3 + (2.0 - 1e-3) * torch.rand(T, P, m, generator=g, dtype=F64))
        self.noise = q(1e-3 * (1.0 - 0.9 * torch.rand(P, generator=g, dtype=F64))) if noise else None
        self.var = torch.maximum(self.var, self.noise.reshape(1, P, 1)) if noise else self.var
        self.best = float(q(torch.quantile(self.mu.flatten(), 0.75 if sign == 1 else 0.25)))
        self.strips = -(-m // BLOCK) if strips == 'blocks' else strips

    def spec(self, kind, dtype=F64):
        """the specification on these inputs in `dtype` on the CPU -> [T,m] as fp64"""
        c = lambda t: None if t is None else t.to(dtype)
        return A.mixture_acquisition(c(self.mu), c(self.var), kind, self.best, XI, BETA, self.sign, c(self.noise)).double()

    def sd_mix(self):
        return A.mixture_acquisition(self.mu, self.var, 'std')

    def dev(self):
        d = lambda t: None if t is None else t.to(self.dtype).to(DEV).contiguous()
        return d(self.mu.reshape(self.T * self.P, self.m)), d(self.var.reshape(self.T * self.P, self.m)), d(self.noise)

    def run(self, L, kind, mask=None, want_values=True, strips=None, largest=None, **kw):
        mu, var, noise = self.dev()
        largest = largest_of(kind, self.sign) if largest is None else largest
        bv, bi, values = L.mixture_acq(mu, var, self.T, self.P, kind, self.best, XI, BETA, self.sign, noise=noise,
                                       mask=None if mask is None else mask.to(DEV), want_values=want_values, largest=largest,
                                       strips=self.strips if strips is None else strips, **kw)
        return bv.cpu(), bi.cpu(), None if values is None else values.cpu()


def largest_of(kind, sign):
    return not (kind in ('mean', 'ucb') and sign == -1)


def same(a, b):
    """torch.equal that lets NaN equal NaN (the value of a task with nothing eligible)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def cases(kind, dtype):
    """eight cases per (kind, dtype): every m once; T, P, sign, noise and strips by rotation over the case number, which is offset per
    kind and dtype so that every value of every axis meets every kind"""
    ki = A.KINDS.index(kind)
    out = []
    for i, m in enumerate(MS):
        c = 8 * ki + i + (3 if dtype == F64 else 0)
        out.append(Case(TS[(c // 3) % 2], PS[c % 5], m, dtype, seed=100 * ki + i + (50 if dtype == F64 else 0), noise=c % 3 != 0,
                        sign=(1, -1)[(c // 2) % 2], strips=STRIPS[c % 4], tag='case %d' % c))
    return out


def errors(kind, h, ref, sd):
    """per task: max_s |h - r| / sd_mix_ref ('pi': max_s |h - r|) -> list of T floats"""
    d = (h.double() - ref).abs()
    d = d if kind == 'pi' else d / sd
    return [float(x) for x in d.max(dim=1).values]


def measure(L, case, kind):
    """-> (err_hip [T], err_torch32 [T] | None, values, best_val, best_idx, ref, sd)"""
    bv, bi, values = case.run(L, kind)
    ref, sd = case.spec(kind), case.sd_mix()
    eh = errors(kind, values, ref, sd)
    ec = errors(kind, case.spec(kind, F32), ref, sd) if case.dtype == F32 else None
    return eh, ec, values, bv, bi, ref, sd


def check_winner(kind, case, bi, ref, sd, bars, mask=None):
    """the winner is right by the specification's measure: within 2 bar sd of the reference's own extremum over the eligible points"""
    largest = largest_of(kind, case.sign)
    for t in range(case.T):
        r = ref[t] if mask is None else ref[t][mask]
        i = int(bi[t])
        assert 0 <= i < case.m
        slack = 2.0 * bars[t] * (1.0 if kind == 'pi' else float(sd[t, i]))
        if largest:
            assert float(ref[t, i]) >= float(r.max()) - slack, (case.tag, t, i)
        else:
            assert float(ref[t, i]) <= float(r.min()) + slack, (case.tag, t, i)


# ------------------------------------------------------------------------------------------------------------------- 1. sweep
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', A.KINDS)
def test_values_and_selection_sweep(L, kind, dtype):
    if dtype == F32:
        assert A32[kind] is not None, 'A32[%r] has not been set from profiles/acq_fp32_errors.txt' % kind
    for case in cases(kind, dtype):
        eh, ec, values, bv, bi, ref, sd = measure(L, case, kind)
        bars = [BAR64] * case.T if dtype == F64 else [max(R40 * c, A32[kind]) for c in ec]
        print('%s %s %s T=%d P=%d m=%d sign=%+d noise=%s strips=%d: hip %s torch32 %s' % (
            kind, str(dtype)[6:], case.tag, case.T, case.P, case.m, case.sign, case.noise is not None, case.strips,
            ['%.1e' % e for e in eh], None if ec is None else ['%.1e' % e for e in ec]))
        for t in range(case.T):
            assert eh[t] <= bars[t], (case.tag, t, eh[t], bars[t])
        largest = largest_of(kind, case.sign)
        idx, val = PP.first_best(values, None, largest)
        assert torch.equal(bi, idx) and same(bv, val), case.tag
        check_winner(kind, case, bi, ref, sd, bars)
        for strips in (0, 1, 2, -(-case.m // BLOCK), 10 ** 6):
            for want in (False, True):
                bv2, bi2, v2 = case.run(L, kind, want_values=want, strips=strips)
                assert torch.equal(bi2, bi) and torch.equal(bv2, bv), (case.tag, strips, want)
                assert v2 is None or torch.equal(v2, values)


@pytest.mark.parametrize('dtype', DTYPES)
def test_single_row_mean_and_std_are_exact(L, dtype):
    for m in (65, 1000):
        case = Case(3, 1, m, dtype, seed=900 + m, noise=False)
        mu, var, _ = case.dev()
        assert torch.equal(case.run(L, 'mean')[2], mu.cpu())
        assert torch.equal(case.run(L, 'std')[2], torch.sqrt(var).cpu())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['ei', 'mean'])
def test_more_strips_than_lanes_and_long_strips(L, kind, dtype):
    """m = 70 blocks + 3 points: with one block per strip a lane of the merging wave holds two partial pairs (the only other path of the
    second launch); with 1, 2 and 7 strips a thread walks up to 71 blocks.  The winners are planted in the last blocks."""
    m = 70 * BLOCK + 3
    case = Case(2, 2, m, dtype, seed=1500, sign=-1 if kind == 'mean' else 1)
    case.mu[0, :, m - 2] = -9.0 if kind == 'mean' else 9.0          # task 0: the last block (3 points), strip 70 = lane 6 again
    case.mu[1, :, 66 * BLOCK + 5] = -9.0 if kind == 'mean' else 9.0
    largest = largest_of(kind, case.sign)
    bv, bi, values = case.run(L, kind)
    idx, val = PP.first_best(values, None, largest)
    assert torch.equal(bi, idx) and same(bv, val) and bi.tolist() == [m - 2, 66 * BLOCK + 5]
    g = torch.Generator().manual_seed(15)
    mask = torch.rand(m, generator=g) < 0.5
    mask[m - 2] = False
    for mk in (None, mask):
        idx, val = PP.first_best(values, mk, largest)
        for strips in (0, 1, 2, 7, 64, 65, 71):
            bv2, bi2, _ = case.run(L, kind, mask=mk, want_values=False, strips=strips)
            assert torch.equal(bi2, idx) and same(bv2, val), (strips, mk is None)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['ei', 'pi', 'std', 'ucb'])
def test_zero_latent_variance(L, kind, dtype):
    """var == noise exactly at a third of the points of every row (s == 0: the limit forms), and in one row only at another third"""
    case = Case(2, 3, 300, dtype, seed=950, noise=True)
    case.var[:, :, 0::3] = case.noise.reshape(1, 3, 1)
    case.var[:, 1, 1::3] = case.noise[1]
    eh, ec, values, bv, bi, ref, sd = measure(L, case, kind)
    bars = [BAR64] * 2 if dtype == F64 else [max(R40 * c, A32[kind] or 0.0) for c in ec]
    if kind in ('ei', 'pi'):
        zero = values[:, 0::3]
        d = case.mu[:, :, 0::3] - case.best - XI
        want = (torch.clamp(d, min=0.0) if kind == 'ei' else (d > 0).double()).mean(1)
        assert float((zero.double() - want).abs().max()) <= (1e-5 if dtype == F32 else 1e-14)
    for t in range(2):
        assert eh[t] <= bars[t], (t, eh[t], bars[t])
    idx, val = PP.first_best(values, None, True)
    assert torch.equal(bi, idx) and same(bv, val)


# -------------------------------------------------------------------------------------------------------------------- 2. masks
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['ei', 'ucb'])
def test_masks(L, kind, dtype):
    case = Case(3, 3, 600, dtype, seed=1000, sign=-1 if kind == 'ucb' else 1)
    largest = largest_of(kind, case.sign)
    _, bi0, values = case.run(L, kind)
    g = torch.Generator().manual_seed(5)
    half = torch.rand(case.m, generator=g) < 0.5
    no_winner = torch.ones(case.m, dtype=torch.bool)
    no_winner[bi0] = False                                         # every task's winner masked: each runner-up wins
    one = torch.zeros(case.m, dtype=torch.bool)
    one[517] = True
    for tag, mask in (('half', half), ('winner masked', no_winner), ('one eligible', one), ('half as uint8', half.to(torch.uint8))):
        for strips in (0, 1, 2, 3):
            bv, bi, _ = case.run(L, kind, mask=mask, want_values=strips == 0, strips=strips)
            idx, val = PP.first_best(values, mask.bool(), largest)
            assert torch.equal(bi, idx) and same(bv, val), (tag, strips)
        if tag == 'winner masked':
            assert not bool((bi == bi0).any())
        if tag == 'one eligible':
            assert bi.tolist() == [517] * 3
    bv, bi, _ = case.run(L, kind, mask=torch.zeros(case.m, dtype=torch.bool))
    assert bi.tolist() == [-1] * 3 and bool(torch.isnan(bv).all())


# --------------------------------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', A.KINDS)
def test_ties_go_to_the_first_index(L, kind, dtype):
    """70 points repeated three times: the copies sit at other lane, wave and (strips = 'blocks') strip positions"""
    case = Case(2, 3, 70, dtype, seed=1100)
    case.mu, case.var, case.m = case.mu.repeat(1, 1, 3).contiguous(), case.var.repeat(1, 1, 3).contiguous(), 210
    for sign in (1, -1):
        case.sign = sign
        for strips in (0, 1):
            bv, bi, values = case.run(L, kind, strips=strips)
            assert torch.equal(values[:, :70], values[:, 70:140]) and torch.equal(values[:, :70], values[:, 140:])
            idx, val = PP.first_best(values, None, largest_of(kind, sign))
            assert torch.equal(bi, idx) and same(bv, val) and int(bi.max()) < 70
    # with the first copy masked the winner is the same point of the second copy
    mask = torch.ones(210, dtype=torch.bool)
    mask[:70] = False
    bv2, bi2, _ = case.run(L, kind, mask=mask)
    assert torch.equal(bi2, bi + 70) and torch.equal(bv2, bv)


@pytest.mark.parametrize('dtype', DTYPES)
def test_all_zero_ei_picks_the_first_eligible_point(L, dtype):
    case = Case(3, 2, 700, dtype, seed=1200)
    case.best = 1.0e4                                              # z < -5000 everywhere: every 'ei' is exactly 0
    bv, bi, values = case.run(L, 'ei')
    assert float(values.abs().max()) == 0.0 and not bool(torch.signbit(values).any())
    assert bi.tolist() == [0, 0, 0] and bv.tolist() == [0.0] * 3
    mask = torch.ones(700, dtype=torch.bool)
    mask[:300] = False
    for strips in (0, 1, 2):
        bv, bi, _ = case.run(L, 'ei', mask=mask, want_values=False, strips=strips)
        assert bi.tolist() == [300] * 3 and bv.tolist() == [0.0] * 3


# ---------------------------------------------------------------------------------------------------------------------- 4. NaN
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', A.KINDS)
def test_nan_row_among_good_neighbours(L, kind, dtype):
    """task 1 of 3 has a NaN row (mu and var): all its values are NaN, it gives -1 / NaN, and its neighbours are what a clean run
    gives; a NaN at single points of another task never wins"""
    case = Case(3, 3, 300, dtype, seed=1300)
    bv0, bi0, v0 = case.run(L, kind)
    case.mu[1, 2], case.var[1, 2] = float('nan'), float('nan')
    case.mu[0, 1, int(bi0[0])], case.var[0, 1, int(bi0[0])] = float('nan'), float('nan')      # task 0 loses its winner
    bv, bi, v = case.run(L, kind)
    assert bool(torch.isnan(v[1]).all()) and int(bi[1]) == -1 and bool(torch.isnan(bv[1]))
    assert torch.equal(v[2], v0[2]) and int(bi[2]) == int(bi0[2]) and float(bv[2]) == float(bv0[2])
    assert bool(torch.isnan(v[0, int(bi0[0])])) and int(torch.isnan(v[0]).sum()) == 1
    idx, val = PP.first_best(v, None, True)
    assert torch.equal(bi, idx) and same(bv, val) and int(bi[0]) != int(bi0[0])
    # merged into a running best: a task with nothing keeps what it had
    keep_v = torch.tensor([-1.0e30, 0.25, -1.0e30], dtype=dtype, device=DEV)
    keep_i = torch.tensor([7, 100000, 7], dtype=torch.int64, device=DEV)
    bv3, bi3, _ = case.run(L, kind, want_values=False, first=False, best_pair=(keep_v, keep_i), idx_base=1000)
    assert int(bi3[1]) == 100000 and float(bv3[1]) == 0.25 and bi3[0::2].tolist() == [int(bi[0]) + 1000, int(bi[2]) + 1000]


# ------------------------------------------------------------------------------------------------------------------- 5. chunks
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['ei', 'mean'])
def test_chunks_in_any_order_equal_the_single_call(L, kind, dtype):
    """m = 200 as chunks (64, 1, 135), merged ascending and descending through first = 0; with and without a mask; a chunk with
    nothing eligible first or last"""
    case = Case(3, 3, 200, dtype, seed=1400, sign=-1 if kind == 'mean' else 1)
    largest = largest_of(kind, case.sign)
    mu, var, noise = case.dev()
    mu3, var3 = mu.reshape(3, 3, 200), var.reshape(3, 3, 200)
    g = torch.Generator().manual_seed(9)
    half = torch.rand(200, generator=g) < 0.5
    first_empty, last_empty = half.clone(), half.clone()
    first_empty[:64] = False
    last_empty[65:] = False
    ranges = ((0, 64), (64, 65), (65, 200))
    for mask in (None, half, first_empty, last_empty):
        bv, bi, _ = case.run(L, kind, mask=mask)
        for order in (ranges, ranges[::-1]):
            best = None
            for k, (lo, hi) in enumerate(order):
                out = L.mixture_acq(mu3[:, :, lo:hi].contiguous(), var3[:, :, lo:hi].contiguous(), 3, 3, kind, case.best, XI, BETA, case.sign,
                                    noise=noise, mask=None if mask is None else mask[lo:hi].to(DEV), largest=largest, idx_base=lo,
                                    first=k == 0, best_pair=best)
                best = out[:2]
            assert torch.equal(best[1].cpu(), bi) and torch.equal(best[0].cpu(), bv), (None if mask is None else int(mask.sum()), order)


# ----------------------------------------------------------------------------------------------------------- 6. refused calls
def test_refused_calls_launch_nothing(L):
    """every refusal of pacoh_mixture_acq leaves best_val / best_idx / values (a sentinel before) untouched"""
    lib = L.load_library()
    p = lambda t: None if t is None else L._ptr(t)
    for dtype in DTYPES:
        T, P, m = 3, 2, 300
        mu, var = torch.zeros(T * P, m, dtype=dtype, device=DEV), torch.ones(T * P, m, dtype=dtype, device=DEV)
        noise, mask = torch.zeros(P, dtype=dtype, device=DEV), torch.ones(m, dtype=torch.uint8, device=DEV)
        values = torch.full((T, m), -77.0, dtype=dtype, device=DEV)
        bv, bi = torch.full((T,), -77.0, dtype=dtype, device=DEV), torch.full((T,), -77, dtype=torch.int64, device=DEV)
        ws = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
        code = L.dtype_code(mu)
        ok = dict(mu=mu, var=var, noise=noise, mask=mask, values=values, bv=bv, bi=bi, ws=ws, ws_bytes=ws.numel() * 8, kind=0, sign=1, T=T,
                  P=P, m=m, idx_base=0, largest=1, first=1, strips=0, dt=code)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.pacoh_mixture_acq(p(a['mu']), p(a['var']), p(a['noise']), p(a['mask']), p(a['values']), p(a['bv']), p(a['bi']),
                                         p(a['ws']), a['ws_bytes'], a['kind'], 0.5, 0.0, 2.0, a['sign'], a['T'], a['P'], a['m'],
                                         a['idx_base'], a['largest'], a['first'], a['strips'], a['dt'], L._stream())

        refused = [dict(mu=None), dict(var=None), dict(bv=None), dict(bi=None), dict(ws=None), dict(kind=-1), dict(kind=5), dict(sign=0),
                   dict(sign=2), dict(strips=-1), dict(idx_base=-1), dict(largest=2), dict(largest=-1), dict(first=2), dict(first=-1),
                   dict(T=0), dict(P=0), dict(m=0), dict(ws_bytes=lib.pacoh_mixture_acq_workspace_bytes(T, m, 0, code) - 1), dict(dt=5),
                   dict(T=65536)]
        assert len(refused) >= 20
        for kw in refused:
            rc = call(**kw)
            assert rc == (-3 if 'dt' in kw else -2 if kw.get('T') == 65536 else -1), (kw, rc)
        torch.cuda.synchronize()
        assert bool((values == -77.0).all()) and bool((bv == -77.0).all()) and bool((bi == -77).all())
        assert call() == 0                                           # the same buffers, a well-formed call: now they are written
        torch.cuda.synchronize()
        assert not bool((values == -77.0).any()) and not bool((bv == -77.0).any()) and not bool((bi == -77).any())


# ------------------------------------------------------------------------------------------------------- 7. the public API
def _pool(m):
    return np.linspace(-3.6, 3.6, m).reshape(-1, 1) + 0.013 * np.sin(np.arange(m)).reshape(-1, 1)


def _condition(kind):
    model, kw = TC.build_learner(kind)
    cx, cy = TL.tiny_tasks()[1]
    torch.manual_seed(4321)                      # VI 'Bayes' draws its rows at condition()
    return model, kw, model.condition(cx, cy, **kw), cx, cy


def spec_through_predict(cond, tx, kind, observation_noise=False, **kw):
    """the specification applied in fp64 on the CPU to the components of cond.predict(tx, return_density=True), in original units
    -> (values [m], predictive std [m])"""
    dist = cond.predict(tx, return_density=True)
    mu, var = dist._mu_n.double().cpu().unsqueeze(0), dist._var_n.double().cpu().unsqueeze(0)
    noise = None if observation_noise else cond._state.hypers[2].double().cpu().reshape(-1)
    y_mean, y_std = dist.y_mean, dist.y_std
    maximize = kw.get('maximize', True)
    if kw.get('best_f') is None:
        seen = cond._state.ctx_y[:cond.n].double().cpu()
        best_n, xi_n = float(seen.max() if maximize else seen.min()), kw.get('xi', 0.0) / y_std
    else:
        best_n, xi_n = A.to_normalised(kw['best_f'], kw.get('xi', 0.0), y_mean, y_std)
    v = A.mixture_acquisition(mu, var, kind, best_n, xi_n, kw.get('beta', 2.0), 1 if maximize else -1, noise)[0]
    return A.to_original(v, kind, y_mean, y_std), dist.stddev.double().cpu()


def learner_differences(kind):
    """-> (dict: per acquisition kind and direction, the worst |cond.acquisition - specification on cond.predict's components| in
    units of the predictive std ('pi': absolute); cond; tx)"""
    model, kw, cond, cx, cy = _condition(kind)
    tx = _pool(173)
    out = {}
    for acq in A.KINDS:
        for maximize in (True, False):
            args = dict(best_f=0.9, xi=0.02, beta=1.5, maximize=maximize)
            got = cond.acquisition(acq, tx, **args).double().cpu()
            ref, sd = spec_through_predict(cond, tx, acq, **args)
            d = (got - ref).abs()
            out['%s%s' % (acq, '+' if maximize else '-')] = float((d if acq == 'pi' else d / sd).max())
    # the learner's own density object (observation noise included) against the conditioned object asked for the noisy target
    torch.manual_seed(4321)
    dist = model.predict(cx, cy, tx, return_density=True, **kw)
    for maximize in (True, False):
        d = (dist.acquisition('ucb', maximize=maximize) - cond.acquisition('ucb', tx, maximize=maximize, observation_noise=True)).abs()
        out['density_ucb%s' % ('+' if maximize else '-')] = float((d / dist.stddev).max())
    return out, model, kw, cond, tx


@pytest.mark.parametrize('kind', TC.KINDS)
def test_learners_through_the_public_api(L, kind):
    assert LEARNER_BAR is not None and LEARNER_BAR <= 1e-3, 'LEARNER_BAR has not been set from profiles/acq_fp32_errors.txt'
    diffs, model, kw, cond, tx = learner_differences(kind)
    print(kind, diffs)
    for q, v in diffs.items():
        assert v <= LEARNER_BAR, (q, v, diffs)
    m = len(tx)
    y_mean, y_std = float(cond._y_mean.reshape(-1)[0]), float(cond._y_std.reshape(-1)[0])
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(m, generator=g) < 0.6
    for acq in A.KINDS:
        for maximize in (True, False):
            largest = largest_of(acq, 1 if maximize else -1)
            values = cond.acquisition(acq, tx, maximize=maximize)
            assert values.shape == (m,) and values.is_cuda
            # acquire is first_best of acquisition's values in NORMALISED order (the affine map back is increasing: the same order,
            # but it may merge neighbours, so compare through the engine's normalised values)
            st = cond._state
            best_n = float(st.ctx_y[:st.n].max() if maximize else st.ctx_y[:st.n].min())
            _, _, vn = cond._engine.cond_acq(st, cond._norm_x(tx), acq, best_n if acq in ('ei', 'pi') else 0.0, 0.0, 2.0,
                                             1 if maximize else -1, True, None, None, True)
            for mk in (None, mask):
                want_i, want_v = PP.first_best(vn, None if mk is None else mk.to(DEV), largest)
                idx, val = cond.acquire(acq, tx, maximize=maximize, mask=mk)
                assert idx.dtype == torch.int64 and idx.dim() == 0 and int(idx) == int(want_i)
                assert torch.equal(val, A.to_original(want_v, acq, y_mean, y_std))
                assert torch.equal(val, values[int(idx)])
                for chunk in (50, 64, 172, 173, 1000):
                    i2, v2 = cond.acquire(acq, tx, maximize=maximize, mask=mk, chunk=chunk)
                    assert int(i2) == int(idx) and torch.equal(v2, val), (acq, maximize, chunk)
    # best_f=None is the best observed target
    cy = TL.tiny_tasks()[1][1]
    for maximize, seen in ((True, float(cy.max())), (False, float(cy.min()))):
        a = cond.acquisition('ei', tx, maximize=maximize)
        b = cond.acquisition('ei', tx, best_f=seen, maximize=maximize)
        sd = cond.predict(tx, return_density=True).stddev
        # (the two incumbents differ by the fp32 rounding of the normalised target, 2^-24 |best_n| <= 2e-7, and |d ei / d best| <= 1:
        # 1e-5 of a predictive std has a factor of five in hand down to a std of 0.1 in normalised units)
        assert float(((a - b).abs() / sd).max()) <= 1e-5
    # minimising: the 'mean' argmin
    idx, val = cond.acquire('mean', tx, maximize=False)
    mean = cond.acquisition('mean', tx)
    want_i, want_v = PP.first_best(mean, None, largest=False)
    assert int(idx) == int(want_i) and torch.equal(val, want_v)
    # nothing eligible
    idx, val = cond.acquire('ei', tx, mask=np.zeros(m, dtype=bool))
    assert int(idx) == -1 and bool(torch.isnan(val))
    # the density object of cond.predict scores the noisy target: the same launch on the same moments
    dist = cond.predict(tx, return_density=True)
    assert dist.acquisition('ucb').shape == (m,)
    assert torch.equal(dist.acquisition('ucb', beta=1.5), cond.acquisition('ucb', tx, beta=1.5, observation_noise=True))
    assert torch.equal(dist.acquisition('ei', best_f=0.9), cond.acquisition('ei', tx, best_f=0.9, observation_noise=True))
    # a sign test: after observing a large value at the acquired point, 'pi' there drops (the incumbent moved up)
    idx, _ = cond.acquire('pi', tx)
    before = float(cond.acquisition('pi', tx)[int(idx)])
    cond.append(tx[int(idx)].reshape(1, 1), np.array([[float(cy.max()) + 20.0]]))
    after = float(cond.acquisition('pi', tx)[int(idx)])
    assert after < before, (before, after)


# ------------------------------------------------------------------------------------------------------ 8. no dense intermediate
def test_no_dense_intermediate(L):
    """m = 50 000 candidates, the three SVGD rows, chunk = 4096: the allocator's peak rises during cond.acquire by less than HALF of
    what cond.predict on the whole pool allocates.  A condition, not a measurement."""
    model, kw, cond, cx, cy = _condition('svgd')
    m = 50000
    tx = _pool(m)
    cond.acquire('ei', tx[:100])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dist = cond.predict(tx, return_density=True)
    torch.cuda.synchronize()
    dense = torch.cuda.max_memory_allocated() - before
    del dist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, val = cond.acquire('ei', tx, chunk=4096)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise during cond.acquire: %d bytes; cond.predict on the whole pool: %d bytes' % (rise, dense))
    assert 0 <= int(idx) < m and rise < dense // 2, (rise, dense)
