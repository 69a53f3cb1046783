"""The two networks' forward inside the task-GP launch (csrc/gp_fwd_reg.hip, pacoh_fwd_gp_lml_fwdbwd; PACOH_FWD_GP): it is the
arithmetic of pacoh_mlp2_fwd followed by pacoh_gp_lml_fwdbwd, operation by operation, so every output -- and the activation stash
the unchanged backward reads -- must be the SAME BITS as the two launches': no tolerance anywhere in this file.
Part 1: the entry point against the two-launch sequence on tiny batches (the hazards are inside one 64-point problem).
Part 2: the SVGD learner with PACOH_FWD_GP=1 against =0, eager and replayed.  Part 3: shapes outside the path keep the old sequence.
Host-side checks (not marked gpu) are at the end."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    return _lib


def same_bits(a, b):
    """bit-for-bit equality (NaNs of a failed problem included)"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def net_params(d_in, hidden, d_out):
    prev, c = d_in, 0
    for h in hidden:
        c += h * (prev + 1)
        prev = h
    return c + d_out * (prev + 1)


def problem(T, P, d_in, hidden, f, seed):
    """theta rows with the mean network at column 3 and the kernel-feature network behind it (odd offsets: no 16-byte alignment)"""
    g = torch.Generator().manual_seed(seed)
    n = 64
    off_m = 3
    off_k = off_m + net_params(d_in, hidden, 1) + 2
    D = off_k + net_params(d_in, hidden, f) + 5
    dev = 'cuda'
    return dict(T=T, P=P, n=n, d_in=d_in, hidden=list(hidden), f=f, off_m=off_m, off_k=off_k,
                theta=(0.4 * torch.randn(P, D, generator=g)).to(dev), x=torch.randn(T, n, d_in, generator=g).to(dev),
                y=torch.randn(T, n, generator=g).to(dev), ls=(torch.rand(P, f, generator=g) + 0.5).to(dev),
                noise=(torch.rand(P, generator=g) * 0.3 + 0.05).to(dev))


def both_sequences(L, q, n_valid=None, g_lml=None, active=None):
    """-> (outputs, stash) of the two-launch sequence and of the fused launch; the stash starts as zeros in both"""
    T, P, n, f = q['T'], q['P'], q['n'], q['f']
    B = T * P
    res = []
    for fused in (False, True):
        stash = L.mlp2_stash(q['x'], P, q['d_in'], q['hidden'], 1, f, B, n)
        if stash is not None:
            stash.zero_()
        if fused:
            out = L.fwd_gp_lml_fwdbwd(q['x'], P, q['theta'], P, q['d_in'], q['hidden'], q['off_m'], q['off_k'], f, q['y'], P, q['ls'],
                                      q['noise'], B, n, n_valid=n_valid, g_lml=g_lml, stash=stash, active=active)
        else:
            mean, z = L.mlp2_fwd(q['x'], P, q['theta'], P, q['d_in'], q['hidden'], q['off_m'], 1, q['off_k'], f, B, n, stash=stash,
                                 active=active)
            out = L.gp_lml_fwdbwd(z, 1, mean.reshape(B, n), L.MEAN_VECTOR, q['y'], P, q['ls'], None, q['noise'], B, P, n_valid=n_valid,
                                  g_lml=g_lml, want_dz=True, active=active)
        torch.cuda.synchronize()
        res.append((out, stash))
    return res


NAMES = ('lml', 'd_z', 'd_mean', 'd_ls', 'd_os', 'd_noise', 'info')


def assert_same(res, live):
    """the first `live` problems' outputs (the others are not evaluated: left as allocated) and the whole stash"""
    (o0, s0), (o1, s1) = res
    for name, a, b in zip(NAMES, o0, o1):
        if a is None and b is None:
            continue
        assert same_bits(a[:live], b[:live]), name
    assert (s0 is None) == (s1 is None)
    if s0 is not None:
        assert torch.equal(s0, s1), 'stash'
        assert bool((s0 != 0).any())
    assert bool(torch.isfinite(o1[0][:live]).all())


# ---- part 1: the entry point, bit for bit ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('hidden', [(32, 32), (8, 12), (32,)])
@pytest.mark.parametrize('d_in', [1, 4])
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('T', [1, 3, 5])
def test_fused_launch_equals_the_two_launches_bit_for_bit(L, T, P, d_in, hidden):
    f = 2 if d_in == 4 else 1
    q = problem(T, P, d_in, hidden, f, seed=100 * T + 10 * P + d_in + len(hidden))
    assert L.fwd_gp_applicable(T * P, P, 64, P, d_in, list(hidden), f, False, L.MEAN_VECTOR, torch.float32)
    assert_same(both_sequences(L, q), T * P)
    # ragged tasks (1, 49 and 64 valid points in one batch), fewer active tasks than T with multiplicities != 1, upstream weight != 1
    n_valid = torch.tensor(([49, 1, 64] * 2)[:T], dtype=torch.int32, device='cuda')
    n_act = max(1, T - 1)
    active = (torch.tensor([n_act], dtype=torch.int32, device='cuda'),
              torch.tensor(([3.0, 1.0, 2.0, 5.0, 0.0])[:T], dtype=torch.float32, device='cuda'))
    g_lml = torch.full((T * P,), 0.37, dtype=torch.float32, device='cuda')
    assert_same(both_sequences(L, q, n_valid=n_valid, g_lml=g_lml, active=active), n_act * P)


@gpu
def test_jitter_ladder_takes_the_same_rung_and_raises_the_same_flag(L):
    """task 1: 64 copies of one point (a rank-one Gram matrix) under a noise of 1e-12 for particle 2 -- the Cholesky fails without
    jitter; both sequences must climb to the same rung (info) and return the same numbers, NaNs of a lost problem included"""
    T, P = 3, 3
    q = problem(T, P, 4, (32, 32), 2, seed=7)
    q['x'][1] = q['x'][1, :1].expand(64, 4).clone()
    q['noise'][2] = 1e-12
    res = both_sequences(L, q)
    info = res[1][0][6].cpu().reshape(T, P)
    print('info', info.tolist())
    assert int(info[1, 2]) != 0, 'the singular problem was meant to need jitter'
    (o0, s0), (o1, s1) = res
    for name, a, b in zip(NAMES, o0, o1):
        assert same_bits(a, b), name
    assert torch.equal(s0, s1)


# ---- part 2: the learner ------------------------------------------------------------------------------------------------------------------
def tasks64(T=5, d=2, seed=4):
    rs = np.random.RandomState(seed)
    return [(x, np.sin(x[:, :1]) + 0.3 * x[:, -1:] + 0.05 * rs.randn(64, 1)) for x in (rs.uniform(-3, 3, size=(64, d)) for _ in range(T))]


def run_learner(monkeypatch, fwd_gp, graph, dedup):
    import meta_learning_pacoh_amd as M
    from meta_learning_pacoh_amd import _lib
    monkeypatch.setenv('PACOH_FWD_GP', fwd_gp)
    monkeypatch.setenv('PACOH_GRAPH', graph)
    monkeypatch.setenv('PACOH_SVGD_DEDUP', dedup)
    monkeypatch.setenv('PACOH_SVGD_TASK_FUSED', '0')       # (small grids take the task-fused step otherwise: the throughput kernels are meant)
    calls = []
    real = _lib.fwd_gp_lml_fwdbwd
    monkeypatch.setattr(_lib, 'fwd_gp_lml_fwdbwd', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m = M.GPRegressionMetaLearnedSVGD(tasks64(), num_particles=3, task_batch_size=5, lr=1e-2, lr_decay=0.9, random_seed=3)
    m.meta_fit(verbose=False, n_iter=6, log_period=2)
    assert m.opt_step == 6 and m._task_ws is None and m._feed.dedup == (dedup == '1')
    m.svgd_step(np.array([1, 3, 1, 0, 3]), 0.25)               # a draw with repeats, then one without
    m.svgd_step(np.array([4, 2, 0, 1, 3]), 0.25)
    torch.cuda.synchronize()
    assert (len(calls) > 0) == (fwd_gp == '1')
    assert int(m._fail.item()) == 0 and bool(torch.isfinite(m.particles).all())
    return m.particles.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone(), m._lik.clone(), float(m.last_bandwidth)


@gpu
@pytest.mark.parametrize('dedup', ['0', '1'])
def test_svgd_learner_is_the_same_bits_with_and_without_the_fused_launch(L, dedup, monkeypatch):
    """6 + 2 steps on 5 tasks x 3 particles (5 draws from 5 tasks: repeats; PACOH_SVGD_DEDUP=1 evaluates each distinct task once):
    particles, both Adam moments, lik and the bandwidth (the distance block moved launches) -- and a replayed graph equals eager"""
    off = run_learner(monkeypatch, '0', '0', dedup)
    on = run_learner(monkeypatch, '1', '0', dedup)
    on_graph = run_learner(monkeypatch, '1', '1', dedup)
    for other in (on, on_graph):
        assert all(same_bits(a, b) for a, b in zip(off[:4], other[:4])) and off[4] == other[4]


# ---- part 3: outside the path -----------------------------------------------------------------------------------------------------------
@gpu
def test_other_shapes_keep_the_two_launch_sequence(L, monkeypatch):
    """PACOH_FWD_GP=1, but n = 48 or an outputscale: the query says no and lml_and_grad runs the forward and the GP launch"""
    from meta_learning_pacoh_amd.engine import GPEngine, TaskBatch, ParamLayout
    monkeypatch.setenv('PACOH_FWD_GP', '1')
    calls = []
    real = L.fwd_gp_lml_fwdbwd
    monkeypatch.setattr(L, 'fwd_gp_lml_fwdbwd', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    rs = np.random.RandomState(0)
    for n, with_os, want in ((64, False, True), (48, False, False), (64, True, False)):
        lay = ParamLayout(2, feature_dim=2, with_outputscale=with_os)
        eng = GPEngine(lay)
        tasks = TaskBatch([(rs.randn(n, 2), rs.randn(n, 1)) for _ in range(3)], torch.device('cuda'))
        theta = (0.3 * torch.randn(2, lay.D, generator=torch.Generator().manual_seed(1))).cuda()
        batch = tasks.select(torch.arange(3, device='cuda'))
        del calls[:]
        lml, grad, info = eng.lml_and_grad(theta, batch)
        torch.cuda.synchronize()
        assert (len(calls) == 1) == want
        assert bool(torch.isfinite(lml).all()) and bool(torch.isfinite(grad).all())


# ---- host only ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from meta_learning_pacoh_amd._build import build_library
    build_library(verbose=False)              # no-op when the in-tree .so is up to date
    from meta_learning_pacoh_amd import _lib
    return _lib.load_library()


def test_applicability_query_over_shapes(lib):
    F32, F64, RBF, MATERN32, VECTOR, CONST = 0, 1, 0, 4, 1, 2
    h = lambda *w: (ctypes.c_int32 * len(w))(*w)

    def ok(B=15, P=3, n=64, x_div=3, d_in=4, hidden=(32, 32), f=2, has_os=0, mode=VECTOR, dtype=F32, kernel=RBF):
        return lib.pacoh_fwd_gp_applicable(B, P, n, x_div, d_in, h(*hidden), len(hidden), f | (kernel << 8), has_os, mode, dtype)

    assert ok() == 1 and ok(hidden=(32,)) == 1 and ok(hidden=(8, 12)) == 1 and ok(d_in=1, f=1) == 1 and ok(B=20480, P=20, x_div=20) == 1
    assert ok(n=48) == 0 and ok(n=128) == 0                       # one stash tile is one task only at n = 64
    assert ok(has_os=1) == 0 and ok(dtype=F64) == 0 and ok(kernel=MATERN32) == 0 and ok(mode=CONST) == 0
    assert ok(f=3) == 0 and ok(d_in=5) == 0 and ok(hidden=(32, 32, 32)) == 0 and ok(hidden=(64, 64)) == 0 and ok(hidden=(32, 33)) == 0
    assert ok(x_div=1) == 0 and ok(B=16) == 0                     # per-problem inputs (VI with per-task theta); B not a multiple of P


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays(lib):
    from meta_learning_pacoh_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pacoh_gp.h')).read(), flags=re.S)
    for name in ('pacoh_fwd_gp_lml_fwdbwd', 'pacoh_fwd_gp_applicable'):
        assert re.search(r'\b%s\s*\(' % name, src) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.pacoh_abi_version() == _lib.ABI_VERSION == 14
    null, fake, ELIMIT, EINVAL = None, ctypes.c_void_p(4096), -2, -1
    hidden = (ctypes.c_int32 * 2)(32, 32)
    args = lambda n, x: (null, x, 3, fake, 2500, 3, 4, hidden, 2, 0, 1300, null, null, null, 0, 0, null, fake, 3, fake, null, fake, null,
                         null, fake, fake, fake, fake, null, fake, fake, 15, n, 2, 0, null)
    assert lib.pacoh_fwd_gp_lml_fwdbwd(*args(48, fake)) == ELIMIT          # limits are checked before anything is launched
    assert lib.pacoh_fwd_gp_lml_fwdbwd(*args(64, null)) == EINVAL
