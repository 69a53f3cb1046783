"""pacoh_distinct_rows (csrc/distinct.hip): the device-side rewrite of a chunk's task draws as each row's distinct tasks, their draw
counts and their number.  engine.distinct_rows (numpy, tests/test_dedup_host.py) is the specification: integer work only, so every
comparison here is exact.  Part 1: the kernel against it.  Part 2: the shapes it declines, and the feed's fallback.  Part 3: the
PACOH-SVGD learner on the device path against PACOH_DEDUP_HOST=1, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from meta_learning_pacoh_amd.engine import StepFeed, distinct_rows

DTYPES = [torch.float32, torch.float64]
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


def check_against_numpy(L, idx, T, dtype):
    """both forms of the call on the draws idx [k, tb]: into separate buffers (the draws stay as they are) and in place"""
    k, tb = idx.shape
    want_rows, want_mult, want_n = distinct_rows(idx, NP_DTYPE[dtype])
    assert want_mult.dtype == NP_DTYPE[dtype] and want_n.dtype == np.int32
    dev = torch.from_numpy(idx).cuda()
    for in_place in (False, True):
        src = dev.clone()
        rows = src if in_place else torch.full_like(src, -7)
        mult = torch.full((k, tb), -1.0, dtype=dtype, device='cuda')
        n_act = torch.full((k,), -1, dtype=torch.int32, device='cuda')
        assert L.distinct_rows(src, mult, n_act, T, rows=None if in_place else rows) is True
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy(), want_rows), 'rows, in_place=%s' % in_place
        assert np.array_equal(mult.cpu().numpy(), want_mult), 'mult, in_place=%s' % in_place
        assert np.array_equal(n_act.cpu().numpy(), want_n), 'n_act, in_place=%s' % in_place
        if not in_place:
            assert torch.equal(src, dev)
    return want_n


# ---- part 1: the kernel against the specification ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,tb,T', [(1, 1, 1), (3, 7, 1), (4, 64, 5000), (5, 65, 9), (2, 257, 300), (8, 1024, 1024)])
def test_kernel_equals_the_host_rewrite(L, k, tb, T, dtype):
    """one draw; all draws equal; (almost surely) no repeats; more draws than a wavefront and few ids; a row that is no multiple of the
    workgroup; the flagship's row (four draws per thread, eight workgroups)"""
    idx = np.random.RandomState(1000 * k + tb).randint(0, T, size=(k, tb))
    n = check_against_numpy(L, idx, T, dtype)
    if T == 1:
        assert (n == 1).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_kernel_on_built_rows_and_on_a_chunk_as_upload_lays_it_out(L, dtype):
    """a permutation (n_act == tb, the row comes back as it is); one id drawn tb - 1 times and another in the last position; and three
    real rows followed by copies of the last one (the rows a several-steps graph reads behind a short chunk)"""
    rs = np.random.RandomState(5)
    tb, T = 300, 300
    perm = rs.permutation(T)
    tail = np.full(tb, 17)
    tail[-1] = 4
    built = np.stack([perm, tail])
    n = check_against_numpy(L, built, T, dtype)
    assert n.tolist() == [tb, 2]
    real = rs.randint(0, T, size=(3, tb))
    chunk = np.concatenate([real, np.repeat(real[-1:], 3, axis=0)])
    n = check_against_numpy(L, chunk, T, dtype)
    assert (n[3:] == n[2]).all()


def test_kernel_at_the_limits_of_the_device_path(L):
    """the largest row and task count the entry point takes: 16 draws per thread, 56 KB of LDS tables"""
    idx = np.random.RandomState(9).randint(0, L.DISTINCT_MAX_TASKS, size=(2, L.DISTINCT_MAX_DRAWS))
    idx[1, :] = idx[1, :] % 50 + L.DISTINCT_MAX_TASKS - 50          # (the last table entries, many repeats)
    check_against_numpy(L, idx, L.DISTINCT_MAX_TASKS, torch.float32)


# ---- part 2: declined shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,tb,T', [(2, 5, 8193), (1, 4097, 10)])
def test_entry_point_declines_beyond_its_limits_and_touches_nothing(L, k, tb, T):
    idx = torch.from_numpy(np.random.RandomState(2).randint(0, T, size=(k, tb))).cuda()
    keep = idx.clone()
    mult = torch.full((k, tb), -1.0, device='cuda')
    n_act = torch.full((k,), -1, dtype=torch.int32, device='cuda')
    assert L.distinct_rows(idx, mult, n_act, T) is False
    torch.cuda.synchronize()
    assert torch.equal(idx, keep) and bool((mult == -1.0).all()) and bool((n_act == -1).all())


def feed_rows(L, n_tasks, draws, monkeypatch, host=None):
    """what a distinct-task StepFeed of draws.shape[1] tasks per step holds after upload(draws): (idx_all, mult_all, nact_all) of the
    rows the step's kernels may read, and whether the device rewrote them"""
    if host is None:
        monkeypatch.delenv('PACOH_DEDUP_HOST', raising=False)
    else:
        monkeypatch.setenv('PACOH_DEDUP_HOST', host)
    k, tb = draws.shape
    feed = StepFeed(torch.device('cuda'), torch.float32, tb, chunk=8)
    feed.enable_dedup(n_tasks)
    for _ in range(2):                                     # (both staging sets)
        feed.upload(draws, [L.step_scalars(1.0, 1e-3, j + 1) for j in range(k)])
    torch.cuda.synchronize()
    return feed, feed.dedup_on_device


def test_feed_rewrites_on_the_device_and_falls_back_to_the_host(L, monkeypatch):
    """the same draws through the device path, through PACOH_DEDUP_HOST=1 and through a feed whose task count the entry point declines:
    the same three buffers, equal to the numpy result, the rows behind the chunk repeating its last row"""
    from meta_learning_pacoh_amd.engine import GRAPH_STEPS
    draws = np.random.RandomState(3).randint(0, 9, size=(3, 12))
    want_rows, want_mult, want_n = distinct_rows(draws)
    kk = max(3, GRAPH_STEPS) + 1
    for n_tasks, host, on_device in ((9, None, True), (9, '1', False), (9, '0', True), (L.DISTINCT_MAX_TASKS + 1, None, False)):
        feed, dev = feed_rows(L, n_tasks, draws, monkeypatch, host)
        assert dev is on_device
        rows, mult, n = feed.idx_all.cpu().numpy(), feed.mult_all.cpu().numpy(), feed.nact_all.cpu().numpy()
        assert np.array_equal(rows[:3], want_rows) and np.array_equal(mult[:3], want_mult) and np.array_equal(n[:3], want_n)
        assert (rows[3:kk] == want_rows[2]).all() and (mult[3:kk] == want_mult[2]).all() and (n[3:kk] == want_n[2]).all()


# ---- part 3: the learner ------------------------------------------------------------------------------------------------------------
def small_tasks(T=6, n=8, d=2, seed=4):
    rs = np.random.RandomState(seed)
    return [(x, np.sin(x[:, :1]) + 0.3 * x[:, -1:] + 0.05 * rs.randn(n, 1)) for x in (rs.uniform(-3, 3, size=(n, d)) for _ in range(T))]


@pytest.mark.parametrize('no_graph', ['0', '1'])
@pytest.mark.parametrize('calls', [(5,), (2, 3)])
def test_learner_on_the_device_path_equals_the_host_path_bit_for_bit(L, calls, no_graph, monkeypatch):
    """6 tasks x 8 points, 3 particles, 8 draws per step (repeats are certain), 5 steps in one call or as 2 + 3, replayed or launch by
    launch: particles, both Adam moments and the bandwidth of the device-side rewrite are those of PACOH_DEDUP_HOST=1"""
    import meta_learning_pacoh_amd as M
    monkeypatch.setenv('PACOH_SVGD_DEDUP', '1')
    monkeypatch.setenv('PACOH_SVGD_TASK_FUSED', '0')       # (the throughput kernels are the ones that read the distinct-task feed)
    monkeypatch.setenv('PACOH_NO_GRAPH', no_graph)
    out = []
    for host in ('0', '1'):
        monkeypatch.setenv('PACOH_DEDUP_HOST', host)
        m = M.GPRegressionMetaLearnedSVGD(small_tasks(), num_particles=3, task_batch_size=8, lr=1e-2, lr_decay=0.9, random_seed=3)
        for n in calls:
            m._train_steps(n)
        torch.cuda.synchronize()
        assert m._feed.dedup and m._feed.dedup_on_device == (host == '0') and m.opt_step == 5
        assert int(m._fail.item()) == 0 and int(m._feed.nact_all[0].item()) < 8
        out.append((m.particles.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone(), m.last_bandwidth.clone(),
                    m._feed.idx_all.clone(), m._feed.mult_all.clone(), m._feed.nact_all.clone()))
    assert bool(torch.isfinite(out[0][0]).all()) and bool((out[0][2] > 0).any())
    for a, b in zip(*out):
        assert torch.equal(a, b)
