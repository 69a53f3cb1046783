"""The distinct-task PACOH-SVGD step (include/pacoh_gp.h, pacoh_active_tasks): a step's tasks are drawn with replacement
(GPR_meta_svgd.py:102), and where the step runs on the throughput kernels every DISTINCT task of the draw is evaluated once and counts
as often as it was drawn -- sum_{draws t} g(t, p) = sum_{distinct u} count_u g(u, p) (random_gp.py:204-222, the sum over the batch).
PACOH_SVGD_DEDUP=1 forces the path on at these small shapes (default: steps of at least 4096 (task, particle) problems).
Part 1: a draw without repeats gives the bits of the plain step, and the four launch sequences of the step (pipelined or not,
replayed or eager) give the same bits as each other.  Part 2: a draw with repeats against the fp64 oracle and against the plain
step (which sums the same terms in another order: agreement to rounding), at the shapes where the kernels take another path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacoh_oracle as O


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    import meta_learning_pacoh_amd as m
    return m


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def keep_cols(layout):
    """every column of a parameter row but the kernel network's OUTPUT BIAS: its derivative is exactly zero (a stationary kernel sees
    feature differences only), what two differently ordered sums return there is rounding noise (tests/test_gpu_svgd_task.py)"""
    keep = torch.ones(layout.D, dtype=torch.bool)
    sl = layout.slices.get('kernel_nn.out.bias')
    if sl is not None:
        keep[sl[0]:sl[1]] = False
    return keep


def ragged_tasks(T=7, d=2, seed=11):
    """T tasks of 9, 11, 13 points (the tasks of test_pipelined_svgd_step_equals_the_step_begin_sequence)"""
    rs = np.random.RandomState(seed)
    tasks = []
    for t in range(T):
        n = 9 + 2 * (t % 3)
        x = rs.uniform(-3, 3, size=(n, d))
        tasks.append((x, np.sin(x[:, :1]) + 0.3 * x[:, 1:2] + 0.05 * rs.randn(n, 1)))
    return tasks


def even_tasks(T, n, d=2, seed=4):
    rs = np.random.RandomState(seed)
    return [(x, np.sin(x[:, :1]) + 0.3 * x[:, -1:] + 0.05 * rs.randn(n, 1)) for x in (rs.uniform(-3, 3, size=(n, d)) for _ in range(T))]


def learner(M, monkeypatch, dedup, tasks, **kw):
    monkeypatch.setenv('PACOH_SVGD_DEDUP', dedup)
    monkeypatch.setenv('PACOH_SVGD_TASK_FUSED', '0')       # (small grids take the task-fused step otherwise: the throughput kernels are meant)
    args = dict(num_particles=5, lr=1e-2, lr_decay=0.9, random_seed=3)
    args.update(kw)
    return M.GPRegressionMetaLearnedSVGD(tasks, **args)


# ---- part 1: exact bits, and the same bits from every launch sequence -----------------------------------------------------------------
@pytest.mark.parametrize('graph', ['0', '1'])
def test_draws_without_repeats_give_the_bits_of_the_plain_step(M, graph, monkeypatch):
    """no repeated draw: the feed's rows are the draws themselves, all weights 1.0 and n_act == tb -- the device-side split is the host
    plan's, a multiplication by 1.0f is exact: particles, Adam state and bandwidth are those of PACOH_SVGD_DEDUP=0, bit for bit"""
    monkeypatch.setenv('PACOH_GRAPH', graph)
    out = []
    for dedup in ('0', '1'):
        m = learner(M, monkeypatch, dedup, ragged_tasks(), task_batch_size=1)
        m.meta_fit(verbose=False, n_iter=6, log_period=2)               # one task per step: never a repeat
        assert m._feed.dedup == (dedup == '1') and m._task_ws is None and m.opt_step == 6
        for draw in ([1, 5, 2, 0], [6, 0, 3, 4], [2, 1, 0, 5, 6, 4, 3]):
            m.svgd_step(np.array(draw), 0.25)
            assert m._feed.dedup == (dedup == '1')
        out.append((m.particles.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone(), float(m.last_bandwidth)))
    assert bool(torch.isfinite(out[1][0]).all())
    assert all(torch.equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


def test_all_launch_sequences_of_the_distinct_task_step_agree_bit_for_bit(M, monkeypatch):
    """6 draws from 7 tasks (repeats are certain), 13 steps in chunks of 1 + 2 + 3 + ...: pipelined or with pacoh_step_begin, replayed
    or eager -- the same rows, counts and splits reach the same kernels"""
    out = []
    for pipe in ('0', '1'):
        for graph in ('0', '1'):
            monkeypatch.setenv('PACOH_SVGD_PIPELINE', pipe)
            monkeypatch.setenv('PACOH_GRAPH', graph)
            m = learner(M, monkeypatch, '1', ragged_tasks(), task_batch_size=6)
            m.meta_fit(verbose=False, n_iter=13, log_period=3)
            assert m._feed.dedup and m._pipelined == (pipe == '1') and m.opt_step == 13
            out.append((m.particles.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone(), float(m.last_bandwidth)))
    assert bool(torch.isfinite(out[0][0]).all())
    for other in out[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out[0][:3], other[:3])) and out[0][3] == other[3]


# ---- part 2: repeated draws against the oracle and against the plain step -------------------------------------------------------------
@pytest.mark.parametrize('pipe', ['0', '1'])
def test_likelihood_score_of_a_draw_with_repeats_matches_the_oracle(M, pipe, monkeypatch):
    """draw [3, 3, 1, 3, 0, 1]: lik[p] = sum over the six draws of mll[t, p] and its gradient, against O.meta_score on the same six
    (task, ...) entries without the prior term -- the bars of test_svgd_score_and_step_match_oracle (1e-4 on the sums, 1e-2 norm-wise
    on the fp32 score)"""
    from meta_learning_pacoh_amd import _lib as L
    monkeypatch.setenv('PACOH_SVGD_PIPELINE', pipe)
    tasks = ragged_tasks()
    draw = [3, 3, 1, 3, 0, 1]
    m = learner(M, monkeypatch, '1', tasks)
    m._setup_step(len(draw))
    assert m._feed.dedup
    pre = O.meta_pre_factor([tasks[t][0].shape[0] for t in draw])
    m._feed.upload(np.asarray(draw).reshape(1, -1), [L.step_scalars(pre, 1e-2, 1)])
    m._prologue()
    m._body_likelihood()
    torch.cuda.synchronize()
    assert int(m._feed.nact.item()) == 3 and m._feed.mult.tolist() == [3.0, 2.0, 1.0, 0.0, 0.0, 0.0] and int(m._fail.item()) == 0
    cfg = O.GPConfig(2, 'NN', 'NN')
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    lp_o, score_o = O.meta_score(m.particles.cpu().double(), [otasks[t] for t in draw], cfg, pm, ps, 0.0)      # = pre * (sums, gradient)
    print('lik rel %.3e  score rel %.3e' % (rel(m._lik, lp_o / pre), rel(m._score, score_o / pre)))
    assert rel(m._lik, lp_o / pre) < 1e-4
    assert rel(m._score, score_o / pre) < 1e-2


def compare_learners(m1, m0, tag):
    keep = keep_cols(m1.layout).to(m1.device)
    figures = (rel(m1.particles[:, keep], m0.particles[:, keep]), rel(m1.exp_avg[:, keep], m0.exp_avg[:, keep]),
               rel(m1.exp_avg_sq[:, keep], m0.exp_avg_sq[:, keep]))
    print('%s: particles %.3e  exp_avg %.3e  exp_avg_sq %.3e  (|exp_avg| %.3e)' % ((tag,) + figures + (float(m0.exp_avg.norm()),)))
    assert bool(torch.isfinite(m1.particles).all()) and float(m0.exp_avg.norm()) > 0           # (a step was taken)
    # two differently ordered fp32 sums of the same step: the bounds of test_svgd_learner_on_the_task_fused_step
    assert figures[0] < 5e-5 and figures[1] < 2e-3 and figures[2] < 2e-3


@pytest.mark.parametrize('graph', ['0', '1'])
def test_twelve_steps_with_repeats_track_the_plain_step(M, graph, monkeypatch):
    monkeypatch.setenv('PACOH_GRAPH', graph)
    out = []
    for dedup in ('0', '1'):
        m = learner(M, monkeypatch, dedup, ragged_tasks(), task_batch_size=6)
        m.meta_fit(verbose=False, n_iter=12, log_period=5)
        assert m._feed.dedup == (dedup == '1') and m.opt_step == 12
        out.append(m)
    compare_learners(out[1], out[0], 'graph=' + graph)


EDGES = {
    # name: (tasks, draw, learner arguments)                     (feature_dim is 2 in every learner: the f <= 2 GP kernels)
    'one distinct task': (lambda: ragged_tasks(), [2, 2, 2, 2], {}),
    'n_act = tb - 1': (lambda: ragged_tasks(), [1, 5, 2, 1], {}),
    'ragged rows, 3 of 7': (lambda: ragged_tasks(), [6, 0, 6, 6, 4, 0, 4], {}),      # R_eff = 35 of 77 rows: no multiple of a tile
    '40 draws of one 64-point task': (lambda: even_tasks(5, 64), [3] * 40, dict(num_particles=8)),   # R_eff = 64 of 2560: idle workgroups
    'n = 64': (lambda: even_tasks(4, 64), [1, 3, 1, 0, 3, 1], {}),                   # GP: 4 blocks
    'n = 128': (lambda: even_tasks(3, 128), [1, 1, 0], dict(num_particles=2)),        # GP: 8 blocks
    'one parameter row': (lambda: ragged_tasks(), [0, 4, 4, 6, 0], dict(num_particles=1)),
    '20 parameter rows': (lambda: ragged_tasks(), [0, 4, 4, 6, 0], dict(num_particles=20)),
    '4 inputs, 3 hidden layers': (lambda: ragged_tasks(d=4), [5, 5, 1, 5], dict(mean_nn_layers=(32,) * 3, kernel_nn_layers=(32,) * 3)),
}


@pytest.mark.parametrize('name', sorted(EDGES))
@pytest.mark.parametrize('pipe', ['0', '1'])
def test_one_step_at_the_edges_tracks_the_plain_step(M, name, pipe, monkeypatch):
    make, draw, kw = EDGES[name]
    monkeypatch.setenv('PACOH_SVGD_PIPELINE', pipe)
    tasks = make()
    out = []
    for dedup in ('0', '1'):
        m = learner(M, monkeypatch, dedup, tasks, **kw)
        m.svgd_step(np.array(draw), 0.25)
        torch.cuda.synchronize()
        assert m._feed.dedup == (dedup == '1') and m._task_ws is None
        if dedup == '1':
            assert int(m._feed.nact_all[0].item()) == len(set(draw)) and int(m._fail.item()) == 0
        out.append(m)
    compare_learners(out[1], out[0], name)


def test_the_default_follows_the_problem_count(M, monkeypatch):
    """without PACOH_SVGD_DEDUP: off below one resident round of the GP kernel (4096 problems), on from there"""
    monkeypatch.delenv('PACOH_SVGD_DEDUP', raising=False)
    monkeypatch.setenv('PACOH_SVGD_TASK_FUSED', '0')
    tasks = even_tasks(205, 5, d=1)
    for tb, P, want in ((4, 5, False), (204, 20, False), (205, 20, True)):
        m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, task_batch_size=tb, random_seed=1)
        m._setup_step(tb)
        assert tb * P < 4096 or want
        assert m._feed.dedup is want
    m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=20, task_batch_size=205, random_seed=1, mean_nn_layers=(64, 64),
                                      kernel_nn_layers=(64, 64))       # (networks wider than the fused kernels take: not eligible)
    m._setup_step(205)
    assert m._feed.dedup is False
