"""End-to-end parity of the three meta-learners (host classes + HIP kernels through the C ABI) against
the CPU oracle, the recorded reference trajectory (demo.ipynb) and the behaviours asserted by the
reference's own tests (tests/test_GPR.py:173-222: seed consistency, state_dict round trip)."""
import json
import os

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


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def demo_data():
    env = O.SinusoidDataset(np.random.RandomState(26))
    return env.generate_meta_train_data(20, 5), env.generate_meta_test_data(20, 5, 50)


# ------------------------------------------------------------------------------------------ MAP
def test_map_first_iterations_match_oracle(M):
    train, test = demo_data()
    model = M.GPRegressionMetaLearned(train, weight_decay=0.2, num_iter_fit=50, random_seed=30)
    orc = O.MapOracle(train, weight_decay=0.2, num_iter_fit=50, random_seed=30)
    # same initial parameters (same RNG consumption order as the reference: kernel net, then mean net)
    lay = model.layout
    lo, hi = lay.slices['kernel_nn.fc_1.weight']
    assert relerr(model.theta[0, lo:hi], orc.kernel_net[0].weight.reshape(-1)) == 0
    lo, hi = lay.slices['mean_nn.out.bias']
    assert relerr(model.theta[0, lo:hi], orc.mean_net[-1].bias.reshape(-1)) == 0
    log_o = orc.meta_fit(test, log_period=50, n_iter=50)
    model.meta_fit(test, log_period=50, n_iter=50, verbose=False)
    ll, rmse, calib = model.eval_datasets(test)
    assert abs(ll - log_o[-1][2]) < 2e-3 and abs(rmse - log_o[-1][3]) < 2e-3 and abs(calib - log_o[-1][4]) < 5e-3
    # parameters after 50 AdamW steps
    got = torch.cat([model.theta[0, lay.slices['kernel_nn.fc_2.weight'][0]:lay.slices['kernel_nn.fc_2.weight'][1]].cpu()])
    assert relerr(got, orc.kernel_net[1].weight.reshape(-1)) < 1e-3
    cx, cy, tx, _ = test[0]
    pm, ps = model.predict(cx, cy, tx)
    mean_n, cov_n = orc.predict_normalized(cx, cy, tx)
    assert relerr(pm, mean_n * orc.stats[3][0] + orc.stats[2][0]) < 1e-3
    assert relerr(ps, torch.sqrt(torch.diagonal(cov_n)) * orc.stats[3][0]) < 1e-3


def test_map_reproduces_recorded_reference_trajectory(M, golden_dir):
    """config #1: the demo.py run of the real reference (demo.ipynb:115-127,164-166), now on the HIP path.
    fp32 trajectories drift with summation order, so later log lines get a wider band."""
    with open(os.path.join(golden_dir, 'demo_log.json')) as f:
        gold = json.load(f)
    train, test = demo_data()
    model = M.GPRegressionMetaLearned(train, weight_decay=0.2, num_iter_fit=12000, random_seed=30)
    logs = []

    class Grab:
        def info(self, msg):
            logs.append(msg)
    model.logger = Grab()
    model.meta_fit(test, log_period=1000)
    assert len(logs) == 13
    for msg, ref in zip(logs, gold['log']):
        parts = msg.replace('Iter ', '').split(' - ')
        itr = int(parts[0].split('/')[0])
        loss = float(parts[1].split(': ')[1])
        ll, rmse, calib = (float(parts[k].split(' ')[-1]) for k in (3, 4, 5))
        assert itr == ref[0]
        if itr == 1:
            assert abs(loss - ref[1]) < 2e-5 and abs(ll - ref[2]) < 1.5e-3 and abs(rmse - ref[3]) < 1.5e-3
        else:
            assert abs(loss - ref[1]) < 0.03 + 0.02 * abs(ref[1]), (msg, ref)
            assert abs(ll - ref[2]) < 0.03 and abs(rmse - ref[3]) < 0.02 and abs(calib - ref[4]) < 0.02, (msg, ref)
    ll, rmse, calib = model.eval_datasets(test)
    assert abs(ll - gold['final_test']['ll']) < 0.03
    assert abs(rmse - gold['final_test']['rmse']) < 0.02
    assert abs(calib - gold['final_test']['calib']) < 0.02


def sample_data_nonstationary(rs, size=1):
    def _sample_fun():
        slope = rs.normal(loc=1, scale=0.2)
        freq = lambda x: 1 + np.abs(x)
        mean = lambda x: slope * x
        return lambda x: (mean(x) + np.sin(freq(x) * x)) / 5
    func = _sample_fun()
    X = rs.uniform(-5, 5, size=(size, 1))
    Y = func(X)
    return X, Y


def test_map_seed_consistency_and_state_dict_roundtrip(M, tmp_path):
    """reference tests/test_GPR.py:173-222"""
    rs = np.random.RandomState(23)
    train = [sample_data_nonstationary(rs, 5) for _ in range(3)]
    test = [sample_data_nonstationary(rs, 55) for _ in range(3)]
    test = [(x[:5], t[:5], x[5:], t[5:]) for x, t in test]
    m1 = M.GPRegressionMetaLearned(train[:2], learning_mode='both', num_iter_fit=5, random_seed=22)
    m2 = M.GPRegressionMetaLearned(train[:2], learning_mode='both', num_iter_fit=5, random_seed=22)
    m1.meta_fit(valid_tuples=test, verbose=False)
    m2.meta_fit(valid_tuples=test, verbose=False)
    for cx, cy, tx, _ in test:
        p1, p2 = m1.predict(cx, cy, tx), m2.predict(cx, cy, tx)
        assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])          # bitwise, as in the reference
    for mean_module in ['constant', 'NN']:
        a = M.GPRegressionMetaLearned(train, learning_mode='both', num_iter_fit=5, mean_module=mean_module, random_seed=22)
        a.meta_fit(verbose=False)
        pred_1 = a.predict(*test[0][:3])
        b = M.GPRegressionMetaLearned(train, learning_mode='both', num_iter_fit=5, mean_module=mean_module, random_seed=25)
        b.meta_fit(verbose=False)
        pred_2 = b.predict(*test[0][:3])
        torch.save(a.state_dict(), str(tmp_path / 'test_torch_serialization.pkl'))
        b.load_state_dict(torch.load(str(tmp_path / 'test_torch_serialization.pkl')))
        pred_3 = b.predict(*test[0][:3])
        assert not np.array_equal(pred_1[0], pred_2[0])
        assert np.array_equal(pred_1[0], pred_3[0]) and np.array_equal(pred_1[1], pred_3[1])
        a.rds_numpy, b.rds_numpy = np.random.RandomState(55), np.random.RandomState(55)
        a.meta_fit(verbose=False)
        b.meta_fit(verbose=False)
        assert np.array_equal(a.predict(*test[0][:3])[0], b.predict(*test[0][:3])[0])


@pytest.mark.parametrize('mean_module,covar_module,mode', [('constant', 'SE', 'both'), ('zero', 'SE', 'learn_kernel'),
                                                            ('NN', 'SE', 'learn_mean'), ('zero', 'SE', 'vanilla')])
def test_map_module_variants_match_oracle(M, mean_module, covar_module, mode):
    train, test = demo_data()
    model = M.GPRegressionMetaLearned(train, learning_mode=mode, weight_decay=0.1, num_iter_fit=30, mean_module=mean_module,
                                      covar_module=covar_module, random_seed=4)
    loss = model.meta_fit(log_period=1000, verbose=False)
    if mode == 'both':
        orc = O.MapOracle(train, weight_decay=0.1, num_iter_fit=30, mean_module=mean_module, covar_module=covar_module,
                          random_seed=4)
        orc.meta_fit(None, log_period=1000)
        got = model.eval_datasets(test)
        ref = orc.eval_datasets(test)
        assert np.allclose(got, ref, atol=3e-3)
    else:
        assert np.isfinite(loss)
        lay = model.layout
        lo, hi = lay.slices['lengthscale_raw']
        moved = float(model.theta[0, lo:hi].abs().sum()) > 0
        assert moved == (mode in ('learn_kernel',))          # raw lengthscale starts at 0 and only moves if trained


# ------------------------------------------------------------------------------------------ SVGD
def tasks_nd(T, n, d):
    return O.sinusoid_tasks_nd(T, n, d, seed0=1000)


@pytest.mark.parametrize('mean_module,covar_module,d,n', [('NN', 'NN', 4, 64), ('constant', 'SE', 4, 64), ('NN', 'SE', 1, 32)])
def test_svgd_score_and_step_match_oracle(M, mean_module, covar_module, d, n):
    T, P = 6, 5
    tasks = tasks_nd(T, n, d)
    model = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, mean_module=mean_module, covar_module=covar_module,
                                          random_seed=3, lr=1e-2, bandwidth=None)
    cfg = O.GPConfig(d, mean_module, covar_module)
    assert cfg.D == model.layout.D
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    # same particle initialisation stream as the reference (model construction, then one prior draw)
    torch.manual_seed(3)
    O.consume_vectorized_gp_init_rng(cfg)
    theta0 = O.hyperprior_sample(cfg.layout, pm, ps, P)
    assert relerr(model.particles, theta0) == 0
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    idx = np.arange(T)
    pre = O.meta_pre_factor([n] * T)
    lp, score = model._log_prob_and_score(model.particles, idx, pre)
    lp_o, score_o = O.meta_score(theta0.double(), otasks, cfg, pm, ps, 0.01)
    assert relerr(lp, lp_o) < 1e-4
    assert relerr(score, score_o) < 1e-2                       # fp32 bar, norm-wise
    # three full SVGD steps vs oracle (closed-form phi + torch Adam), same task order
    X = theta0.double().clone()
    opt = torch.optim.Adam([X], lr=1e-2)
    for _ in range(3):
        _, s = O.meta_score(X, otasks, cfg, pm, ps, 0.01)
        phi, _ = O.svgd_phi_closed_form(X.detach(), s, None)
        X.grad = -phi
        opt.step()
        model.svgd_step(idx, pre)
    assert relerr(model.particles, X) < 2e-3


def test_svgd_predict_and_eval_match_oracle(M):
    T, P, n, d = 5, 4, 20, 2
    tasks = tasks_nd(T, n, d)
    model = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, random_seed=1, num_iter_fit=3)
    model.meta_fit(verbose=False)
    cfg = O.GPConfig(d, 'NN', 'NN')
    theta = model.particles.cpu().double()
    stats = O.compute_normalization_stats(tasks)
    x, y = tasks[0]
    rs = np.random.RandomState(5)
    tx = rs.uniform(-5, 5, size=(30, d))
    ty = rs.normal(size=(30, 1)) * 0.3 + 5
    cx, cy = O.prepare_task(x, y, stats, torch.float64)
    txn = torch.from_numpy(O.normalize(tx, stats)).float().double()
    m_c, z_c, ls, noise = O.vectorized_gp_features(theta, cx, cfg)
    m_t, z_t, _, _ = O.vectorized_gp_features(theta, txn, cfg)
    mean_n, cov_n = O.gp_predict(z_c, m_c, cy.unsqueeze(0).expand(P, -1), z_t, m_t, ls, 1.0, noise)
    mu_o, sd_o = O.mixture_mean_std(mean_n, cov_n, stats[2], stats[3])
    mu, sd = model.predict(x, y, tx)
    assert relerr(mu, mu_o) < 1e-3 and relerr(sd, sd_o) < 1e-3
    ll, rmse, calib = model.eval(x, y, tx, ty)
    ll_o, rmse_o, calib_o = O.eval_metrics(mean_n, cov_n, ty, stats[2], stats[3])
    assert abs(ll - ll_o) < 1e-3 * max(1, abs(ll_o)) and abs(rmse - rmse_o) < 1e-3 and abs(calib - calib_o) < 0.04
    ucb, lcb = model.confidence_intervals(x, y, tx, confidence=0.9)
    assert bool((ucb > lcb).all()) and bool((ucb.numpy() > mu).all()) and bool((lcb.numpy() < mu).all())


def test_svgd_ragged_tasks(M):
    """tasks of different sizes in one meta-batch (harmonic-mean pre-factor, random_gp.py:209-212)"""
    rs = np.random.RandomState(0)
    sizes = [5, 12, 7, 5]
    tasks = [(rs.uniform(-5, 5, size=(s, 2)), rs.normal(size=(s, 1))) for s in sizes]
    model = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=3, mean_module='constant', covar_module='SE', random_seed=2)
    cfg = O.GPConfig(2, 'constant', 'SE')
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    pre = O.meta_pre_factor(sizes)
    lp, score = model._log_prob_and_score(model.particles, np.arange(4), pre)
    lp_o, score_o = O.meta_score(model.particles.cpu().double(), otasks, cfg, pm, ps, 0.01)
    assert relerr(lp, lp_o) < 1e-4 and relerr(score, score_o) < 1e-3


# ------------------------------------------------------------------------------------------ VI
def test_vi_elbo_and_grad_match_oracle(M):
    T, n, d, S = 5, 32, 2, 4
    tasks = tasks_nd(T, n, d)
    model = M.GPRegressionMetaLearnedVI(tasks, svi_batch_size=S, random_seed=9, lr=1e-2)
    cfg = O.GPConfig(d, 'NN', 'NN')
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    loc = model.loc.cpu().double().clone().requires_grad_(True)
    scale = model.scale.cpu().double().clone().requires_grad_(True)
    torch.manual_seed(77)
    eps = torch.normal(torch.zeros(S, cfg.D), torch.ones(S, cfg.D)).double()
    loss_o = O.vi_neg_elbo(loc, scale, eps, otasks, cfg, pm, ps, 0.01)
    loss_o.backward()
    torch.manual_seed(77)
    loss, grad = model.get_neg_elbo_and_grad(np.arange(T), O.meta_pre_factor([n] * T))
    assert abs(float(loss) - float(loss_o)) < 1e-4 * abs(float(loss_o))
    assert relerr(grad[0], loc.grad) < 1e-2 and relerr(grad[1], scale.grad) < 1e-2
    # a few optimisation steps run and reduce the loss
    l0 = model.meta_fit(n_iter=1, verbose=False)
    l1 = model.meta_fit(n_iter=60, verbose=False)
    assert np.isfinite(l1)
    mu, sd = model.predict(tasks[0][0], tasks[0][1], tasks[1][0], n_posterior_samples=20)
    assert mu.shape == (n,) and bool((sd > 0).all())
    mu_map, sd_map = model.predict(tasks[0][0], tasks[0][1], tasks[1][0], mode='MAP')
    assert mu_map.shape == (n,)


# ------------------------------------------------------------------------------------------ single task
def test_single_task_learner_reproduces_recorded_reference_log(M, golden_dir):
    """GPRegressionLearned cell of demo.ipynb (learn_mean / SE / constant, seed 30) on the HIP path"""
    with open(os.path.join(golden_dir, 'demo_log.json')) as f:
        gold = json.load(f)['single_task']['log']
    _, test = demo_data()
    xc, yc, xt, yt = test[0]
    gp = M.GPRegressionLearned(xc, yc, learning_mode='learn_mean', covar_module='SE', mean_module='constant', random_seed=30)
    logs = []
    for n_it in (1, 499, 500):
        loss = gp.fit(xt, yt, verbose=False, n_iter=n_it, log_period=10 ** 9)
        logs.append((loss,) + gp.eval(xt, yt))
    for got, ref in zip(logs, gold):
        for k in range(4):
            assert abs(got[k] - ref[k + 1]) < 1.5e-3, (got, ref)


@pytest.mark.parametrize('mode,covar,mean', [('both', 'NN', 'NN'), ('learn_kernel', 'SE', 'zero'), ('both', 'SE', 'constant'),
                                             ('vanilla', 'SE', 'constant')])
def test_single_task_learner_matches_oracle(M, mode, covar, mean):
    tasks = O.sinusoid_tasks_nd(2, 40, 2, seed0=77)
    (x, t), (vx, vt) = tasks[0], (tasks[0][0][:15] + 0.3, tasks[0][1][:15])
    kw = dict(learning_mode=mode, covar_module=covar, mean_module=mean, weight_decay=0.1, lr=5e-3, random_seed=12)
    gp = M.GPRegressionLearned(x, t, **kw)
    orc = O.SingleTaskOracle(x, t, **kw)
    log_o = orc.fit(vx, vt, log_period=20, n_iter=60)
    loss = gp.fit(vx, vt, verbose=False, log_period=20, n_iter=60)
    assert abs(loss - log_o[-1][1]) < 2e-3 * max(1.0, abs(log_o[-1][1]))
    ll, rmse, calib = gp.eval(vx, vt)
    assert abs(ll - log_o[-1][2]) < 5e-3 * max(1.0, abs(log_o[-1][2])) and abs(rmse - log_o[-1][3]) < 2e-3
    lay = gp.layout
    for name, ref in (('noise_raw', orc.raw_noise), ('lengthscale_raw', orc.raw_lengthscale), ('outputscale_raw', orc.raw_outputscale)):
        lo, hi = lay.slices[name]
        assert torch.allclose(gp.theta[0, lo:hi].cpu(), ref.detach().reshape(-1), atol=2e-4), name
    pm, ps = gp.predict(vx)
    mean_n, cov_n = orc.predict_single(vx)
    assert relerr(pm, mean_n * orc.stats[3][0] + orc.stats[2][0]) < 1e-3
    assert relerr(ps, torch.sqrt(torch.diagonal(cov_n)) * orc.stats[3][0]) < 2e-3
    ucb, lcb = gp.confidence_intervals(vx)
    assert bool((ucb > lcb).all())


def test_single_task_state_dict_round_trip(M):
    x, t = O.sinusoid_tasks_nd(1, 30, 1, seed0=5)[0]
    a = M.GPRegressionLearned(x, t, random_seed=3)
    a.fit(verbose=False, n_iter=20)
    b = M.GPRegressionLearned(x, t, random_seed=4)
    b.load_state_dict(a.state_dict())
    pa, pb = a.predict(x[:7]), b.predict(x[:7])
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    a.fit(verbose=False, n_iter=5); b.fit(verbose=False, n_iter=5)
    assert torch.equal(a.theta, b.theta)


def _toy_1d():
    """data of the reference's single-task tests (tests/test_GPR.py:12-33)"""
    np.random.seed(25)
    x = np.linspace(-2, 2, num=60)
    y_two = x * 0 + 2 + np.random.normal(scale=0.02, size=x.shape)
    return x, y_two, np.sin(4 * x)


def test_single_task_random_seed_consistency(M):
    """tests/test_GPR.py:26-39"""
    x, y_two, _ = _toy_1d()
    kw = dict(learning_mode='both', num_iter_fit=5, mean_module='NN', covar_module='NN')
    g1, g2, g3 = (M.GPRegressionLearned(x, y_two, random_seed=s, **kw) for s in (22, 22, 23))
    for g in (g1, g2, g3):
        g.fit(verbose=False)
    xt = np.linspace(-2.1, 2.1, num=80)
    p1, p2, p3 = g1.predict(xt), g2.predict(xt), g3.predict(xt)
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])
    assert not np.array_equal(p1[0], p3[0])


def test_single_task_mean_and_kernel_learning_help(M):
    """tests/test_GPR.py:67-84,113-143: a learned NN mean / NN kernel beats the vanilla GP on sin(4x)"""
    x, _, y_sin = _toy_1d()
    torch.manual_seed(22)
    vanilla = M.GPRegressionLearned(x, y_sin, learning_mode='vanilla', num_iter_fit=20, mean_module='constant', covar_module='SE')
    vanilla.fit(verbose=False)
    learn_mean = M.GPRegressionLearned(x, y_sin, learning_mode='learn_mean', num_iter_fit=100, mean_module='NN',
                                       covar_module='SE', mean_nn_layers=(16, 16))
    learn_mean.fit(verbose=False)
    ll_v, rmse_v, _ = vanilla.eval(x, y_sin)
    ll_m, rmse_m, _ = learn_mean.eval(x, y_sin)
    assert ll_m > ll_v and rmse_m < rmse_v
    for mode in ('learn_kernel', 'both'):
        base = M.GPRegressionLearned(x, y_sin, learning_mode='learn_kernel', num_iter_fit=1, mean_module='zero', covar_module='NN')
        base.fit(verbose=False)
        learned = M.GPRegressionLearned(x, y_sin, learning_mode=mode, num_iter_fit=500, mean_module='constant', covar_module='NN',
                                        kernel_nn_layers=(16, 16), mean_nn_layers=(16, 16))
        learned.fit(valid_x=x, valid_t=y_sin, verbose=False)
        ll_b, rmse_b, _ = base.eval(x, y_sin)
        ll_k, rmse_k, _ = learned.eval(x, y_sin)
        assert ll_k > ll_b and rmse_k < rmse_b


def test_svgd_imq_kernel_steps_match_oracle(M):
    """GPRegressionMetaLearnedSVGD(kernel='IMQ') (GPR_meta_svgd.py:176-177): three steps vs oracle phi + torch Adam"""
    T, P, n, d = 6, 5, 16, 2
    tasks = tasks_nd(T, n, d)
    model = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, random_seed=3, lr=1e-2, kernel='IMQ')
    cfg = O.GPConfig(d, 'NN', 'NN')
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    idx, pre = np.arange(T), O.meta_pre_factor([n] * T)
    X = model.particles.cpu().double().clone()
    opt = torch.optim.Adam([X], lr=1e-2)
    for _ in range(3):
        _, s = O.meta_score(X, otasks, cfg, pm, ps, 0.01)
        phi, _ = O.svgd_phi_imq_closed_form(X.detach(), s)
        X.grad = -phi
        opt.step()
        model.svgd_step(idx, pre)
    assert relerr(model.particles, X) < 2e-3
    model.meta_fit(verbose=False, n_iter=5)
    with pytest.raises(NotImplementedError):
        M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, kernel='laplace')


@pytest.mark.parametrize('opt', ['Adam', 'SGD'])
def test_svgd_imq_steps_run_from_the_step_feed_and_replay_bit_identically(M, opt, monkeypatch):
    """the IMQ particle kernel takes the RBF kernel's route through meta_fit since round 4: task draws and step scalars from the
    device-side feed, the launch sequence captured once and replayed -- the same bits as the launches issued one by one
    (PACOH_NO_GRAPH=1), ragged tasks (per-step pre-factor), decaying learning rate; and the trajectory of meta_fit against the
    oracle's closed-form phi (svgd.py:58-77) driven by the same task draws with torch's optimizers"""
    rs = np.random.RandomState(13)
    tasks = []
    for t in range(6):
        n = 9 + 2 * (t % 3)
        x = rs.uniform(-3, 3, size=(n, 2))
        tasks.append((x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(n, 1)))
    kw = dict(num_particles=6, task_batch_size=4, lr=5e-3, lr_decay=0.95, random_seed=3, kernel='IMQ', optimizer=opt,
              mean_nn_layers=(8, 8), kernel_nn_layers=(8, 8))
    monkeypatch.setenv('PACOH_NO_GRAPH', '1')
    m_e = M.GPRegressionMetaLearnedSVGD(tasks, **kw)
    theta0 = m_e.particles.cpu().double().clone()
    m_e.meta_fit(verbose=False, n_iter=7, log_period=3)
    assert m_e._graphs is None
    monkeypatch.delenv('PACOH_NO_GRAPH')
    monkeypatch.setenv('PACOH_GRAPH', '1')
    m_g = M.GPRegressionMetaLearnedSVGD(tasks, **kw)
    m_g.meta_fit(verbose=False, n_iter=7, log_period=3)
    assert m_g._graphs is not None and len(m_g._graphs) == 1
    assert bool(torch.isfinite(m_g.particles).all()) and torch.equal(m_e.particles, m_g.particles)
    assert m_e.opt_step == m_g.opt_step == 7 and m_g.last_bandwidth.shape == (m_g.particles.shape[1],)
    # oracle trajectory on the same draws (numpy stream of the learner's seed: GPR_meta_svgd.py:102)
    cfg = O.GPConfig(2, 'NN', 'NN', mean_nn_layers=(8, 8), kernel_nn_layers=(8, 8))
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    m_r = M.GPRegressionMetaLearnedSVGD(tasks, **kw)              # a third learner only to read the draws its stream produces
    X = theta0.clone()
    optim = torch.optim.Adam([X], lr=5e-3) if opt == 'Adam' else torch.optim.SGD([X], lr=5e-3)
    sched = torch.optim.lr_scheduler.StepLR(optim, 1000, gamma=0.95)
    for _ in range(7):
        idx = m_r.rds_numpy.randint(0, len(tasks), size=4)
        sel = [otasks[i] for i in idx]
        _, s = O.meta_score(X, sel, cfg, pm, ps, 0.01)          # (pre-factor from the batch's sizes: random_gp.py:209-212)
        phi, _ = O.svgd_phi_imq_closed_form(X.detach(), s)
        X.grad = -phi
        optim.step()
        sched.step()
    assert relerr(m_g.particles, X) < 2e-3


def test_task_draws_consume_the_numpy_stream_like_the_reference(M):
    """one randint call per iteration, nothing drawn ahead (GPR_meta_svgd.py:102): after n iterations and an explicit
    _sample_task_batch() the learner's RandomState(seed + 1) stands exactly n + 1 draws into its stream -- also for the global
    np.random stream of an unseeded learner, which anything the caller draws afterwards depends on (the round-4 prefetch,
    removed in round 5, left it four batches further along)"""
    tasks = tasks_nd(7, 12, 2)
    kw = dict(num_particles=4, task_batch_size=5, lr=1e-2, mean_nn_layers=(8, 8), kernel_nn_layers=(8, 8))
    m = M.GPRegressionMetaLearnedSVGD(tasks, random_seed=21, **kw)
    m.meta_fit(verbose=False, n_iter=6, log_period=4)
    ref = np.random.RandomState(21 + 1)
    for _ in range(6):
        ref.randint(0, 7, size=5)
    idx, _ = m._sample_task_batch()                              # the 7th draw of the stream
    assert np.array_equal(np.sort(idx), np.sort(ref.randint(0, 7, size=5)))
    m.meta_fit(verbose=False, n_iter=5, log_period=100)
    assert np.array_equal(m.rds_numpy.randint(0, 7, size=5), np.random.RandomState(22).randint(0, 7, size=(13, 5))[12]) and m.opt_step == 11
    for cls, extra in ((M.GPRegressionMetaLearnedSVGD, kw), (M.GPRegressionMetaLearned, dict(task_batch_size=5))):
        np.random.seed(77)
        mu = cls(tasks, random_seed=None, **extra)               # unseeded: draws from the process-wide numpy stream
        assert mu.rds_numpy is np.random
        np.random.seed(78)
        mu.meta_fit(verbose=False, n_iter=9, log_period=4)
        after = np.random.randint(0, 1000, size=4)
        np.random.seed(78)
        np.random.randint(0, 7, size=(9, 5))
        assert np.array_equal(after, np.random.randint(0, 1000, size=4))


def test_step_feed_upload_accepts_tensors_lists_and_callables(M):
    """engine.StepFeed.upload: the per-step payload as ONE tensor [k, ...] (any device, dtype, requires_grad), a list of k tensors, or
    a callable filling the pinned staging rows -- the same rows reach the device; select() hands them out in order"""
    from meta_learning_pacoh_amd import _lib as Lb
    from meta_learning_pacoh_amd.engine import StepFeed
    dev = torch.device('cuda')
    k, tb, S, D = 5, 3, 2, 7
    g = torch.Generator().manual_seed(0)
    payload = torch.randn(k, S, D, generator=g)
    idx = np.arange(k * tb).reshape(k, tb) % 4
    sc = [Lb.step_scalars(0.1 * (j + 1), 1e-3, j + 1) for j in range(k)]
    forms = {
        'cpu tensor': payload.clone(),
        'cuda tensor': payload.to(dev),
        'fp64 tensor that requires grad': payload.double().requires_grad_(True),
        'list of tensors': [payload[j].clone() for j in range(k)],
        'list of cuda tensors': [payload[j].to(dev) for j in range(k)],
        'callable': lambda j, out: out.copy_(payload[j]),
    }
    for name, aux in forms.items():
        feed = StepFeed(dev, torch.float32, tb, chunk=16, aux_shape=(S, D))
        feed.upload(idx, sc, aux)
        torch.cuda.synchronize()
        assert torch.equal(feed.aux_all[:k].cpu(), payload), name
        assert torch.equal(feed.idx_all[:k].cpu(), torch.from_numpy(idx)), name
        for j in range(k):
            feed.select()
            torch.cuda.synchronize()
            assert torch.equal(feed.aux.cpu(), payload[j]) and torch.equal(feed.idx.cpu(), torch.from_numpy(idx[j])), (name, j)
            assert abs(float(feed.sc[Lb.SC_SCORE_SCALE]) - 0.1 * (j + 1)) < 1e-6


def test_vi_full_covariance_steps_match_oracle(M):
    """GPRegressionMetaLearnedVI(cov_type='full') (random_gp.py:249-251): init stream and three Adam steps vs the oracle"""
    T, n, d, S = 4, 12, 2, 3
    tasks = tasks_nd(T, n, d)
    kw = dict(mean_module='constant', covar_module='NN', kernel_nn_layers=(4,))
    model = M.GPRegressionMetaLearnedVI(tasks, svi_batch_size=S, random_seed=9, lr=1e-2, cov_type='full', **kw)
    cfg = O.GPConfig(d, 'constant', 'NN', kernel_nn_layers=(4,))
    D = cfg.D
    torch.manual_seed(9)
    O.consume_vectorized_gp_init_rng(cfg)
    loc, tril = O.vi_full_init(D)
    assert torch.equal(model.loc.cpu(), loc) and torch.equal(model.scale.cpu(), tril)
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    loc, tril = loc.double().requires_grad_(True), tril.double().requires_grad_(True)
    opt = torch.optim.Adam([loc, tril], lr=1e-2)
    idx, pre = np.arange(T), O.meta_pre_factor([n] * T)
    for _ in range(3):
        rng = torch.get_rng_state()
        eps = torch.normal(torch.zeros(S, D), torch.ones(S, D)).double()
        torch.set_rng_state(rng)                                  # the model draws the same eps
        opt.zero_grad()
        theta, log_q = O.vi_full_sample(loc, tril, eps)
        lp = O.meta_log_prob(theta, otasks, cfg, pm, ps, 0.01)
        loss_o = -(lp - 0.01 * log_q).mean()
        loss_o.backward()
        opt.step()
        loss, grad = model.get_neg_elbo_and_grad(idx, pre)
        assert abs(float(loss) - float(loss_o)) < 1e-3 * max(1.0, abs(float(loss_o)))
        model.opt_step += 1
        M._lib.adam_step(model.posterior, grad, model.exp_avg, model.exp_avg_sq, 1e-2, model.opt_step)
    assert relerr(model.loc, loc) < 2e-3 and relerr(model.scale, tril) < 2e-3
    model.meta_fit(verbose=False, n_iter=3)
    x, y = tasks[0]
    mu, sd = model.predict(x, y, x[:5], n_posterior_samples=7)
    assert np.isfinite(mu).all() and (sd > 0).all()


# ------------------------------------------------------------------------------------------ large contexts (HBM-resident path)
def test_map_large_context_matches_oracle(M):
    """n_ctx = 200 > LDS-resident limit: meta_fit / predict / eval run through csrc/dense_gp.hip"""
    tasks = tasks_nd(3, 200, 2)
    kw = dict(weight_decay=0.1, num_iter_fit=8, task_batch_size=2, random_seed=5, lr_params=5e-3)
    model = M.GPRegressionMetaLearned(tasks, **kw)
    orc = O.MapOracle(tasks, **kw)
    model.meta_fit(verbose=False)
    orc.meta_fit(None, log_period=100)
    lay = model.layout
    for name, ref in (('noise_raw', orc.raw_noise), ('lengthscale_raw', orc.raw_lengthscale), ('outputscale_raw', orc.raw_outputscale)):
        lo, hi = lay.slices[name]
        assert torch.allclose(model.theta[0, lo:hi].cpu(), ref.detach().reshape(-1), atol=3e-4), name
    lo, hi = lay.slices['kernel_nn.fc_2.weight']
    assert relerr(model.theta[0, lo:hi], orc.kernel_net[1].weight.reshape(-1)) < 2e-3
    cx, cy = tasks[0]
    tx = tasks[1][0][:40]
    pm, ps = model.predict(cx, cy, tx)
    mean_n, cov_n = orc.predict_normalized(cx, cy, tx)
    assert relerr(pm, mean_n * orc.stats[3][0] + orc.stats[2][0]) < 2e-3
    assert relerr(ps, torch.sqrt(torch.diagonal(cov_n)) * orc.stats[3][0]) < 5e-3
    ll, rmse, calib = model.eval(cx, cy, tx, tasks[1][1][:40])
    ll_o, rmse_o, calib_o = orc.eval(cx, cy, tx, tasks[1][1][:40])
    assert abs(ll - ll_o) < 5e-3 * max(1, abs(ll_o)) and abs(rmse - rmse_o) < 2e-3


def test_svgd_large_context_score_matches_oracle(M):
    T, P, n, d = 3, 3, 160, 2
    tasks = tasks_nd(T, n, d)
    model = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, random_seed=3, lr=1e-2)
    cfg = O.GPConfig(d, 'NN', 'NN')
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    pre = O.meta_pre_factor([n] * T)
    lp, score = model._log_prob_and_score(model.particles, np.arange(T), pre)
    lp_o, score_o = O.meta_score(model.particles.cpu().double(), otasks, cfg, pm, ps, 0.01)
    assert relerr(lp, lp_o) < 1e-4 and relerr(score, score_o) < 1e-2
    model.meta_fit(verbose=False, n_iter=3)
    mu, sd = model.predict(tasks[0][0], tasks[0][1], tasks[1][0][:9])
    assert np.isfinite(mu).all() and (sd > 0).all()


def test_svgd_120_iterations_track_oracle_on_demo_data(M):
    """longer horizon: PACOH-SVGD on the demo sinusoid tasks (20 x 5 points, 10 particles, sampled task batches of 5) for 120
    iterations on the HIP path vs the oracle's SVGD loop (closed-form phi + torch Adam) fed the same task draws -- the particles
    stay close and the test-set metrics agree"""
    train, test = demo_data()
    P, B, iters, lr = 10, 5, 120, 3e-3
    model = M.GPRegressionMetaLearnedSVGD(train, num_particles=P, task_batch_size=B, lr=lr, random_seed=30)
    cfg = O.GPConfig(1, 'NN', 'NN')
    pm, ps = O.hyperprior_mean_std(cfg.layout, 0.5, 3.0)
    stats = O.compute_normalization_stats(train)
    otasks = [O.prepare_task(x, y, stats, torch.float64) for x, y in train]
    X = model.particles.cpu().double().clone()
    opt = torch.optim.Adam([X], lr=lr)
    rds = np.random.RandomState(31)                                 # the learner's task stream: RandomState(seed + 1)
    for _ in range(iters):
        idx = rds.randint(0, len(train), size=B)
        _, s = O.meta_score(X, [otasks[i] for i in idx], cfg, pm, ps, 0.01)
        phi, _ = O.svgd_phi_closed_form(X.detach(), s, None)
        X.grad = -phi
        opt.step()
    model.meta_fit(verbose=False, n_iter=iters)
    assert relerr(model.particles, X) < 2e-2
    # test-set metrics of the two particle sets through the same (HIP) predictive
    ll, rmse, calib = model.eval_datasets(test)
    model.particles.copy_(X.to(model.particles.dtype))
    ll_o, rmse_o, calib_o = model.eval_datasets(test)
    assert abs(ll - ll_o) < 0.03 and abs(rmse - rmse_o) < 0.02 and abs(calib - calib_o) < 0.03


def test_more_meta_train_tasks_help_and_meta_beats_single_task(M):
    """behaviours the reference asserts in tests/test_GPR.py:224-278: meta-learning on 10 tasks generalises better than on 2
    (test log-likelihood up, RMSE down), and beats GPs fitted per test task from the 5 context points alone"""
    rs = np.random.RandomState(23)
    train = [sample_data_nonstationary(rs, 5) for _ in range(10)]
    test = [sample_data_nonstationary(rs, 55) for _ in range(10)]
    test = [(x[:5], t[:5], x[5:], t[5:]) for x, t in test]
    res = {}
    for k in (2, 10):
        torch.manual_seed(40)
        m = M.GPRegressionMetaLearned(train[:k], learning_mode='both', mean_nn_layers=(16, 16), kernel_nn_layers=(16, 16),
                                      num_iter_fit=3000, covar_module='SE', mean_module='NN', weight_decay=0.0)
        m.meta_fit(valid_tuples=test, verbose=False)
        res[k] = m.eval_datasets(test)
    assert res[10][0] > res[2][0] and res[10][1] < res[2][1]

    torch.manual_seed(60)
    meta = M.GPRegressionMetaLearned(train, learning_mode='both', mean_nn_layers=(64, 64), covar_module='SE', mean_module='NN',
                                     weight_decay=0.0, num_iter_fit=1000)
    meta.meta_fit(valid_tuples=test, verbose=False)
    ll_meta = meta.eval_datasets(test)[0]
    ll_single = []
    for cx, cy, tx, ty in test:
        g = M.GPRegressionLearned(cx, cy, learning_mode='both', mean_nn_layers=(64, 64), covar_module='SE', mean_module='NN',
                                  weight_decay=0.0, num_iter_fit=1000)
        g.fit(valid_x=tx, valid_t=ty, verbose=False)
        ll_single.append(g.eval(tx, ty)[0])
    assert ll_meta > float(np.mean(ll_single))


def test_eval_datasets_batched_equals_per_task_eval(M):
    """eval_datasets (abstract.py:165-181) runs all equally shaped test tasks in one batched pass for MAP and SVGD: same numbers as
    the reference's loop over eval(), also with test tasks of mixed shapes and when the covariance budget forces several passes"""
    import meta_learning_pacoh_amd.abstract as A
    train, test = demo_data()
    env = O.SinusoidDataset(np.random.RandomState(3))
    odd = env.generate_meta_test_data(3, 8, 30) + env.generate_meta_test_data(2, 5, 30)
    mixed = test + odd
    models = [M.GPRegressionMetaLearned(train, num_iter_fit=30, random_seed=4),
              M.GPRegressionMetaLearned(train, num_iter_fit=30, mean_module='constant', covar_module='SE', random_seed=4),
              M.GPRegressionMetaLearnedSVGD(train, num_iter_fit=10, num_particles=6, random_seed=4)]
    for model in models:
        model.meta_fit(verbose=False)
        for tuples in (test, mixed):
            loop = np.array([model.eval(*t) for t in tuples]).mean(0)
            batched = np.array(model.eval_datasets(tuples))
            assert np.all(np.isfinite(batched))
            np.testing.assert_allclose(batched, loop, rtol=2e-5, atol=2e-6)
        budget, A.EVAL_COV_BYTES = A.EVAL_COV_BYTES, 7 * model._eval_params()[0].shape[0] * 50 * 50 * 4      # 7 tasks per pass
        try:
            np.testing.assert_allclose(np.array(model.eval_datasets(test)), np.array([model.eval(*t) for t in test]).mean(0),
                                       rtol=2e-5, atol=2e-6)
        finally:
            A.EVAL_COV_BYTES = budget
    # VI draws fresh posterior samples inside every predict(): the batched pass draws them per task in task order (same CPU stream)
    for cov_type, layers in (('diag', (32, 32)), ('full', (8,))):
        vi = M.GPRegressionMetaLearnedVI(train, num_iter_fit=5, svi_batch_size=3, cov_type=cov_type, mean_nn_layers=layers,
                                         kernel_nn_layers=layers, random_seed=4)
        vi.meta_fit(verbose=False)
        for kw in ({'n_posterior_samples': 7}, {'mode': 'MAP'}, {}):
            torch.manual_seed(9)
            loop = np.array([vi.eval(*t, **kw) for t in mixed]).mean(0)
            torch.manual_seed(9)
            batched = np.array(vi.eval_datasets(mixed, **kw))
            np.testing.assert_allclose(batched, loop, rtol=2e-5, atol=2e-6)


# ---- whole steps as hipGraphs: same launch sequence replayed -> bit-identical to issuing it eagerly ------------------------------

def _fit(M, kind, tasks, n_iter, **kw):
    if kind == 'svgd':
        m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=5, task_batch_size=4, lr=1e-2, lr_decay=0.9, random_seed=3, **kw)
        m.meta_fit(verbose=False, n_iter=n_iter, log_period=3)
        return m, m.particles
    if kind == 'vi':
        m = M.GPRegressionMetaLearnedVI(tasks, svi_batch_size=3, task_batch_size=4, lr=1e-2, random_seed=3, **kw)
        m.meta_fit(verbose=False, n_iter=n_iter, log_period=3)
        return m, m.posterior
    m = M.GPRegressionMetaLearned(tasks, task_batch_size=4, lr_params=1e-2, weight_decay=0.05, lr_decay=0.9, random_seed=3, **kw)
    m.meta_fit(verbose=False, n_iter=n_iter, log_period=3)
    return m, m.theta


@pytest.mark.parametrize('kind', ['svgd', 'vi', 'map'])
def test_step_graph_with_the_captured_rccl_all_reduce(M, kind, monkeypatch):
    """the multi-rank step as ONE hipGraph: PACOH_COMM=rccl puts the step's exchange -- pacoh_allreduce_sum on the compute stream, a
    world-size-1 RCCL communicator on this one-GPU box -- INSIDE the captured step (and the four-steps-per-replay graph); the
    communicator's own capture self-test must pass, and the replayed run must equal the run without any collective bit for bit"""
    monkeypatch.setenv('PACOH_MAP_PERSIST', '0')      # (the launch sequence is the subject here; test_gpu_map_persist.py covers the other paths)
    monkeypatch.setenv('PACOH_MAP_TASK_FUSED', '0')
    from meta_learning_pacoh_amd import parallel
    rs = np.random.RandomState(7)
    tasks = [(x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(12, 1)) for x in (rs.uniform(-3, 3, size=(12, 2)) for _ in range(6))]
    parallel.disable_direct_rccl()
    m_ref, ref = _fit(M, kind, tasks, 11)
    assert parallel._direct_comm() is None
    monkeypatch.setenv('PACOH_COMM', 'rccl')
    try:
        calls = []
        real = parallel.RcclComm.all_reduce_
        monkeypatch.setattr(parallel.RcclComm, 'all_reduce_', lambda self, buf: (calls.append(buf.numel()), real(self, buf))[1])
        m_c, got = _fit(M, kind, tasks, 11)
        comm = parallel._direct_comm()
        assert comm is not None and comm.world_size == 1 and comm.graph_ok and parallel.collective_in_graph()
        assert m_c._graphs is not None and len(m_c._graphs) == 1 and m_c._graph_many is not None
        # captured, not called per step: 3 self-test calls + (2 warm-ups + 1 capture) x (1 + 4 steps) = 18 Python-level calls for
        # 11 steps, every one of them on the learner's packed buffer
        assert len(calls) == 3 + 3 * 5 and set(calls[3:]) == {m_c._packed.numel()}
        assert bool(torch.isfinite(got).all()) and torch.equal(ref, got)
    finally:
        monkeypatch.delenv('PACOH_COMM')
        parallel.disable_direct_rccl()


@pytest.mark.parametrize('layers', [(32, 32), (32, 32, 32, 32), (128, 128, 128, 128)])
@pytest.mark.parametrize('kind', ['svgd', 'vi', 'map'])
def test_graph_replay_is_bit_identical_to_eager_launches(M, kind, layers, monkeypatch):
    """meta_fit replays captured step graphs; PACOH_NO_GRAPH=1 issues the same launches one by one: identical bits, also for the
    launchers' 4 x 32 / 4 x 128 networks, ragged tasks (per-step pre-factor from the device scalars) and a decaying learning rate"""
    monkeypatch.setenv('PACOH_MAP_PERSIST', '0')      # (the launch sequence is the subject here; test_gpu_map_persist.py covers the other paths)
    monkeypatch.setenv('PACOH_MAP_TASK_FUSED', '0')
    if kind != 'map' and layers[0] == 128:
        pytest.skip('4 x 128 is the PACOH-MAP launcher configuration')
    rs = np.random.RandomState(7)
    tasks = []
    for t in range(6):
        n = 9 + 2 * (t % 3)                                   # ragged: 9, 11, 13 points
        x = rs.uniform(-3, 3, size=(n, 2))
        tasks.append((x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(n, 1)))
    kw = dict(mean_nn_layers=layers, kernel_nn_layers=layers)
    monkeypatch.setenv('PACOH_NO_GRAPH', '1')
    m_e, eager = _fit(M, kind, tasks, 8, **kw)
    assert m_e._graphs is None
    monkeypatch.delenv('PACOH_NO_GRAPH')
    m_g, graphed = _fit(M, kind, tasks, 8, **kw)
    assert m_g._graphs is not None and len(m_g._graphs) == 1
    assert bool(torch.isfinite(graphed).all()) and torch.equal(eager, graphed)
    assert m_e.opt_step == m_g.opt_step == 8 and m_e.lr_scheduler.epoch == 8


@pytest.mark.parametrize('cfg', [
    dict(),                                                                         # two fused 2 x 32 networks: tail of the forward launch
    dict(mean_nn_layers=(32, 32, 32, 32), kernel_nn_layers=(32, 32, 32, 32)),
    dict(mean_nn_layers=(16, 16), kernel_nn_layers=(16, 16)),                       # general MLP path: distance launch behind it
    dict(mean_module='constant', covar_module='SE'),                                # no network at all
    dict(mean_module='constant', covar_module='NN', feature_dim=3),                  # one network
    dict(optimizer='SGD', bandwidth=0.7),
    dict(num_particles=70),                                                         # median of > 64 particles: its own launch stays
    # the bandwidth block riding in the fused MLP backward at the register sort's 8, 16 and 32 values per lane (24 .. 32, 33 .. 45,
    # 46 .. 64 particles; 50 is the reference sweeps' larger count)
    dict(num_particles=24), dict(num_particles=40), dict(num_particles=50), dict(num_particles=64),
])
@pytest.mark.parametrize('graph', ['0', '1'])
def test_pipelined_svgd_step_equals_the_step_begin_sequence(M, cfg, graph, monkeypatch):
    """csrc/step_tail.h: distance matrix in the forward launch, hyper-parameter transforms by the update's own threads, next step's
    scalars and task batch fetched by the update launch -- the same bits as the six-launch sequence with pacoh_step_begin
    (PACOH_SVGD_PIPELINE=0), eager and replayed, ragged tasks, decaying learning rate, chunks of 1 + 2 + 3 + ... steps"""
    rs = np.random.RandomState(11)
    tasks = []
    for t in range(7):
        n = 9 + 2 * (t % 3)
        x = rs.uniform(-3, 3, size=(n, 2))
        tasks.append((x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(n, 1)))
    monkeypatch.setenv('PACOH_GRAPH', graph)
    kw = dict(num_particles=5, task_batch_size=4, lr=1e-2, lr_decay=0.9, random_seed=3)
    kw.update(cfg)
    out = []
    for pipe in ('0', '1'):
        monkeypatch.setenv('PACOH_SVGD_PIPELINE', pipe)
        m = M.GPRegressionMetaLearnedSVGD(tasks, **kw)
        m.meta_fit(verbose=False, n_iter=13, log_period=3)
        assert m._pipelined == (pipe == '1') and m.opt_step == 13
        m.svgd_step(np.array([1, 5, 2]), 0.25)                     # explicit draw, other batch size: a fresh feed
        out.append((m.particles.clone(), m.exp_avg.clone(), float(m.last_bandwidth)))
    assert bool(torch.isfinite(out[1][0]).all())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


@pytest.mark.parametrize('kind', ['svgd', 'vi'])
def test_small_first_chunk_does_not_change_the_run(M, kind, monkeypatch):
    """engine.first_chunk: a training call with many steps to issue starts with a chunk of 16 (the GPU gets work while the host
    prepares the rest); the task draws, PACOH-VI's noise and the schedule are consumed in the same order either way: same bits"""
    from meta_learning_pacoh_amd import engine
    rs = np.random.RandomState(5)
    tasks = [(x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(10, 1)) for x in (rs.uniform(-3, 3, size=(10, 2)) for _ in range(6))]
    out = []
    for first in (16, 10 ** 9):
        monkeypatch.setattr(engine, 'FIRST_CHUNK', first)
        sizes = []
        real = engine.StepFeed.upload
        monkeypatch.setattr(engine.StepFeed, 'upload', lambda self, idx, sc, aux=None: (sizes.append(len(sc)), real(self, idx, sc, aux))[1])
        m, res = _fit(M, kind, tasks, 80)                       # log_period 3 ... chunks of <= 3 steps
        m._train_steps(90)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine.StepFeed, 'upload', real)
        # PACOH-SVGD: 16, then the rest; PACOH-VI grows by half (its chunks cost the host 0.15 ms of noise per step)
        ramp = [16, 74] if kind == 'svgd' else [16, 24, 36, 14]
        assert (sizes[-len(ramp):] == ramp) if first == 16 else sizes[-1] == 90
        out.append((m.particles if kind == 'svgd' else m.posterior).clone())
    assert bool(torch.isfinite(out[0]).all()) and torch.equal(out[0], out[1])


@pytest.mark.parametrize('cfg', [
    dict(),                                                                         # two fused networks: slab reduction + tail
    dict(covar_module='SE', mean_module='NN'),                                      # one network (BASELINE config #2)
    dict(covar_module='NN', mean_module='constant', feature_dim=3),
    dict(covar_module='SE', mean_module='constant'),                                # no network: pacoh_hyper_bwd alone
    dict(mean_nn_layers=(16, 16), kernel_nn_layers=(16, 16)),                       # general MLP path: AdamW launches behind the gradient
    dict(learning_mode='learn_mean', covar_module='SE'), dict(learning_mode='learn_kernel', mean_module='constant'),   # trained column ranges
    dict(mean_nn_layers=(32, 32, 32, 32), kernel_nn_layers=(32, 32, 32, 32), weight_decay=0.0),
    dict(mean_nn_layers=(32, 32), kernel_nn_layers=(16,)),                         # two shapes: no single call finishes every entry
])
@pytest.mark.parametrize('graph', ['0', '1'])
def test_map_adam_folded_into_the_gradient_epilogue(M, cfg, graph, monkeypatch):
    """pacoh_adam_inline: the AdamW step applied by the threads that finish a gradient entry (slab reduction, hyper-parameter
    reduction) -- the same bits as the separate pacoh_adam_step_dev launch (PACOH_MAP_ADAM_INLINE=0): parameters, optimizer state,
    logged loss; weight decay on every group, decaying learning rate, ragged tasks, eager and replayed"""
    monkeypatch.setenv('PACOH_MAP_PERSIST', '0')      # (the launch sequence is the subject here; test_gpu_map_persist.py covers the other paths)
    monkeypatch.setenv('PACOH_MAP_TASK_FUSED', '0')
    rs = np.random.RandomState(13)
    tasks = []
    for t in range(7):
        n = 8 + 2 * (t % 3)
        x = rs.uniform(-3, 3, size=(n, 2))
        tasks.append((x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(n, 1)))
    monkeypatch.setenv('PACOH_GRAPH', graph)
    kw = dict(task_batch_size=4, lr_params=1e-2, weight_decay=0.05, lr_decay=0.9, random_seed=3)
    kw.update(cfg)
    out = []
    for inline in ('0', '1'):
        monkeypatch.setenv('PACOH_MAP_ADAM_INLINE', inline)
        m = M.GPRegressionMetaLearned(tasks, **kw)
        loss = m.meta_fit(verbose=False, n_iter=14, log_period=4)
        two_shapes = 'kernel_nn_layers' in cfg and cfg['kernel_nn_layers'] != cfg['mean_nn_layers']
        assert m._adam_inline() == (inline == '1' and not two_shapes) and m.opt_step == 14
        out.append((m.theta.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone(), float(loss)))
    assert bool(torch.isfinite(out[1][0]).all())
    assert all(torch.equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


@pytest.mark.parametrize('cfg', [
    dict(),                                                                         # two fused networks
    dict(covar_module='SE', mean_module='NN'),                                      # one network (BASELINE config #2)
    dict(covar_module='NN', mean_module='constant', feature_dim=2),
    dict(learning_mode='learn_mean', covar_module='SE'),
    dict(mean_nn_layers=(32, 32, 32, 32), kernel_nn_layers=(32, 32, 32, 32)),
    dict(mean_nn_layers=(16, 16), kernel_nn_layers=(16, 16)),
    dict(mean_nn_layers=(64, 64), kernel_nn_layers=(64, 64)),                       # not on the fused kernels: stays with step_begin
    dict(covar_module='NN', mean_module='constant', feature_dim=3),                 # (three outputs: neither)
])
@pytest.mark.parametrize('graph', ['0', '1'])
def test_map_iteration_in_four_launches_equals_the_step_begin_sequence(M, cfg, graph, monkeypatch):
    """pacoh_step_next: the gradient epilogue of a PACOH-MAP iteration (with the AdamW step in it) also fetches the next iteration's
    scalars and task batch and publishes the updated hyper-parameters' transforms; the backward launch advances the feed -- the same
    bits as with the step_begin launch (PACOH_MAP_PIPELINE=0), eager and replayed, ragged tasks, chunks of 1 + 3 + 4 + ... steps"""
    monkeypatch.setenv('PACOH_MAP_PERSIST', '0')      # (the launch sequence is the subject here; test_gpu_map_persist.py covers the other paths)
    monkeypatch.setenv('PACOH_MAP_TASK_FUSED', '0')
    rs = np.random.RandomState(17)
    tasks = []
    for t in range(7):
        n = 8 + 2 * (t % 3)
        x = rs.uniform(-3, 3, size=(n, 2))
        tasks.append((x, np.sin(x[:, :1]) + 0.3 * x[:, 1:] + 0.05 * rs.randn(n, 1)))
    monkeypatch.setenv('PACOH_GRAPH', graph)
    kw = dict(task_batch_size=4, lr_params=1e-2, weight_decay=0.05, lr_decay=0.9, random_seed=3)
    kw.update(cfg)
    out = []
    for pipe in ('0', '1'):
        monkeypatch.setenv('PACOH_MAP_PIPELINE', pipe)
        m = M.GPRegressionMetaLearned(tasks, **kw)
        loss = m.meta_fit(verbose=False, n_iter=14, log_period=4)
        fused = cfg.get('mean_nn_layers', (32, 32))[0] <= 32 and cfg.get('feature_dim', 2) <= 2
        assert m._pipelined == (pipe == '1' and fused) and m.opt_step == 14
        mean, std = m.predict(*tasks[0], tasks[1][0])
        out.append((m.theta.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone(), float(loss), mean, std))
    assert bool(torch.isfinite(out[1][0]).all())
    assert all(torch.equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]
    assert np.array_equal(out[0][4], out[1][4]) and np.array_equal(out[0][5], out[1][5])


@pytest.mark.parametrize('seed', range(8))
def test_pipelined_steps_on_random_shapes(M, seed, monkeypatch):
    """the pipelined SVGD / PACOH-MAP steps against their launch sequences on random shapes: 1-70 particles (64 / 65: register sort
    vs bisection median), 1-6 tasks per step, 3-20 points, one or two input dimensions, ragged or not, 1-3 hidden layers"""
    monkeypatch.setenv('PACOH_MAP_PERSIST', '0')      # (the launch sequence is the subject here; test_gpu_map_persist.py covers the other paths)
    monkeypatch.setenv('PACOH_MAP_TASK_FUSED', '0')
    rs = np.random.RandomState(100 + seed)
    d = int(rs.randint(1, 3))
    ragged = bool(rs.randint(0, 2))
    n_tasks = int(rs.randint(2, 8))
    tasks = []
    for t in range(n_tasks):
        n = int(rs.randint(3, 21)) if ragged or t == 0 else tasks[0][0].shape[0]
        x = rs.uniform(-3, 3, size=(n, d))
        tasks.append((x, np.sin(x[:, :1]) + 0.05 * rs.randn(n, 1)))
    layers = tuple([32] * int(rs.randint(1, 4)))
    tb = int(rs.randint(1, 7))
    P = int([1, 2, 5, 20, 64, 65, 70, 3][seed])
    monkeypatch.setenv('PACOH_GRAPH', str(seed % 2))
    out = []
    for pipe in ('0', '1'):
        monkeypatch.setenv('PACOH_SVGD_PIPELINE', pipe)
        monkeypatch.setenv('PACOH_MAP_PIPELINE', pipe)
        m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, task_batch_size=tb, lr=5e-3, lr_decay=0.95, mean_nn_layers=layers,
                                          kernel_nn_layers=layers, random_seed=seed)
        m.meta_fit(verbose=False, n_iter=9, log_period=4)
        mm = M.GPRegressionMetaLearned(tasks, task_batch_size=tb, lr_params=5e-3, weight_decay=0.01, mean_nn_layers=layers,
                                       kernel_nn_layers=layers, random_seed=seed)
        mm.meta_fit(verbose=False, n_iter=9, log_period=4)
        assert m._pipelined == (pipe == '1') and mm._pipelined == (pipe == '1')
        out.append((m.particles.clone(), mm.theta.clone()))
    assert bool(torch.isfinite(out[1][0]).all()) and bool(torch.isfinite(out[1][1]).all())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_launcher_networks_run_through_the_learners(M):
    """experiments/meta_GPR_SVGD_base_exp.py:29-30,83 (4 x 32, 10 particles, bandwidth 0.1, prior_factor 0.1, 2 tasks per step) and
    experiments/meta_GPR_mll_base_exp.py:29-30 (4 x 128, 2 tasks x 5 points per step): construct, train a few steps, predict; the
    SVGD likelihood score is checked against the oracle"""
    tasks = O.sinusoid_tasks_nd(20, 20, 1, seed0=40)
    layers = (32, 32, 32, 32)
    m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=10, task_batch_size=2, lr=1e-3, lr_decay=0.98, bandwidth=0.1,
                                      prior_factor=0.1, weight_prior_std=0.5, mean_nn_layers=layers, kernel_nn_layers=layers,
                                      random_seed=28)
    idx = np.array([3, 11])
    pre = O.meta_pre_factor([20, 20])
    _, score = m._log_prob_and_score(m.particles, idx, pre, with_prior=False)
    cfg = O.GPConfig(1, 'NN', 'NN', mean_nn_layers=layers, kernel_nn_layers=layers)
    stats = O.compute_normalization_stats(tasks)
    otasks = [O.prepare_task(*tasks[i], stats, torch.float64) for i in idx]
    th = m.particles.detach().cpu().double().requires_grad_(True)
    lik = pre * torch.stack([O.vectorized_gp_mll(th, *ot, cfg) for ot in otasks], -1).sum(-1)
    (ref,) = torch.autograd.grad(lik.sum(), th)
    assert float((score.cpu().double() - ref).norm() / ref.norm()) < 2e-3
    m.meta_fit(verbose=False, n_iter=20, log_period=10)
    mean, std = m.predict(*tasks[0], tasks[1][0])
    assert np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()
    tasks5 = O.sinusoid_tasks_nd(20, 5, 1, seed0=41)
    layers = (128, 128, 128, 128)
    mm = M.GPRegressionMetaLearned(tasks5, task_batch_size=2, lr_params=1e-3, lr_decay=0.98, mean_nn_layers=layers,
                                   kernel_nn_layers=layers, random_seed=28)
    l0 = mm.meta_fit(verbose=False, n_iter=1)
    mm.meta_fit(verbose=False, n_iter=150, log_period=50)
    mean, std = mm.predict(*tasks5[0], tasks5[1][0])
    assert np.isfinite(l0) and np.isfinite(mean).all() and (std > 0).all()


def test_failed_cholesky_raises_like_the_reference(M):
    """NaN parameters make every jittered Cholesky fail (info = -1); gpytorch raises NotPSDError inside the loss evaluation, the
    learners raise at their next synchronisation point instead of training on NaNs silently"""
    from meta_learning_pacoh_amd.engine import NotPSDError
    tasks = O.sinusoid_tasks_nd(5, 8, 1, seed0=50)
    m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=3, task_batch_size=3, random_seed=1)
    m.particles[1, m.layout.slices['lengthscale_raw'][0]] = float('nan')
    with pytest.raises(NotPSDError):
        m.meta_fit(verbose=False, n_iter=2)
    mm = M.GPRegressionMetaLearned(tasks, task_batch_size=3, random_seed=1)
    mm.theta[0, mm.layout.slices['noise_raw'][0]] = float('nan')
    with pytest.raises(NotPSDError):
        mm.meta_fit(verbose=False, n_iter=2)


def test_module_objects_run_like_their_string_options(M):
    """GPRegressionMetaLearned(mean_module=ConstantMean(), covar_module=ScaleKernel(RBFKernel())) (objects, as the reference accepts
    them: GPR_meta_mll.py:207-251) trains exactly like mean_module='constant', covar_module='SE' when the objects carry the default
    raw values, starts from their values otherwise, and an unsupported kernel object is refused"""
    class ConstantMean:
        def __init__(self, c=0.0):
            self.constant = torch.nn.Parameter(torch.tensor([c]))

    class RBFKernel:
        def __init__(self, d, raw=0.0):
            self.raw_lengthscale = torch.nn.Parameter(torch.full((1, d), raw))

    class ScaleKernel:
        def __init__(self, base, raw=0.0):
            self.base_kernel, self.raw_outputscale = base, torch.nn.Parameter(torch.tensor(raw))

    class MaternKernel:
        pass

    tasks = O.sinusoid_tasks_nd(8, 12, 2, seed0=70)
    a = M.GPRegressionMetaLearned(tasks, mean_module='constant', covar_module='SE', task_batch_size=4, random_seed=9)
    b = M.GPRegressionMetaLearned(tasks, mean_module=ConstantMean(), covar_module=ScaleKernel(RBFKernel(2)), task_batch_size=4, random_seed=9)
    a.meta_fit(verbose=False, n_iter=6)
    b.meta_fit(verbose=False, n_iter=6)
    assert torch.equal(a.theta, b.theta)
    c = M.GPRegressionMetaLearned(tasks, mean_module=ConstantMean(0.3), covar_module=ScaleKernel(RBFKernel(2, 0.5), -0.2), task_batch_size=4,
                                  random_seed=9)
    lay = c.layout
    assert abs(float(c.theta[0, lay.slices['constant_mean'][0]]) - 0.3) < 1e-7
    assert abs(float(c.theta[0, lay.slices['outputscale_raw'][0]]) + 0.2) < 1e-7
    assert torch.allclose(c.theta[0, lay.slices['lengthscale_raw'][0]:lay.slices['lengthscale_raw'][1]].cpu(), torch.full((2,), 0.5))
    with pytest.raises(NotImplementedError):
        M.GPRegressionMetaLearned(tasks, mean_module='constant', covar_module=MaternKernel())


class _CosineKernel:
    """stand-in for gpytorch.kernels.CosineKernel (recognised by class name, modules.py): one raw period_length, softplus-constrained"""

    def __init__(self, raw=0.0):
        self.raw_period_length = torch.nn.Parameter(torch.full((1, 1), raw))


_CosineKernel.__name__ = 'CosineKernel'


def test_cosine_kernel_object_single_task_learner_matches_oracle_and_learns(M):
    """the reference's tests/test_GPR.py:95-120 (test_kernel_learning_COS): GPRegressionLearned(covar_module=CosineKernel()) -- (a) the
    first iterations against the oracle's restatement with the same kernel, (b) the behaviour the reference asserts: learning the
    period beats the vanilla model on sinusoidal targets"""
    rs = np.random.RandomState(22)
    x = rs.uniform(-2, 2, size=(40, 1))
    y = np.sin(3.0 * x) + 0.05 * rs.randn(40, 1)
    kw = dict(mean_module='constant', num_iter_fit=1)
    m = M.GPRegressionLearned(x, y, learning_mode='learn_kernel', covar_module=_CosineKernel(), lr=1e-2, random_seed=4, **kw)
    o = O.SingleTaskOracle(x, y, learning_mode='learn_kernel', covar_module='COS', lr=1e-2, random_seed=4, dtype=torch.float64, **kw)
    assert m.layout.D == 4 and m.layout.blocks['lengthscale_raw'] == 1              # constant | period | outputscale | noise
    # a plain CosineKernel has no learnable output scale: pin the oracle's at softplus^-1(1) and keep it out of the comparison
    with torch.no_grad():
        o.raw_outputscale.fill_(float(np.log(np.e - 1.0)))
    o.raw_outputscale.requires_grad_(False)
    losses = []
    for _ in range(6):
        losses.append(m.fit(verbose=False, n_iter=1))
    ref = [rec[1] for rec in o.fit(n_iter=6, log_period=1)]
    assert abs(losses[0] - ref[0]) < 2e-4 * max(1.0, abs(ref[0]))
    lo = m.layout.slices['lengthscale_raw'][0]
    assert abs(float(m.theta[0, lo]) - float(o.raw_lengthscale.reshape(-1)[0])) < 2e-3          # six AdamW steps of 1e-2 each
    # (b) tests/test_GPR.py:95-120
    vanilla = M.GPRegressionLearned(x, y, learning_mode='vanilla', num_iter_fit=1, mean_module='constant', covar_module=_CosineKernel(),
                                    random_seed=4)
    vanilla.fit(verbose=False)
    learned = M.GPRegressionLearned(x, y, learning_mode='learn_kernel', num_iter_fit=500, mean_module='constant',
                                    covar_module=_CosineKernel(), random_seed=4)
    learned.fit(valid_x=x, valid_t=y, verbose=False)
    ll_v, rmse_v, _ = vanilla.eval(x, y)
    ll_k, rmse_k, _ = learned.eval(x, y)
    assert ll_k > ll_v and rmse_k < rmse_v


def test_cosine_kernel_object_meta_learner_ties_the_period_over_input_dimensions(M):
    """GPRegressionMetaLearned(covar_module=ScaleKernel(CosineKernel())) on 2-d inputs: ONE period parameter, the device sees it
    replicated over both dimensions and hands back their summed gradient; first iterations vs the oracle, graph replay included"""
    class ScaleKernel:
        def __init__(self, base, raw=0.0):
            self.base_kernel, self.raw_outputscale = base, torch.nn.Parameter(torch.tensor(raw))

    rs = np.random.RandomState(3)
    tasks = []
    for _ in range(6):
        x = rs.uniform(-1, 1, size=(9, 2))
        tasks.append((x, np.sin(2 * x[:, :1]) + 0.1 * rs.randn(9, 1)))
    # (cos(pi |x - x'| / p) is positive semi-definite in one dimension only: in two the output scale is kept small against the noise,
    #  |lambda_min(os K)| <= os n = 0.44 < 0.69)
    m = M.GPRegressionMetaLearned(tasks, mean_module='constant', covar_module=ScaleKernel(_CosineKernel(0.3), -3.0), task_batch_size=6,
                                  lr_params=5e-3, random_seed=2)
    assert m.layout.blocks['lengthscale_raw'] == 1 and m.layout.feature_dim == 2
    o = O.MapOracle(tasks, mean_module='constant', covar_module='COS', task_batch_size=6, lr_params=5e-3, random_seed=2, dtype=torch.float64)
    with torch.no_grad():
        o.raw_lengthscale.fill_(0.3)
        o.raw_outputscale.fill_(-3.0)
    m.meta_fit(verbose=False, n_iter=5)
    o.meta_fit(n_iter=5)
    lay = m.layout
    got = m.theta[0].cpu().double()
    assert abs(float(got[lay.slices['lengthscale_raw'][0]]) - float(o.raw_lengthscale.reshape(-1)[0])) < 5e-4
    assert abs(float(got[lay.slices['outputscale_raw'][0]]) - float(o.raw_outputscale)) < 5e-4
    assert abs(float(got[lay.slices['noise_raw'][0]]) - float(o.raw_noise.reshape(-1)[0])) < 5e-4
    mean, std = m.predict(*tasks[0], tasks[1][0])
    assert np.isfinite(mean).all() and (std > 0).all()


def test_svgd_with_more_than_64_particles(M, monkeypatch):
    """80 particles (the reference has no limit): graph replay == eager launches, bandwidth == numpy.median heuristic on the final
    particles' predecessor, finite predictions"""
    tasks = O.sinusoid_tasks_nd(6, 12, 1, seed0=50)
    runs = []
    for no_graph in ('0', '1'):
        monkeypatch.setenv('PACOH_NO_GRAPH', no_graph)
        monkeypatch.setenv('PACOH_GRAPH', '1')
        m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=80, task_batch_size=3, lr=1e-2, mean_nn_layers=(8, 8),
                                          kernel_nn_layers=(8, 8), random_seed=5)
        before = m.particles.clone()
        m.meta_fit(verbose=False, n_iter=1)
        _, bw_o = O.svgd_phi_closed_form(before.cpu().double(), torch.zeros_like(before).cpu().double(), None)
        assert abs(float(m.last_bandwidth) - float(bw_o)) < 1e-5 * float(bw_o)
        m.meta_fit(verbose=False, n_iter=11, log_period=4)
        runs.append(m.particles.clone())
        mean, std = m.predict(*tasks[0], tasks[1][0])
        assert np.isfinite(mean).all() and (std > 0).all()
    assert torch.equal(runs[0], runs[1])
    # the IMQ particle kernel takes the same particle counts since round 3 (its pair table used to cap it at 64): three steps of an
    # 80-particle learner against the oracle's closed form on the same score
    m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=80, kernel='IMQ', task_batch_size=3, lr=1e-2, mean_nn_layers=(8, 8),
                                      kernel_nn_layers=(8, 8), random_seed=5)
    theta0 = m.particles.clone()
    idx, pre = m._sample_task_batch()
    _, score = m._log_prob_and_score(theta0, idx, pre)
    from meta_learning_pacoh_amd import _lib as Lb
    phi, _, _ = Lb.svgd_phi_imq(theta0, score)
    phi_o, _ = O.svgd_phi_imq_closed_form(theta0.cpu().double(), score.cpu().double())
    assert float((phi.cpu().double() - phi_o).norm() / phi_o.norm()) < 1e-4
    m.meta_fit(verbose=False, n_iter=3)
    assert bool(torch.isfinite(m.particles).all()) and not torch.equal(m.particles, theta0)
    with pytest.raises(AssertionError):
        M.GPRegressionMetaLearnedSVGD(tasks, num_particles=1025, kernel='IMQ', random_seed=5)


def test_vi_fused_update_equals_the_launch_sequence_it_replaces(M, monkeypatch):
    """pacoh_vi_update_dev (pre-factor + hyper-prior score and density + ELBO value + reparameterisation gradient + Adam in one
    launch) against the seven launches it replaces, over a few steps of the same learner"""
    tasks = O.sinusoid_tasks_nd(8, 10, 1, seed0=60)
    out = []
    for unfused in ('1', '0'):
        monkeypatch.setenv('PACOH_VI_UNFUSED', unfused)
        monkeypatch.setenv('PACOH_GRAPH', '0')
        m = M.GPRegressionMetaLearnedVI(tasks, svi_batch_size=4, task_batch_size=3, lr=1e-2, lr_decay=0.9, mean_nn_layers=(8, 8),
                                        kernel_nn_layers=(8, 8), random_seed=9)
        loss = m.meta_fit(verbose=False, n_iter=7, log_period=3)
        out.append((m.posterior.clone(), float(loss)))
    assert float((out[0][0] - out[1][0]).abs().max()) < 2e-5 * float(out[0][0].abs().max())
    assert abs(out[0][1] - out[1][1]) < 1e-5 * abs(out[0][1])


@pytest.mark.parametrize('graph', ['0', '1'])
def test_vi_device_noise_changes_the_noise_source_and_nothing_else(M, graph, monkeypatch):
    """noise='device' (not in the reference: the reparameterisation noise from the device generator instead of torch's CPU stream,
    which bounds the step at the launchers' shape): the rows the device generator wrote, fed to a noise='host' learner through its
    own staging path, must give the same posterior bit for bit; the rows are standard normal; two seeded runs agree"""
    import meta_learning_pacoh_amd.GPR_meta_vi as V
    monkeypatch.setenv('PACOH_GRAPH', graph)
    tasks = O.sinusoid_tasks_nd(8, 10, 1, seed0=61)
    kw = dict(svi_batch_size=6, task_batch_size=3, lr=1e-2, lr_decay=0.9, mean_nn_layers=(16, 16), kernel_nn_layers=(16, 16), random_seed=11)

    def run_device(record):
        m = M.GPRegressionMetaLearnedVI(tasks, noise='device', **kw)
        m._setup_step(m._local_batch_size())
        feed_upload = m._feed.upload

        def spy(idx_rows, sc_rows, aux_rows=None):
            feed_upload(idx_rows, sc_rows, aux_rows)
            assert aux_rows == 'device'
            record.append(m._feed.aux_all[:len(sc_rows)].cpu().clone())
        m._feed.upload = spy
        loss = m.meta_fit(verbose=False, n_iter=41, log_period=20)
        del m._feed.upload                                                     # (the spy closes over m: no reference cycle left behind)
        return m.posterior.clone(), float(loss)

    rows, rows2 = [], []
    post_a, loss_a = run_device(rows)
    post_b, loss_b = run_device(rows2)
    assert torch.equal(post_a, post_b) and loss_a == loss_b                      # seeded: the device generator is seeded too
    assert np.isfinite(loss_a) and bool(torch.isfinite(post_a).all())
    eps = torch.cat([r.reshape(-1) for r in rows]).double()
    assert eps.numel() == 41 * 6 * post_a.shape[1]
    assert abs(float(eps.mean())) < 0.02 and abs(float(eps.std()) - 1.0) < 0.02
    assert abs(float((eps ** 3).mean())) < 0.05 and abs(float((eps ** 4).mean()) - 3.0) < 0.1

    # the same rows through the host path
    flat = [row for r in rows for row in r]                                       # one [S, D] row per step, in step order
    it = iter(flat)

    def replayed(n, D, out=None):
        row = next(it)
        assert row.shape == (n, D)
        if out is not None:
            out.copy_(row)
            return out
        return row.clone()
    monkeypatch.setattr(V, 'standard_normal', replayed)
    m = M.GPRegressionMetaLearnedVI(tasks, noise='host', **kw)
    loss_h = m.meta_fit(verbose=False, n_iter=41, log_period=20)
    assert torch.equal(m.posterior, post_a) and float(loss_h) == loss_a


def test_vi_device_noise_predict_and_eval(M):
    """predict / eval_datasets with noise='device': posterior samples from the device generator -- finite, calibrated like the
    host-noise learner's (same posterior, another sample of it)"""
    train, test = demo_data()
    out = []
    for noise in ('host', 'device'):
        m = M.GPRegressionMetaLearnedVI(train, noise=noise, svi_batch_size=5, task_batch_size=4, lr=5e-3, mean_nn_layers=(16, 16),
                                        kernel_nn_layers=(16, 16), random_seed=3, num_iter_fit=60)
        m.meta_fit(verbose=False, log_period=30)
        x_c, y_c, x_t, y_t = test[0]
        mu, std = m.predict(x_c, y_c, x_t, n_posterior_samples=40)
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(std)) and np.all(std > 0) and mu.shape == std.shape and mu.shape[0] == x_t.shape[0]
        ll, rmse, calib = m.eval_datasets(test, n_posterior_samples=40)
        assert np.isfinite(ll) and np.isfinite(rmse) and np.isfinite(calib)
        out.append((ll, rmse))
    assert abs(out[0][1] - out[1][1]) < 0.25 * max(out[0][1], out[1][1])         # same model class, 60 steps: the same ballpark


def test_graph_capture_survives_a_dead_reference_cycle_that_holds_graphs(M, monkeypatch):
    """A discarded learner caught in a reference cycle keeps its hipGraphs, events and pinned staging buffers until the garbage collector
    finds it -- at some allocation of its own choosing.  If that is inside another learner's stream capture the process aborts
    (destroying a graph inside a capture); torch.cuda.graph() does not collect before capturing any more.  engine.capture_graph
    collects first and keeps the collector off during the capture (util.gc_paused): with the collector set to run at every
    allocation this test ended the process before that."""
    import gc
    monkeypatch.setenv('PACOH_GRAPH', '1')
    tasks = O.sinusoid_tasks_nd(6, 10, 1, seed0=70)
    kw = dict(num_particles=3, task_batch_size=2, mean_nn_layers=(8, 8), kernel_nn_layers=(8, 8), random_seed=2)
    old = gc.get_threshold()
    gc.collect()
    gc.disable()
    try:
        m = M.GPRegressionMetaLearnedSVGD(tasks, **kw)
        m.meta_fit(verbose=False, n_iter=9, log_period=100)
        assert m._graphs is not None                                         # (it holds captured graphs)
        m._cycle = m                                                         # a cycle: only the collector can free it
        del m
        gc.set_threshold(1, 1, 1)                                            # the collector runs at (nearly) every allocation from here on
        gc.enable()
        m2 = M.GPRegressionMetaLearnedSVGD(tasks, **kw)
        m2.meta_fit(verbose=False, n_iter=9, log_period=100)
        assert bool(torch.isfinite(m2.particles).all()) and m2._graphs is not None
    finally:
        gc.set_threshold(*old)
        gc.enable()
