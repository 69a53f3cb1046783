"""Parity at BASELINE.json's FULL configuration sizes.  Where the CPU oracle finishes in seconds the whole
batch is compared; otherwise size-independent properties are used: additivity of the score over task
sub-batches, permutation invariance, fp32-vs-fp64 agreement, plus an oracle spot check of random problems."""
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


def test_cfg2_map_256_tasks_n32_d1_se_kernel_all_tasks_vs_oracle(M):
    env = O.SinusoidDataset(np.random.RandomState(27))
    train = env.generate_meta_train_data(256, 32)
    model = M.GPRegressionMetaLearned(train, covar_module='SE', mean_module='NN', task_batch_size=256, random_seed=5)
    orc = O.MapOracle(train, covar_module='SE', mean_module='NN', task_batch_size=256, random_seed=5)
    lml, grad, info = model.engine.lml_and_grad(model.theta, model.tasks, weight=-1.0)
    ref = torch.stack([orc.task_mll(x, y) for x, y in orc.tasks])
    assert int(info.abs().max()) == 0
    assert relerr(lml[:, 0], ref) < 1e-4
    (-ref.sum()).backward()
    lo, hi = model.layout.slices['mean_nn.fc_2.weight']
    # fp32 bar: 1e-2 norm-wise; asserted with the headroom the kernels actually have, so that a regression shows before the bar
    assert relerr(grad[0, lo:hi], orc.mean_net[1].weight.grad.reshape(-1)) < 2e-3
    lo, hi = model.layout.slices['lengthscale_raw']
    assert relerr(grad[0, lo:hi], orc.raw_lengthscale.grad.reshape(-1)) < 2e-3


def test_cfg3_svgd_1024_tasks_n64_d4_20_particles_properties(M):
    T, n, d, P = 1024, 64, 4, 20
    tasks = O.sinusoid_tasks_nd(T, n, d, seed0=1000)
    model = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=P, random_seed=0)
    th = model.particles
    full = model.tasks
    lml, grad, info = model.engine.lml_and_grad(th, full, weight=1.0)
    assert lml.shape == (T, P) and bool(torch.isfinite(lml).all()) and int(info.min()) >= 0
    # (a) additivity over task sub-batches (what the multi-GPU sharding relies on)
    parts = [model.tasks.select(torch.arange(q, T, 4, device=th.device)) for q in range(4)]
    g_sum = sum(model.engine.lml_and_grad(th, pb, weight=1.0)[1] for pb in parts)
    assert relerr(g_sum, grad) < 1e-4
    # (b) permutation invariance of the per-task values
    perm = torch.randperm(T, device=th.device)
    lml_p, _, _ = model.engine.lml_and_grad(th, model.tasks.select(perm), weight=1.0)
    assert float((lml_p - lml[perm]).abs().max()) == 0.0
    # (c) determinism: two evaluations are bit-identical
    lml2, grad2, _ = model.engine.lml_and_grad(th, full, weight=1.0)
    assert torch.equal(lml, lml2) and torch.equal(grad, grad2)
    # (d) oracle spot check of random (task, particle) pairs, fp64 oracle
    cfg = O.GPConfig(d, 'NN', 'NN')
    stats = O.compute_normalization_stats(tasks)
    rs = np.random.RandomState(0)
    for t in rs.randint(0, T, 6):
        x, y = O.prepare_task(*tasks[t], stats, torch.float64)
        ref = O.vectorized_gp_mll(th.cpu().double(), x, y, cfg)
        assert relerr(lml[t], ref) < 1e-3
    # (e) the full score [P, D] of a 64-task sub-batch vs oracle autograd in fp64: norm-wise over the whole array and per particle
    #     (bar 1e-2 in fp32; asserted at 2e-3 so that a regression shows before the bar is crossed)
    sub = list(range(0, 64))
    otasks = [O.prepare_task(*tasks[t], stats, torch.float64) for t in sub]
    thd = th.cpu().double().clone().requires_grad_(True)
    ref = torch.stack([O.vectorized_gp_mll(thd, x, y, cfg) for x, y in otasks], -1).sum()
    ref.backward()
    _, g64, _ = model.engine.lml_and_grad(th, model.tasks.select(torch.tensor(sub, device=th.device)), weight=1.0)
    assert g64.shape == (P, model.layout.D)
    assert relerr(g64, thd.grad) < 2e-3
    per_particle = [relerr(g64[q], thd.grad[q]) for q in range(P)]
    assert max(per_particle) < 5e-3, per_particle


def test_cfg4_vi_512_tasks_n128_10_samples(M):
    T, n, d, S = 512, 128, 1, 10
    env = O.SinusoidDataset(np.random.RandomState(28))
    tasks = env.generate_meta_train_data(T, n)
    model = M.GPRegressionMetaLearnedVI(tasks, svi_batch_size=S, random_seed=3)
    torch.manual_seed(1)
    theta, eps, _ = model._rsample(S)
    lml, grad, info = model.engine.lml_and_grad(theta, model.tasks, weight=1.0)
    assert lml.shape == (T, S) and bool(torch.isfinite(lml).all())
    halves = [model.tasks.select(torch.arange(q, T, 2, device=theta.device)) for q in range(2)]
    g_sum = sum(model.engine.lml_and_grad(theta, h, weight=1.0)[1] for h in halves)
    assert relerr(g_sum, grad) < 1e-4
    cfg = O.GPConfig(d, 'NN', 'NN')
    stats = O.compute_normalization_stats(tasks)
    for t in (0, 101, 511):
        x, y = O.prepare_task(*tasks[t], stats, torch.float64)
        ref = O.vectorized_gp_mll(theta.cpu().double(), x, y, cfg)
        assert relerr(lml[t], ref) < 2e-3
    # the full score [S, D] of a 16-task sub-batch at n = 128 vs oracle autograd in fp64 (bar 1e-2 in fp32; asserted at 2e-3)
    sub = list(range(7, 512, 32))
    assert len(sub) == 16
    otasks = [O.prepare_task(*tasks[t], stats, torch.float64) for t in sub]
    thd = theta.cpu().double().clone().requires_grad_(True)
    torch.stack([O.vectorized_gp_mll(thd, x, y, cfg) for x, y in otasks], -1).sum().backward()
    _, g16, _ = model.engine.lml_and_grad(theta, model.tasks.select(torch.tensor(sub, device=theta.device)), weight=1.0)
    assert g16.shape == (S, model.layout.D)
    assert relerr(g16, thd.grad) < 2e-3
    assert max(relerr(g16[q], thd.grad[q]) for q in range(S)) < 5e-3
    loss = model.meta_fit(n_iter=2, verbose=False)
    assert np.isfinite(loss)


def test_cfg5_large_context_256_tasks_n512_d8_fp64_all_tasks_vs_oracle(M):
    from meta_learning_pacoh_amd import _lib as L
    T, n, d = 256, 512, 8
    tasks = O.sinusoid_tasks_nd(T, n, d, seed0=5000)
    stats = O.compute_normalization_stats(tasks)
    xy = [O.prepare_task(x, y, stats, torch.float64) for x, y in tasks]
    X, Y = torch.stack([a for a, _ in xy]), torch.stack([b for _, b in xy])
    ls = torch.nn.functional.softplus(torch.zeros(1, d, dtype=torch.float64))
    noise = torch.nn.functional.softplus(torch.tensor([-1.0], dtype=torch.float64))
    K = L.gram_rbf_ard(X.cuda(), 1, X.cuda(), 1, ls.cuda(), None, noise.cuda(), True, T, 1)
    logp, alpha, info = L.mvn_logprob_dense(K, Y.cuda(), 1.0 / n, want_alpha=True)
    assert int(info.abs().max()) == 0
    torch.set_num_threads(max(1, torch.get_num_threads()))
    ref = O.gp_mll(X, torch.zeros(T, n, dtype=torch.float64), Y, ls.unsqueeze(0), 1.0, noise)
    assert float(((logp.cpu() - ref).abs() / ref.abs()).max()) < 1e-8          # bar: 1e-4 rel
    # K^-1 y round trip: (K + s2 I) alpha == y
    K2 = L.gram_rbf_ard(X.cuda(), 1, X.cuda(), 1, ls.cuda(), None, noise.cuda(), True, T, 1)
    assert relerr(torch.bmm(K2, alpha.unsqueeze(-1)).squeeze(-1), Y) < 1e-10
    # the gradient path at full size (pacoh_gp_lml_dense over all 256 problems: Cholesky -> triangular inverse -> Z^T Z ->
    # contractions): LML of every problem, gradients of 4 of them against oracle autograd in fp64 at 1e-7
    Xd, Yd = X.cuda(), Y.cuda()
    os1 = torch.ones(1, dtype=torch.float64, device='cuda')
    lml, d_z, d_mean, d_ls, d_os, d_noise, info2 = L.gp_lml_fwdbwd(Xd, 1, None, L.MEAN_ZERO, Yd, 1, ls.cuda(), os1, noise.cuda(), T, 1)
    assert int(info2.abs().max()) == 0 and float(((lml.cpu() - ref).abs() / ref.abs()).max()) < 1e-8
    for t in (0, 85, 170, 255):
        z = X[t:t + 1].clone().requires_grad_(True)
        lsr, nzr, osr = ls.clone().requires_grad_(True), noise.clone().requires_grad_(True), torch.ones((), dtype=torch.float64, requires_grad=True)
        O.gp_mll(z, torch.zeros(1, n, dtype=torch.float64), Y[t:t + 1], lsr.unsqueeze(0), osr, nzr).sum().backward()
        assert relerr(d_z[t], z.grad[0]) < 1e-7
        assert relerr(d_ls[t], lsr.grad.reshape(-1)) < 1e-7
        assert relerr(d_noise[t], nzr.grad.reshape(-1)[0]) < 1e-7 and relerr(d_os[t], osr.grad) < 1e-7


def test_bench_dump_outputs_repeat(tmp_path):
    """`python bench.py --dump-outputs DIR` (child process, twice): the timed steps start from the same state in every run, so two
    runs with the same arguments write the same arrays -- what the last timed cfg #3 step left: particles, Adam state, likelihoods"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for run in ('a', 'b'):
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '3', '--warmup', '2', '--no-other-configs',
                            '--no-cpu-baseline', '--dump-outputs', str(tmp_path / run)], cwd=root,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(str(tmp_path / 'a')))
    assert names == ['exp_avg.npy', 'exp_avg_sq.npy', 'lik.npy', 'particles.npy'] and sorted(os.listdir(str(tmp_path / 'b'))) == names
    for name in names:
        a, b = np.load(str(tmp_path / 'a' / name)), np.load(str(tmp_path / 'b' / name))
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), name
    assert np.load(str(tmp_path / 'a' / 'particles.npy')).shape[0] == 20


def test_bench_plain_line_is_the_headline_alone():
    """`python bench.py` without --full (child process) prints ONE JSON line with the driver's keys, BASELINE.json's metric and a
    value consistent with ms_per_step, and runs none of the side measurements: their keys are null"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '3', '--warmup', '2'], cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'host_ms_per_step', 'step_mode'):
        assert key in d, key
    base = json.load(open(os.path.join(root, 'BASELINE.json')))
    assert d['metric'].split(';')[0].strip() in base['metric'] and d['unit'] == 'evals/s'
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 2 and d['scaling'] == 'weak' and d['data'] == 'synthetic'
    assert d['higher_is_better'] is True and d['vs_baseline'] is None and d['dtype'] == 'f32' and d['full'] is False
    assert d['config']['finite'] is True and d['config']['evals_per_step'] == 1024 * 20
    assert abs(d['value'] - d['config']['evals_per_step'] / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    assert d['value'] >= 10000 and d['world_size_seen'] == 1 and d['host_ms_per_step'] < d['ms_per_step']
    for key in ('steady', 'roofline', 'kernel_rooflines', 'gram_roofline', 'kernel_ms_per_step', 'kernel_sum_ms_per_step',
                'profile_pass_ms_per_step', 'step_algorithmic_tflops', 'other_configs', 'predictive', 'cpu_baseline', 'legs'):
        assert d[key] is None, key


def test_bench_line_contract():
    """`python bench.py --full` (child process) prints ONE JSON line with the driver's keys, BASELINE.json's metric, a live
    roofline object and a bounded cpu_baseline; value is consistent with ms_per_step."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '3', '--warmup', '2', '--full'], cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert key in d, key
    base = json.load(open(os.path.join(root, 'BASELINE.json')))
    assert d['metric'].split(';')[0].strip() in base['metric']
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 2 and d['scaling'] == 'weak' and d['data'] == 'synthetic'
    assert d['higher_is_better'] is True and d['vs_baseline'] is None and d['dtype'] == 'f32'
    assert 'workload' in d['config'] and 'model' not in d['config'] and d['config']['finite'] is True
    evals = d['config']['evals_per_step']
    assert evals == 1024 * 20
    assert abs(d['value'] - evals / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    roof = d['roofline']
    assert roof['bound'] in ('hbm', 'mfma') and roof['unit'] in ('GB/s', 'TFLOP/s')
    assert abs(roof['frac'] - roof['achieved'] / roof['peak']) < 1e-3 and 0 < roof['frac'] < 1
    gram = d['gram_roofline']
    assert gram['bound'] == 'hbm' and gram['peak'] == 8000.0 and gram['algorithmic_bytes'] == 16896 * evals
    assert gram['frac'] >= 0.40                      # BASELINE.json: >= 40 % of the HBM roofline on the Gram build
    cpu = d['cpu_baseline']
    assert cpu['kind'] in ('port', 'reference') and cpu['value'] > 0 and cpu['cores'] >= 1 and cpu['sample']
    assert d['value'] >= 10000                       # BASELINE.json: >= 10 k evals/s on one MI355X
    # the step is replayed from a captured graph: the host needs far less than the step takes, and the per-kernel times
    # (separate eager pass) plus the reported launch gaps add up to the step
    assert d['world_size_seen'] == 1 and d['host_ms_per_step'] < d['ms_per_step']
    assert 0 < roof['algorithmic_frac'] <= roof['executed_frac'] < 1 and 'not measured in this run' in roof['traffic_source']
    # the per-kernel breakdown describes its OWN pass: kernel times <= that pass's wall time per step
    assert abs(d['kernel_sum_ms_per_step'] + d['launch_gaps_ms_per_step'] - d['profile_pass_ms_per_step']) < 1e-3
    assert d['kernel_sum_ms_per_step'] <= d['profile_pass_ms_per_step'] and d['launch_gaps_ms_per_step'] >= 0
    assert abs(sum(d['kernel_ms_per_step'].values()) - d['kernel_sum_ms_per_step']) < 1e-2
    # the other BASELINE configurations ride along, bounded, so that the driver sees them too
    oc = d['other_configs']
    # (round 6: the reference launchers' own SVGD / VI shape -- 2 tasks x 10 particles / samples per step -- and cfg #3's 1/8 shard)
    evals_of = {'cfg1': 5, 'cfg2': 256, 'cfg4': 5120, 'cfg5': 256, 'ref_svgd': 20, 'ref_vi': 20, 'ref_map': 2, 'shard128': 2560}
    assert set(oc) == set(evals_of)
    for key, leg in oc.items():
        assert leg['finite'] is True and leg['value'] > 0 and leg['ms_per_step'] > 0, key
        assert abs(leg['value'] - evals_of[key] / (leg['ms_per_step'] * 1e-3)) <= 2e-3 * leg['value'], key
        assert 0 < leg['dominant_kernel']['algorithmic_frac'] < 1, key
    assert oc['ref_svgd']['cpu_baseline']['value'] > 0 and oc['ref_vi']['cpu_baseline']['value'] > 0 and oc['ref_map']['cpu_baseline']['value'] > 0
    # PACOH-VI at the launcher's shape: host-noise step >= the same step with the noise resident; the noise='device' step in between
    assert 0 < oc['ref_vi']['gpu_ms_per_step_noise_resident'] <= oc['ref_vi']['ms_per_step']
    assert 0 < oc['ref_vi']['ms_per_step_device_noise'] < oc['ref_vi']['ms_per_step']
    assert oc['cfg5']['dtype'] == 'f64' and oc['cfg1']['dtype'] == oc['cfg2']['dtype'] == oc['cfg4']['dtype'] == 'f32'
    # ... and the marginal posterior predictive at the context sizes of cfg #3 / cfg #4 (row A11)
    pr = d['predictive']
    assert set(pr) == {'cfg3_shape', 'cfg4_shape'}
    for leg in pr.values():
        assert leg['finite'] is True and leg['info_max'] == 0 and abs(leg['value'] - leg['problems'] / (leg['ms_per_call'] * 1e-3)) <= 2e-3 * leg['value']
