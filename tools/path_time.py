"""time of pathwise posterior function draws on a conditioned GP:  python tools/path_time.py [out] [--repeats K]

Setup: fp32, 4 x 32 mean and feature networks (feature_dim 2), d = 1, after 3 meta-iterations; a MAP row (P = 1) and PACOH-SVGD with
P = 20 particles; context n = 128, D = 1024 random features, S = 16 draws per row; m in {2048, 10^4, 10^5} candidates.  Per shape:
  fit      paths = cond.sample_paths(16)      (the random base on the device + one pacoh_gp_path_fit launch)
  eval     paths(candidates)                  (network forwards for the candidates + one pacoh_gp_path_eval launch), result on the device
  baseline model.predict(cx, cy, candidates, return_density=True).rsample((16,)): what the package offered for joint draws before --
           it refactors the context, builds the m x m predictive covariance of every row and factors it.  Run at m = 2048 only: at the
           larger m it is not run: the covariances alone need P m^2 4 bytes (stated below; 8 GB for 20 rows at m = 10^4, 800 GB
           at m = 10^5, where it cannot run at all), before P Cholesky factorisations of order m.  Note that it returns 16 draws
           of the mixture in all, the pathwise call 16 draws PER ROW.
Figures in us per call: CALL, the wall clock around the public call, synchronised; GP, the HIP-event time that _lib.PROFILE records
around the pacoh_gp_path_fit / pacoh_gp_path_eval launch alone (a separate pass).  From GP of eval: the rate of left-operand entries
(P m (D + n) cosines / kernel values per call) and of the GEMM's flops (2 P m (D + n) S).  After a warm-up of every side, the sides
ALTERNATE in the same process; reported: the median of K repeats of `reps` calls and the min .. max spread.  No ratio is fixed in
advance: the table records what was measured.  It is written to `out` (default profiles/path_time.txt)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meta_learning_pacoh_amd as M                                   # noqa: E402
from meta_learning_pacoh_amd import _lib as L                         # noqa: E402

N_CTX, D_FEAT, S_DRAWS = 128, 1024, 16
MS = (2048, 10000, 100000)
BASELINE_M = 2048


def tasks(rs, T=8, n=32):
    out = []
    for t in range(T):
        x = rs.uniform(-3, 3, size=(n, 1))
        out.append((x, (0.8 + 0.1 * t) * np.sin(x + 0.2 * t) + 0.1 * rs.randn(n, 1)))
    return out


def call_time(run, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def gp_time(run, reps, name):
    torch.cuda.synchronize()
    L.PROFILE = {}
    try:
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        summary = L.profile_summary()
    finally:
        L.PROFILE = None
    return sum(ms for k, (_, ms) in summary.items() if k == name) / reps * 1e3


def fmt(v):
    return '%10.1f [%9.1f .. %9.1f]' % (statistics.median(v), min(v), max(v))


def measure(sides, repeats):
    """sides = [(run, PROFILE name | None)] -> reps, [(call times, gp times)] per side, the sides alternating"""
    for run, _ in sides:
        call_time(run, 2)                                              # warm-up (code objects, allocator, workspaces)
    t0 = max(call_time(run, 2) for run, _ in sides)
    reps = max(3, min(100, int(0.2e6 / max(t0, 1.0))))
    res = [([], []) for _ in sides]
    for _ in range(repeats):
        for i, (run, _) in enumerate(sides):
            res[i][0].append(call_time(run, reps))
        for i, (run, name) in enumerate(sides):
            if name:
                res[i][1].append(gp_time(run, reps, name))
    return reps, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'path_time.txt'))
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('path_time.py needs a HIP device: nothing is measured without one')
    L.load_library()
    lines = ['# measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0),
             '# pathwise posterior draws on a conditioned GP (python tools/path_time.py): fp32, 4 x 32 networks, n = %d context points,'
             % N_CTX,
             '# D = %d random features, S = %d draws per parameter row.  us per call, median of %d alternating repeats [min .. max].'
             % (D_FEAT, S_DRAWS, a.repeats),
             '# call = wall clock of the public call, synchronised; gp = HIP events around the pacoh_gp_path_* launch alone.',
             '# fit = cond.sample_paths(16); eval = paths(candidates) -> [P * 16, m] on the device;',
             '# baseline = model.predict(cx, cy, candidates, return_density=True).rsample((16,)) (16 draws of the mixture in all).']
    rs = np.random.RandomState(0)
    kw = dict(num_iter_fit=3, feature_dim=2, mean_nn_layers=(32, 32, 32, 32), kernel_nn_layers=(32, 32, 32, 32), task_batch_size=4)
    models = (('map', 1, M.GPRegressionMetaLearned(tasks(rs), random_seed=1, **kw)),
              ('svgd', 20, M.GPRegressionMetaLearnedSVGD(tasks(rs), num_particles=20, random_seed=20, **kw)))
    cx = rs.uniform(-3, 3, size=(N_CTX, 1))
    cy = np.sin(cx) + 0.1 * rs.randn(N_CTX, 1)
    for name, P, model in models:
        model.meta_fit(verbose=False, log_period=1000)
        cond = model.condition(cx, cy)
        for m in MS:
            tx = rs.uniform(-3.5, 3.5, size=(m, 1))
            torch.manual_seed(m)
            paths = cond.sample_paths(S_DRAWS, D_FEAT)
            out = paths(tx)
            assert tuple(out.shape) == (P * S_DRAWS, m) and bool(torch.isfinite(out).all())
            # a gross check that these are draws of THIS posterior, in the right units: their mean over rows and draws against the
            # predictive mean, in predictive standard deviations (the standard error alone is up to 1 / sqrt(16) per row)
            mean, std = cond.predict(tx)
            z = float(np.max(np.abs(out.mean(0).cpu().numpy() - mean) / std))
            assert z < 2.0, z
            sides = [(lambda: cond.sample_paths(S_DRAWS, D_FEAT), 'gp_path_fit'), (lambda: paths(tx), 'gp_path_eval')]
            if m == BASELINE_M:
                sides.append((lambda: model.predict(cx, cy, tx, return_density=True).rsample((S_DRAWS,)), None))
            reps, res = measure(sides, a.repeats)
            gp = statistics.median(res[1][1]) * 1e-6
            entries, flops = P * m * (D_FEAT + N_CTX), 2.0 * P * m * (D_FEAT + N_CTX) * S_DRAWS
            lines.append('%-4s P=%2d m=%6d reps=%3d' % (name, P, m, reps))
            lines.append('    fit      call %s | gp %s' % (fmt(res[0][0]), fmt(res[0][1])))
            lines.append('    eval     call %s | gp %s | %.2f G left-operand entries/s, %.2f TFLOP/s in the GEMM'
                         % (fmt(res[1][0]), fmt(res[1][1]), entries / gp * 1e-9, flops / gp * 1e-12))
            if m == BASELINE_M:
                lines.append('    baseline call %s | fit + eval / baseline = %.3f'
                             % (fmt(res[2][0]), (statistics.median(res[0][0]) + statistics.median(res[1][0])) / statistics.median(res[2][0])))
            else:
                lines.append('    baseline not run at this m: the %d predictive covariance(s) of order %d alone need %.1f GB (%.1f GB per '
                             'row), before their O(m^3) Cholesky factors' % (P, m, P * m * m * 4 / 1e9, m * m * 4 / 1e9))
            for ln in lines[-4:]:
                print(ln)
            sys.stdout.flush()
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
