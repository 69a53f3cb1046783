"""time of a conditioned posterior against the learner's own calls:  python tools/cond_time.py [out] [--repeats K]

Setup: fp32, PACOH-SVGD with P particles, 4 x 32 mean and feature networks (feature_dim 2), d = 1, after 3 meta-iterations;
P in {10, 20}, context n in {20, 64, 128}, m in {64, 1000, 20000} test points.  Per shape, on the same inputs:
  predict   cond.predict(test_x)            against   model.predict(cx, cy, test_x)      (the path every call took before)
  append    cond.append(x, y) of ONE point  against   model.condition(cx, cy) on all n + 1 points (the refit it replaces)
            (the object is put back to n points after every append -- n and a copy of alpha, one small device copy inside the call)
Three figures each, in us per call: CALL, the wall clock around the public call (host work and the device-to-host copy of the result
included, synchronised); KERN, the sum of the HIP-event times that _lib.PROFILE records around every C-ABI call inside it (network
forwards + GP launch; a separate pass, so the events do not sit in the call time); GP, the GP launch alone (gp_cond_predict /
gp_cond_append against gp_predict / gp_condition).  After a warm-up of both sides the two sides ALTERNATE in the same process;
reported: the median of K repeats of `reps` calls and the min .. max spread.  model.predict is untouched by the conditioned path, so it
is the baseline.  The table is written to `out` (default profiles/cond_time.txt)."""
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

GP_NAMES = ('gp_cond_predict', 'gp_cond_append', 'gp_predict', 'gp_predict_dense', 'gp_condition')


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


def kernel_time(run, reps):
    """-> (all C-ABI calls, the GP launch alone) in us per call"""
    torch.cuda.synchronize()
    L.PROFILE = {}
    try:
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        summary = L.profile_summary()
    finally:
        L.PROFILE = None
    every = sum(ms for _, ms in summary.values()) / reps * 1e3
    gp = sum(ms for name, (_, ms) in summary.items() if name in GP_NAMES) / reps * 1e3
    return every, gp


def fmt(v):
    return '%9.1f [%8.1f .. %8.1f]' % (statistics.median(v), min(v), max(v))


def measure(sides, repeats):
    """sides = (cond, model) -> reps, the table cells"""
    for s in sides:
        call_time(s, 2)                                                # warm-up (code objects, allocator, workspaces)
    t0 = min(call_time(s, 2) for s in sides)
    reps = max(3, min(200, int(0.1e6 / max(t0, 1.0))))
    res = [[[], [], []], [[], [], []]]
    for _ in range(repeats):
        for i, s in enumerate(sides):
            res[i][0].append(call_time(s, reps))
        for i, s in enumerate(sides):
            every, gp = kernel_time(s, reps)
            res[i][1].append(every)
            res[i][2].append(gp)
    med = statistics.median
    return reps, ' | '.join('%s | %s | %6.3f' % (fmt(res[0][j]), fmt(res[1][j]), med(res[0][j]) / med(res[1][j])) for j in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'cond_time.txt'))
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cond_time.py needs a HIP device: nothing is measured without one')
    L.load_library()
    lines = ['# measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0),
             '# conditioned posterior against the learner\'s own calls (python tools/cond_time.py): fp32, PACOH-SVGD, 4 x 32 networks.',
             '# us per call, median of %d alternating repeats [min .. max].  call = wall clock of the public call; kern = HIP events around' % a.repeats,
             '# every C-ABI call inside it; gp = the GP launch alone.  ratio = cond / model (below 1: the conditioned object is faster).',
             '# predict: cond.predict(tx) vs model.predict(cx, cy, tx).  append: cond.append(one point) vs model.condition(all n + 1 points).']
    cell = '%-31s | %-31s | %6s'
    head = '%-8s %3s %4s %6s %5s | ' % ('what', 'P', 'n', 'm', 'reps') + ' | '.join(
        cell % ('cond %s us' % q, 'model %s us' % q, 'ratio') for q in ('call', 'kern', 'gp'))
    lines.append(head)
    print(head)
    rs = np.random.RandomState(0)
    for P in (10, 20):
        model = M.GPRegressionMetaLearnedSVGD(tasks(rs), num_iter_fit=3, feature_dim=2, mean_nn_layers=(32, 32, 32, 32),
                                              kernel_nn_layers=(32, 32, 32, 32), num_particles=P, task_batch_size=4, random_seed=P)
        model.meta_fit(verbose=False, log_period=1000)
        for n in (20, 64, 128):
            cx = rs.uniform(-3, 3, size=(n + 1, 1))
            cy = np.sin(cx) + 0.1 * rs.randn(n + 1, 1)
            for m in (64, 1000, 20000):
                tx = rs.uniform(-3.5, 3.5, size=(m, 1))
                cond = model.condition(cx[:n], cy[:n])
                sides = (lambda: cond.predict(tx), lambda: model.predict(cx[:n], cy[:n], tx))
                a1, a2 = sides[0](), sides[1]()
                diff = float(np.max(np.abs(a1[0] - a2[0]) / a2[1]))
                assert diff < 1e-3, diff
                reps, text = measure(sides, a.repeats)
                lines.append(('%-8s %3d %4d %6d %5d | ' % ('predict', P, n, m, reps)) + text)
                print(lines[-1])
                sys.stdout.flush()
            cond = model.condition(cx[:n], cy[:n])
            alpha0 = cond._state.bufs[3].clone()

            def append_one():
                cond.append(cx[n:], cy[n:])
                cond._state.n = n                                      # back to n points for the next call
                cond._state.bufs[3].copy_(alpha0)

            reps, text = measure((append_one, lambda: model.condition(cx, cy)), a.repeats)
            lines.append(('%-8s %3d %4d %6s %5d | ' % ('append', P, n, '-', reps)) + text)
            print(lines[-1])
            sys.stdout.flush()
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
