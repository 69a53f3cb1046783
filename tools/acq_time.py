"""time and peak memory of the analytic acquisition with its fused argmax:  python tools/acq_time.py [out] [--repeats K]

Setup as tools/path_argmax_time.py: fp32, 4 x 32 mean and feature networks (feature_dim 2), d = 1, after 3 meta-iterations; a MAP row
(P = 1) and PACOH-SVGD with P = 20 particles; context n = 128; m in {2048, 10^4, 10^5} candidates.  Per shape two ways to the
candidate of greatest expected improvement over the best observed target:
  fused    cond.acquire('ei', candidates)           (per chunk of 131 072: the network forwards, pacoh_gp_cond_predict, pacoh_mixture_acq)
  torch    cond.predict(candidates, return_density=True), then the rule as vectorised torch on the [P, m] moments on the device (about a
           dozen elementwise launches and a mean over the rows), then torch.max   (what there was before)
and one more row, fused only, at m = 10^6 (eight chunks; before, a user had to chunk the pool by hand).
Figures in us per call: CALL, the wall clock around the public call(s), synchronised; PREDICT / ACQ, the HIP-event time that
_lib.PROFILE records around the pacoh_gp_cond_predict call(s) and around the pacoh_mixture_acq call(s) alone (both of its launches,
summed over the chunks).  PEAK: the rise of torch's allocator peak during one call.  BW: the bytes the acquisition launch reads (mu and
var, 8 P m) over its time.  After a warm-up of every side, the sides ALTERNATE in the same process; reported: the median of K repeats
of `reps` calls and the min .. max spread.  The two ways are also compared: the same value to fp32 rounding, the same index unless two
candidates are within that rounding.  No ratio is fixed in advance: the table records what was measured.  It is written to `out`
(default profiles/acq_time.txt)."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_learning_pacoh_amd as M                                   # noqa: E402
from meta_learning_pacoh_amd import _lib as L                         # noqa: E402
from path_time import MS, N_CTX, call_time, fmt, tasks                # noqa: E402
from path_argmax_time import BIG_M, peak_rise                         # noqa: E402

NAMES = ('gp_cond_predict', 'mixture_acq')


def event_times(run, reps):
    """-> {PROFILE name: us per call} for NAMES"""
    torch.cuda.synchronize()
    L.PROFILE = {}
    try:
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        summary = L.profile_summary()
    finally:
        L.PROFILE = None
    return {k: summary.get(k, (0, 0.0))[1] / reps * 1e3 for k in NAMES}


def torch_way(cond, tx, best_n):
    """the parent's way: predict, the rule as vectorised torch on the device (normalised space, latent function), torch.max"""
    dist = cond.predict(tx, return_density=True)
    mu, var = dist._mu_n, dist._var_n
    s = torch.sqrt(torch.clamp(var - cond._state.hypers[2].reshape(-1, 1), min=0.0))
    z = (mu - best_n) / s
    Phi = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    ei = torch.clamp(s * (z * Phi + phi), min=0.0).mean(0) * dist.y_std
    top = torch.max(ei, dim=0)
    return top.indices, top.values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'acq_time.txt'))
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('acq_time.py needs a HIP device: nothing is measured without one')
    L.load_library()
    lines = ['# measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0),
             '# the candidate of greatest expected improvement of a pool (python tools/acq_time.py): fp32, 4 x 32 networks, n = %d context'
             % N_CTX,
             '# points.  us per call, median of %d alternating repeats [min .. max].' % a.repeats,
             '# fused = cond.acquire(\'ei\', candidates); torch = cond.predict(candidates, return_density=True), the rule as vectorised torch',
             '# on the device, torch.max.  call = wall clock of the public call(s), synchronised; predict / acq = HIP events around',
             '# pacoh_gp_cond_predict / pacoh_mixture_acq (both launches) alone, summed over the chunks; peak = rise of the allocator\'s',
             '# peak during one call; bw = 8 P m bytes (mu and var read once) over the acq time.']
    rs = np.random.RandomState(0)
    kw = dict(num_iter_fit=3, feature_dim=2, mean_nn_layers=(32, 32, 32, 32), kernel_nn_layers=(32, 32, 32, 32), task_batch_size=4)
    models = (('map', 1, M.GPRegressionMetaLearned(tasks(rs), random_seed=1, **kw)),
              ('svgd', 20, M.GPRegressionMetaLearnedSVGD(tasks(rs), num_particles=20, random_seed=20, **kw)))
    cx = rs.uniform(-3, 3, size=(N_CTX, 1))
    cy = np.sin(cx) + 0.1 * rs.randn(N_CTX, 1)
    for name, P, model in models:
        model.meta_fit(verbose=False, log_period=1000)
        cond = model.condition(cx, cy)
        best_n = float(cond._state.ctx_y[:cond.n].max())
        for m in MS + (BIG_M,):
            tx = rs.uniform(-3.5, 3.5, size=(m, 1))
            fused = lambda: cond.acquire('ei', tx)
            dense = lambda: torch_way(cond, tx, best_n)
            idx, val = fused()
            assert 0 <= int(idx) < m and bool(torch.isfinite(val))
            sides = [fused]
            same = None
            if m != BIG_M:
                i2, v2 = dense()
                assert abs(float(v2) - float(val)) <= 1e-4 * max(abs(float(val)), 1e-6), (float(v2), float(val))
                same = int(i2) == int(idx)
                sides.append(dense)
            peaks = [peak_rise(run) for run in sides]
            for run in sides:
                call_time(run, 2)                                          # warm-up (code objects, allocator)
            t0 = max(call_time(run, 2) for run in sides)
            reps = max(3, min(100, int(0.2e6 / max(t0, 1.0))))
            calls, events = [[] for _ in sides], [[] for _ in sides]
            for _ in range(a.repeats):
                for i, run in enumerate(sides):
                    calls[i].append(call_time(run, reps))
                for i, run in enumerate(sides):
                    events[i].append(event_times(run, reps))
            pred = [[e['gp_cond_predict'] for e in ev] for ev in events]
            acq = [e['mixture_acq'] for e in events[0]]
            t_acq, t_pred = statistics.median(acq), statistics.median(pred[0])
            first = len(lines)
            lines.append('%-4s P=%2d m=%7d reps=%3d' % (name, P, m, reps))
            lines.append('    fused    call %s | predict %s | acq %s | peak %10.2f MB' % (fmt(calls[0]), fmt(pred[0]), fmt(acq), peaks[0] / 1e6))
            lines.append('             acq / predict %.3f | bw %.3f TB/s' % (t_acq / t_pred, 8.0 * P * m / (t_acq * 1e-6) / 1e12))
            if m != BIG_M:
                lines.append('    torch    call %s | predict %s | peak %10.2f MB | same index: %s'
                             % (fmt(calls[1]), fmt(pred[1]), peaks[1] / 1e6, same))
                lines.append('    fused / torch: call %.2f, peak %.3f'
                             % (statistics.median(calls[0]) / statistics.median(calls[1]), peaks[0] / max(1, peaks[1])))
            else:
                lines.append('    torch    not run at this m')
            for ln in lines[first:]:
                print(ln)
            sys.stdout.flush()
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
