"""The measured per-problem error of the fp32 small-context GP kernels (n <= 128 register- and LDS-resident MFMA kernels, the general
LDS-resident kernel's alpha / L outputs, the register-resident marginal predictive) beside the error of plain torch fp32 on the CPU
(autograd through the same oracle expression; the worst over NORD orders of the context points, see the test module), both against
the fp64 oracle, for every case and every problem of
tests/test_gpu_fp32_accuracy.py (same problems: the test module's own cases and seeds, inputs rounded to fp32 first).
    python tests/small_fp32_errors.py > profiles/small_fp32_errors.txt      (a checker script, not a collected test)
Normalisation (one rule per kind of output, measure() in the test module):
  LML                                    |h - r| / max(|r|, 1)
  d_z, d_mean, d_ls, d_os, d_noise [b]   ||h - r|| / max(||r||, 1e-3 ||(d_ls, d_os, d_noise)_ref[b]||)
  mu, var, alpha, L [b]                  ||h - r|| / max(||r||, 1e-3 sqrt(len))
Each row: problem b, its parameter row (regime), its valid size, then `hip / torch32` per output.  The summary at the end gives, per
kind of launch, regime and output, the worst HIP error and the worst ratio err_hip / max(err_torch32, A[q] / R): what the bars of the
test module are set from.  The `ladder` rows: the problem of test_jitter_ladder_per_problem that needs a rung, against the oracle at
noise + jitter."""
import sys

import torch

sys.path.insert(0, '.')
from meta_learning_pacoh_amd import _lib as L
from tests import test_gpu_fp32_accuracy as M

L.load_library()
torch.set_num_threads(8)
worst = {}          # (kind, regime, q) -> (worst hip error, worst ratio)
print('per-problem relative error vs the fp64 oracle:  HIP fp32 / torch-CPU fp32 (same expression, autograd)')
for kind, case, i in M.ALL:
    pb = M.make(kind, case, i)
    errs = M.measure(L, {'no_os': 'lml', 'mfma': 'lml'}.get(kind, kind), pb)
    print('\n%s #%d  n=%d f=%d T=%d P=%d shared=%s mean=%s sizes=%s%s' % (kind, i, pb.n, pb.f, pb.T, pb.P, pb.z_div != 1, pb.mean_mode,
                                                                         sorted(set(pb.sizes)), ' m=%d' % pb.m if pb.m else ''))
    qs = list(errs)
    print('   b regime    nv | ' + ' | '.join('%-15s' % q for q in qs))
    for b in range(pb.B):
        print('%4d %-8s %4d | ' % (b, pb.row(b), pb.nv(b)) + ' | '.join('%.1e / %.1e' % (errs[q][0][b], errs[q][1][b]) for q in qs))
        for q in qs:
            eh, ec = float(errs[q][0][b]), float(errs[q][1][b])
            a = M.A['lml' if q == 'lml_fwd' else q]
            key = (kind, pb.row(b), q)
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], eh), max(w[1], eh / max(ec, a / M.R)))      # (<= R: passes; the benign row is also capped)
    sys.stdout.flush()

print('\nladder: the laddered problem of test_jitter_ladder_per_problem vs the oracle at noise + 1e-6 10^(info - 1)')
for n in (32, 64, 96, 128):
    out, inputs = M.ladder_launch(L, n, 3, True)
    for b in range(1, 3 * len(M.LADDER_ROWS), len(M.LADDER_ROWS)):
        info = int(out[6][b])
        e = M.ladder_errors(out, inputs, b, 1e-6 * 10 ** (info - 1))
        print('ladder n=%4d b=%2d info %d | ' % (n, b, info) + ' | '.join('%s %.1e' % kv for kv in e.items()))

print('\nsummary: worst HIP error / worst ratio err_hip / max(err_torch32, A[q] / R)  (R = %g)' % M.R)
for kind in dict.fromkeys(k for k, _, _ in worst):
    for reg in [r[0] for r in M.ROWS]:
        qs = [q for (k, r, q) in worst if k == kind and r == reg]
        if qs:
            print('%-8s %-8s | ' % (kind, reg) + ' | '.join('%s %.1e / %.1f' % (q, *worst[(kind, reg, q)]) for q in qs))
