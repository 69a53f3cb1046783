"""The measured per-problem error of the fp32 leave-one-out kernel (csrc/gp_loo.hip) beside the error of the same closed form in plain
torch fp32 on the CPU (tests/loo_ref.closed, the worst over NORD orders of the context points), both against really leaving each point
out in fp64 (tests/loo_ref.brute) on the same fp32-rounded inputs, for every case and every problem of
test_fp32_per_problem_error_against_torch_fp32 in tests/test_gpu_loo.py (the test module's own cases and seeds); then the four learners
of test_learners_loo_is_predict_without_the_point: loo() against predict() on the context without the point.
    python tests/loo_fp32_errors.py [out]      (default out: profiles/loo_fp32_errors.txt; a checker script, not a collected test)
Errors per problem:  mu  max_i |h - r| / sqrt(var_ref),  var  max_i |h - r| / var_ref,  lpd  |h - r| / max(|r|, 1).
Each row: problem b, its valid size, then `hip / torch32` per output.  The summary gives the worst HIP error, the worst ratio
err_hip / err_torch32 among the problems where torch's error is not 0, and -- what the floors A32 of the test module are 4x of -- the
worst HIP error among the problems beyond 10x torch fp32."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402
import test_gpu_loo as M                                # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'loo_fp32_errors.txt')
L.load_library()
torch.set_num_threads(8)
lines = []


def say(s=''):
    print(s)
    sys.stdout.flush()
    lines.append(s)


QS = ('mu', 'var', 'lpd')
worst_hip = dict.fromkeys(QS, 0.0)
worst_ratio = dict.fromkeys(QS, 0.0)
beyond = dict.fromkeys(QS, 0.0)
say('per-problem error vs leaving each point out in fp64:  HIP fp32 / torch-CPU fp32 (closed form, worst of %d point orders)' % M.NORD)
for key, tag, build in M.ALL32:
    batch = build()
    rows = M.measure(L, key, batch)
    say('\n%s  T=%d P=%d z_div=%d y_div=%d mean=%s' % (tag, batch.B // batch.P, batch.P, batch.z_div, batch.y_div, batch.mean_mode))
    say('   b   nv | ' + ' | '.join('%-17s' % q for q in QS))
    for b, (s, eh, ec) in enumerate(rows):
        say('%4d %4d | ' % (b, s) + ' | '.join('%.1e / %.1e' % (h, c) for h, c in zip(eh, ec)))
        for q, h, c in zip(QS, eh, ec):
            worst_hip[q] = max(worst_hip[q], h)
            if c > 0:
                worst_ratio[q] = max(worst_ratio[q], h / c)
            if h > 10 * c:
                beyond[q] = max(beyond[q], h)

say('\nsummary (R = %g):' % M.R40)
for q in QS:
    say('%-4s worst HIP error %.1e | worst ratio hip / torch32 %.1f | worst HIP error among problems beyond 10x torch32 %.1e'
        % (q, worst_hip[q], worst_ratio[q], beyond[q]))

say('\nlearners: loo() / eval_loo() / eval_loo_datasets() against predict() on the context without point i (4 tasks x 6 points, fp32 both')
say('sides); mean, std, rmse in units of the predictive std, ll / calib / datasets absolute')
worst = 0.0
for kind in ('map', 'svgd', 'vi', 'single'):
    diffs, _, _ = M.learner_differences(kind)
    worst = max(worst, max(diffs.values()))
    say('%-6s | ' % kind + ' | '.join('%s %.1e' % kv for kv in diffs.items()))
say('worst learner difference %.1e' % worst)

with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
