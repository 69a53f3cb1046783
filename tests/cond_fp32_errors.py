"""The measured per-problem error of the fp32 conditioned-posterior kernels (csrc/gp_cond.hip) beside the error of the same closed form
(predict), or of the incremental form (append), in plain torch fp32 on the CPU (tests/cond_ref.py, the worst over NORD orders of the
context points), both against the oracle's posterior predictive in fp64 on the same fp32-rounded inputs, for every case and every
problem of test_fp32_per_problem_error_against_torch_fp32 in tests/test_gpu_cond.py (the test module's own cases and seeds); then the
four learner cases of test_learners_condition_is_predict.
    python tests/cond_fp32_errors.py [out]      (default out: profiles/cond_fp32_errors.txt; a checker script, not a collected test)
Errors per problem:  mu  max_s |h - r| / sqrt(var_ref),  var  max_s |h - r| / var_ref.
Each row: problem b, then `hip / torch32` per output.  The summary gives, for predict and for append, the worst HIP error, the worst
ratio err_hip / err_torch32 among the problems where torch's error is not 0, and -- what the floors A32 of the test module are 4x of --
the worst HIP error among the problems beyond 10x torch fp32."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402
import test_gpu_cond as M                               # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'cond_fp32_errors.txt')
L.load_library()
torch.set_num_threads(8)
lines = []


def say(s=''):
    print(s)
    sys.stdout.flush()
    lines.append(s)


QS = ('mu', 'var')
KEYS = [k + '_' + q for k in 'pa' for q in QS]
worst_hip = dict.fromkeys(KEYS, 0.0)
worst_ratio = dict.fromkeys(KEYS, 0.0)
beyond = dict.fromkeys(KEYS, 0.0)
say('measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0))
say('per-problem error vs the oracle predictive in fp64:  HIP fp32 / torch-CPU fp32 (worst of %d point orders)' % M.NORD)
for tag, kind, build, n0, k in M.cases32(L):
    case = build()
    rows = M.measure(L, case, n0, k)
    b_ = case.b
    say('\n%s  T=%d P=%d m=%d z_div=%d zt_div=%d y_div=%d mean=%s' % (tag, b_.B // b_.P, b_.P, case.m, b_.z_div, case.zt_div, b_.y_div,
                                                                    b_.mean_mode))
    say('   b | ' + ' | '.join('%-17s' % q for q in QS))
    for b, (eh, ec) in enumerate(rows):
        say('%4d | ' % b + ' | '.join('%.1e / %.1e' % (h, c) for h, c in zip(eh, ec)))
        for q, h, c in zip(QS, eh, ec):
            key = kind + '_' + q
            worst_hip[key] = max(worst_hip[key], h)
            if c > 0:
                worst_ratio[key] = max(worst_ratio[key], h / c)
            if h > 10 * c:
                beyond[key] = max(beyond[key], h)

say('\nsummary (R = %g; p = predict after condition, a = predict after condition + append):' % M.R40)
for key in KEYS:
    say('%-5s worst HIP error %.1e | worst ratio hip / torch32 %.1f | worst HIP error among problems beyond 10x torch32 %.1e'
        % (key, worst_hip[key], worst_ratio[key], beyond[key]))

say('\nlearners: condition().predict() / condition(first 3).append(rest).predict() / .confidence_intervals() against predict() /')
say('confidence_intervals() of the learner on the same context (4 tasks x 6 points, fp32 both sides), in units of the predictive std')
worst = 0.0
for kind in M.KINDS:
    diffs = M.learner_differences(kind)[0]
    worst = max(worst, max(diffs.values()))
    say('%-8s | ' % kind + ' | '.join('%s %.1e' % kv for kv in diffs.items()))
say('worst learner difference %.1e' % worst)

with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
