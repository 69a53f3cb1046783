"""The measured per-task error of the fp32 acquisition kernel (csrc/acq.hip) beside the error of the same rule
(meta_learning_pacoh_amd/acquisition.py) in plain torch fp32 on the CPU, both against that rule in fp64 on the same fp32-rounded
inputs, for every case and every task of test_values_and_selection_sweep in tests/test_gpu_acq.py (the test module's own cases and
seeds); then the learner cases of test_learners_through_the_public_api.
    python tests/acq_fp32_errors.py [out]      (default out: profiles/acq_fp32_errors.txt; a checker script, not a collected test)
Errors per task:  'ei', 'ucb', 'mean', 'std'  max_s |h - r| / sd_mix_ref(s),  'pi'  max_s |h - r|.
Each row: task t, then `hip / torch32`.  The summary gives per kind the worst HIP error, the worst ratio err_hip / err_torch32 among
the tasks where torch's error is not 0, and -- what the floors A32 of the test module are 4x of -- the worst HIP error among the
tasks beyond 10x torch fp32."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402
from meta_learning_pacoh_amd import acquisition as A    # noqa: E402
import test_gpu_acq as M                                # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'acq_fp32_errors.txt')
L.load_library()
torch.set_num_threads(8)
lines = []


def say(s=''):
    print(s)
    sys.stdout.flush()
    lines.append(s)


worst_hip = dict.fromkeys(A.KINDS, 0.0)
worst_ratio = dict.fromkeys(A.KINDS, 0.0)
beyond = dict.fromkeys(A.KINDS, 0.0)
say('measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0))
say('per-task error vs the rule in fp64:  HIP fp32 / torch-CPU fp32')
for kind in A.KINDS:
    for case in M.cases(kind, torch.float32):
        eh, ec = M.measure(L, case, kind)[:2]
        say('\n%-4s %s  T=%d P=%d m=%d sign=%+d noise=%s strips=%d' % (kind, case.tag, case.T, case.P, case.m, case.sign,
                                                                      case.noise is not None, case.strips))
        for t, (h, c) in enumerate(zip(eh, ec)):
            say('%4d | %.1e / %.1e' % (t, h, c))
            worst_hip[kind] = max(worst_hip[kind], h)
            if c > 0:
                worst_ratio[kind] = max(worst_ratio[kind], h / c)
            if h > 10 * c:
                beyond[kind] = max(beyond[kind], h)

say('\nsummary (R = %g):' % M.R40)
for kind in A.KINDS:
    say('%-5s worst HIP error %.1e | worst ratio hip / torch32 %.1f | worst HIP error among tasks beyond 10x torch32 %.1e'
        % (kind, worst_hip[kind], worst_ratio[kind], beyond[kind]))

say('\nlearners: cond.acquisition(kind, x) against the rule in fp64 on the components of cond.predict(x, return_density=True) (kind+ :')
say('maximize, kind- : minimize), and the learner\'s predict(..., return_density=True).acquisition(\'ucb\') against')
say('cond.acquisition(\'ucb\', x, observation_noise=True); 173 candidates, fp32, in units of the predictive std (\'pi\': absolute)')
worst = 0.0
for kind in M.TC.KINDS:
    diffs = M.learner_differences(kind)[0]
    worst = max(worst, max(diffs.values()))
    say('%-8s | ' % kind + ' | '.join('%s %.1e' % kv for kv in diffs.items()))
say('worst learner difference %.1e' % worst)

with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
