"""The measured per-problem error of the fp32 pathwise-draw kernels (csrc/gp_path.hip: fit + eval on a state of csrc/gp_cond.hip)
beside the error of the same formulas in plain torch fp32 on the CPU (tests/path_ref.paths through X of tests/cond_ref.direct, the
worst over NORD orders of the context points), both against tests/path_ref.paths_direct in fp64 on the same fp32-rounded inputs and
base, for every case and every problem of test_fp32_per_problem_error_against_torch_fp32 in tests/test_gpu_path.py (the test
module's own cases and seeds); then the learner cases of test_learners_seeded_paths_snapshot_and_like.
    python tests/path_fp32_errors.py [out]      (default out: profiles/path_fp32_errors.txt; a checker script, not a collected test)
Error per problem:  e = max_{s,t} |out - ref| / sqrt(outputscale)  in normalised space.
Each row: problem b, then `hip / torch32`.  The summary gives the worst HIP error, the worst ratio e_hip / e_torch32 among the
problems where torch's error is not 0, and -- what the floor A32 of the test module is 4x of -- the worst HIP error among the
problems beyond 10x torch fp32."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402
import test_gpu_path as M                               # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'path_fp32_errors.txt')
L.load_library()
torch.set_num_threads(8)
lines = []


def say(s=''):
    print(s)
    sys.stdout.flush()
    lines.append(s)


worst_hip = worst_ratio = beyond = 0.0


def account(h, c):
    global worst_hip, worst_ratio, beyond
    worst_hip = max(worst_hip, h)
    if c > 0:
        worst_ratio = max(worst_ratio, h / c)
    if h > 10 * c:
        beyond = max(beyond, h)


say('measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0))
say('per-problem error vs the fp64 direct reference:  HIP fp32 / torch-CPU fp32 (worst of %d point orders)' % M.NORD)
for spec in M.specs(M.TC.limit_of(L, torch.float32)):
    rows = M.measure(L, spec)
    say('\n%s' % spec.tag)
    for b, (h, c) in enumerate(rows):
        say('%4d | %.1e / %.1e' % (b, h, c))
        account(h, c)

say('\nlearners: sample_paths(5, 128) on 4 context points, then like= on 6, against the reference on the state pulled to the CPU')
for kind in M.TC.KINDS:
    model, cond, cx, cy = M._condition(kind)
    tx = M._tx()
    torch.manual_seed(77)
    paths = cond.sample_paths(5, 128)
    rows = M.learner_errors(cond, paths, tx)
    cond.append(cx[4:], cy[4:])
    rows += M.learner_errors(cond, cond.sample_paths(5, 128, like=paths), tx)
    say('%-8s | ' % kind + ' | '.join('%.1e / %.1e' % r for r in rows))
    for h, c in rows:
        account(h, c)

say('\nsummary (R = %g): worst HIP error %.1e | worst ratio hip / torch32 %.1f | worst HIP error among problems beyond 10x torch32 %.1e'
    % (M.R40, worst_hip, worst_ratio, beyond))

with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
