"""The measured per-block error of the fused per-particle MLP backward kernels in their LARGE-launch form (csrc/mlp_fused.hip: 64-point
tiles, several tiles per wave, a gradient slab per workgroup or per wave) beside the error of plain torch fp32 on the CPU (autograd
through O.mlp_vectorized_forward, the worst over NORD orders of a particle's rows), both against the same expression in fp64 from the
same fp32-rounded inputs, for every case and entry point of test_backward_blocks_against_fp64 and
test_backward_hyper_live_tasks_on_the_larger_searched_shape in tests/test_gpu_mlp_large.py (the test module's own shapes and seeds).
    python tests/mlp_large_fp32_errors.py [out]    (default out: profiles/mlp_large_fp32_errors.txt; a checker script, not a collected test)
Error of a parameter block (a layer's bias or weight) of one particle and network:
    ||h - r|| / max(||r||, 1e-3 ||the gradient of that particle and network||)
Each row: case, entry point, network, then per block the worst particle's `hip / torch32`.  The summary gives the worst HIP error, the
worst ratio err_hip / max(err_torch32, FLOOR / F) with its block -- what F of the test module is judged by (<= F passes) --, the worst
HIP error among the blocks beyond 10x torch fp32 -- what FLOOR is judged by -- and the worst error over a whole gradient."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402
import test_gpu_mlp_large as M                          # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'mlp_large_fp32_errors.txt')
L.load_library()
torch.set_num_threads(8)
lines = []


def say(s=''):
    print(s)
    sys.stdout.flush()
    lines.append(s)


worst_hip, worst_ratio, beyond, worst_glob = (0.0, ''), (0.0, ''), (0.0, ''), (0.0, '')


def account(case, q, refc, grads):
    global worst_hip, worst_ratio, beyond, worst_glob
    for entry, grad in grads.items():
        rows, glob = refc.errors(grad)
        worst_glob = max(worst_glob, (glob, '%s %s' % (case, entry)))
        for k, eh, ec in rows:
            names = [s[0] for s in M.block_spans(q.d_in, q.hidden, q.block(k)[1])]
            cells = []
            for j, nm in enumerate(names):
                p = int(eh[:, j].argmax())
                cells.append('%s %.1e / %.1e' % (nm, eh[p, j], ec[p, j]))
                for p in range(q.P):
                    where = '%s %s network %d particle %d %s' % (case, entry, k, p, nm)
                    h, c = float(eh[p, j]), float(ec[p, j])
                    worst_hip = max(worst_hip, (h, where))
                    worst_ratio = max(worst_ratio, (h / max(c, M.FLOOR / M.F), where + ': hip %.2e torch32 %.2e' % (h, c)))
                    if h > 10 * c:
                        beyond = max(beyond, (h, where + ': torch32 %.2e' % c))
            say('%-22s %-21s net %d | ' % (case, entry, k) + ' | '.join(cells))
        say('%-22s %-21s whole gradient %.2e' % (case, entry, glob))


say('measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0))
say('per-block relative error vs fp64 autograd:  HIP fp32 / torch-CPU fp32 (worst of %d row orders), the worst particle of each block' % M.NORD)
for name, up in M.bwd_cases():
    q, pl, refc, grads = M.measure_bwd(L, name, up)
    say('\n%s %s: T %d n %d P %d hidden %s, %d network(s); backward plan: %d-point tiles, %d workgroups of %d tiles'
        % (name, up, q.T, q.n, q.P, q.hidden, q.nets, *pl))
    account('%s %s' % (name, up), q, refc, grads)

name = M.live_shape(L)
T = M.bwd_shape(L, name)[0].T
for n_act in (1, T // 2):
    q, refc, grads = M.measure_live(L, n_act)
    say('\n%s dense, %d of %d tasks live (pacoh_mlp2_bwd_hyper_active)' % (name, n_act, T))
    account('%s live %d' % (name, n_act), q, refc, grads)

say('\nsummary (F = %g, FLOOR = %g)' % (M.F, M.FLOOR))
say('worst HIP error %.2e (%s)' % worst_hip)
say('worst ratio hip / max(torch32, FLOOR / F) %.2f (%s)' % worst_ratio)
say('worst HIP error among blocks beyond 10x torch32 %.2e (%s)' % beyond)
say('worst error over a whole gradient %.2e (%s)' % worst_glob)

with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
