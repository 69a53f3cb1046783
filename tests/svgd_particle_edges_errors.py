"""The measured error of the SVGD step-tail kernels at the particle-count edges -- bandwidth, phi, updated particles, the IMQ
bandwidths -- beside the error of plain torch fp32 on the CPU on the same closed form (oracle/pacoh_oracle.py evaluated on fp32
tensors, torch.optim in fp32), both against the fp64 references of tests/test_gpu_svgd_particle_edges.py, for every case of that
module (its own inputs and seeds).
    python tests/svgd_particle_edges_errors.py [out]    (default out: profiles/svgd_particle_edges_errors.txt; a checker script, not a collected test)
Each row: case, then per quantity `HIP fp32 / torch-CPU fp32 | HIP fp64`.  The summary gives, per quantity, the worst HIP error in either
dtype with its case, and the worst ratio HIP fp32 / max(torch fp32, bar / 10): a bar of the test module is one of the project's
existing ones where that ratio stays <= 10 (the F = 10 convention of tests/test_gpu_mlp_large.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from meta_learning_pacoh_amd import _lib as L           # noqa: E402
from oracle import pacoh_oracle as O                    # noqa: E402
import test_gpu_svgd_particle_edges as E                # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'svgd_particle_edges_errors.txt')
L.load_library()
torch.set_num_threads(8)
F32, F64 = torch.float32, torch.float64
lines = []
worst = {}          # quantity -> [(hip32, case), (hip64, case), (ratio, case)]


def say(s=''):
    print(s)
    sys.stdout.flush()
    lines.append(s)


def account(case, quantity, bar32, hip32, t32, hip64):
    w = worst.setdefault(quantity, [(0.0, ''), (0.0, ''), (0.0, '')])
    w[0], w[1] = max(w[0], (hip32, case)), max(w[1], (hip64, case))
    if t32 == t32:                                       # (torch fp32 gave a number)
        w[2] = max(w[2], (hip32 / max(t32, bar32 / 10), '%s: hip %.2e torch32 %.2e' % (case, hip32, t32)))
    return '%s %.1e / %.1e | %.1e' % (quantity, hip32, t32, hip64)


def torch32_bandwidth(X):
    X32 = X.float()
    return O.svgd_bandwidth(O.svgd_norm_sq(X32, X32))


say('measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0))
say('relative errors vs fp64:  HIP fp32 / torch-CPU fp32 | HIP fp64')

say('\n(a) median bandwidth of Sidon-set particles on a line, worst of the consumers (which agree bit for bit)')
for P in E.A_COUNTS:
    for D in (1, 7):
        X = E.sidon_line(P, D)
        bw_o = E.median_bandwidth(X)
        h = {dt: max(E.bw_err(b, bw_o) for b in E.bandwidth_consumers(L, X, dt).values()) for dt in (F32, F64)}
        case = 'P %d D %d' % (P, D)
        say('%-14s gap %.1e  ' % (case, E.middle_gap(E.direct_d2(X))) +
            account('(a) ' + case, 'bandwidth', E.BW_TOL[F32], h[F32], E.bw_err(torch32_bandwidth(X), bw_o), h[F64]))

say('\n(b) median bandwidth under ties (integer positions), identical particles, one particle')
for P in [24, 33, 46, 64, 65, 100]:
    X = E.line_particles(np.arange(P, dtype=np.float64), 3, seed=1)
    bw_o = E.median_bandwidth(X)
    score = E.rounded(torch.Generator().manual_seed(P), P, 3)
    h = {dt: E.bw_err(E.tie_consumers(L, X, score, dt)[1], bw_o) for dt in (F32, F64)}
    case = 'ties P %d' % P
    say('%-14s ' % case + account('(b) ' + case, 'bandwidth', E.BW_TOL[F32], h[F32], E.bw_err(torch32_bandwidth(X), bw_o), h[F64]))
for P in (24, 1):
    for at_origin in (True, False):
        r = {dt: E.identical_case(L, P, at_origin, dt) for dt in (F32, F64)}
        X, score, mean = r[F32][4]
        t32 = E.relerr(O.svgd_phi_closed_form(X.float(), score.float(), None)[0], mean)
        case = 'identical P %d %s' % (P, 'at the origin' if at_origin else 'at a generic point')
        say('%-36s ' % case + account('(b) ' + case, 'phi', E.PHI_TOL[F32], r[F32][0], t32, r[F64][0]) + '  ' +
            account('(b) ' + case, 'particles', E.PHI_TOL[F32], r[F32][1], float('nan'), r[F64][1]))

say('\n(c) Gaussian particles, median bandwidth, prior term: phi, particles after 3 steps of Adam / SGD, one device-scalar SGD step')
for P in E.C_COUNTS:
    for D in E.C_DIMS:
        r = E.loop_edge_reference(P, D)
        X32, s32, mu32, sd32 = (t.float() for t in (r.X, r.score, r.mu, r.sd))
        phi32, bw32 = O.svgd_phi_closed_form(X32, s32, None)
        t = {'phi': E.relerr(phi32, r.phi), 'bw': E.bw_err(bw32, r.bw), 'bw_steps': 0.0}
        for optimizer in ('Adam', 'SGD'):
            Xo = X32.clone().requires_grad_(True)
            opt = torch.optim.Adam([Xo], lr=E.LR) if optimizer == 'Adam' else torch.optim.SGD([Xo], lr=E.LR)
            for k in range(3):
                ph, b = O.svgd_phi_closed_form(Xo.detach(), s32 + E.PF * (-(Xo.detach() - mu32) / sd32 ** 2), None)
                t['bw_steps'] = max(t['bw_steps'], E.bw_err(b, r.bws[optimizer][k]))
                Xo.grad = -ph
                opt.step()
                if optimizer == 'SGD' and k == 0:
                    t['X_dev'] = E.relerr(Xo, r.traj['SGD'][0])
            t['X_' + optimizer] = E.relerr(Xo, r.traj[optimizer][2])
        h = {dt: E.loop_edge_errors(L, P, D, dt) for dt in (F32, F64)}
        case = 'P %d D %d' % (P, D)
        bars = {'phi': E.PHI_TOL, 'bw': E.BW_TOL, 'bw_steps': E.BW_TOL, 'X_Adam': E.PHI_TOL, 'X_SGD': E.PHI_TOL, 'X_dev': E.PHI_TOL}
        say('%-12s ' % case + '  '.join(account('(c) ' + case, q, bars[q][F32], h[F32][q], t[q], h[F64][q]) for q in sorted(bars)))

say('\n(c) a score in one particle\'s row only (D = %d), worst over the rows' % E.ONE_HOT_D)
for P in E.C_COUNTS:
    h = {dt: E.one_hot_errors(L, P, dt) for dt in (F32, F64)}
    g = torch.Generator().manual_seed(7000 + P)          # (the draws of E.one_hot_errors)
    X = E.rounded(g, P, E.ONE_HOT_D)
    t32 = 0.0
    for j in E.one_hot_rows(P):
        score = torch.zeros(P, E.ONE_HOT_D, dtype=F64)
        score[j] = 100.0 * E.rounded(g, E.ONE_HOT_D)
        t32 = max(t32, E.relerr(O.svgd_phi_closed_form(X.float(), score.float(), None)[0], O.svgd_phi_closed_form(X, score, None)[0]))
    case = 'one row P %d' % P
    say('%-14s rows %-22s ' % (case, E.one_hot_rows(P)) + account('(c) ' + case, 'phi', E.PHI_TOL[F32], h[F32][0], t32, h[F64][0]) + '  ' +
        account('(c) ' + case, 'particles', E.PHI_TOL[F32], h[F32][1], float('nan'), h[F64][1]))

say('\n(e) IMQ kernel: phi with the per-dimension median bandwidths, the bandwidths h, phi with a fixed bandwidth')
for P in E.E_COUNTS:
    for D in E.E_DIMS:
        X, score = E.imq_inputs(P, D)
        ref_m, ref_f = O.svgd_phi_imq_closed_form(X, score, 0.5, -0.5, None), O.svgd_phi_imq_closed_form(X, score, 0.5, -0.5, E.IMQ_FIXED_BW)
        t_m, t_f = (O.svgd_phi_imq_closed_form(X.float(), score.float(), 0.5, -0.5, b) for b in (None, E.IMQ_FIXED_BW))
        h = {dt: E.imq_errors(L, P, D, dt) for dt in (F32, F64)}
        case = 'P %d D %d' % (P, D)
        say('%-12s gap %.1e  ' % (case, E.imq_median_gap(X)) +
            account('(e) ' + case, 'imq phi', E.IMQ_PHI_TOL[F32], h[F32][0], E.relerr(t_m[0], ref_m[0]), h[F64][0]) + '  ' +
            account('(e) ' + case, 'imq h', E.IMQ_H_TOL[F32], h[F32][1], E.relerr(t_m[1], ref_m[1]), h[F64][1]) + '  ' +
            account('(e) ' + case, 'imq phi fixed', E.IMQ_PHI_TOL[F32], h[F32][2], E.relerr(t_f[0], ref_f[0]), h[F64][2]))

say('\nsummary: quantity: worst HIP fp32 (case) | worst HIP fp64 (case) | worst ratio HIP fp32 / max(torch32, bar / 10) (case)')
for q, w in sorted(worst.items()):
    say('%-14s %.2e (%s) | %.2e (%s) | %.2g (%s)' % (q, w[0][0], w[0][1], w[1][0], w[1][1], w[2][0], w[2][1]))

with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
