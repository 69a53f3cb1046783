"""time and peak memory of the fused per-draw argmax over a candidate pool:  python tools/path_argmax_time.py [out] [--repeats K]

Setup as tools/path_time.py: fp32, 4 x 32 mean and feature networks (feature_dim 2), d = 1, after 3 meta-iterations; a MAP row (P = 1)
and PACOH-SVGD with P = 20 particles; context n = 128, D = 1024 random features, S = 16 draws per row; m in {2048, 10^4, 10^5}
candidates.  Per shape two ways to each draw's best candidate:
  fused    paths.argmax(candidates)                     (per chunk of 131 072: the network forwards + one pacoh_gp_path_argmax)
  dense    paths(candidates) followed by torch.max(dim=1)   (what there was before: the [P * 16, m] tensor, then a second pass over it)
and one more row, fused only, at P = 20, m = 10^6 (eight chunks; the dense way would hold 1.28 GB).
Figures in us per call: CALL, the wall clock around the public call(s), synchronised; GP, the HIP-event time that _lib.PROFILE
records around the pacoh_gp_path_argmax (both of its launches, summed over the chunks) / pacoh_gp_path_eval call alone (a separate
pass; torch.max is not in it).  PEAK: the rise of torch's allocator peak during one call.  After a warm-up of every side, the sides
ALTERNATE in the same process; reported: the median of K repeats of `reps` calls and the min .. max spread.  The two ways are also
compared: the same indices, the same values.  No ratio is fixed in advance: the table records what was measured.  It is written to
`out` (default profiles/path_argmax_time.txt)."""
import argparse
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
from path_time import D_FEAT, MS, N_CTX, S_DRAWS, fmt, measure, tasks  # noqa: E402

BIG_M = 1000000


def peak_rise(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'path_argmax_time.txt'))
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('path_argmax_time.py needs a HIP device: nothing is measured without one')
    L.load_library()
    lines = ['# measured on an AMD Instinct MI355X (%s)' % torch.cuda.get_device_name(0),
             '# each draw\'s best candidate of a pool (python tools/path_argmax_time.py): fp32, 4 x 32 networks, n = %d context points,'
             % N_CTX,
             '# D = %d random features, S = %d draws per parameter row.  us per call, median of %d alternating repeats [min .. max].'
             % (D_FEAT, S_DRAWS, a.repeats),
             '# fused = paths.argmax(candidates); dense = paths(candidates) then torch.max(dim=1).  call = wall clock of the public call(s),',
             '# synchronised; gp = HIP events around pacoh_gp_path_argmax (both launches, all chunks) / pacoh_gp_path_eval alone (torch.max',
             '# is not in it); peak = rise of the allocator\'s peak during one call.']
    rs = np.random.RandomState(0)
    kw = dict(num_iter_fit=3, feature_dim=2, mean_nn_layers=(32, 32, 32, 32), kernel_nn_layers=(32, 32, 32, 32), task_batch_size=4)
    models = (('map', 1, M.GPRegressionMetaLearned(tasks(rs), random_seed=1, **kw)),
              ('svgd', 20, M.GPRegressionMetaLearnedSVGD(tasks(rs), num_particles=20, random_seed=20, **kw)))
    cx = rs.uniform(-3, 3, size=(N_CTX, 1))
    cy = np.sin(cx) + 0.1 * rs.randn(N_CTX, 1)
    for name, P, model in models:
        model.meta_fit(verbose=False, log_period=1000)
        cond = model.condition(cx, cy)
        for m in MS + ((BIG_M,) if P == 20 else ()):
            tx = rs.uniform(-3.5, 3.5, size=(m, 1))
            torch.manual_seed(m)
            paths = cond.sample_paths(S_DRAWS, D_FEAT)
            fused = lambda: paths.argmax(tx)
            dense = lambda: torch.max(paths(tx), dim=1)
            idx, val = fused()
            assert tuple(idx.shape) == (P * S_DRAWS,) and bool(((idx >= 0) & (idx < m)).all()) and bool(torch.isfinite(val).all())
            sides = [(fused, 'gp_path_argmax')]
            if m != BIG_M:
                top = dense()
                assert torch.equal(top.values, val)                     # the same values; the same indices wherever the maximum is single
                single = (paths(tx) == top.values.unsqueeze(1)).sum(1) == 1
                assert torch.equal(top.indices[single], idx[single])
                sides.append((dense, 'gp_path_eval'))
            peaks = [peak_rise(run) for run, _ in sides]
            reps, res = measure(sides, a.repeats)
            lines.append('%-4s P=%2d m=%7d reps=%3d' % (name, P, m, reps))
            lines.append('    fused    call %s | gp %s | peak %10.2f MB' % (fmt(res[0][0]), fmt(res[0][1]), peaks[0] / 1e6))
            if m != BIG_M:
                lines.append('    dense    call %s | gp %s | peak %10.2f MB' % (fmt(res[1][0]), fmt(res[1][1]), peaks[1] / 1e6))
                lines.append('    fused / dense: call %.2f, gp %.2f, peak %.3f'
                             % (statistics.median(res[0][0]) / statistics.median(res[1][0]),
                                statistics.median(res[0][1]) / statistics.median(res[1][1]), peaks[0] / max(1, peaks[1])))
            else:
                lines.append('    dense    not run at this m: paths(candidates) alone is %.2f GB' % (P * S_DRAWS * m * 4 / 1e9))
            for ln in lines[-(4 if m != BIG_M else 3):]:
                print(ln)
            sys.stdout.flush()
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
