"""The LARGE-launch form of the fused per-particle MLP kernels (csrc/mlp_fused.hip), kernel by kernel, at the smallest shapes that reach
each variant.  Small launches -- ceil(R / 64) * P * nets <= 512 (fused_small) -- run 32-point tiles, four tiles per workgroup and one
backward round; everything larger runs 64-point tiles in the forward (and in the backward of 1-2 hidden layers), 8 / 16 / 32 tiles per
workgroup in the forward (fused_fwd_tpw) and a backward whose tiles per workgroup and slab count come from an occupancy query
(fused_chunks, fused_bwd_plan), one gradient slab per workgroup (1-2 hidden layers) or per wave.  Every test asks pacoh_mlp_fused_plan
(plan() of tests/test_dedup_host.py) first and ASSERTS the tile size and the tiles per workgroup it was written for: a retuned
threshold fails here instead of quietly testing the small form again.

Forward (part 1): a point's arithmetic does not depend on the tile size or on the tiles per workgroup (f_layer1, f_hidden, stage_tile:
the same MFMA / fmaf chain per 16-point block), so one large launch must give the BITS of the same tasks run in small launches of at
most 64 tasks.  No tolerance.  The outputs are prefilled with NaN: a row that no tile writes cannot pass on stale memory.

Backward (part 2): against O.mlp_vectorized_forward in fp64 on the CPU (autograd) from the same fp32-rounded theta, x and upstream
gradients, per PARAMETER BLOCK (each layer's bias and weight) of each particle and network,
    err = ||h - r|| / max(||r||, 1e-3 ||gradient of that particle and network||)   <=   max(F * err_torch32, FLOOR),
err_torch32 being the same block of the same expression in fp32 on the CPU, the worst over NORD orders of the rows (the method of
tests/test_gpu_fp32_accuracy.py), and relerr < 2e-4 over the whole gradient besides.  The upstream gradient is dense, or zero except on
rows chosen from the launch's plan (the ends, the first tile boundary, the first and the last workgroup boundary, every row of a
partial last tile): there a row lost or counted twice is an O(1) error.  The slab workspace is prefilled with NaN patterns: a slab that
no workgroup writes shows.  The measured errors: profiles/mlp_large_fp32_errors.txt (tests/mlp_large_fp32_errors.py, which shares
bwd_cases() / measure_bwd() below)."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dedup_host import plan                                   # noqa: E402

from oracle import pacoh_oracle as O                               # noqa: E402

gpu = pytest.mark.gpu
DEV = 'cuda'
F64 = torch.float64
NORD = 3                               # orders of a particle's rows torch fp32 is evaluated in (the first: as given)
GLOBAL_BAR = 2e-4                      # the suite's bar on the whole gradient (tests/test_gpu_kernels.py): holds here too
# Per-block bars: the F = 10 and floor 2e-5 of tests/test_gpu_matern.py, which hold as they are.  Measured (profiles/mlp_large_fp32_errors.txt,
# tests/mlp_large_fp32_errors.py on an MI355X; the searched shapes were T = 385 at 768 resident workgroups and T = 129 at 512): worst
# HIP error of a block 1.37e-6 (wave_slab sparse, mlp2_bwd_hyper+stash, kernel network, particle 0, fc_1.weight; torch fp32 there 1.07e-6),
# which is also the worst ratio err_hip / max(err_torch32, FLOOR / F) = 0.68; no block beyond 10x torch fp32; worst error over a whole
# gradient 8.1e-7.  The kernels' tanh (v_exp / v_rcp, csrc/mlp_act.h) costs nothing against torch's at this level.
F = 10.0
FLOOR = 2e-5


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


def net_params(d_in, hidden, d_out):
    return sum(O.nn_param_layout(d_in, d_out, hidden).values())


def block_spans(d_in, hidden, d_out):
    """[(name, first column, end column)] of a network's parameter blocks inside its block of a theta row"""
    spans, at = [], 0
    for name, size in O.nn_param_layout(d_in, d_out, hidden).items():
        spans.append((name, at, at + size))
        at += size
    return spans


class Shape:
    """one launch shape and its seeded inputs (CPU, fp32, never modified): theta rows with the mean network (d_out 1) at column 3, the
    kernel-feature network (d_out 2) two columns behind it, then two lengthscale and one noise column and two more (odd offsets: no
    16-byte alignment, and pad columns on every side that a launch must leave alone); b = t * P + p"""

    def __init__(self, T, n=64, d_in=4, hidden=(32, 32), P=4, nets=2, shared=True):
        self.T, self.n, self.d_in, self.hidden, self.P, self.nets, self.shared = T, n, d_in, tuple(hidden), P, nets, shared
        self.B, self.R = T * P, T * n
        self.Dm, self.Dk = net_params(d_in, hidden, 1), net_params(d_in, hidden, 2)
        self.off_m = 3
        self.off_k = self.off_m + self.Dm + 2
        self.off_h = self.off_k + self.Dk
        self.D = self.off_h + 3 + 2
        g = torch.Generator().manual_seed(100000 * len(hidden) + 100 * T + n + d_in + P)
        self.theta = 0.5 * torch.randn(P, self.D, generator=g)
        self.x = torch.randn(T if shared else self.B, n, d_in, generator=g)
        self.g_dense = [torch.randn(self.B, n, 1, generator=g), torch.randn(self.B, n, 2, generator=g)]
        self.d_ls = torch.randn(T, P, 2, generator=g)
        self.d_nz = torch.randn(T, P, generator=g)
        self._dev = None

    @property
    def x_div(self):
        return self.P if self.shared else 1

    def block(self, k):
        """(first column, d_out, parameters) of network k of this shape's calls: two networks -> the mean and the
        kernel-feature network; ONE network -> the kernel-feature network through the single-network entry points"""
        if self.nets == 1 or k == 1:
            return self.off_k, 2, self.Dk
        return self.off_m, 1, self.Dm

    def net_cols(self):
        cols = torch.zeros(self.D, dtype=torch.bool)
        for k in range(self.nets):
            off, _, Dn = self.block(k)
            cols[off:off + Dn] = True
        return cols

    def dev(self):
        if self._dev is None:
            self._dev = dict(theta=self.theta.to(DEV), x=self.x.to(DEV), d_ls=self.d_ls.to(DEV), d_nz=self.d_nz.to(DEV))
        return self._dev

    def rows(self, t):
        """[B, n, w] -> [P, R, w]: the rows of every particle, tasks one after the other"""
        return t.reshape(self.T, self.P, self.n, -1).permute(1, 0, 2, 3).reshape(self.P, self.R, -1)

    def rows_x(self):
        """the inputs of every particle's rows [P, R, d_in]"""
        return self.x.reshape(1, self.R, -1).expand(self.P, self.R, self.d_in) if self.shared else self.rows(self.x)

    def upstream(self, kind, bwd_plan):
        """the upstream gradients of the shape's networks: 'dense', or 'sparse' -- zero except on sparse_rows() of every particle"""
        gs = self.g_dense if self.nets == 2 else self.g_dense[1:]
        if kind == 'dense':
            return gs
        keep = torch.zeros(self.R, dtype=torch.bool)
        keep[sparse_rows(self.R, *bwd_plan)] = True
        keep = keep.reshape(self.T, 1, self.n, 1)
        return [torch.where(keep, g.reshape(self.T, self.P, self.n, -1), torch.zeros(())).reshape(g.shape) for g in gs]


def sparse_rows(R, tp, wgs, tpw):
    """rows of a particle where a tile loop or a slab sum goes wrong first, from the backward plan of the launch (tile points,
    workgroups per particle and network, tiles per workgroup): rows 0 and R - 1, the last row of the first tile and the first of the
    second, the rows on either side of the first workgroup boundary and of the first tile of the last workgroup that has tiles, and
    every row of a partial last tile"""
    tiles = -(-R // tp)
    w_last = (tiles - 1) // tpw
    rows = {0, R - 1, tp - 1, tp, tpw * tp - 1, tpw * tp, w_last * tpw * tp - 1, w_last * tpw * tp}
    if R % tp:
        rows |= set(range((tiles - 1) * tp, R))
    return sorted(r for r in rows if 0 <= r < R)


@functools.lru_cache(maxsize=None)
def shape(*args, **kw):
    return Shape(*args, **kw)


def is_fused(L, q):
    return all(L.mlp_fused_path(q.B, q.P, q.n, q.d_in, list(q.hidden), q.block(k)[1], torch.float32) for k in range(q.nets))


# ---------------------------------------------------------------------------------------------------------------------- forward launches
def fwd(L, q, lo=0, hi=None, stash=None, active=None):
    """pacoh_mlp2_fwd[_active] (two networks) or pacoh_mlp_fwd (one) on the tasks [lo, hi) of shape q, into outputs prefilled with NaN
    -> the list of the networks' outputs [(hi - lo) * P, n, d_out]"""
    hi = q.T if hi is None else hi
    lib, d = L.load_library(), q.dev()
    P, n, B = q.P, q.n, (hi - lo) * q.P
    x = d['x'][lo:hi] if q.shared else d['x'][lo * P:hi * P]
    harr, nh = L._hidden_arr(q.hidden), len(q.hidden)
    outs = [torch.full((B, n, q.block(k)[1]), float('nan'), device=DEV) for k in range(q.nets)]
    if q.nets == 2:
        assert lib.pacoh_mlp2_fwd_workspace_bytes(B, P, n, q.d_in, harr, nh, 1, 2, L.F32) == 0
        L._check(L._active_call(lib, 'pacoh_mlp2_fwd', L._active_tasks(active), L._ptr(x), q.x_div, L._ptr(d['theta']), q.D, P, q.d_in,
                                harr, nh, q.off_m, 1, L._ptr(outs[0]), q.off_k, 2, L._ptr(outs[1]), None, L._ptr(stash), B, n, L.F32,
                                L._stream()), 'pacoh_mlp2_fwd')
    else:
        assert stash is None and active is None
        assert lib.pacoh_mlp_fwd_workspace_bytes(B, P, n, q.d_in, harr, nh, 2, L.F32) == 0
        th = d['theta'][:, q.off_k:]
        L._check(lib.pacoh_mlp_fwd(L._ptr(x), q.x_div, ctypes.c_void_p(th.data_ptr()), q.D, P, q.d_in, harr, nh, 2, L._ptr(outs[0]), None, B, n, L.F32,
                                   L._stream()), 'pacoh_mlp_fwd')
    return outs


def fwd_in_small_launches(L, q, sub=64):
    """the same tasks in launches of at most `sub` tasks, each of them a small launch (32-point tiles, 4 per workgroup): the query says so"""
    lib = L.load_library()
    parts = []
    for lo in range(0, q.T, sub):
        hi = min(q.T, lo + sub)
        tp, _, tpw = plan(lib, (hi - lo) * q.n, q.P, q.nets, len(q.hidden), 0, 0)
        assert (tp, tpw) == (32, 4), (lo, hi, tp, tpw)
        parts.append(fwd(L, q, lo, hi))
    return [torch.cat([p[k] for p in parts]) for k in range(q.nets)]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_fwd_plan(L, q, expect):
    assert is_fused(L, q)
    tp, wgs, tpw = plan(L.load_library(), q.R, q.P, q.nets, len(q.hidden), 0, 0)
    assert (tp, tpw) == expect, 'forward plan of R = %d: %d-point tiles, %d per workgroup; this case was written for %s' % (q.R, tp, tpw, expect)
    return tp, wgs, tpw


# the table of the issue (confirmed by the query: test_forward_table_holds_the_smallest_task_counts), then T = 129 in other
# networks and input layouts, then ragged ends: R mod 64 = 63, 49 (n = 63, 49 at T = 129) and 1, 15, 16, 17 (n = 63) -- a particle's rows
# end inside a 64-point tile, inside its first 16-point block, at its end and one row into the second
FWD_TABLE = [(64, (32, 4)), (65, (64, 4)), (129, (64, 8)), (257, (64, 16)), (769, (64, 32))]
FWD_CASES = [dict(T=T, expect=e) for T, e in FWD_TABLE] + [
    dict(T=129, hidden=(32,), expect=(64, 8)),
    dict(T=129, hidden=(24, 31), expect=(64, 8)),
    dict(T=129, hidden=(32, 32, 32), expect=(64, 8)),
    dict(T=129, d_in=1, expect=(64, 8)),
    dict(T=129, shared=False, expect=(64, 8)),
    dict(T=129, n=63, expect=(64, 4), rmod=63),
    dict(T=129, n=49, expect=(64, 4), rmod=49),
    dict(T=191, n=63, expect=(64, 8), rmod=1),
    dict(T=177, n=63, expect=(64, 8), rmod=15),
    dict(T=176, n=63, expect=(64, 8), rmod=16),
    dict(T=175, n=63, expect=(64, 8), rmod=17),
    dict(T=103, P=5, nets=1, expect=(64, 4)),            # ONE network crossing the boundary on its own: 103 * 5 = 515 > 512
]


def _fwd_id(c):
    return '-'.join('%s%s' % (k, ''.join(str(v).split())) for k, v in c.items() if k not in ('expect', 'rmod')) + '-tp%d-tpw%d' % c['expect']


def test_forward_table_holds_the_smallest_task_counts():
    """(no GPU: the forward plan does not depend on the device) each T of FWD_TABLE is the smallest task count at which n = 64, P = 4, two
    networks run that tile size and that many tiles per workgroup"""
    from meta_learning_pacoh_amd import _lib
    lib = _lib.load_library()
    first = {}
    for T in range(1, 1025):
        tp, _, tpw = plan(lib, T * 64, 4, 2, 2, 0, 0)
        first.setdefault((tp, tpw), T)
    assert first[(32, 4)] == 1 and plan(lib, 64 * 64, 4, 2, 2, 0, 0)[::2] == (32, 4)
    assert [(first[e], e) for _, e in FWD_TABLE[1:]] == FWD_TABLE[1:]
    assert plan(lib, 102 * 64, 5, 1, 2, 0, 0)[0] == 32 and plan(lib, 103 * 64, 5, 1, 2, 0, 0)[0] == 64


@gpu
@pytest.mark.parametrize('case', FWD_CASES, ids=_fwd_id)
def test_forward_large_launch_equals_small_launches_bit_for_bit(L, case):
    kw = {k: v for k, v in case.items() if k not in ('expect', 'rmod')}
    q = shape(**kw)
    assert_fwd_plan(L, q, case['expect'])
    if 'rmod' in case:
        assert q.R % 64 == case['rmod']
    small = fwd_in_small_launches(L, q, 40 if q.T == 64 else 64)
    large = fwd(L, q)
    for k in range(q.nets):
        assert bool(torch.isfinite(large[k]).all()), 'network %d: rows left unwritten or not finite' % k
        diff = (large[k].view(torch.int32) != small[k].view(torch.int32)).reshape(q.T, q.P, q.n, -1).any(-1)
        assert same_bits(large[k], small[k]), 'network %d: first differing (task, particle, point): %s' % (k, diff.nonzero()[:4].tolist())


@gpu
@pytest.mark.parametrize('T,expect', [(65, (64, 4)), (129, (64, 8))])
def test_forward_with_stash_keeps_the_bits_and_feeds_the_backward(L, T, expect):
    """a stash full of NaN patterns handed to the large forward: the same output bits, and the backward that reads it back (every block it
    reads must have been written) gives finite gradients -- their accuracy: test_backward_blocks_against_fp64, entries `+stash`"""
    q = shape(T)
    assert_fwd_plan(L, q, expect)
    plain = fwd(L, q)
    stash = L.mlp2_stash(q.dev()['x'], q.P, q.d_in, list(q.hidden), 1, 2, q.B, q.n)
    assert stash is not None
    stash.fill_(0xff)
    kept = fwd(L, q, stash=stash)
    assert all(bool(torch.isfinite(o).all()) for o in plain)
    assert same_bits(kept[0], plain[0]) and same_bits(kept[1], plain[1])
    gs = [g.to(DEV) for g in q.g_dense]
    grad = bwd(L, q, 'mlp2_bwd', gs, stash=stash)
    assert bool(torch.isfinite(grad).all())


@gpu
def test_forward_live_tasks_on_the_16_tile_launch(L):
    """pacoh_mlp2_fwd_active on the T = 257 launch (16 tiles per workgroup, re-split on the device: mlp_fused_split.h): n_act = T gives
    the bits of the plain call; fewer live tasks give the plain call's rows for those tasks and leave every other row alone"""
    q = shape(257)
    assert_fwd_plan(L, q, (64, 16))
    plain = fwd(L, q)
    assert all(same_bits(a, b) for a, b in zip(plain, fwd_in_small_launches(L, q)))
    w = torch.ones(q.T, device=DEV)
    for n_act in (q.T, 1, 130, 256):
        live = fwd(L, q, active=(torch.tensor([n_act], dtype=torch.int32, device=DEV), w))
        for k in range(2):
            assert same_bits(live[k][:n_act * q.P], plain[k][:n_act * q.P]), (n_act, k)
            assert bool(torch.isnan(live[k][n_act * q.P:]).all()), (n_act, k)


# ---------------------------------------------------------------------------------------------------------------------- backward launches
def nan_workspace(L, q):
    """the slab workspace of the shape's backward, every byte 0xff"""
    lib, harr, nh = L.load_library(), L._hidden_arr(q.hidden), len(q.hidden)
    if q.nets == 2:
        need = lib.pacoh_mlp2_bwd_workspace_bytes(q.B, q.P, q.n, q.d_in, harr, nh, 1, 2, L.F32)
    else:
        need = lib.pacoh_mlp_bwd_workspace_bytes(q.B, q.P, q.n, q.d_in, harr, nh, 2, L.F32)
    assert need > 0
    return torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)


def bwd(L, q, entry, gs, prefill=7.0, accumulate=False, stash=None, active=None):
    """one backward launch of shape q -> d_theta[P, D] (prefilled).  entry: mlp2_bwd | mlp2_bwd_hyper (two networks), mlp_bwd (one)"""
    d = q.dev()
    grad = torch.full((q.P, q.D), prefill, device=DEV)
    ws = nan_workspace(L, q)
    hid = list(q.hidden)
    if entry == 'mlp2_bwd':
        L.mlp2_bwd(d['x'], q.x_div, d['theta'], q.P, q.d_in, hid, q.off_m, 1, gs[0], q.off_k, 2, gs[1], grad, accumulate, q.B, q.n,
                   workspace=ws, stash=stash)
    elif entry == 'mlp2_bwd_hyper':
        assert not accumulate
        L.mlp2_bwd_hyper(d['x'], q.x_div, d['theta'], q.P, q.d_in, hid, q.off_m, 1, gs[0], q.off_k, 2, gs[1], grad, q.B, q.n, q.T,
                         q.off_h, 2, -1, q.off_h + 2, -1, d['d_ls'], None, d['d_nz'], None, workspace=ws, stash=stash, active=active)
    else:
        assert entry == 'mlp_bwd' and q.nets == 1 and stash is None and active is None
        L.mlp_bwd(d['x'], q.x_div, d['theta'][:, q.off_k:], q.D, q.P, q.d_in, hid, 2, gs[0], grad[:, q.off_k:], q.D, accumulate, q.B, q.n,
                  workspace=ws)
    return grad


def filled_stash(L, q, active=None):
    """the activation stash as the forward of the same step leaves it (NaN patterns wherever the forward wrote nothing)"""
    stash = L.mlp2_stash(q.dev()['x'], q.P, q.d_in, list(q.hidden), 1, 2, q.B, q.n)
    assert stash is not None
    stash.fill_(0xff)
    fwd(L, q, stash=stash, active=active)
    return stash


def oracle_grads(q, gs, dtype, order=0, live_tasks=None):
    """the networks' gradient blocks [P, D_net] of sum(out * g) through O.mlp_vectorized_forward in `dtype` on the CPU (autograd), the
    rows of every particle in order `order` (0: as given); live_tasks: the sums run over the first live_tasks tasks only"""
    R = q.R if live_tasks is None else live_tasks * q.n
    perm = torch.arange(R) if order == 0 else torch.randperm(R, generator=torch.Generator().manual_seed(977 * order + R))
    xp = q.rows_x()[:, :R][:, perm].to(dtype)
    out = []
    for k, g in enumerate(gs):
        off, d_out, Dn = q.block(k)
        th = q.theta[:, off:off + Dn].to(dtype).clone().requires_grad_(True)
        y = O.mlp_vectorized_forward(xp, th, q.d_in, d_out, q.hidden)
        (y * q.rows(g)[:, :R][:, perm].to(dtype)).sum().backward()
        out.append(th.grad.double())
    return out


def block_errors(q, k, h, r):
    """[P, blocks] per-block error of network k's gradient h [P, D_net] against the fp64 r"""
    full = r.norm(dim=1)
    cols = []
    for _, lo, hi in block_spans(q.d_in, q.hidden, q.block(k)[1]):
        den = torch.maximum(r[:, lo:hi].norm(dim=1), 1e-3 * full)
        cols.append((h[:, lo:hi].double() - r[:, lo:hi]).norm(dim=1) / den)
    return torch.stack(cols, 1)


class Reference:
    """fp64 gradients of one (shape, upstream gradients, live tasks) and the per-block error of torch fp32 on them, worst of NORD orders"""

    def __init__(self, q, gs, live_tasks=None):
        self.q = q
        self.ref = oracle_grads(q, gs, F64, 0, live_tasks)
        assert all(float(r.norm(dim=1).min()) > 0 for r in self.ref)
        c32 = [oracle_grads(q, gs, torch.float32, order, live_tasks) for order in range(NORD)]
        self.err32 = [torch.stack([block_errors(q, k, c[k], self.ref[k]) for c in c32]).max(0).values for k in range(len(gs))]
        T = q.T if live_tasks is None else live_tasks
        sig = torch.sigmoid(q.theta[:, q.off_h:q.off_h + 3].double())
        self.hyper = torch.cat([q.d_ls[:T].double().sum(0), q.d_nz[:T].double().sum(0).unsqueeze(1)], 1) * sig

    def errors(self, grad):
        """-> [(network, err_hip [P, blocks], err_torch32 [P, blocks])], global relerr of d_theta[P, D] from a launch"""
        q, g = self.q, grad.detach().cpu()
        rows = []
        num = den = 0.0
        for k, r in enumerate(self.ref):
            off, _, Dn = q.block(k)
            h = g[:, off:off + Dn]
            rows.append((k, block_errors(q, k, h, r), self.err32[k]))
            num += float((h.double() - r).norm() ** 2)
            den += float(r.norm() ** 2)
        return rows, (num / den) ** 0.5


def check_blocks(q, refc, grad, tag):
    """the per-block bars and the global one; prints the worst figures first"""
    assert bool(torch.isfinite(grad).all()), '%s: not finite (a slab or a stash block read before it was written?)' % (tag,)
    rows, glob = refc.errors(grad)
    bad, worst = [], (0.0, '')
    for k, eh, ec in rows:
        names = [s[0] for s in block_spans(q.d_in, q.hidden, q.block(k)[1])]
        bar = torch.clamp_min(F * ec, FLOOR)
        ratio = eh / torch.clamp_min(ec, FLOOR / F)
        i = int(ratio.argmax())
        p, j = divmod(i, len(names))
        if float(ratio.max()) > worst[0]:
            worst = (float(ratio.max()), 'network %d particle %d %s: hip %.2e torch32 %.2e' % (k, p, names[j], eh[p, j], ec[p, j]))
        for p, j in (eh > bar).nonzero().tolist():
            bad.append('network %d particle %d %s: hip %.2e torch32 %.2e bar %.2e' % (k, p, names[j], eh[p, j], ec[p, j], bar[p, j]))
    print('%s: whole gradient %.2e | worst ratio hip / max(torch32, FLOOR / F) %.2f (%s)' % (tag, glob, *worst))
    assert not bad, '%s\n  ' % (tag,) + '\n  '.join(bad[:20])
    assert glob < GLOBAL_BAR, (tag, glob)


def check_outside(q, grad, prefill, tag, hyper=None):
    """columns outside the network blocks: as prefilled (the hyper-parameter columns of a *_hyper launch: their reduced gradient)"""
    g = grad.detach().cpu()
    outside = ~q.net_cols()
    if hyper is not None:
        outside[q.off_h:q.off_h + 3] = False
        h = g[:, q.off_h:q.off_h + 3].double()
        assert float((h - hyper).norm() / hyper.norm()) < GLOBAL_BAR, tag
    assert bool((g[:, outside] == prefill).all()), '%s: a column outside the network blocks was written' % (tag,)


@functools.lru_cache(maxsize=None)
def searched_T(P, nets, n_hidden):
    """the smallest T in 65 .. 1024 (n = 64) whose backward plan ON THIS DEVICE (resident = 0: the occupancy query) gives a
    workgroup more than four tiles, i.e. a wave more than one"""
    from meta_learning_pacoh_amd import _lib
    lib = _lib.load_library()
    for T in range(65, 1025):
        tp, wgs, tpw = plan(lib, T * 64, P, nets, n_hidden, 1, 0)
        if tpw > 4:
            return T
    raise AssertionError('no T in 65 .. 1024 gives the backward of %d particles, %d network(s), %d hidden layers more than 4 tiles per workgroup'
                         % (P, nets, n_hidden))


# name -> (Shape arguments (T = None: searched_T), tile points, more than 4 tiles per workgroup required)
BWD_SHAPES = {
    'first64': (dict(T=65), 64, False),                                   # the first 64-point-tile launch of two networks
    'wg_slab': (dict(T=None), 64, True),                                  # 64-point tiles, several tiles per wave, a slab per workgroup
    'wave_slab': (dict(T=None, hidden=(32, 32, 32, 32)), 32, True),       # 32-point tiles, several tiles per wave, a slab per wave
    'ragged': (dict(T=97, n=49), 64, False),                              # R = 4753 = 74 * 64 + 17: one row in the last tile's second block
    'one_first64': (dict(T=65, P=8, nets=1), 64, False),                  # pacoh_mlp_bwd: ONE network (8 particles), as the first two
    'one_wg_slab': (dict(T=None, P=8, nets=1), 64, True),
}
ENTRIES = {2: ['mlp2_bwd', 'mlp2_bwd+stash', 'mlp2_bwd_hyper', 'mlp2_bwd_hyper+stash'], 1: ['mlp_bwd']}


def bwd_shape(L, name):
    """-> (Shape, its backward plan on this device), the variant the case was written for asserted"""
    kw, tp_want, many = BWD_SHAPES[name]
    kw = dict(kw)
    if kw['T'] is None:
        kw['T'] = searched_T(kw.get('P', 4), kw.get('nets', 2), len(kw.get('hidden', (32, 32))))
    q = shape(**kw)
    assert is_fused(L, q)
    lib = L.load_library()
    tp, wgs, tpw = plan(lib, q.R, q.P, q.nets, len(q.hidden), 1, 0)
    assert tp == tp_want, '%s: backward plan of R = %d has %d-point tiles, written for %d' % (name, q.R, tp, tp_want)
    assert wgs >= 2 and (tpw > 4 or not many), (name, tp, wgs, tpw)
    assert plan(lib, q.R, q.P, q.nets, len(q.hidden), 0, 0)[0] == 64              # (the forward that fills the stash: a large launch too)
    if name == 'ragged':
        assert q.R % 64 == 17
    return q, (tp, wgs, tpw)


def bwd_cases():
    return [(name, up) for name in BWD_SHAPES for up in ('dense', 'sparse')]


def measure_bwd(L, name, up):
    """run every entry point of one case -> (Shape, plan, Reference, {entry: d_theta[P, D]}); prefill 7.0"""
    q, pl = bwd_shape(L, name)
    gs_cpu = q.upstream(up, pl)
    refc = Reference(q, gs_cpu)
    gs = [g.to(DEV) for g in gs_cpu]
    grads = {}
    for entry in ENTRIES[q.nets]:
        base, _, st = entry.partition('+')
        grads[entry] = bwd(L, q, base, gs, stash=filled_stash(L, q) if st else None)
    return q, pl, refc, grads


@gpu
@pytest.mark.parametrize('name,up', bwd_cases(), ids=['%s-%s' % c for c in bwd_cases()])
def test_backward_blocks_against_fp64(L, name, up):
    q, pl, refc, grads = measure_bwd(L, name, up)
    print('%s %s: T %d R %d, %d-point tiles, %d workgroups of %d tiles; %d live rows' % (
        name, up, q.T, q.R, *pl, q.R if up == 'dense' else len(sparse_rows(q.R, *pl))))
    for entry, grad in grads.items():
        check_blocks(q, refc, grad, (name, up, entry))
        check_outside(q, grad, 7.0, (name, up, entry), refc.hyper if 'hyper' in entry else None)
    # two identical launches: the same bits (slabs are summed in a fixed order); accumulate adds exactly that sum onto what is there
    gs = [g.to(DEV) for g in q.upstream(up, pl)]
    first = 'mlp2_bwd' if q.nets == 2 else 'mlp_bwd'
    again = bwd(L, q, first, gs)
    assert torch.equal(again, grads[first]), 'two identical launches differ'
    acc = bwd(L, q, first, gs, prefill=1.0, accumulate=True)
    cols = q.net_cols().to(DEV)
    assert torch.equal(acc[:, cols], 1.0 + grads[first][:, cols]) and bool((acc[:, ~cols] == 1.0).all())


def live_shape(L):
    """the larger of the two searched two-network shapes"""
    return max(('wg_slab', 'wave_slab'), key=lambda s: bwd_shape(L, s)[0].T)


def _active(q, n_act):
    return torch.tensor([n_act], dtype=torch.int32, device=DEV), torch.ones(q.T, device=DEV)


def measure_live(L, n_act):
    """pacoh_mlp2_bwd_hyper_active with n_act live tasks, without and with the stash -> (Shape, Reference over the live tasks, {entry: d_theta})"""
    q, pl = bwd_shape(L, live_shape(L))
    gs_cpu = q.upstream('dense', pl)
    gs = [g.to(DEV) for g in gs_cpu]
    refc = Reference(q, gs_cpu, live_tasks=n_act)
    act = _active(q, n_act)
    return q, refc, {'mlp2_bwd_hyper': bwd(L, q, 'mlp2_bwd_hyper', gs, active=act),
                     'mlp2_bwd_hyper+stash': bwd(L, q, 'mlp2_bwd_hyper', gs, active=act, stash=filled_stash(L, q, act))}


@gpu
@pytest.mark.parametrize('part', ['all', 'one', 'half'])
def test_backward_hyper_live_tasks_on_the_larger_searched_shape(L, part):
    """pacoh_mlp2_bwd_hyper_active: n_act = T gives the bits of the plain call; fewer live tasks match fp64 over the live tasks only -- the
    tiles are dealt out again over the launch's workgroups, and those left without tiles must add exact zeros"""
    name = live_shape(L)
    q, pl = bwd_shape(L, name)
    if part == 'all':
        gs = [g.to(DEV) for g in q.upstream('dense', pl)]
        assert torch.equal(bwd(L, q, 'mlp2_bwd_hyper', gs, active=_active(q, q.T)), bwd(L, q, 'mlp2_bwd_hyper', gs))
        return
    n_act = 1 if part == 'one' else q.T // 2
    q, refc, grads = measure_live(L, n_act)
    for entry, grad in grads.items():
        tag = (name, 'n_act %d of %d' % (n_act, q.T), entry)
        check_blocks(q, refc, grad, tag)
        check_outside(q, grad, 7.0, tag, refc.hyper)
