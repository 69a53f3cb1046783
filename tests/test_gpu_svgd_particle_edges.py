"""The SVGD step-tail kernels along ONE axis, the particle count P, at the counts where they select code: the register bitonic
sort behind the median bandwidth (`wave_median_full_matrix<T, VPL>`, csrc/step_tail.h: VPL = 4 for P <= 23, 8 for 24 .. 32, 16 for
33 .. 45, 32 for 46 .. 64), the bisection kernel beyond 64, the particle loop of `svgd_update_kernel` (a 20-particle prefetch, rounds
of 10, rounds of 4, a remainder) and the two per-dimension median kernels of the IMQ particle kernel (P <= 32 in registers, 33 and
beyond from LDS).  Everything is compared with numpy / the CPU oracle in fp64; the bars are the project's own for these quantities
(tests/test_gpu_kernels.py: test_svgd_update_fused, test_svgd_many_particles, test_svgd_phi_imq_*), the measured errors beside plain
torch fp32 on the CPU are in profiles/svgd_particle_edges_errors.txt (python tests/svgd_particle_edges_errors.py).

Every random input is drawn in fp64 and rounded to fp32 once, so that both dtypes and the fp64 reference see the same numbers."""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacoh_oracle as O


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from meta_learning_pacoh_amd import _lib
    _lib.load_library()
    return _lib


DEV = 'cuda'
DTYPES = [torch.float32, torch.float64]
BW_TOL = {torch.float32: 1e-5, torch.float64: 1e-12}        # the median bandwidth (test_svgd_many_particles)
PHI_TOL = {torch.float32: 2e-4, torch.float64: 1e-10}       # phi and the updated particles (test_svgd_update_fused, test_svgd_many_particles)
IMQ_PHI_TOL = {torch.float32: 5e-5, torch.float64: 1e-11}   # (test_svgd_phi_imq_beyond_64_particles_matches_reference_fixture)
IMQ_H_TOL = {torch.float32: 1e-6, torch.float64: 1e-14}     # (test_svgd_phi_imq_matches_reference_fixture)


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def bw_err(bw, bw_o):
    """relative error of a bandwidth (absolute where the expected one is exactly 0)"""
    return abs(float(bw) - float(bw_o)) / (float(bw_o) if float(bw_o) > 0 else 1.0)


def dev(t, dtype):
    return t.to(dtype).to(DEV).contiguous()


def rounded(g, *shape):
    """standard normal, fp64 holding fp32-representable values"""
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()


def direct_d2(X):
    """the full P x P matrix of squared distances in fp64, from differences (the kernels' form; the oracle's own matmul form rounds
    at |x|^2, which the separation argument of the line inputs below cannot afford)"""
    Xn = X.detach().double().cpu().numpy()
    df = Xn[:, None, :] - Xn[None, :, :]
    return (df * df).sum(-1)


def median_bandwidth(X):
    """sqrt(numpy.median(full matrix) / (2 ln(P + 1))) in fp64"""
    return O.svgd_bandwidth(torch.from_numpy(direct_d2(X)))


# ------------------------------------------------------------------------------------------ (a) the median is the right order statistic
A_COUNTS = [1, 2, 3, 22, 23, 24, 32, 33, 45, 46, 50, 63, 64, 65, 66]
SIDON_Q, SIDON_S = 67, 6                                     # prime > every P of A_COUNTS; coordinates in 1/64


def line_particles(coords, D, seed=0):
    """particles on a line along coordinate 0; the other D - 1 coordinates are ONE random vector shared by all (their differences are
    exactly 0 in either dtype)"""
    X = np.zeros((len(coords), D))
    X[:, 0] = coords
    if D > 1:
        X[:, 1:] = np.random.RandomState(seed).randn(D - 1).astype(np.float32)
    return torch.from_numpy(X)


def sidon_line(P, D, q=SIDON_Q, s=SIDON_S):
    """c_i = (2 q i + (i^2 mod q)) / 2^s, q prime > P: an Erdos-Turan Sidon set, so all pairwise differences are distinct integers
    (/ 2^s) -- no two pairs share a distance, and neighbouring order statistics of the squared distances are well apart"""
    assert q > P
    i = np.arange(P, dtype=np.int64)
    return line_particles((2 * q * i + (i * i) % q).astype(np.float64) / 2.0 ** s, D)


def middle_gap(d2):
    """smallest relative gap between adjacent DISTINCT values of the full matrix around its two middle entries (each middle entry
    against the next smaller and the next larger value): a pick that is off by one order statistic moves the median by at least
    half of it, the bandwidth by a quarter"""
    N = d2.size
    flat, u = np.sort(d2.ravel()), np.unique(d2)
    gap = math.inf
    for m in ((N - 1) // 2, N // 2):
        k = int(np.searchsorted(u, flat[m]))
        for a, b in ((k - 1, k), (k, k + 1)):
            if a >= 0 and b < len(u):
                gap = min(gap, (u[b] - u[a]) / u[b])
    return gap


def bandwidth_consumers(L, X, dtype):
    """the median bandwidth of particles X as every consumer of the median reports it -> {entry point: tensor [1]}:
    pacoh_svgd_phi (svgd_kmat_kernel), pacoh_svgd_update and pacoh_svgd_update_dev (svgd_update_kernel), and for P <= 64 the
    workgroup riding in pacoh_hyper_bwd (svgd_bandwidth_block) on the distances pacoh_svgd_dist_advance left in the workspace"""
    P, D = X.shape
    Xd = dev(X, dtype)
    zero = torch.zeros_like(Xd)
    out = {'svgd_phi': L.svgd_phi(Xd, zero, None)[1],
           'svgd_update': L.svgd_update(Xd, zero, None, None, 0.0, None, 'SGD', 0.0, 1, None, None)[1]}
    sc = torch.tensor(L.step_scalars(1.0, 0.0, 1), dtype=dtype, device=DEV)
    out['svgd_update_dev'] = L.svgd_update_dev(Xd.clone(), zero, None, None, 0.0, None, 'SGD', sc, None, None)[0]
    if P <= 64:
        ws = L.svgd_update_workspace(Xd)
        L.svgd_dist_advance(Xd, ws, torch.full((1,), -1, dtype=torch.int64, device=DEV))
        # (the reduction itself runs on parameters of its own, the shape of test_pipelined_step_entry_points: the bandwidth block
        #  only reads the workspace)
        Tt, Dh, f, off_ls, off_noise = 3, 61, 3, 50, 58
        g = torch.Generator().manual_seed(5)
        theta, dl, dn = (dev(rounded(g, *s), dtype) for s in ((P, Dh), (Tt, P, f), (Tt, P)))
        L.hyper_bwd(theta, Tt, off_ls, f, -1, off_noise, -1, dl, None, dn, None, torch.zeros(P, Dh, dtype=dtype, device=DEV),
                    svgd_bw=(ws, P, D))
        out['hyper_bwd'] = ws.view(dtype)[P * P + P * D + 2].reshape(1).clone()
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', [1, 7])
@pytest.mark.parametrize('P', A_COUNTS)
def test_median_is_the_right_order_statistic(L, P, D, dtype):
    """Sidon-set particles on a line: the input guarantees (asserted on the host, before any launch) that the neighbouring order
    statistics are >= 1e-4 apart, so a pick that is off by one entry misses the bandwidth bar; every consumer of the median, and
    the consumers against each other bit for bit"""
    X = sidon_line(P, D)
    d2 = direct_d2(X)
    assert middle_gap(d2) >= 1e-4
    bw_o = O.svgd_bandwidth(torch.from_numpy(d2))
    got = bandwidth_consumers(L, X, dtype)
    assert len(got) == (4 if P <= 64 else 3)
    for name, bw in got.items():
        print('%s P %d D %d %s: bandwidth error %.2e' % (name, P, D, dtype, bw_err(bw, bw_o)))
        assert bw_err(bw, bw_o) <= BW_TOL[dtype], name
    for name, bw in got.items():
        assert torch.equal(bw, got['svgd_phi']), name


# ------------------------------------------------------------------------------------------ (b) ties
def tie_consumers(L, X, score, dtype):
    """(phi, bandwidth) of pacoh_svgd_phi and (particles after one SGD step of size 1 without a prior, bandwidth) of pacoh_svgd_update"""
    Xd, sd = dev(X, dtype), dev(score, dtype)
    phi, bw, _ = L.svgd_phi(Xd, sd, None)
    Xn, bw2, _ = L.svgd_update(Xd, sd, None, None, 0.0, None, 'SGD', 1.0, 1, None, None)
    return phi, bw, Xn, bw2


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('P', [24, 33, 46, 64, 65, 100])
def test_median_under_ties(L, P, dtype):
    """particles at the integers 0 .. P - 1 of a line: d^2 = (i - j)^2 is exact in fp32 and P - |i - j| pairs share it, so both
    middle entries lie inside a run of equal values (asserted) -- numpy.median semantics for the register sort's `(a > c) == up`
    and the bisection's `<` against a candidate bit pattern"""
    X = line_particles(np.arange(P, dtype=np.float64), 3, seed=1)
    d2 = direct_d2(X)
    flat = np.sort(d2.ravel())
    for m in ((P * P - 1) // 2, P * P // 2):
        assert int((flat == flat[m]).sum()) > 2             # (more than one pair holds the value)
    bw_o = O.svgd_bandwidth(torch.from_numpy(d2))
    score = rounded(torch.Generator().manual_seed(P), P, 3)
    phi, bw, Xn, bw2 = tie_consumers(L, X, score, dtype)
    print('P %d %s: bandwidth error %.2e / %.2e' % (P, dtype, bw_err(bw, bw_o), bw_err(bw2, bw_o)))
    assert bw_err(bw, bw_o) <= BW_TOL[dtype] and bw_err(bw2, bw_o) <= BW_TOL[dtype]
    assert torch.equal(bw, bw2)
    assert bool(torch.isfinite(phi).all()) and bool(torch.isfinite(Xn).all())


def identical_case(L, P, at_origin, dtype):
    """all P particles identical: every distance is 0, so are the median and the bandwidth, gamma = 1 / 1e-8; every K_ij is 1 and the
    repulsion vanishes, so phi_i is the mean score (what the reference's autograd gives: it differentiates K through x_i - x_j = 0)
    -> (error of phi, error of the particles after an SGD step of size 1, the two bandwidths, the mean score)"""
    D = 5
    g = torch.Generator().manual_seed(40 + P)
    row = torch.zeros(D, dtype=torch.float64) if at_origin else rounded(g, D)
    X = row.expand(P, D).contiguous()
    score = rounded(g, P, D)
    mean = score.mean(0, keepdim=True).expand(P, D)
    phi, bw, Xn, bw2 = tie_consumers(L, X, score, dtype)
    assert bool(torch.isfinite(phi).all()) and bool(torch.isfinite(Xn).all())
    return relerr(phi, mean), relerr(Xn, X + mean), float(bw), float(bw2), (X, score, mean)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('at_origin', [True, False])
@pytest.mark.parametrize('P', [24, 1])
def test_identical_particles_and_one_particle(L, P, at_origin, dtype):
    """the degenerate median: bandwidth exactly 0, phi finite and the mean score -- at the origin (where the oracle's closed form
    2 gamma (x_i sum_j k_ij - sum_j k_ij x_j) is exact too and is compared) and at a generic point, where a kernel that forms the
    repulsion from x_i sum_j k_ij and sum_j k_ij x_j separately loses the score to rounding at gamma |x| = 1e8 |x|"""
    e_phi, e_x, bw, bw2, (X, score, mean) = identical_case(L, P, at_origin, dtype)
    print('P %d origin %s %s: phi error %.2e, particle error %.2e' % (P, at_origin, dtype, e_phi, e_x))
    assert bw == 0.0 and bw2 == 0.0
    assert e_phi < PHI_TOL[dtype] and e_x < PHI_TOL[dtype]
    if at_origin:
        phi_o, bw_o = O.svgd_phi_closed_form(X, score, None)
        assert bw_o == 0.0 and relerr(phi_o, mean) < 1e-14


# ------------------------------------------------------------------------------------------ (c) phi and the fused update across the loop edges
C_COUNTS = [20, 21, 24, 29, 30, 34, 39, 50, 64]
C_DIMS = [1, 255, 256, 257]
PF, LR = 0.3, 1e-2
_REF = {}


def loop_edge_reference(P, D):
    """inputs and the fp64 reference of one (P, D): phi without a prior, and three steps of Adam and of SGD on the prior-augmented score
    (oracle phi + torch.optim, as test_svgd_update_fused) -- computed once, shared by both dtypes, never modified"""
    if (P, D) in _REF:
        return _REF[(P, D)]
    g = torch.Generator().manual_seed(1000 * P + D)
    X, score, mu = rounded(g, P, D), rounded(g, P, D), rounded(g, D)
    sd = (torch.rand(D, generator=g, dtype=torch.float64) + 0.5).float().double()
    r = SimpleNamespace(X=X, score=score, mu=mu, sd=sd, traj={}, bws={})
    r.phi, r.bw = O.svgd_phi_closed_form(X, score, None)
    for optimizer in ('Adam', 'SGD'):
        Xo = X.clone().requires_grad_(True)
        opt = torch.optim.Adam([Xo], lr=LR) if optimizer == 'Adam' else torch.optim.SGD([Xo], lr=LR)
        r.traj[optimizer], r.bws[optimizer] = [], []
        for _ in range(3):
            s_tot = score + PF * (-(Xo.detach() - mu) / sd ** 2)
            phi, bw = O.svgd_phi_closed_form(Xo.detach(), s_tot, None)
            Xo.grad = -phi
            opt.step()
            r.traj[optimizer].append(Xo.detach().clone())
            r.bws[optimizer].append(bw)
    _REF[(P, D)] = r
    return r


def loop_edge_errors(L, P, D, dtype):
    """device errors of one case against loop_edge_reference -> dict: phi, bw (pacoh_svgd_phi), X_Adam / X_SGD (particles after three
    steps of pacoh_svgd_update), bw_steps (worst bandwidth of those six steps), X_dev (one SGD step of pacoh_svgd_update_dev)"""
    r = loop_edge_reference(P, D)
    Xd, sd_, mu, sd = (dev(t, dtype) for t in (r.X, r.score, r.mu, r.sd))
    phi, bw, _ = L.svgd_phi(Xd, sd_, None)
    e = {'phi': relerr(phi, r.phi), 'bw': bw_err(bw, r.bw), 'bw_steps': 0.0}
    for optimizer in ('Adam', 'SGD'):
        Xk, ws = Xd, None
        m, v = torch.zeros(P, D, dtype=dtype, device=DEV), torch.zeros(P, D, dtype=dtype, device=DEV)
        for step in (1, 2, 3):
            Xk, bwk, ws = L.svgd_update(Xk, sd_, mu, sd, PF, None, optimizer, LR, step, m, v, workspace=ws)
            e['bw_steps'] = max(e['bw_steps'], bw_err(bwk, r.bws[optimizer][step - 1]))
        e['X_' + optimizer] = relerr(Xk, r.traj[optimizer][2])
    Xk = Xd.clone()
    sc = torch.tensor(L.step_scalars(1.0, LR, 1), dtype=dtype, device=DEV)
    bwk, _ = L.svgd_update_dev(Xk, sd_, mu, sd, PF, None, 'SGD', sc, None, None)
    e['X_dev'] = relerr(Xk, r.traj['SGD'][0])
    e['bw_steps'] = max(e['bw_steps'], bw_err(bwk, r.bws['SGD'][0]))
    return e


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', C_DIMS)
@pytest.mark.parametrize('P', C_COUNTS)
def test_phi_and_fused_update_across_the_loop_edges(L, P, D, dtype):
    """Gaussian particles and scores, median bandwidth, prior term; P at every change of the particle loop's path (prefetch alone,
    + remainder, + a round of 4, + two rounds of 4 and a remainder, + a round of 10 ...), D at one workgroup, one short of it, and two"""
    e = loop_edge_errors(L, P, D, dtype)
    print('P %d D %d %s: %s' % (P, D, dtype, ' '.join('%s %.2e' % kv for kv in sorted(e.items()))))
    assert e['bw'] <= BW_TOL[dtype] and e['bw_steps'] <= BW_TOL[dtype]
    assert e['phi'] < PHI_TOL[dtype]
    assert e['X_Adam'] < PHI_TOL[dtype] and e['X_SGD'] < PHI_TOL[dtype] and e['X_dev'] < PHI_TOL[dtype]


ONE_HOT_D = 257


def one_hot_rows(P):
    """the particles at the loop's round boundaries: the last of the prefetch, the first behind it, the last / first of a round of 10,
    the last one"""
    return sorted({j for j in (19, 20, 29, 30, P - 1) if j < P})


def one_hot_errors(L, P, dtype):
    """a score that is zero except in ONE particle's row (100 x standard normal, so that its kernel-weighted share dominates phi): a
    particle the loop drops or visits twice is an O(1) error in phi.  No prior (it would fill the other rows).  -> worst error of
    pacoh_svgd_phi's phi and of the particles after one SGD step of size 1 of pacoh_svgd_update, over one_hot_rows(P)"""
    g = torch.Generator().manual_seed(7000 + P)
    X = rounded(g, P, ONE_HOT_D)
    worst = [0.0, 0.0]
    for j in one_hot_rows(P):
        score = torch.zeros(P, ONE_HOT_D, dtype=torch.float64)
        score[j] = 100.0 * rounded(g, ONE_HOT_D)
        phi_o, _ = O.svgd_phi_closed_form(X, score, None)
        phi, _, Xn, _ = tie_consumers(L, X, score, dtype)
        worst = [max(worst[0], relerr(phi, phi_o)), max(worst[1], relerr(Xn, X + phi_o))]
    return worst


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('P', C_COUNTS)
def test_one_particles_score_reaches_every_phi(L, P, dtype):
    e_phi, e_x = one_hot_errors(L, P, dtype)
    print('P %d %s rows %s: phi error %.2e, particle error %.2e' % (P, dtype, one_hot_rows(P), e_phi, e_x))
    assert e_phi < PHI_TOL[dtype] and e_x < PHI_TOL[dtype]


# ------------------------------------------------------------------------------------------ (e) IMQ
E_COUNTS = [2, 3, 31, 32, 33, 50, 64]
E_DIMS = [5, 17, 101]
IMQ_FIXED_BW = 0.7
IMQ_SEPARATION = 1e-6        # > 4 fp32 roundings of (x_b - x_a)^2: the fp32 kernel then ranks the pairs around the median as fp64 does


def imq_median_gap(X):
    """per dimension, the relative gap of the lower median of the squared coordinate differences to its two neighbours; the smallest"""
    P = X.shape[0]
    iu, ju = torch.triu_indices(P, P, offset=1)
    srt = torch.sort((X[ju] - X[iu]) ** 2, dim=0).values
    k = (srt.shape[0] - 1) // 2
    gap = math.inf
    for a, b in ((k - 1, k), (k, k + 1)):
        if a >= 0 and b < srt.shape[0]:
            gap = min(gap, float(((srt[b] - srt[a]) / srt[b]).min()))
    return gap


def imq_inputs(P, D):
    """Gaussian particles and scores: the first seed whose per-dimension medians are IMQ_SEPARATION apart from their neighbours (no
    tied or nearly tied input: the gradient through the bandwidth follows the median PAIR, and which of two tied pairs torch.median
    names is unspecified -- that would test the oracle, not the kernel)"""
    for seed in itertools.count(100 * P + D):
        g = torch.Generator().manual_seed(seed)
        X, score = rounded(g, P, D), rounded(g, P, D)
        if imq_median_gap(X) >= IMQ_SEPARATION:
            return X, score


def imq_errors(L, P, D, dtype):
    """-> (phi error with the median bandwidth, error of h, phi error with a fixed bandwidth) against O.svgd_phi_imq_closed_form"""
    X, score = imq_inputs(P, D)
    assert imq_median_gap(X) >= IMQ_SEPARATION
    Xd, sd = dev(X, dtype), dev(score, dtype)
    phi, h, _ = L.svgd_phi_imq(Xd, sd, 0.5, -0.5, None)
    phi_o, h_o = O.svgd_phi_imq_closed_form(X, score, 0.5, -0.5, None)
    phi_f, h_f, _ = L.svgd_phi_imq(Xd, sd, 0.5, -0.5, IMQ_FIXED_BW)
    phi_fo, _ = O.svgd_phi_imq_closed_form(X, score, 0.5, -0.5, IMQ_FIXED_BW)
    assert h_f is None
    return relerr(phi, phi_o), relerr(h, h_o), relerr(phi_f, phi_fo)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', E_DIMS)
@pytest.mark.parametrize('P', E_COUNTS)
def test_imq_phi_and_bandwidths_at_the_kernel_switch(L, P, D, dtype):
    """imq_bw_small_kernel up to P = 32 (31 pair values per lane: P = 32 fills them), imq_bw_kernel from 33, both dtypes; D below,
    just above and well above the 16 dimensions of a workgroup"""
    e_phi, e_h, e_fixed = imq_errors(L, P, D, dtype)
    print('P %d D %d %s: phi %.2e h %.2e phi (fixed bandwidth) %.2e' % (P, D, dtype, e_phi, e_h, e_fixed))
    assert e_h < IMQ_H_TOL[dtype]
    assert e_phi < IMQ_PHI_TOL[dtype] and e_fixed < IMQ_PHI_TOL[dtype]


@pytest.mark.parametrize('dtype', DTYPES)
def test_imq_one_particle(L, dtype):
    """one particle has no pair to take a median of: refused; with a fixed bandwidth phi = alpha^beta score"""
    g = torch.Generator().manual_seed(3)
    X, score = rounded(g, 1, 17), rounded(g, 1, 17)
    with pytest.raises(RuntimeError):
        L.svgd_phi_imq(dev(X, dtype), dev(score, dtype), 0.5, -0.5, None)
    phi, h, _ = L.svgd_phi_imq(dev(X, dtype), dev(score, dtype), 0.5, -0.5, IMQ_FIXED_BW)
    phi_o, _ = O.svgd_phi_imq_closed_form(X, score, 0.5, -0.5, IMQ_FIXED_BW)
    assert h is None and relerr(phi_o, 0.5 ** -0.5 * score) < 1e-15
    assert relerr(phi, phi_o) < IMQ_PHI_TOL[dtype]


# ------------------------------------------------------------------------------------------ learner level
def test_learner_with_50_particles_reports_the_median_bandwidth(L):
    """plumbing at the reference sweeps' larger particle count: the bandwidth of a learner's first step is the median heuristic on
    the particles before it (Gaussian initialisation has no separation guarantee: the order statistic itself is checked above)"""
    import meta_learning_pacoh_amd as M
    tasks = O.sinusoid_tasks_nd(6, 12, 1, seed0=50)
    m = M.GPRegressionMetaLearnedSVGD(tasks, num_particles=50, task_batch_size=3, lr=1e-2, random_seed=5)
    before = m.particles.clone()
    m.meta_fit(verbose=False, n_iter=1)
    bw_o = median_bandwidth(before)
    assert bool(torch.isfinite(m.particles).all())
    assert abs(float(m.last_bandwidth) - bw_o) < 1e-5 * bw_o
