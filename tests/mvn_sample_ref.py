"""fp64 torch restatement of pacoh_mvn_factor / pacoh_mvn_sample (the joint draws of the posterior predictive): gpytorch's
psd_safe_cholesky jitter ladder, the grouping of the draws by component, and y = y_mean + y_std (mu_c + L_c eps)."""
import torch

F32, F64 = 0, 1
JITTER_BASE = {F32: 1e-6, F64: 1e-8}


def rung_jitter(rung, dtype):
    """the diagonal jitter of a rung: 0, then base * 10^(k-1) for k = 1..3"""
    return 0.0 if rung == 0 else JITTER_BASE[dtype] * 10.0 ** (rung - 1)


def symmetrise(cov):
    """the matrix the factorisation sees: the lower triangle mirrored"""
    lo = torch.tril(cov)
    return lo + torch.tril(cov, -1).transpose(-1, -2)


def factor_ref(cov, dtype):
    """(rung [B] int, L [B,m,m] fp64): the first rung at which cov + j I has a Cholesky factor, decided in the kernel's dtype
    (fp32: 1e-6 .. 1e-4, fp64: 1e-8 .. 1e-6); rung -1 and a NaN factor when the ladder is exhausted.  L is the fp64 factor at
    that rung."""
    A = symmetrise(cov.to(torch.float64))
    tdt = torch.float32 if dtype == F32 else torch.float64
    B, m = A.shape[0], A.shape[-1]
    eye = torch.eye(m, dtype=torch.float64)
    rungs = torch.full((B,), -1, dtype=torch.int64)
    Ls = torch.full_like(A, float('nan'))
    for b in range(B):
        for rung in range(4):
            Aj = A[b] + rung_jitter(rung, dtype) * eye
            _, bad = torch.linalg.cholesky_ex(Aj.to(tdt))
            if int(bad) == 0:
                rungs[b] = rung
                Ls[b] = torch.linalg.cholesky(Aj)
                break
    return rungs, Ls


def factor_at(cov, rungs, dtype):
    """fp64 factors of cov + j I at given rungs (those a kernel reported); NaN where rung < 0"""
    A = symmetrise(cov.to(torch.float64))
    m = A.shape[-1]
    Ls = torch.full_like(A, float('nan'))
    for b, r in enumerate(rungs.tolist()):
        if r >= 0:
            Ls[b] = torch.linalg.cholesky(A[b] + rung_jitter(r, dtype) * torch.eye(m, dtype=torch.float64))
    return Ls


def group(comp, P):
    """order, offsets (int64) of the draws grouped by component: a stable sort, offsets = [0, cumsum(bincount)]"""
    comp = torch.as_tensor(comp).to(torch.int64).cpu()
    order = torch.sort(comp, stable=True).indices
    offsets = torch.zeros(P + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(comp, minlength=P), 0)
    return order, offsets


def sample_ref(Ls, mu, eps, comp=None, y_mean=0.0, y_std=1.0):
    """out [S,m] fp64 in draw order: y_mean + y_std (mu[c_s] + L[c_s] eps[s]); comp None: every draw from component 0.  Computed
    component by component through the grouping, as the kernel does"""
    Ls, mu, eps = Ls.to(torch.float64).cpu(), mu.to(torch.float64).cpu(), eps.to(torch.float64).cpu()
    S, m = eps.shape
    P = Ls.shape[0]
    comp = torch.zeros(S, dtype=torch.int64) if comp is None else torch.as_tensor(comp).to(torch.int64).cpu()
    order, offsets = group(comp, P)
    out = torch.empty(S, m, dtype=torch.float64)
    for c in range(P):
        rows = order[offsets[c]:offsets[c + 1]]
        if rows.numel():
            out[rows] = y_mean + y_std * (mu[c] + eps[rows] @ torch.tril(Ls[c]).T)
    return out
