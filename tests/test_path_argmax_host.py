"""Per-draw argmax of the posterior paths over a candidate pool, on the host side (no GPU): the two C entry points (declared,
exported, bound; every refusal without a launch; the workspace query) and the pure functions of paths.py that ARE the selection rule
(first_best / merge_best / chunk_ranges), which tests/test_gpu_path_argmax.py holds the kernel to."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from meta_learning_pacoh_amd import _lib                           # noqa: E402
from meta_learning_pacoh_amd import paths as PP                    # noqa: E402

EINVAL, ELIMIT, EDTYPE = -1, -2, -3
NEW = ('pacoh_gp_path_argmax_workspace_bytes', 'pacoh_gp_path_argmax')
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def lib():
    return _lib.load_library()


def test_new_symbols_are_declared_exported_and_bound(lib):
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pacoh_gp.h')) as fh:
        header = fh.read()
    for name in NEW:
        assert name + '(' in header
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert 'the reference has no pathwise sampler' in header
    assert _lib.ABI_VERSION == 14 and lib.pacoh_abi_version() == 14
    assert callable(_lib.gp_path_argmax)


def test_argument_validation_without_a_device(lib):
    fake, null = ctypes.c_void_p(4096), None

    def am(zs=fake, v=fake, w=fake, info=fake, omega=fake, phase=fake, zt=fake, zt_div=1, mean=fake, mode=_lib.MEAN_VECTOR, ls=fake,
           os_=fake, mask=fake, bv=fake, bi=fake, ws=fake, ws_bytes=None, B=6, P=3, n=16, cap=32, S=5, D=64, m=7, f=2, idx_base=0,
           largest=1, first=1, strips=0, dt=0):
        if ws_bytes is None:
            ws_bytes = max(1, lib.pacoh_gp_path_argmax_workspace_bytes(B, S, m, strips, dt))
        return lib.pacoh_gp_path_argmax(zs, v, w, info, omega, phase, zt, zt_div, mean, mode, ls, os_, mask, bv, bi, ws, ws_bytes,
                                        B, P, n, cap, S, D, m, f, idx_base, largest, first, strips, dt, null)

    for name in ('zs', 'v', 'w', 'info', 'omega', 'phase', 'zt', 'ls', 'bv', 'bi', 'ws'):
        assert am(**{name: null}) == EINVAL, name
    assert am(mean=null) == EINVAL and am(mean=null, mode=_lib.MEAN_CONST) == EINVAL and am(zt_div=0) == EINVAL and am(zt_div=-1) == EINVAL
    assert am(dt=5) == EDTYPE
    assert am(dt=5, zs=null, n=99, D=8, strips=-1) == EDTYPE        # the dtype is looked at first
    assert am(B=0) == EINVAL and am(P=0) == EINVAL and am(f=0) == EINVAL
    assert am(n=33) == ELIMIT                                       # n > cap
    assert am(n=0) == ELIMIT
    for dt in (0, 1):
        limit = lib.pacoh_gp_cond_max_n(dt)
        assert am(cap=limit + 1, dt=dt) == ELIMIT
        assert am(n=limit + 1, cap=limit + 1, dt=dt) == ELIMIT
    assert am(cap=4096) == ELIMIT
    assert am(f=17) == ELIMIT
    assert am(f=2 | (2 << _lib.KERNEL_SHIFT)) == ELIMIT             # family code 2 is unassigned
    assert am(f=1 | (_lib.KERNEL_COSINE << _lib.KERNEL_SHIFT)) == ELIMIT
    for D in (8, 24, 16400, 0, -16):
        assert am(D=D) == ELIMIT, D
    assert am(S=0) == ELIMIT
    assert am(m=0) == ELIMIT and am(m=-3) == ELIMIT
    assert am(strips=-1, ws_bytes=1 << 20) == EINVAL
    assert am(idx_base=-1) == EINVAL
    for bad in (-1, 2):
        assert am(largest=bad) == EINVAL and am(first=bad) == EINVAL
    for dt in (0, 1):
        for strips in (0, 1, 3):
            need = lib.pacoh_gp_path_argmax_workspace_bytes(6, 5, 200, strips, dt)
            assert am(m=200, strips=strips, dt=dt, ws_bytes=need - 1) == EINVAL
            assert am(m=200, strips=strips, dt=dt, ws_bytes=0) == EINVAL


def test_workspace_query(lib):
    q = lib.pacoh_gp_path_argmax_workspace_bytes
    for dt, size in ((0, 4), (1, 8)):
        assert q(1, 1, 1, 0, dt) > 0 and q(1, 1, 1, 1, dt) > 0
        # a forced strip count, clamped to the number of 64-point tiles: exactly one (index, value) pair per (problem, draw, strip)
        assert q(3, 5, 200, 2, dt) == 3 * 5 * 2 * (8 + size)
        assert q(3, 5, 200, 9, dt) == 3 * 5 * 4 * (8 + size)
        for strips in (0, 1, 2, 7):
            for m in (1, 65, 2373, 100000):
                last = 0
                for B in (1, 2, 3, 20, 64, 1000, 1024, 1025, 5000):
                    now = q(B, 16, m, strips, dt)
                    assert now >= last > -1 and now > 0, (B, m, strips)
                    last = now
                last = 0
                for S in (1, 16, 17, 64, 65, 128, 129, 1000):
                    now = q(20, S, m, strips, dt)
                    assert now >= last and now > 0, (S, m, strips)
                    last = now
        for m in (1, 65, 2373, 100000):
            last = 0
            for strips in (1, 2, 3, 37, 38, 39, 5000):
                now = q(3, 17, m, strips, dt)
                assert now >= last and now > 0, (m, strips)
                last = now
    assert q(1, 1, 1, 0, 5) == 0 and q(0, 1, 1, 0, 0) == 0 and q(1, 0, 1, 0, 0) == 0 and q(1, 1, 0, 0, 0) == 0 and q(1, 1, 1, -1, 0) == 0


def test_wrapper_validates_before_any_call():
    B, P, n, f, S, D, m = 6, 3, 8, 2, 5, 32, 7
    state = _lib.gp_cond_alloc(B, 16, f, torch.float32, 'cpu')
    omega, phase, w, v, zt = torch.zeros(D, f), torch.zeros(D), torch.zeros(B, S, D), torch.zeros(B, S, n), torch.zeros(B, m, f)
    ls, os_ = torch.ones(P, f), torch.ones(P)

    def am(**kw):
        a = dict(zs=state[0], n=n, v=v, omega=omega, phase=phase, w=w, info=state[4], z_tst=zt, zt_div=1, mean_tst=None,
                 mean_mode=_lib.MEAN_ZERO, lengthscale=ls, outputscale=os_, B=B, P=P)
        a.update(kw)
        return _lib.gp_path_argmax(**a)

    with pytest.raises(ValueError, match='v must be'):
        am(v=torch.zeros(B, S, n + 1))
    with pytest.raises(ValueError, match='info must be'):
        am(info=state[4].long())
    with pytest.raises(ValueError, match='z_tst must be'):
        am(z_tst=zt[:, :, :1])
    with pytest.raises(ValueError, match='lengthscale must be'):
        am(lengthscale=torch.ones(P, f + 1))
    with pytest.raises(ValueError, match='mask must be'):
        am(mask=torch.ones(m + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='mask must be'):
        am(mask=torch.ones(m))
    with pytest.raises(ValueError, match='must not be negative'):
        am(strips=-1)
    with pytest.raises(ValueError, match='must not be negative'):
        am(idx_base=-1)
    with pytest.raises(ValueError, match='first=False needs'):
        am(first=False)
    with pytest.raises(ValueError, match='best must be'):
        am(first=False, best=(torch.zeros(B, S), torch.zeros(B, S)))
    with pytest.raises(NotImplementedError, match='cosine'):
        am(kernel=_lib.KERNEL_COSINE)
    with pytest.raises(RuntimeError, match='HIP device'):           # a well-formed call on CPU tensors: no CPU path
        am()


# ------------------------------------------------------------------------------------------------------------- the rule itself
def _fb(row, mask=None, largest=True, dtype=torch.float64):
    idx, val = PP.first_best(torch.tensor(row, dtype=dtype), None if mask is None else torch.tensor(mask), largest)
    return int(idx), float(val)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_first_best_on_hand_made_rows(dtype):
    fb = lambda *a, **k: _fb(*a, dtype=dtype, **k)
    assert fb([1.0, 3.0, 2.0]) == (1, 3.0) and fb([1.0, 3.0, 2.0], largest=False) == (0, 1.0)
    assert fb([1.0, 3.0, 3.0, 3.0, 0.0]) == (1, 3.0)                # ties: the first index
    assert fb([5.0, 1.0, 7.0, 1.0], largest=False) == (1, 1.0)
    for row, sign in (([-1.0, -0.0, 0.0], -1.0), ([-1.0, 0.0, -0.0], 1.0)):          # -0.0 == +0.0: the first, with ITS sign
        i, v = fb(row)
        assert i == 1 and v == 0.0 and math.copysign(1.0, v) == sign
    i, v = fb([1.0, 0.0, -0.0], largest=False)
    assert i == 1 and math.copysign(1.0, v) == 1.0
    assert fb([NAN, 1.0, NAN, 2.0, NAN]) == (3, 2.0) and fb([NAN, 1.0, NAN, 2.0, NAN], largest=False) == (1, 1.0)
    assert fb([NAN, -INF]) == (1, -INF) and fb([NAN, INF], largest=False) == (1, INF)  # a valid infinity beats "nothing"
    assert fb([-INF, NAN, -INF]) == (0, -INF)
    for largest in (True, False):
        i, v = fb([NAN, NAN, NAN], largest=largest)
        assert i == -1 and math.isnan(v)
        i, v = fb([1.0, 2.0, 3.0], mask=[False, False, False], largest=largest)
        assert i == -1 and math.isnan(v)
        i, v = fb([1.0, NAN, 3.0], mask=[False, True, False], largest=largest)       # the only eligible point is NaN
        assert i == -1 and math.isnan(v)
        assert fb([9.0, 2.0, -9.0], mask=[False, True, False], largest=largest) == (1, 2.0)     # one eligible point
    assert fb([9.0, 2.0, 5.0, 5.0], mask=[False, True, True, True]) == (2, 5.0)
    assert fb([4.0]) == (0, 4.0)
    # batched: [..., m] with one mask [m]
    out = torch.tensor([[[1.0, 2.0, 2.0], [NAN, NAN, NAN]], [[0.0, -1.0, 5.0], [3.0, 3.0, 3.0]]], dtype=dtype)
    idx, val = PP.first_best(out, torch.tensor([True, True, False]))
    assert idx.dtype == torch.int64 and val.dtype == dtype
    assert idx.tolist() == [[1, -1], [0, 0]] and val[0, 0] == 2.0 and math.isnan(float(val[0, 1])) and val[1].tolist() == [0.0, 3.0]


@pytest.mark.parametrize('largest', [True, False])
def test_merge_best_is_commutative_and_agrees_with_first_best_on_the_concatenation(largest):
    g = torch.Generator().manual_seed(11)
    for trial in range(200):
        m = int(torch.randint(2, 40, (1,), generator=g))
        rows = 5
        # few distinct values (ties across the split), zeros of both signs, NaNs, and a mask that may empty a side
        out = torch.randint(-2, 3, (rows, m), generator=g).double()
        out = torch.where(torch.rand(rows, m, generator=g) < 0.15, -out * 0.0, out)
        out = torch.where(torch.rand(rows, m, generator=g) < 0.2, torch.full_like(out, NAN), out)
        mask = torch.rand(m, generator=g) < (0.1, 0.5, 0.9)[trial % 3]
        cut = int(torch.randint(1, m, (1,), generator=g))
        ia, va = PP.first_best(out[:, :cut], mask[:cut], largest)
        ib, vb = PP.first_best(out[:, cut:], mask[cut:], largest)
        ib = torch.where(ib >= 0, ib + cut, ib)                      # global indices
        i1, v1 = PP.merge_best(va, ia, vb, ib, largest)
        i2, v2 = PP.merge_best(vb, ib, va, ia, largest)
        iw, vw = PP.first_best(out, mask, largest)
        for i, v in ((i1, v1), (i2, v2)):
            assert torch.equal(i, iw)
            assert torch.equal(v.view(torch.int64), vw.view(torch.int64))    # bit for bit: NaN where nothing, the sign of a zero
        # three-way, any order
        if m >= 3:
            c2 = int(torch.randint(cut, m, (1,), generator=g))
            parts = []
            for lo, hi in ((0, cut), (cut, c2), (c2, m)):
                if hi > lo:
                    i, v = PP.first_best(out[:, lo:hi], mask[lo:hi], largest)
                    parts.append((v, torch.where(i >= 0, i + lo, i)))
            for order in (parts, parts[::-1]):
                v, i = order[0]
                for vb_, ib_ in order[1:]:
                    i, v = PP.merge_best(v, i, vb_, ib_, largest)
                assert torch.equal(i, iw) and torch.equal(v.view(torch.int64), vw.view(torch.int64))


def test_chunk_ranges_cover_the_pool_exactly_once():
    for chunk in (1, 7, 64, 131072):
        for m in (1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5):
            if m < 1:
                continue
            r = PP.chunk_ranges(m, chunk)
            assert r[0][0] == 0 and r[-1][1] == m
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            assert all(0 < hi - lo <= chunk for lo, hi in r)
            assert len(r) == -(-m // chunk)
            if m <= chunk:
                assert r == [(0, m)]
    with pytest.raises(ValueError):
        PP.chunk_ranges(0, 4)
    with pytest.raises(ValueError):
        PP.chunk_ranges(4, 0)


def test_public_interface():
    from meta_learning_pacoh_amd import engine as E
    from meta_learning_pacoh_amd.conditioned import ConditionedGP
    assert callable(E.GPEngine.cond_paths_argmax) and E.PATH_ARGMAX_CHUNK == 131072
    for name in ('argmax', 'argmin'):
        assert callable(getattr(PP.PosteriorPaths, name))
    assert callable(ConditionedGP.thompson)
    doc = sys.modules[ConditionedGP.__module__].__doc__
    assert 'paths.argmax' in doc and 'thompson' in doc
