"""Host side of the distinct-task SVGD step (no GPU): engine.distinct_rows, which rewrites a step's task draw (with replacement) as
its distinct tasks and their multiplicities, and the device-side re-split of the fused networks' tile range (csrc/mlp_fused_split.h,
reached through pacoh_mlp_fused_split / pacoh_mlp_fused_plan of the built library)."""
import ctypes

import numpy as np
import pytest

from meta_learning_pacoh_amd import _lib
from meta_learning_pacoh_amd.engine import distinct_rows


def check_row(draw, row, mult, n_act, tb):
    assert 1 <= n_act <= tb
    ids = list(row[:n_act])
    assert len(set(ids)) == n_act                                           # distinct ...
    firsts = []
    for v in draw:
        if v not in firsts:
            firsts.append(v)
    assert ids == firsts                                                    # ... in order of first occurrence
    assert mult.sum() == tb and (mult[:n_act] >= 1).all()
    assert (mult[n_act:] == 0).all() and all(v in draw for v in row[n_act:])       # padding: count 0, a valid id
    rebuilt = sorted(int(v) for v, c in zip(row, mult) for _ in range(int(c)))
    assert rebuilt == sorted(int(v) for v in draw)                          # the multiset of the draw


@pytest.mark.parametrize('T,tb,k', [(7, 4, 9), (5, 12, 6), (1024, 1024, 3), (3, 1, 5), (40000, 17, 4), (2, 33, 8)])
def test_distinct_rows_of_random_draws(T, tb, k):
    rs = np.random.RandomState(T + tb)
    idx = rs.randint(0, T, size=(k, tb))
    rows, mult, n_act = distinct_rows(idx)
    assert rows.shape == mult.shape == (k, tb) and n_act.shape == (k,)
    assert rows.dtype == np.int64 and mult.dtype == np.float32 and n_act.dtype == np.int32
    for r in range(k):
        check_row(list(idx[r]), rows[r], mult[r], int(n_act[r]), tb)
    assert np.array_equal(distinct_rows(idx, np.float64)[1], mult.astype(np.float64))


def test_distinct_rows_edge_rows():
    idx = np.array([[3, 3, 3, 3, 3, 3],          # all equal
                    [4, 0, 5, 2, 1, 3],          # all distinct
                    [3, 3, 1, 3, 0, 1],
                    [0, 1, 2, 3, 4, 0]])         # the repeat is the last draw: n_act = tb - 1
    rows, mult, n_act = distinct_rows(idx)
    assert list(n_act) == [1, 6, 3, 5]
    assert list(rows[0]) == [3] * 6 and list(mult[0]) == [6, 0, 0, 0, 0, 0]
    assert list(rows[2][:3]) == [3, 1, 0] and list(mult[2]) == [3, 2, 1, 0, 0, 0]
    assert list(rows[3][:5]) == [0, 1, 2, 3, 4] and list(mult[3]) == [2, 1, 1, 1, 1, 0]
    # a draw without repeats comes back as it is: the exact-bits anchor of the device path
    assert np.array_equal(rows[1], idx[1]) and (mult[1] == 1).all()
    one = distinct_rows(np.array([[5], [0]]))
    assert np.array_equal(one[0], [[5], [0]]) and (one[1] == 1).all() and list(one[2]) == [1, 1]
    perm = np.stack([np.random.RandomState(s).permutation(50) for s in range(4)])
    rows, mult, n_act = distinct_rows(perm)
    assert np.array_equal(rows, perm) and (mult == 1).all() and (n_act == 50).all()


def test_mean_distinct_count_of_a_full_draw():
    """1024 draws from 1024 tasks hold 1024 (1 - (1 - 1/1024)^1024) = 647.4 distinct tasks on average"""
    idx = np.random.RandomState(0).randint(0, 1024, size=(256, 1024))
    n_act = distinct_rows(idx)[2]
    assert abs(n_act.mean() - 1024 * (1 - (1 - 1 / 1024) ** 1024)) < 3.0


@pytest.fixture(scope='module')
def lib():
    return _lib.load_library()


def plan(lib, R, P, nets, n_hidden, bwd, resident):
    tp, wgs, tpw = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.pacoh_mlp_fused_plan(R, P, nets, n_hidden, bwd, resident, ctypes.byref(tp), ctypes.byref(wgs), ctypes.byref(tpw)) == 0
    return tp.value, wgs.value, tpw.value


def tiles_of_launch(R_eff, tp, wgs, tpw):
    """the tiles the kernels' tile loop visits: workgroup w, wave v takes tiles w * tpw + v, + 4, ... below tpw while their rows start
    below R_eff (mlp_fused.hip)"""
    seen = []
    for w in range(wgs):
        for wave in range(4):
            for tl in range(wave, tpw, 4):
                row0 = (w * tpw + tl) * tp
                if row0 >= R_eff:
                    break
                seen.append(w * tpw + tl)
    return seen


PLANS = [(1, 2, 2), (20, 2, 2), (5, 1, 4), (3, 2, 1)]          # (parameter rows, networks, hidden layers)


def test_split_reproduces_the_host_plan_when_every_task_is_live(lib):
    """n_act == tb: the device-side split returns the host plan's tiles per workgroup -- forward and backward plans, 32- and 64-point
    tiles, every R in 1 .. 4096"""
    tps = set()
    for P, nets, nh in PLANS:
        for bwd in (0, 1):
            for resident in ((768, 512) if bwd else (0,)):
                for R in range(1, 4097):
                    tp, wgs, tpw = plan(lib, R, P, nets, nh, bwd, resident)
                    tiles = -(-R // tp)
                    tps.add(tp)
                    assert wgs >= 1 and wgs * tpw >= tiles
                    assert lib.pacoh_mlp_fused_split(tiles, tiles, wgs, tpw) == tpw, (R, P, nets, nh, bwd, resident)
    assert tps == {32, 64}


def test_split_covers_the_live_tiles_exactly_once(lib):
    """every n_act: the workgroups' tile ranges cover [0, tiles_eff) exactly once, and no workgroup takes more than the plan gave it"""
    n = 13                                                          # points per task: R = tb * n, R_eff = n_act * n
    for P, nets, nh in PLANS:
        for bwd in (0, 1):
            for tb in list(range(1, 25)) + [40, 64, 97, 160, 315]:
                R = tb * n
                tp, wgs, tpw = plan(lib, R, P, nets, nh, bwd, 768)
                tiles = -(-R // tp)
                for n_act in range(1, tb + 1):
                    R_eff = n_act * n
                    tiles_eff = -(-R_eff // tp)
                    t = lib.pacoh_mlp_fused_split(tiles_eff, tiles, wgs, tpw)
                    assert 1 <= t <= tpw and wgs * t >= tiles_eff
                    assert sorted(tiles_of_launch(R_eff, tp, wgs, t)) == list(range(tiles_eff)), (P, nets, nh, bwd, tb, n_act)
    # the flagship shape: 1024 tasks of 64 points, 20 parameter rows, both networks; 647 distinct tasks
    for bwd in (0, 1):
        tp, wgs, tpw = plan(lib, 65536, 20, 2, 2, bwd, 768)
        assert tp == 64
        t = lib.pacoh_mlp_fused_split(647, 1024, wgs, tpw)
        assert t % 4 == 0 and t < tpw and sorted(tiles_of_launch(647 * 64, tp, wgs, t)) == list(range(647))
