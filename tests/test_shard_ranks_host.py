"""tests/shard_ranks.py on the host: the two callbacks of the in-process rank group, driven directly from p Python
threads on NumPy buffers (no staging by the library, no GPU), and the ways a group ends when a rank fails."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd._lib import check
from dftk_jl_amd.comm import split_evenly

from shard_ranks import RankGroup

DP = C.POINTER(C.c_double)
SP = C.POINTER(C.c_size_t)


def _dp(a):
    return a.ctypes.data_as(DP)


def _sp(a):
    return a.ctypes.data_as(SP)


def _alive(group):
    return [t.name for t in group.threads if t.is_alive()]


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_allreduce_is_the_rank_ordered_sum_bitwise_on_every_rank(p):
    """Terms of very different magnitude: the sum depends on its order, and every rank must hold the bits of
    ((b0 + b1) + b2) + b3.  Three calls in a row of different lengths reuse the deposits."""
    rng = np.random.default_rng(p)
    group = RankGroup(p)
    lengths = [1, 257, 40]
    data = [[rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n) for n in lengths] for _ in range(p)]

    def fn(r, _comm):
        out = []
        for buf in data[r]:
            work = buf.copy()
            assert group.allreduce[r](None, _dp(work), len(work)) == 0
            out.append(work)
        return out

    got = group.run(fn, with_comms=False)
    for i, n in enumerate(lengths):
        want = data[0][i].copy()
        for r in range(1, p):
            want += data[r][i]
        for r in range(p):
            assert np.array_equal(got[r][i].view(np.uint64), want.view(np.uint64)), (i, r)
        if p == 4 and n == 257:     # (the order matters for these data: another association gives other bits)
            other = (data[0][i] + (data[1][i] + (data[2][i] + data[3][i])))
            assert not np.array_equal(other, want)
    assert group.calls == [len(lengths)] * p and not _alive(group)


def _plans(lib, p, nb, rows):
    plans = []
    for me in range(p):
        c0 = np.zeros(p + 1, dtype=np.int32)
        arrs = [np.zeros(p, dtype=np.int64) for _ in range(4)]
        check(lib.dftk_mi_shard_plan_host(p, me, nb, rows.ctypes.data, c0.ctypes.data, *[a.ctypes.data for a in arrs]))
        plans.append((c0, *arrs))
    return plans


def _row_splits(p, n):
    splits = [[r.start for r in split_evenly(n, p)] + [n]]
    if p == 2:
        splits += [[0, 1, n]]
    if p == 3:
        splits += [[0, 1, n - 7, n], [0, n - 2, n - 1, n]]
    if p == 4:
        splits += [[0, 1, 2, n - 1, n]]
    return splits


@pytest.mark.parametrize("p", [2, 3, 4])
def test_alltoallv_transposes_slabs_to_bands_and_back(p):
    """The plan of the device Transposer (dftk_mi_shard_plan_host), counts and offsets in DOUBLES as comm.cpp passes them:
    slab -> band through the helper's all-to-all gives every rank all rows of exactly its bands (pieces placed at
    row_starts, as Transposer::to_bands does), band -> slab gives the input back bit for bit.  Band counts include none,
    fewer than ranks, and ragged shares; receive buffers are NaN-filled with a guard beyond the last piece."""
    lib = dftk.load_library()
    rng = np.random.default_rng(10 + p)
    n = 23
    group = RankGroup(p)
    n_calls = 0
    for rows in _row_splits(p, n):
        rows = np.array(rows, dtype=np.int64)
        for nb in sorted({0, 1, p - 1, p, p + 1, 2 * p + 1}):
            X = rng.standard_normal((n, nb)) + 1j * rng.standard_normal((n, nb))
            plans = _plans(lib, p, nb, rows)
            c0 = plans[0][0]
            assert all(np.array_equal(pl[0], c0) for pl in plans) and c0[0] == 0 and c0[-1] == nb

            def fn(r, _comm):
                _, so, sc, bo, bc = plans[r]
                nloc, mine = rows[r + 1] - rows[r], c0[r + 1] - c0[r]
                slab = np.ascontiguousarray(X[rows[r]:rows[r + 1], :].flatten(order="F"))
                assert sc.sum() == nloc * nb and bc.sum() == n * mine
                dbl = [(2 * a).astype(np.uintp) for a in (sc, so, bc, bo)]
                band = np.full(n * mine + 3, complex(np.nan, np.nan))
                rc = group.alltoallv[r](None, _dp(slab.view(np.float64)), _sp(dbl[0]), _sp(dbl[1]),
                                        _dp(band.view(np.float64)), _sp(dbl[2]), _sp(dbl[3]))
                assert rc == 0 and np.isnan(band[n * mine:]).all()
                full = np.zeros((n, mine), dtype=complex)
                for s in range(p):
                    ns = rows[s + 1] - rows[s]
                    full[rows[s]:rows[s + 1], :] = band[bo[s]:bo[s] + bc[s]].reshape((ns, mine), order="F")
                back = np.full(nloc * nb + 3, complex(np.nan, np.nan))
                rc = group.alltoallv[r](None, _dp(band.view(np.float64)), _sp(dbl[2]), _sp(dbl[3]),
                                        _dp(back.view(np.float64)), _sp(dbl[0]), _sp(dbl[1]))
                assert rc == 0 and np.isnan(back[nloc * nb:]).all()
                return full, back[:nloc * nb], slab

            for r, (full, back, slab) in enumerate(group.run(fn, with_comms=False)):
                assert np.array_equal(full, X[:, c0[r]:c0[r + 1]]), (rows, nb, r)
                assert np.array_equal(back.view(np.uint64), slab.view(np.uint64)), (rows, nb, r)
            n_calls += 2
    assert group.calls == [n_calls] * p and not _alive(group)


def test_mismatched_collectives_fail_on_every_rank():
    """Ranks that disagree about the length of an all-reduce get a nonzero return, all of them, at once."""
    group = RankGroup(3)

    def fn(r, _comm):
        buf = np.ones(4 + (r == 2))
        return group.allreduce[r](None, _dp(buf), len(buf))

    t0 = time.monotonic()
    rcs = group.run(fn, with_comms=False)
    assert all(rc != 0 for rc in rcs) and time.monotonic() - t0 < group.timeout / 2 and not _alive(group)


def test_a_rank_that_raises_releases_the_others(capfd):
    """Rank 1 raises before it reaches the collective: the others come back from it with a nonzero return long before
    the barrier's timeout, run() joins every thread and re-raises the exception of rank 1.  The group works again
    afterwards."""
    group = RankGroup(3)
    rcs = {}

    def fn(r, _comm):
        if r == 1:
            raise KeyError("rank 1 gives up")
        buf = np.ones(5)
        rcs[r] = group.allreduce[r](None, _dp(buf), 5)
        return buf

    t0 = time.monotonic()
    with pytest.raises(KeyError, match="rank 1 gives up"):
        group.run(fn, with_comms=False)
    assert time.monotonic() - t0 < group.timeout / 2
    assert rcs == {0: 1, 2: 1} and not _alive(group)
    assert "collective failed" in capfd.readouterr().out       # printed, not propagated through the C frames

    def again(r, _comm):
        buf = np.full(2, float(r + 1))
        assert group.allreduce[r](None, _dp(buf), 2) == 0
        return buf

    assert all(np.array_equal(b, [6.0, 6.0]) for b in group.run(again, with_comms=False))


def test_a_rank_that_never_arrives_costs_the_timeout_not_a_hang():
    """Rank 1 stays alive but never enters the collective: the barrier's timeout (short here) ends the wait of the
    others with a nonzero return."""
    group = RankGroup(3, timeout=0.2)
    done = threading.Event()
    rcs = {}

    def fn(r, _comm):
        if r == 1:
            return done.wait(30.0)
        buf = np.ones(3)
        rcs[r] = group.allreduce[r](None, _dp(buf), 3)
        done.set()
        return None

    t0 = time.monotonic()
    results = group.run(fn, with_comms=False)
    assert results[1] is True and rcs == {0: 1, 2: 1} and not _alive(group)
    assert time.monotonic() - t0 < 10.0


def test_communicators_are_created_and_destroyed_by_the_group():
    """dftk_mi_comm_create_host(p, r, 0, ...) per rank: size and rank as the library reports them; run() hands rank r
    its own handle."""
    lib = dftk.load_library()
    group = RankGroup(4)
    got = group.run(lambda r, comm: (lib.dftk_mi_comm_rank(comm), lib.dftk_mi_comm_size(comm)))
    assert got == [(r, 4) for r in range(4)] and group.calls == [0] * 4
    group.close()
    with pytest.raises(AssertionError):
        RankGroup(5)
