"""p ranks of a host-staged communicator (``dftk_mi_comm_create_host``) as p THREADS of one process.

The library keeps its per-call state thread-local (last error, batch recorder) and releases nothing of its own between
two handles, and ctypes drops the GIL around every foreign call: rank r is a thread with its own ``dftk_mi_basis`` /
``dftk_mi_comm`` / ``dftk_mi_kblock`` on device 0, and the two host callbacks of the communicator meet over one
``threading.Barrier``.  Nothing is spawned; every rank layout costs the same.

Rules the callbacks keep (they run below C frames, inside a collective the other ranks are waiting in):

* an all-reduce is summed in rank order 0 .. p-1 by EVERY rank, so all ranks get bit-identical numbers (they take
  convergence and fallback decisions from them: ranks that disagree would stop matching their collectives);
* no exception leaves a callback: it is printed, the barrier is aborted and the callback returns 1, which the library
  reports as DFTK_MI_ERCCL;
* every barrier wait has a timeout (a cap, not a measurement), and a rank whose function has returned or raised aborts
  the barrier, so that nobody waits for a rank that will not come.

Helper module, not a conftest: tests import it by name.  p <= 4, one process, one GPU context.
"""
import ctypes as C
import threading
import traceback

import numpy as np

MAX_RANKS = 4
TIMEOUT = 60.0


class RankGroup:
    def __init__(self, p, timeout=TIMEOUT):
        from dftk_jl_amd._lib import ALLREDUCE_FN, ALLTOALLV_FN
        assert 1 <= p <= MAX_RANKS, p
        self.p, self.timeout = p, timeout
        self.calls = [0] * p                  # callback invocations per rank (all-reduce + all-to-all)
        self._generation = 0                  # completed barriers: advanced by the releasing thread, under the barrier's lock
        self.barrier = threading.Barrier(p, action=self._advance)
        self._slots = [None] * p
        self.allreduce = [ALLREDUCE_FN(self._make_allreduce(r)) for r in range(p)]
        self.alltoallv = [ALLTOALLV_FN(self._make_alltoallv(r)) for r in range(p)]
        self._comms = None
        self.threads = []                     # of the last run()

    # ---- the barrier ----------------------------------------------------------------------------------------------
    def _advance(self):
        self._generation += 1

    def _wait(self):
        """One rendezvous of all ranks.  A barrier that COMPLETED stays a success for a waiter that wakes up only after
        a faster rank has already returned and aborted it (threading.Barrier reports that as broken)."""
        generation = self._generation
        try:
            self.barrier.wait(self.timeout)
        except threading.BrokenBarrierError:
            if self._generation == generation:
                raise

    # ---- the callbacks --------------------------------------------------------------------------------------------
    def _guard(self, rank, body):
        def callback(*args):
            try:
                self.calls[rank] += 1
                body(*args)
                return 0
            except BaseException:             # never unwind through the C frames
                print(f"[shard_ranks] rank {rank}: collective failed", flush=True)
                traceback.print_exc()
                self.barrier.abort()
                return 1
        return callback

    def _make_allreduce(self, rank):
        def body(_user, buf, n):
            mine = np.ctypeslib.as_array(buf, shape=(n,)) if n else np.empty(0)
            self._slots[rank] = mine.copy()
            self._wait()
            parts = list(self._slots)
            if any(len(part) != n for part in parts):
                raise ValueError(f"all-reduce lengths differ: {[len(part) for part in parts]}")
            total = parts[0].copy()
            for part in parts[1:]:            # rank order: the same bits everywhere
                total += part
            self._wait()                      # everybody has read the deposits before the next call replaces them
            mine[:] = total
        return self._guard(rank, body)

    def _make_alltoallv(self, rank):
        p = self.p

        def body(_user, send, scnt, soff, recv, rcnt, roff):
            sc, so = [scnt[i] for i in range(p)], [soff[i] for i in range(p)]
            rc, ro = [rcnt[i] for i in range(p)], [roff[i] for i in range(p)]
            stot = max(o + c for o, c in zip(so, sc))
            rtot = max(o + c for o, c in zip(ro, rc))
            sbuf = np.ctypeslib.as_array(send, shape=(stot,)) if stot else np.empty(0)
            rbuf = np.ctypeslib.as_array(recv, shape=(rtot,)) if rtot else np.empty(0)
            self._slots[rank] = (sbuf, so, sc)            # a view: the buffer stays put until the second barrier
            self._wait()
            for src in range(p):
                src_buf, src_off, src_cnt = self._slots[src]
                if src_cnt[rank] != rc[src]:
                    raise ValueError(f"all-to-all: rank {src} sends {src_cnt[rank]} doubles, rank {rank} expects {rc[src]}")
                rbuf[ro[src]:ro[src] + rc[src]] = src_buf[src_off[rank]:src_off[rank] + rc[src]]
            self._wait()                      # the staging buffers are reused by the next call
        return self._guard(rank, body)

    # ---- communicators --------------------------------------------------------------------------------------------
    def comms(self):
        """The p ``dftk_mi_comm`` handles (created on first use; they borrow the callbacks of this object)."""
        if self._comms is None:
            from dftk_jl_amd._lib import check, load
            lib = load()
            handles = []
            for r in range(self.p):
                h = C.c_void_p()
                check(lib.dftk_mi_comm_create_host(self.p, r, 0, C.cast(self.allreduce[r], C.c_void_p),
                                                   C.cast(self.alltoallv[r], C.c_void_p), None, C.byref(h)))
                handles.append(h)
            self._comms = handles
        return self._comms

    def close(self):
        if self._comms is not None:
            from dftk_jl_amd._lib import load
            for h in self._comms:
                load().dftk_mi_comm_destroy(h)
            self._comms = None

    # ---- running the ranks ----------------------------------------------------------------------------------------
    def run(self, fn, with_comms=True):
        """``fn(rank, comm_handle)`` in p threads; the p results in rank order, or the exception that was raised FIRST (the
        ranks it released from a collective fail after it, with DFTK_MI_ERCCL).  All threads are joined before this
        returns or raises.  ``with_comms=False`` passes None (callbacks driven directly)."""
        handles = self.comms() if with_comms else [None] * self.p
        self.barrier.reset()                  # (no thread is inside: the last run joined them all)
        self._slots = [None] * self.p
        results, errors = [None] * self.p, []

        def rank_main(r):
            try:
                results[r] = fn(r, handles[r])
            except BaseException as exc:
                errors.append(exc)
            finally:
                self.barrier.abort()          # whoever still waits for this rank in a collective comes back at once

        self.threads = [threading.Thread(target=rank_main, args=(r,), name=f"rank{r}") for r in range(self.p)]
        for t in self.threads:
            t.start()
        for t in self.threads:
            t.join()
        if errors:
            raise errors[0]
        return results
