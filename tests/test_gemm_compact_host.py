"""The compact launch of a DFTK_MI_GEMM_UPPER product (csrc/gemm_kernels.hip, k_zgemm_3m, `upper & 16`) on the host: the
work items that dftk_mi_zgemm_compact_host lists -- produced by the same work-item function the kernel runs -- cover every
live (k-chunk, tile) exactly once and no dead one, for gm x gn up to 12 x 24 tiles, 1 ... 8 k-chunks and the column tiles per
row panel of every product type (q = 2: REAL, 128 x 64 tiles; 4: complex 128 x 32, or the symmetric result of a tall REAL
product; 8: the symmetric result of a tall complex one).  Row panel r keeps its column tiles >= r q."""
import ctypes as C

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd._lib import check

GEMM_UPPER, GEMM_REAL = 1, 8


@pytest.fixture(scope="module")
def lib():
    return dftk.load_library()


def compact_items(lib, gm, gn, q, nsplit):
    cnt = C.c_int()
    cap = gm * gn * nsplit
    buf = (C.c_int * (3 * cap))()
    check(lib.dftk_mi_zgemm_compact_host(gm, gn, q, nsplit, cap, buf, C.byref(cnt)))
    assert cnt.value <= cap
    return np.array(buf[:3 * cnt.value], dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize("q", [2, 4, 8])
@pytest.mark.parametrize("gm", range(1, 13))
def test_compact_items_cover_every_live_chunk_tile_exactly_once(lib, gm, q):
    for gn in range(1, 25):
        live = {(r, c) for r in range(gm) for c in range(gn) if c >= r * q}
        for nsplit in range(1, 9):
            items = compact_items(lib, gm, gn, q, nsplit)
            want = {(z, r, c) for z in range(nsplit) for (r, c) in live}
            got = [tuple(int(v) for v in it) for it in items]
            assert len(got) == len(want), (gm, gn, q, nsplit, len(got), len(want))       # nothing twice ...
            assert set(got) == want, (gm, gn, q, nsplit)                                 # ... nothing dead, nothing missing
            # the order of the list: workgroup id = xcd + 8 slot, item = xcd * per + slot (8 contiguous blocks of items)
            per = (len(want) + 7) // 8
            order = sorted(want)                                                         # (chunk, row panel, column tile)
            by_id = [order[x * per + s] for s in range(per) for x in range(8) if x * per + s < len(order) and s < per]
            assert got == by_id, (gm, gn, q, nsplit)


def test_compact_list_matches_the_plan_of_the_gram_products(lib):
    """The REAL UPPER Gram products of the 250-atom cell: 503^2 -> 4 x 8 tiles, 20 live, 25 k-chunks = 500 work items;
    1006^2 -> 8 x 16 tiles, 72 live, 7 k-chunks = 504 (one round of the 512 resident workgroups each)."""
    for n, live, nsplit in ((503, 20, 25), (1006, 72, 7)):
        out = (C.c_int * 12)()
        check(lib.dftk_mi_zgemm_plan_host(b"C", n, n, 132430, GEMM_REAL | GEMM_UPPER, out))
        BN, gmf, gnf, ns, placement, shift = out[0], out[1], out[2], out[5], out[7], out[11]
        assert (BN, ns, placement) == (64, nsplit, 2)
        gm, gn = gmf + (1 if n % 128 else 0), gnf + shift
        items = compact_items(lib, gm, gn, 128 // BN, ns)
        assert len(items) == live * nsplit and len({tuple(i) for i in items.tolist()}) == live * nsplit


def test_compact_host_rejects_bad_arguments(lib):
    cnt = C.c_int()
    assert lib.dftk_mi_zgemm_compact_host(0, 4, 2, 1, 0, None, C.byref(cnt)) != 0
    assert lib.dftk_mi_zgemm_compact_host(4, 4, 0, 1, 0, None, C.byref(cnt)) != 0
    assert lib.dftk_mi_zgemm_compact_host(4, 4, 2, 1, 8, None, C.byref(cnt)) != 0
    check(lib.dftk_mi_zgemm_compact_host(4, 8, 2, 25, 0, None, C.byref(cnt)))      # count only
    assert cnt.value == 500
