"""The folded launch of a triangular X * inv(R) product (csrc/gemm_kernels.hip, k_zgemm_3m FOLD) on the host: the tiles that
dftk_mi_zgemm_fold_host lists -- produced by the same work-item function the kernel runs -- cover every tile of the plan
exactly once, each over the k range a triangular B needs; the two tiles of a workgroup belong to one row panel and are the
pair (gn - 1 - p, p); shapes whose plan splits K (and every other flag combination) do not fold."""
import ctypes as C

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd._lib import check

B_UPPER, GEMM_REAL = 2, 8


@pytest.fixture(scope="module")
def lib():
    return dftk.load_library()


def fold_items(lib, trans, m, n, k, flags):
    cnt = C.c_int()
    cap = 4 * (m // 128 + 2) * (n // 32 + 2)
    buf = (C.c_int * (4 * cap))()
    check(lib.dftk_mi_zgemm_fold_host(trans, m, n, k, flags, cap, buf, C.byref(cnt)))
    assert cnt.value <= cap
    return np.array(buf[:4 * cnt.value]).reshape(-1, 4)


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 192, 200, 503])
@pytest.mark.parametrize("m", [128 * 600, 128 * 77 + 5, 132430])
def test_folded_items_cover_the_plan_exactly_once(lib, m, n, real):
    flags = B_UPPER | (GEMM_REAL if real else 0)
    out = (C.c_int * 12)()
    check(lib.dftk_mi_zgemm_plan_host(b"N", m, n, n, flags, out))
    BN, gmf, gnf, nright, nbottom, nsplit, shift = out[0], out[1], out[2], out[3], out[4], out[5], out[11]
    assert BN == (64 if real else 32)
    items = fold_items(lib, b"N", m, n, n, flags)
    gn = gnf + shift
    if nsplit > 1 or gn < 2:
        assert len(items) == 0
        return
    gm = gmf + (1 if m % 128 else 0)        # a ragged last row tile is a full tile shifted up (m >= 128 here)
    assert nright == 0 and nbottom == 0
    # every (row panel, column tile) exactly once
    assert len(items) == gm * gn
    assert len({(r, c) for r, c, _, _ in items}) == gm * gn
    assert items[:, 0].min() == 0 and items[:, 0].max() == gm - 1 and items[:, 1].min() == 0 and items[:, 1].max() == gn - 1
    for r, c, k0, k1 in items:
        j0 = n - BN if (shift and c == gnf) else c * BN
        assert k0 == 0 and k1 == min(n, j0 + BN)       # all k <= j of the tile's last column, nothing beyond the diagonal block
    # workgroup order: the long tile gn - 1 - p, then its partner p of the same row panel; the middle tile of an odd count alone
    i = 0
    while i < len(items):
        r, c = items[i, 0], items[i, 1]
        p = gn - 1 - c
        assert 0 <= p <= c
        if p != c:
            assert tuple(items[i + 1, :2]) == (r, p)
            i += 2
        else:
            i += 1


def test_no_fold_outside_the_triangular_no_split_case(lib):
    m, n = 132430, 503
    assert len(fold_items(lib, b"N", m, n, n, GEMM_REAL)) == 0                 # dense
    assert len(fold_items(lib, b"N", m, n, n, GEMM_REAL | B_UPPER | 1)) == 0   # UPPER as well
    assert len(fold_items(lib, b"C", n, n, m, GEMM_REAL | B_UPPER)) == 0       # 'C'
    assert len(fold_items(lib, b"N", 1000, n, n, GEMM_REAL | B_UPPER)) == 0    # K split (fewer tiles than resident workgroups)
    assert len(fold_items(lib, b"N", m, n, n, GEMM_REAL | B_UPPER)) == 1035 * 8
