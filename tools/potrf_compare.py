#!/usr/bin/env python
"""Compare dftk_mi_potrf_trtri / dftk_mi_potrf_trtri_real between two builds of the library.

python tools/potrf_compare.py metrics OUT.json   residuals (long double) and a SHA-256 of R and inv(R) for the 36 inputs of
                                                 tests/test_gpu_potrf_panels.py, and the status of an indefinite input
python tools/potrf_compare.py time OUT.json      ms per call at n = 259 / 503 / 512, both entries: 40 calls, the first 5
                                                 dropped, minimum and median of the other 35 (host clock around the call
                                                 and a device synchronise: Cholesky + inverse + norm estimates + host fetch)
python tools/potrf_compare.py diff A.json B.json what differs between two `metrics` files (nothing, for bit-identical builds)

Run it from the checkout whose library is to be measured, one fresh process per measurement, alternating the builds."""
import hashlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1]
if mode == "diff":
    a, b = (json.load(open(p)) for p in sys.argv[2:4])
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    print(f"{len(a)} entries, different: {bad}")
    sys.exit(1 if bad else 0)

sys.path.insert(0, ROOT)
import torch  # noqa: E402
import dftk_jl_amd as dftk  # noqa: E402

spec = importlib.util.spec_from_file_location("potrf_panels", os.path.join(ROOT, "tests", "test_gpu_potrf_panels.py"))
tpp = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tpp)
lib = dftk.load_library()
print(mode, lib.dftk_mi_version().decode(), flush=True)
bs = tpp.Basis(lib)
res = {}
if mode == "metrics":
    for kind in ("real", "complex"):
        for n in tpp.SIZES:
            for cond in tpp.CONDS:
                (e_r, e_i), R, Z = tpp.measure(lib, bs, kind, n, cond)
                h = hashlib.sha256(np.ascontiguousarray(R).tobytes() + np.ascontiguousarray(Z).tobytes()).hexdigest()
                res[f"{kind} {n} {cond:.0e}"] = [e_r, e_i, h]
                print(f"{kind} n={n} cond={cond:.0e}: |R'R-G|/|G| = {e_r:.3e}, |R inv(R) - I| = {e_i:.3e}, sha256 {h[:12]}",
                      flush=True)
            G = tpp.gram(kind, n, 1e2)
            st, _, _ = tpp.factor(lib, bs, kind, G - 2.0 * np.trace(G).real / n * np.eye(n))
            res[f"{kind} {n} indefinite"] = st
elif mode == "time":
    for kind in ("real", "complex"):
        fn = lib.dftk_mi_potrf_trtri if kind == "complex" else lib.dftk_mi_potrf_trtri_real
        for n in (259, 503, 512):
            G = tpp.gram(kind, n, 1e2)
            A0 = torch.from_numpy(np.ascontiguousarray(G.T)).cuda()
            Z = torch.empty_like(A0)
            ts = []
            for rep in range(40):
                A = A0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tpp.check(fn(bs.h, n, A.data_ptr(), n, Z.data_ptr(), n))
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            ts = sorted(ts[5:])
            res[f"{kind} {n}"] = [1e3 * ts[0], 1e3 * ts[len(ts) // 2]]
            print(f"{kind} n={n}: min {1e3 * ts[0]:.3f} ms, median {1e3 * ts[len(ts) // 2]:.3f} ms per call", flush=True)
else:
    sys.exit(__doc__)
with open(sys.argv[2], "w") as fh:
    json.dump(res, fh, indent=1)
