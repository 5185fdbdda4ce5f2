"""Writes the multiprecision truth of the direct inverse of the Gram route (tests/gram_reference.py): tests/golden/gram_solve_truth.npz.
Run from the repository root:

    python tests/golden/make_gram_truth.py [-j N]

Per positive definite bin 's<C>_<bin>/<key>' of solve_input(C): lam [2][C] (the eigenvalues of the FP64 matrix, hi + lo), Mu [2][C (C + 1) / 2]
(the upper triangle of M = V diag(s_reg / s) V^H, hi + lo; M = A^-1 where cond_2(A) <= 1e4), lapack_inv [1] (the relative Frobenius error
numpy.linalg.inv makes on the bin; nan where M is not the inverse), lapack_eigh [1] (the largest element error of M through numpy.linalg.eigh
relative to the largest element), sum (checksum of the matrix the truth belongs to).  mpmath at 60 digits; about a minute on eight cores.
"""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import factor_reference as R   # noqa: E402
import gram_reference as G     # noqa: E402


def one(job):
    C, b = job
    A = G.solve_matrix(C, b)[0]
    tr, (mp, Am, M) = G.mp_truth(A)
    lam = tr["lam"][0]
    assert lam.min() > 0, (C, b)
    clipped = lam.max() / lam.min() > 1.0 / G.REG_C ** 2
    if not clipped and C <= 9:      # M is the inverse: M A = I at the working precision
        Pm = M * Am
        assert max(abs(Pm[i, j] - (1 if i == j else 0)) for i in range(C) for j in range(C)) < mp.mpf(10) ** -45, (C, b)
    tr["lapack_inv"] = np.array([np.nan if clipped else G.inv_error(np.linalg.inv(A), tr)])
    tr["lapack_eigh"] = np.array([G.chain_error(R.gram_lapack(A, G.REG_C)[1], tr)])
    tr["sum"] = np.array([R.checksum(A)], dtype=np.uint64)
    iu = np.triu_indices(C)
    tr["Mu"] = tr.pop("M")[..., iu[0], iu[1]]
    return (C, b), tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    jobs = [(C, b) for C in reversed(G.SOLVE_C) for b in range(G.SOLVE_NBINS) if G.SOLVE_BINS[b][0] == "r"]
    out = {}
    with ProcessPoolExecutor(a.j) as ex:
        for (C, b), tr in ex.map(one, jobs):
            print("C %2d bin %2d class %-6s cond %.4g  inv %.3g  eigh %.3g" % (C, b, G.solve_class(b), tr["lam"][0].max() / tr["lam"][0].min(),
                                                                              tr["lapack_inv"][0], tr["lapack_eigh"][0]), flush=True)
            for k, v in tr.items():
                out["s%d_%d/%s" % (C, b, k)] = v
    path = G.FIXTURE
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
