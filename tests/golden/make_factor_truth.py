"""Writes the multiprecision truth of the factor-chain tests (tests/factor_reference.py):

    tests/golden/factor_truth.npz        the cases of csrc/factor.hip (path 0)
    tests/golden/factor_truth_wide.npz   the cases of launch_wa_factor (path 1)
    tests/golden/factor_truth_gram.npz   the Gram-form chains
    tests/golden/factor_truth_tiled.npz  the cases of launch_wa_factor_tiled (path 2)

(four files: with hi + lo doubles of P, Z and M one file would pass the size limit of a committed file).  Run from the repository root:

    python tests/golden/make_factor_truth.py [-j N] [case name ...]

Per case '<name>/<key>': s, s_reg [2][C], W [2][2][C], Z [2][rows][C] and rows, Pu [2][C (C + 1) / 2] (the upper triangle of the Hermitian P,
row after row) -- each a hi + lo stack of float64 --, sum (checksum of the input the truth belongs to), zmax (the largest |Z|, a scale),
lapack [5] = the errors A, B, C, DW, DZ of numpy.linalg.svd through the same formulas: the tests allow 8 x max(that, C eps).
The generator asserts the stated condition of each matrix class.  Takes about a minute on eight cores (mpmath at 100 digits; the Gram matrices X^H X are formed in exact integer arithmetic first).
The 36 cases of 9 ... 32 columns and of the tiled form (up to 16384 x 32: the exact Gram matrix is an object-array product) were written by a partial
run, `-j 8` with their names: 17 s on eight cores (110 s of CPU time).
For the Gram chains: s [2][11][C], Mu (upper triangle of M per bin), cond_limit (between the two largest conditionings of the chain),
lapack [11][2] = the errors A, M of numpy.linalg.eigh per bin.
"""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import factor_reference as R   # noqa: E402

KEYS = ("A", "B", "C", "DW", "DZ")


def pack_upper(a):
    """[2][C][C] Hermitian -> [2][C (C + 1) / 2]"""
    iu = np.triu_indices(a.shape[-1])
    return a[..., iu[0], iu[1]]


def check_class(case, s):
    """the condition the class states, on the true singular values"""
    cls, smax = case["cls"], s.max()
    if cls == "K1":
        assert s.min() > R.REG_C * smax and smax / s.min() < 40.0, case["name"]
    if cls in ("K2", "K3"):
        assert np.all(np.abs(s / (R.REG_C * smax) - 1.0) > 1e-3), case["name"]
    if cls == "K3":
        assert smax / s.min() >= 1e12, (case["name"], smax / s.min())
    if cls in ("K4", "K5"):
        tol = R.pinv_tol(smax, case["tol_dim"])
        assert np.all((s > 100.0 * tol) | (s == 0.0)), case["name"]
        assert (cls == "K5") == bool(np.any(s == 0.0)), case["name"]
    if cls == "K6":     # every leaf but the whole matrix is deficient: nothing is clipped
        assert s.min() > R.REG_C * smax, case["name"]
    if cls == "K4":
        assert 4e3 < smax / s.min() < 2e4, case["name"]


def one_case(name):
    case = R.CASE[name]
    tr = R.truth(case)
    check_class(case, tr["s"][0])
    X, Hq = R.build_input(case)
    sv, Z, W = R.lapack_route(X, Hq, case["mode"], case["reg_c"], case["tol_dim"])
    tr["zmax"] = np.array([np.abs(Z).max()])
    m = R.measures(tr, X, sv, Z, W)
    tr["lapack"] = np.array([m[k] for k in KEYS])
    tr["Pu"] = pack_upper(tr.pop("P"))
    return name, tr


def one_gram(name):
    case = R.GRAM_CASE[name]
    tr = R.gram_truth(case)
    A = R.gram_chain(case)
    s = tr["s"][0]
    cond = s.max(axis=1) / s.min(axis=1)
    used = np.array([k for k in range(R.GRAM_BINS) if k != R.GRAM_SKIP])
    top = used[np.argsort(cond[used])[::-1]]
    assert top[0] == R.GRAM_HIGH and cond[top[1]] < 0.97 * cond[top[0]], (name, cond)
    tr["cond_limit"] = np.array([np.sqrt(cond[top[0]] * cond[top[1]])])   # one bin just above it
    err = np.zeros((R.GRAM_BINS, 2))
    for k in range(R.GRAM_BINS):
        sl, Ml = R.gram_lapack(A[k])
        m = R.gram_measures(tr, k, sl, Ml)
        err[k] = m["A"], m["M"]
    tr["lapack"] = err
    tr["Mu"] = pack_upper(tr.pop("M"))
    return name, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    names = a.names or [c["name"] for c in R.CASES] + [c["name"] for c in R.GRAM_CASES]
    # the long ones first
    cost = lambda n: -(R.CASE[n]["S"] * R.CASE[n]["C"] ** 2 + 40 * R.CASE[n]["C"] ** 3) if n in R.CASE else -11 * 40 * R.GRAM_CASE[n]["C"] ** 3   # noqa: E731
    names = sorted(names, key=cost)
    files = {"p0": {}, "p1": {}, "p2": {}, "g": {}}
    with ProcessPoolExecutor(a.j) as ex:
        futs = [ex.submit(one_case if n in R.CASE else one_gram, n) for n in names]
        for f in futs:
            name, tr = f.result()
            print(name, "lapack", tr["lapack"].max(axis=0) if tr["lapack"].ndim == 2 else tr["lapack"], flush=True)
            for k, v in tr.items():
                files[name.split("_")[0]]["%s/%s" % (name, k)] = v
    here = os.path.dirname(os.path.abspath(__file__))
    for key, fn in (("p0", "factor_truth.npz"), ("p1", "factor_truth_wide.npz"), ("p2", "factor_truth_tiled.npz"), ("g", "factor_truth_gram.npz")):
        if not files[key]:
            continue
        path = os.path.join(here, fn)
        if a.names and os.path.exists(path):   # a partial run replaces its cases only
            old = dict(np.load(path))
            old.update(files[key])
            files[key] = old
        np.savez_compressed(path, **files[key])
        print(fn, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
