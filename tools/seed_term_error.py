"""How good is one agent's term of d loss / d fraction in float32?  ("Seeding by agent group".)

CPU only, numpy: the restatement of gj_adjoint_seed (tests/gj_seed_ref.py) in float32 against its float64 form on random
inputs, per agent, and - for the library's own noise - the float64 form with the pair of draws e0 = theta * s,
e1 = (1 - theta) * s formed in float32 against the same with s one ulp larger (what a different logf gives), next to
the same comparison with the products formed in float64 as the kernel does.

    python tools/seed_term_error.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import gj_seed_ref as R  # noqa: E402


def rel(a, b):
    m = np.abs(b) > 1e-30
    return float(np.max(np.abs(a - b)[m] / np.abs(b)[m]))


def main(n=20000):
    rng = np.random.default_rng(0)
    ones, zeros = np.ones(n, np.float32), np.zeros(n, np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    p = np.full(1, 0.8, np.float32)
    e = rng.exponential(size=(2, n)).astype(np.float32)
    nu = R.decisions(p[np.zeros(n, int)], e[0], e[1])
    f64 = R.seed_adjoint(p, None, 1, ones, zeros, 1.5, e[0], e[1], g_inf=g, nu=nu)["contrib"]
    f32 = R.seed_adjoint(p, None, 1, ones, zeros, 1.5, e[0], e[1], g_inf=g, nu=nu, dtype=np.float32)["contrib"]
    big = np.abs(f64) > 1e-6 * np.abs(f64).max()
    print(f"float32 against float64, per agent (terms above 1e-6 of the largest): {rel(f32[big], f64[big]):.2e}")
    print(f"float32 terms that are 0 where float64 is not: {int(((f32 == 0) & (f64 != 0)).sum())} of {n}")
    e0, e1, theta = R.library_draws(0x1234567, 9, 0, n)
    s = (e0 / theta.astype(np.float64)).astype(np.float32)
    s_up = np.nextafter(s, np.float32(np.inf))
    one_minus = np.float32(1.0) - theta

    def terms(s_, dtype):
        a, b = (theta.astype(dtype) * s_.astype(dtype)), (one_minus.astype(dtype) * s_.astype(dtype))
        return R.seed_adjoint(p, None, 1, ones, zeros, 1.5, a, b, theta, g_inf=g)["contrib"]

    print(f"s one ulp larger, products in float32: {rel(terms(s_up, np.float32), terms(s, np.float32)):.2e}")
    print(f"s one ulp larger, products in float64: {rel(terms(s_up, np.float64), terms(s, np.float64)):.2e}")


if __name__ == "__main__":
    main()
