#!/usr/bin/env python3
"""Derives the constants of pmv_atan and pmv_tan (practical-multi-view_amd/csrc/pmv_lift.h, restated in tests/twin/fisheye_twin.cpp) with
mpmath at 60 digits, and prints them as C hexadecimal double literals.

  atan: on |t| <= 7/16,  atan(t) = t - t * (z * A(z)),  z = t*t,  A(z) ~ (t - atan t) / t^3 = 1/3 - z/5 + z^2/7 - ..
        the argument is brought there by  atan x = atan c + atan((x - c) / (1 + c x))  for c in {0.5, 1, 1.5}  and  atan x = pi/2 - atan(1/x)
  tan:  on 0 <= x <= pi/4, tan(x) = x + x * (z * T(z)),  z = x*x,  T(z) ~ (tan x - x) / x^3 = 1/3 + 2 z/15 + ..
        beyond pi/4 the caller takes 1 / tan(pi/2 - x)

A and T are the polynomials that interpolate the two functions at the Chebyshev nodes of the z interval (near-minimax for functions this
smooth), solved in monomial form at 60 digits and then rounded to double once. The script reports the approximation error of the ROUNDED
polynomials in exact arithmetic, relative to atan / tan; the error of the double evaluation is measured by tests/test_fisheye_twin.py.

    python scripts/derive_atan_tan.py            # prints the literals
"""
import mpmath as mp

mp.mp.dps = 60

ATAN_DEG, TAN_DEG = 13, 16
ATAN_ZMAX = mp.mpf(7) / 16 * mp.mpf(7) / 16
TAN_ZMAX = (mp.pi / 4) ** 2 * (1 + mp.mpf(2) ** -40)     # (the double pi/4 and a little more)


def atan_core(z):
    if z == 0:
        return mp.mpf(1) / 3
    t = mp.sqrt(z)
    return (t - mp.atan(t)) / (t * z)


def tan_core(z):
    if z == 0:
        return mp.mpf(1) / 3
    x = mp.sqrt(z)
    return (mp.tan(x) - x) / (x * z)


def cheb_interp(f, zmax, deg):
    """monomial coefficients (lowest first) of the interpolant of f at the deg + 1 Chebyshev nodes of [0, zmax]"""
    n = deg + 1
    nodes = [zmax / 2 * (1 + mp.cos(mp.pi * (2 * k + 1) / (2 * n))) for k in range(n)]
    V = mp.matrix(n, n)
    for r, z in enumerate(nodes):
        for c in range(n):
            V[r, c] = z ** c
    return list(mp.lu_solve(V, mp.matrix([f(z) for z in nodes])))


def as_double(v):
    return float(mp.nstr(v, 40))      # (Python rounds the decimal string to the nearest double)


def horner(co, z):
    acc = mp.mpf(0)
    for c in reversed(co):
        acc = acc * z + mp.mpf(c)
    return acc


def hi_lo(v):
    hi = as_double(v)
    return hi, as_double(v - mp.mpf(hi))


def main():
    a = [as_double(c) for c in cheb_interp(atan_core, ATAN_ZMAX, ATAN_DEG)]
    t = [as_double(c) for c in cheb_interp(tan_core, TAN_ZMAX, TAN_DEG)]
    worst_a = worst_t = mp.mpf(0)
    for k in range(1, 4001):
        x = mp.mpf(7) / 16 * k / 4000
        z = x * x
        worst_a = max(worst_a, abs((x - x * z * horner(a, z)) / mp.atan(x) - 1))
        x = mp.sqrt(TAN_ZMAX) * k / 4000
        z = x * x
        worst_t = max(worst_t, abs((x + x * z * horner(t, z)) / mp.tan(x) - 1))
    print("// atan: degree %d in z on [0, 49/256]; approximation error of the rounded polynomial, relative: %s" % (ATAN_DEG, mp.nstr(worst_a, 3)))
    print(",\n".join("    " + ", ".join(c.hex() for c in a[i:i + 4]) for i in range(0, len(a), 4)))
    print("// tan: degree %d in z on [0, (pi/4)^2]; approximation error of the rounded polynomial, relative: %s" % (TAN_DEG, mp.nstr(worst_t, 3)))
    print(",\n".join("    " + ", ".join(c.hex() for c in t[i:i + 4]) for i in range(0, len(t), 4)))
    for name, v in (("atan(0.5)", mp.atan(mp.mpf(1) / 2)), ("atan(1)", mp.pi / 4), ("atan(1.5)", mp.atan(mp.mpf(3) / 2)), ("pi/2", mp.pi / 2)):
        hi, lo = hi_lo(v)
        print("// %-9s hi %s  lo %s" % (name, hi.hex(), lo.hex()))
    print("// pi/4 as a double: %s" % as_double(mp.pi / 4).hex())


if __name__ == "__main__":
    main()
