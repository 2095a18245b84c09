#!/usr/bin/env python3
"""Derives the series swz_srs_parse evaluates (schwarzwald_amd/csrc/swz_srs.hip) with sympy and prints them: the six beta
coefficients of the inverse Krueger series (rectifying -> conformal latitude, chi = mu - sum beta_j sin 2 j mu), the six
delta coefficients of conformal -> geodetic latitude (phi = chi + sum delta_j sin 2 j chi) and the rectifying radius A, all
in the third flattening n to order n^6.

Everything is a Laurent polynomial in z = exp(2 i phi) whose coefficients are polynomials in n, truncated behind n^6:
  conformal latitude   chi(phi) = gd(psi0 - delta),  delta = e atanh(e sin phi) as a series in e^2 = 4 n / (1 + n)^2,
                       by Taylor's theorem in delta with D = d/dpsi = cos phi d/dphi, D phi = cos phi;
  rectifying latitude  mu(phi) = I(phi) / I(pi / 2) * pi / 2,  I = integral of (1 - e^2 sin^2 t)^(-3/2), the binomial series
                       integrated term by term;
  then phi(mu) by fixed-point iteration, and chi(phi(mu)).
Run: python tools/srs_series.py"""
import sympy as sp

ORDER = 6
n, z, phi = sp.symbols("n z phi")


def trunc(expr):
    """the terms up to n^ORDER of a polynomial in n (Laurent in z)"""
    expr = sp.expand(expr)
    return sum(expr.coeff(n, k) * n ** k for k in range(ORDER + 1))


def to_z(expr):
    """sin / cos phi -> z = exp(2 i phi); only even total degree in (sin, cos) x odd functions appear, via w = sqrt z"""
    w = sp.symbols("w")
    e = expr.subs({sp.sin(phi): (w - 1 / w) / (2 * sp.I), sp.cos(phi): (w + 1 / w) / 2})
    e = sp.expand(e)
    return sp.expand(e.subs(w, sp.sqrt(z)))


def fourier(expr_z, terms):
    """coefficients c_k of sum c_k sin 2 k phi from the Laurent polynomial: c_k = 2 i * [z^k]"""
    expr_z = sp.expand(expr_z)
    return [sp.simplify(2 * sp.I * expr_z.coeff(z, k)) for k in range(1, terms + 1)]


def e2_series():
    return trunc(sp.series(4 * n / (1 + n) ** 2, n, 0, ORDER + 1).removeO())


def chi_minus_phi():
    e2 = e2_series()
    s, c = sp.sin(phi), sp.cos(phi)
    delta = sum(trunc(e2 ** (k + 1)) * s ** (2 * k + 1) / (2 * k + 1) for k in range(ORDER))
    delta = trunc(delta)
    # D^k phi, D = cos phi d/dphi
    d = [phi, c]
    for _ in range(ORDER - 1):
        d.append(sp.expand(c * sp.diff(d[-1], phi)))
    total, power = 0, 1
    for k in range(1, ORDER + 1):
        power = trunc(power * (-delta))
        total += power * d[k] / sp.factorial(k)
    return trunc(to_z(trunc(total)))


def mu_minus_phi():
    e2 = e2_series()
    t = sp.symbols("t")
    integral, quarter = 0, 0
    for k in range(ORDER + 1):
        binom = sp.binomial(sp.Rational(-3, 2), k) * (-1) ** k
        prim = sp.integrate(sp.sin(t) ** (2 * k), (t, 0, phi))
        lin = sp.integrate(sp.sin(t) ** (2 * k), (t, 0, sp.pi / 2)) / (sp.pi / 2)  # the part proportional to phi
        coeff = trunc(binom * e2 ** k)
        integral += coeff * sp.expand(prim - lin * phi)
        quarter += coeff * lin
    quarter = trunc(quarter)
    inv = trunc(sp.series(1 / quarter, n, 0, ORDER + 1).removeO())
    return trunc(to_z(trunc(sp.expand(integral) * inv))), quarter


def shift(coeffs, eps):
    """sum c_k sin 2 k (x + eps) as a Laurent polynomial in z = exp(2 i x), eps a small Laurent polynomial"""
    total = 0
    for k, ck in enumerate(coeffs, start=1):
        base = (z ** k - z ** (-k)) / (2 * sp.I)
        power = 1
        term = base
        for p in range(1, ORDER + 1):
            power = trunc(power * eps)
            if power == 0:
                break
            base = sp.expand(2 * sp.I * z * sp.diff(base, z))  # d/dx of a function of z = exp(2 i x)
            term += power * base / sp.factorial(p)
        total += ck * term
    return trunc(total)


def main():
    chi = fourier(chi_minus_phi(), ORDER)
    mu_z, quarter = mu_minus_phi()
    mu = fourier(mu_z, ORDER)
    # phi = mu + eps(mu), eps = -sum mu_k sin 2 k (mu + eps)
    eps = 0
    for _ in range(ORDER):
        eps = trunc(-shift(mu, eps))
    # chi(mu) - mu = eps + sum chi_k sin 2 k (mu + eps)
    beta = [sp.factor(-b) for b in fourier(trunc(eps + shift(chi, eps)), ORDER)]
    for j, b in enumerate(beta, start=1):
        print("beta%d =" % j, sp.Poly(sp.expand(b), n).as_expr())
    # geodetic from conformal latitude: phi = chi + eps(chi), eps = -sum chi_k sin 2 k (chi + eps)
    eps = 0
    for _ in range(ORDER):
        eps = trunc(-shift(chi, eps))
    for j, d in enumerate(fourier(eps, ORDER), start=1):
        print("delta%d =" % j, sp.Poly(sp.expand(d), n).as_expr())
    # A = a * (1 - e^2) * I(pi/2) / (pi/2), 1 - e^2 = ((1 - n) / (1 + n))^2: print A (1 + n) / a
    radius = trunc(sp.series((1 - n) ** 2 / (1 + n) * quarter, n, 0, ORDER + 1).removeO())
    print("A (1 + n) / a =", sp.Poly(radius, n).as_expr())


if __name__ == "__main__":
    main()
