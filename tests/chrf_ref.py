"""chrF on surface characters restated in plain Python (include/vag_nmt.h: vag_chrf_select has the definition): Counter
intersections on strings, the utility in float64, and again in NumPy float32 with the header's operation order, which the kernel
must reproduce bit for bit."""
from collections import Counter

import numpy as np

ORDER = 6
EOS = 3
F32 = np.float32


def ngrams(s, n):
    return Counter(s[i:i + n] for i in range(len(s) - n + 1))


def matches(h, r):
    """[m_1 .. m_6] of two strings: m_n = sum over n-grams g of min(count_h(g), count_r(g))."""
    return [sum((ngrams(h, n) & ngrams(r, n)).values()) for n in range(1, ORDER + 1)]


def totals(l):
    return [max(0, l - n + 1) for n in range(1, ORDER + 1)]


def utility64(m, lh, lr):
    th, tr = totals(lh), totals(lr)
    eff = [n for n in range(ORDER) if th[n] > 0 and tr[n] > 0]
    if not eff:
        return 0.0
    P = sum(m[n] / th[n] for n in eff) / len(eff)
    R = sum(m[n] / tr[n] for n in eff) / len(eff)
    return 0.0 if P + R == 0 else 5.0 * P * R / (4.0 * P + R)


def utility32(m, lh, lr):
    """The header's order in IEEE float32: every division, product and sum is one NumPy float32 operation."""
    th, tr = totals(lh), totals(lr)
    sp, sr, E = F32(0), F32(0), 0
    for n in range(ORDER):
        if th[n] > 0 and tr[n] > 0:
            sp = sp + F32(m[n]) / F32(th[n])
            sr = sr + F32(m[n]) / F32(tr[n])
            E += 1
    if E == 0:
        return F32(0)
    P, R = sp / F32(E), sr / F32(E)
    if P + R == F32(0):
        return F32(0)
    u = ((F32(5) * P) * R) / ((F32(4) * P) + R)
    assert u.dtype == np.float32
    return u


def expected32(w, u):
    """sum_j w_j u_j in float32, j ascending from 0.0f, product and sum rounded separately."""
    e = F32(0)
    for wj, uj in zip(w, u):
        e = e + F32(wj) * F32(uj)
    return e


def pairwise(hs, rs, Ch, Cr):
    """Strings hs[b][i], rs[b][j], cut to their first Ch / Cr characters -> (m (B, Nh, Nr, 6) int64, u32 (B, Nh, Nr) float32,
    u64 (B, Nh, Nr) float64)."""
    B, Nh, Nr = len(hs), len(hs[0]), len(rs[0])
    m = np.zeros((B, Nh, Nr, ORDER), dtype=np.int64)
    u32 = np.zeros((B, Nh, Nr), dtype=np.float32)
    u64 = np.zeros((B, Nh, Nr), dtype=np.float64)
    for b in range(B):
        for i in range(Nh):
            h = hs[b][i][:Ch]
            for j in range(Nr):
                r = rs[b][j][:Cr]
                m[b, i, j] = matches(h, r)
                u32[b, i, j] = utility32(m[b, i, j], len(h), len(r))
                u64[b, i, j] = utility64(m[b, i, j], len(h), len(r))
    return m, u32, u64


def expected(w, u32):
    """w (B, Nr) float32 as the kernel reads it, u32 (B, Nh, Nr) -> (B, Nh) float32."""
    B, Nh, _ = u32.shape
    return np.array([[expected32(w[b], u32[b, i]) for i in range(Nh)] for b in range(B)], dtype=np.float32)


def first_argmax(e):
    return [int(np.flatnonzero(row == row.max())[0]) for row in e]
