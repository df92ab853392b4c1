"""The attention energies' hoisted form (csrc/common.h: vag_energy_exp / vag_energy_tanh) restated in numpy, and the grid of
operand pairs it is held to -- shared by tests/test_energy_formula.py (host) and tests/test_gpu_attn_energy.py (the device's probe).

Every step is an fp32 step.  A fused multiply-add is formed in float64 and rounded once: the product of two fp32 numbers is exact
there, and the one addition behind it rounds at 2^-53 before the rounding to fp32.  The exponential and the reciprocal are numpy's,
rounded to fp32, times (1 + rel): rel is the relative error tests/ground_ref.py grants the device's instructions (ULP for
v_exp_f32, RCP_REL for v_rcp_f32), with either sign."""
import numpy as np

import ground_ref as G

f32 = np.float32
K = 2.0 * np.log2(np.e)
K_HI = f32(K)
K_LO = f32(K - float(K_HI))
LN2 = f32(np.log(2.0))
XMAX = f32(39.856)            # common.h: VAG_ENERGY_XMAX, |y_hi| <= 115
DOMAIN = 39.0                 # |a|, |b| <= DOMAIN: within TANH_ABS of tanh(a + b)


def _fma(a, b, c):
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def energy_exp(x, rel=0.0, compensated=True):
    """exp(2x) as the kernels form it; compensated=False: the argument x K rounded once and nothing else (what the header says
    must not be done)."""
    x = np.asarray(x, dtype=f32)
    xc = np.minimum(np.maximum(x, -XMAX), XMAX)
    y_hi = xc * K_HI
    e = (np.exp2(y_hi.astype(np.float64)).astype(f32).astype(np.float64) * (1.0 + rel)).astype(f32)
    if not compensated:
        return e
    y_lo = _fma(xc, np.broadcast_to(K_HI, xc.shape), -y_hi) + xc * K_LO
    return _fma(e, LN2 * y_lo, e)


def energy_tanh(Ea, Eq, rel=0.0):
    with np.errstate(over="ignore"):
        d = _fma(Ea, Eq, np.ones_like(Ea))
    r = ((1.0 / d.astype(np.float64)).astype(f32).astype(np.float64) * (1.0 + rel)).astype(f32)
    return _fma(np.full_like(r, -2.0), r, np.ones_like(r))


def energy(a, b, exp_rel=0.0, rcp_rel=0.0, compensated=True):
    return energy_tanh(energy_exp(a, exp_rel, compensated), energy_exp(b, exp_rel, compensated), rcp_rel)


# (exp_rel, rcp_rel): exact instructions, and every sign pattern of the granted errors (both exponentials erring the same way is the
# worst case for the product; opposite ways cancel)
GRANTS = [(0.0, 0.0)] + [(se * G.ULP, sr * G.RCP_REL) for se in (-1, 0, 1) for sr in (-1, 0, 1) if (se, sr) != (0, 0)]


def _magnitudes():
    m = np.concatenate([np.logspace(-6, np.log10(DOMAIN), 157), [1.0, 9.0, 10.0, DOMAIN]])
    tiny = np.array([0.0, 1.4e-45, 1e-40, 1.1754942e-38])                 # zero, the smallest denormal, a denormal, just below normal
    return np.concatenate([m, -m, tiny, -tiny[1:]]).astype(f32)


def grid():
    """(a, b), fp32, every |a|, |b| <= DOMAIN: all pairs of ~330 log-spaced values of both signs with zero and denormals, then the
    cancelling pairs (a, -a +- delta), delta = 2^-20 .. 4."""
    v = _magnitudes()
    a0, b0 = [x.ravel() for x in np.meshgrid(v, v, indexing="ij")]
    big = v[np.abs(v) >= 1e-3]
    d = (2.0 ** np.arange(-20, 3)).astype(f32)
    d = np.concatenate([d, -d])
    a1, d1 = [x.ravel() for x in np.meshgrid(big, d, indexing="ij")]
    b1 = (-a1 + d1).astype(f32)
    keep = np.abs(b1) <= DOMAIN
    a = np.concatenate([a0, a1[keep], [f32(10.0)]]).astype(f32)
    b = np.concatenate([b0, b1[keep], [f32(-9.0)]]).astype(f32)
    return a, b


def reference(a, b):
    return np.tanh(a.astype(np.float64) + b.astype(np.float64))


def outside():
    """Pairs with at least one operand beyond the domain, up to 1e4 and +-inf, and the sign the result must have (0: the clamped
    operands may cancel, the sign is not asked)."""
    far = np.array([39.5, 39.856, 39.9, 40.0, 50.0, 115.0, 1e3, 1e4, np.inf])
    far = np.concatenate([far, -far]).astype(f32)
    near = _magnitudes()
    A, B, S = [], [], []
    for x in far:
        A.append(np.full(near.size, x)); B.append(near); S.append(np.full(near.size, np.sign(x)))          # one operand in the domain:
        A.append(near); B.append(np.full(near.size, x)); S.append(np.full(near.size, np.sign(x)))          # XMAX - DOMAIN > 0 decides
        A.append(np.full(far.size, x)); B.append(far)
        S.append(np.where(np.sign(far) == np.sign(x), np.sign(x), 0.0))
    return np.concatenate(A).astype(f32), np.concatenate(B).astype(f32), np.concatenate(S)
