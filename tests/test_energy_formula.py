"""CPU: the hoisted form of the attention energies (csrc/common.h: vag_energy_exp, vag_energy_tanh), restated step by step in fp32
(tests/energy_ref.py), against float64 tanh(a + b).

Bound: TANH_ABS = 2^-20 of tests/ground_ref.py, the one vag_tanh is held to, for every pair with |a|, |b| <= 39 -- with the
exponential and the reciprocal exact, and with each erring by what ground_ref grants it (ULP, RCP_REL) in every sign pattern.
Where it comes from: the product Ea Eq carries the two exponentials' errors, two roundings of the compensation and its own, about
3.5 * 2^-23 relative at worst, and enters tanh through 2e / (e + 1)^2 <= 1/2; the reciprocal's 2^-22 enters as 2 r 2^-22 <= 2^-21;
the last fma rounds at 2^-24: below 0.75 * 2^-20 in all, nowhere all at once.

The uncompensated form (argument x K rounded once) is here too, so that the compensation cannot be dropped silently: its factors
carry |y| 2^-24 ln 2 each, and where a and b are large and nearly cancel nothing damps that.  On this grid it misses the bound
(3.0 x at (-24.912766, 24.912704)).  At (10, -9), the pair the change's description names, it does NOT: |y| is 29 there, the two
roundings together are at most 1.3e-6 relative and the slope 2e / (e + 1)^2 at a + b = 1 is 0.21 -- it stays under 0.3 of the
bound with every granted error (0.15 with none).  The test asserts what is true of that pair and finds the failure where it is."""
import numpy as np

import energy_ref as E
import ground_ref as G


def _range(rcp_rel):
    """[-1, 1]: Ea Eq + 1 >= 1, so a reciprocal that does not err upward gives r in [0, 1] and 1 - 2r in [-1, 1] exactly (the device's
    own instruction is held to that in tests/test_gpu_attn_energy.py).  A reciprocal GRANTED an upward error of rel leaves the
    interval at Ea Eq = 0 by exactly what it was granted, 2 rel."""
    return 1.0 + 2.0 * max(rcp_rel, 0.0)


def test_grid_is_what_the_bound_is_claimed_for():
    a, b = E.grid()
    assert a.size >= 100000 and a.dtype == np.float32 and b.dtype == np.float32
    assert np.abs(a).max() == E.DOMAIN and np.abs(b).max() == E.DOMAIN
    assert (a == 0).any() and ((a != 0) & (np.abs(a) < 1e-38)).any()                    # zeros and denormals
    s = np.abs(a.astype(np.float64) + b.astype(np.float64))
    big = np.minimum(np.abs(a), np.abs(b)) > 30
    assert (big & (s <= 2.0 ** -19)).any() and (big & (s >= 3.9)).any()                 # large operands cancelling to 2^-20 .. 4
    assert ((a > 0) & (b < 0)).any() and ((a < 0) & (b > 0)).any() and ((a < 0) & (b < 0)).any()


def test_every_pair_of_the_domain_is_within_the_tanh_bound():
    a, b = E.grid()
    ref = E.reference(a, b)
    for exp_rel, rcp_rel in E.GRANTS:
        got = E.energy(a, b, exp_rel, rcp_rel).astype(np.float64)
        err = np.abs(got - ref)
        k = int(err.argmax())
        print("exp_rel %+.1e rcp_rel %+.1e: worst %.3f of TANH_ABS at (%r, %r)" % (exp_rel, rcp_rel, err[k] / G.TANH_ABS, a[k], b[k]))
        assert np.isfinite(got).all() and (np.abs(got) <= _range(rcp_rel)).all()
        assert (err <= G.TANH_ABS).all(), (exp_rel, rcp_rel, a[k], b[k], err[k] / G.TANH_ABS)


def test_outside_the_domain_the_result_saturates():
    a, b, sign = E.outside()
    for exp_rel, rcp_rel in E.GRANTS:
        got = E.energy(a, b, exp_rel, rcp_rel).astype(np.float64)
        assert np.isfinite(got).all() and (np.abs(got) <= _range(rcp_rel)).all()
        asked = sign != 0
        assert (np.sign(got[asked]) == sign[asked]).all()
    # the factors themselves: finite and positive for every input, so that no product is inf * 0
    e = E.energy_exp(np.array([np.inf, -np.inf, 1e4, -1e4, 0.0], dtype=np.float32))
    assert np.isfinite(e).all() and (e > 0).all()
    with np.errstate(over="ignore", under="ignore"):
        assert e[0] * e[0] == np.inf and e[1] * e[1] == 0.0


def test_a_plainly_rounded_argument_misses_the_bound():
    a, b = E.grid()
    ref = E.reference(a, b)
    worst, at = 0.0, None
    for exp_rel, rcp_rel in E.GRANTS:
        err = np.abs(E.energy(a, b, exp_rel, rcp_rel, compensated=False).astype(np.float64) - ref)
        k = int(err.argmax())
        if err[k] > worst:
            worst, at = err[k], (a[k], b[k])
    print("uncompensated: worst %.2f of TANH_ABS at %r" % (worst / G.TANH_ABS, at))
    assert worst > 2.0 * G.TANH_ABS                       # ... with the instructions exact as well:
    assert np.abs(E.energy(a, b, compensated=False).astype(np.float64) - ref).max() > G.TANH_ABS
    assert min(abs(at[0]), abs(at[1])) > 20.0             # where the operands are large
    # (10, -9): inside the bound in either form (see the module docstring)
    p = (np.array([10.0], dtype=np.float32), np.array([-9.0], dtype=np.float32))
    for exp_rel, rcp_rel in E.GRANTS:
        e10 = abs(float(E.energy(*p, exp_rel, rcp_rel, compensated=False)[0]) - np.tanh(1.0))
        assert e10 < 0.3 * G.TANH_ABS
