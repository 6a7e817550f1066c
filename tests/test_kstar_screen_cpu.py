"""The K* screen's certificate (k_q_screen, gp_kq.hip) restated in numpy and held, on
the CPU, to the restated digit planes: over the plane-occupancy mask's case table
and over borderline sweeps whose units sit a few t units either side of the line
(_kstar_screen_cases has the derivation, the slack and the effectiveness rule).

  safety         every element of every certified unit is zero in the restated planes
  effectiveness  every unit whose largest extended-precision t is below the line by
                 more than the certificate's remainder bound plus 2 t units is certified
  mutants        the remainder term dropped, the line moved by +256 t, padding rows
                 treated as live data, PAIR's scale used for d = 97: each is caught
                 by some case (it certifies a unit with a non-zero element, or fails
                 to certify a unit the effectiveness rule names)
"""
import numpy as np
import pytest

import _kstar_cases as KC
import _kstar_screen_cases as SC

CASES = SC.all_cases()

_CERT = {}


def _cert(c, mutant=None):
    key = (c["name"], mutant)
    if key not in _CERT:
        z = SC.inputs(c)
        _CERT[key] = SC.certificate(z["X"], z["U"], z["ell"], c["n"], c["m"], mutant)[0]
    return _CERT[key]


_MUST = {}


def _must(c):
    if c["name"] not in _MUST:
        z = SC.inputs(c)
        _MUST[c["name"]] = SC.must_certify(z["X"], z["U"], z["ell"], c["n"], c["m"])
    return _MUST[c["name"]]


def _caught(c, mutant):
    cert = _cert(c, mutant)
    unsafe = cert & ~SC.zero_units(SC.stored(c), c["n"], c["m"])
    weak = _must(c) & ~cert
    return bool(unsafe.any() or weak.any())


@pytest.mark.skipif(not KC.have_longdouble(), reason="the effectiveness rule's reference needs np.longdouble")
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_certificate(c):
    cert = _cert(c)
    zero = SC.zero_units(SC.stored(c), c["n"], c["m"])
    must = _must(c)
    print("%s: units %d, certified %d, all-zero %d, named by the rule %d" %
          (c["name"], cert.size, int(cert.sum()), int(zero.sum()), int(must.sum())))
    assert not (cert & ~zero).any(), "a certified unit holds a non-zero digit"
    assert not (must & ~cert).any(), "a unit far below the line is not certified"
    # all-padding units (no live row or column) are certified whatever the inputs
    npad, ldk = KC.npad_of(c["n"]), KC.ldk_of(c["m"])
    assert cert[(c["n"] + 63) // 64:, :].all() and cert[:, (c["m"] + 127) // 128:].all()
    assert cert.shape == (npad // 64, ldk // 128)


def test_sweep_sits_on_the_line():
    """the sweeps do what they are for: units on both sides within a few t units of the line,
    certified and uncertified ones among them"""
    near_below = near_above = 0
    for c in SC.SWEEP:
        z = SC.data(c)
        tm = SC.t_ext_unit_max(z["X"], z["U"], z["ell"], c["n"], c["m"])
        live = np.isfinite(tm)
        near_below += int(((tm[live] < SC.LINE) & (tm[live] > SC.LINE - 8.0)).sum())
        near_above += int(((tm[live] >= SC.LINE) & (tm[live] < SC.LINE + 8.0)).sum())
    assert near_below >= 2 and near_above >= 2, (near_below, near_above)
    some = [_cert(c)[: (c["n"] + 63) // 64, : (c["m"] + 127) // 128] for c in SC.SWEEP]
    assert any(s.any() for s in some) and any((~s).any() for s in some)


@pytest.mark.skipif(not KC.have_longdouble(), reason="the effectiveness rule's reference needs np.longdouble")
@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_mutant_caught(mutant):
    hits = [c["name"] for c in CASES if _caught(c, mutant)]
    print(mutant, "caught by", hits)
    assert hits, "no case tells the mutant %s from the certificate" % mutant
    if mutant == "pair_scale":
        assert any(c["d"] == 97 for c in CASES if c["name"] in hits)
