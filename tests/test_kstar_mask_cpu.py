"""The K* sparsity table (tests/_kstar_mask_cases.py) checked on the CPU, so the
device tests (test_gpu_kstar_mask.py) cannot pass vacuously:
 a. the restated planes' occupancy masks contain at least one 32 x 32 block of
    every class -- no plane, each of 1 to 5 leading zero planes, all six -- and a
    128-candidate strip with a dead k stage between two live ones, one with four
    different block masks at one stage, and one with no live stage at all;
 b. where K*'s all-zero blocks come from: wherever the restated exponent x is
    <= -49 * 256 t units all six stored digits are zero (ks <= sf2 2^-eb
    2^(x / 256) < 2^-49, so rint(ks 2^48) = 0), and the 'edge' blocks put
    elements on both sides of that threshold;
 c. the module's restatement is _kstar_cases.restate_q's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _kstar_cases as KC  # noqa: E402
import _kstar_mask_cases as MC  # noqa: E402

# (the restatement of the large cases is a few seconds of matmuls: the table-wide checks share it)
SMALL = [c for c in MC.CASES if c["n"] * c["m"] <= 1000 * 300]


def test_restatement_is_restate_q():
    for c in (MC.CASES[2], MC.CASES[3]):
        z = MC.data(c)
        assert np.array_equal(MC.restate(c)[1], KC.restate_q(z["X"], z["U"], z["ell"], c["sf2"]))


def test_table_reaches_the_shapes():
    assert {c["n"] for c in MC.CASES} == {1, 129, 1000, 2000, 2100}
    assert KC.npad_of(2000) == 2048 and KC.npad_of(2100) > 2048   # at and past the masked kernel's limit
    assert {c["m"] for c in MC.CASES} == {1, 127, 129, 300, 5000}
    assert {c["d"] for c in MC.CASES} == {64, 100} and {c["sf2"] for c in MC.CASES} == {1.0, 1e-3}
    assert any(c["pre_m"] for c in MC.CASES) and any(c["fit_async"] for c in MC.CASES)
    assert [KC.k32_of(d) * 32 <= KC.PAIR_MAX_K for d in (64, 100)] == [True, False]


def test_every_mask_class_is_present():
    classes, dead_between, four_masks, dead_strip = set(), False, False, False
    for c in MC.CASES:
        mk = MC.expected_mask(c)
        nrb, nst = (c["n"] + 31) // 32, (c["m"] + 127) // 128
        blk = mk[:nrb, :(c["m"] + 31) // 32]
        classes |= {"none" if b == 0 else ("all" if b == 0x3f else MC.leading_zero_planes(b))
                    for b in np.unique(blk)}
        for s in range(nst):
            strip = mk[:nrb, 4 * s:4 * s + 4]
            live = strip.any(axis=1)
            idx = np.flatnonzero(live)
            dead_strip |= idx.size == 0
            dead_between |= idx.size > 0 and not live[idx[0]:idx[-1] + 1].all()
            four_masks |= any(len(set(row.tolist())) == 4 for row in strip)
    print("classes", sorted(map(str, classes)), "dead stage between live ones", dead_between,
          "four masks in a strip", four_masks, "strip with no live stage", dead_strip)
    assert classes >= {"none", "all", 1, 2, 3, 4, 5}
    assert dead_between and four_masks and dead_strip


def test_partial_masks_lead_with_zero_planes():
    """K* is non-negative under one exponent: a block's zero planes are its leading
    ones in (nearly) every block, which is what the masked variance kernel skips;
    the count of blocks with a zero plane behind a non-zero one is printed"""
    inner = total = 0
    for c in SMALL:
        mk = MC.expected_mask(c)
        nz = mk[mk != 0].astype(np.int64)
        total += nz.size
        inner += int(np.count_nonzero(nz + (nz & -nz) != 0x40))
    print("blocks with a plane: %d, of them with a zero plane behind a non-zero one: %d" % (total, inner))
    assert inner * 100 <= total


@pytest.mark.parametrize("c", MC.CASES, ids=MC.ids())
def test_zero_digits_under_the_threshold(c):
    t, k = MC.restate(c)
    under = t <= MC.T_UNDER
    assert not np.any(k[under] != 0.0), "a stored digit under the threshold"
    print("%s: %d of %d elements under the threshold, %d within 200 t units of it"
          % (c["name"], int(under.sum()), under.size, int(np.count_nonzero(np.abs(t - MC.T_UNDER) < 200.0))))
    # the threshold has a digit to spare: no element below 2^-49 of the scale holds one either
    s0 = c["sf2"] * 2.0 ** -KC.i8_kstar_exp(c["sf2"])
    assert not np.any(k[t < 256.0 * (-49.0 - np.log2(s0))] != 0.0)
