"""Small-m ut_hash, one wave per row (hash.hip k_hash_wide), against
oracle.hashing.hash_config: digests are hashlib's, bit for bit, at every m up
to the wave-per-row limit and one past it (where the lane-per-row kernel takes
over), on spaces that exercise each digest source (computed, LUT, permutation),
messages shorter than a slab of 64 blocks, longer than one, ending on a block
boundary and ending with a block of padding alone.

One pool of LIMIT + 1 legal rows per space (the engine's own population
initialiser) and one oracle pass over it; every m hashes the pool's first m
columns.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _spaces import oracle_space  # noqa: E402
from oracle import hashing as oh  # noqa: E402
from oracle.space import row_values  # noqa: E402

LIMIT = 1024    # hash.hip HASH_WIDE_M
MS = [1, 2, 63, 64, 65, 511, 512, 513, LIMIT, LIMIT + 1]


def _one_param():
    """message of 52 + 69 = 121 bytes: the 0x80 fits block 1, the length does
    not, block 2 is padding alone"""
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return ConfigurationManipulator([FloatParameter("p" * 52, -1.0, 1.0)])


def _block_boundary():
    """a Float, an Int (LUT) and a Float whose name makes the message 4 * 64 bytes"""
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter, IntegerParameter
    fixed = (1 + 69) + (1 + 69)                # "a", "b": name + b' + 64 hex + ' + index + |
    return ConfigurationManipulator([FloatParameter("a", -5.0, 5.0), IntegerParameter("b", 1, 9),
                                     FloatParameter("c" * (256 - fixed - 69), 0.0, 1e6)])


def _spaces():
    from uptune_amd import spaces
    return {"r64": spaces.r64, "hpl64": spaces.hpl64, "perm": spaces.perm_mixed, "one_param": _one_param,
            "block_boundary": _block_boundary, "r80": lambda: spaces.r64(80), "gcc": spaces.gcc}


# (outer message bytes, outer blocks) where the case depends on them
INFO = {"r64": (4588, 72), "one_param": (121, 3), "block_boundary": (256, 5), "gcc": (30178, 472)}
NAMES = ["r64", "hpl64", "perm", "one_param", "block_boundary", "r80", "gcc"]

_POOL = {}


def pool(name):
    """-> (engine, values [ncols][LIMIT + 1] on the device, oracle hex digests)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if name not in _POOL:
        from uptune_amd.engine import BatchEngine
        manip = _spaces()[name]()
        e = BatchEngine(manip, device=0, seed=7)
        if name in INFO:
            assert e.space_info()[:2] == INFO[name]
        if name == "r80":
            assert e.space_info()[1] > 64          # the slab loop runs twice
        e.population_init(LIMIT + 1)
        vals = e.population_get().contiguous()
        osp = oracle_space(manip)
        host = vals.cpu().numpy()
        want = [oh.hash_config(osp, row_values(osp, host, j)) for j in range(LIMIT + 1)]
        _POOL[name] = (e, vals, want)
    return _POOL[name]


def hexes(d):
    from uptune_amd.engine import digests_to_hex
    return digests_to_hex(d)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", NAMES)
def test_hash_matches_hashlib(name, m):
    e, vals, want = pool(name)
    assert hexes(e.hash(vals[:, :m].contiguous())) == want[:m]


@pytest.mark.parametrize("name", ["r64", "hpl64", "perm"])
def test_hash_columns_of_a_wide_array(name):
    """a few columns of a wide array (ld != m): the scratch is sized and indexed by m"""
    e, vals, want = pool(name)
    for m in (1, 100, 513):
        assert hexes(e.hash(vals, m=m)) == want[:m]
