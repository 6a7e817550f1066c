"""Precision-8 dense scoring's call plan and hint policy (uptune_amd/csrc/gp_i8_plan.h), restated in Python
from their description: what one call runs given the three per-call overrides and the hints, and what the
counts a call reads back make of the hints.  tests/test_i8_plan_cpu.py holds the library's functions to it;
tests/test_gpu_kstar_screen.py steps it beside a real context."""
from collections import namedtuple

UNSET = -1                      # an override that is not in the environment (else 0 or 1)
MASK_MAX_K, QS_MAX_K32 = 2048, 4
UNMASKED, MASKED, LIST = 0, 1, 2

Env = namedtuple("Env", "var_skip screen strips", defaults=(UNSET, UNSET, UNSET))
Hints = namedtuple("Hints", "var_skip screen list backoff", defaults=(True, False, False, 0))
Plan = namedtuple("Plan", "mask screen count var")
Counts = namedtuple("Counts", "nsparse cert zero_bytes blocks")

NO_MASK = Plan(False, False, False, UNMASKED)   # a K* that is not k_gp_kstar_q's


def plan(npad, k32, env, hints):
    """a k_gp_kstar_q call of npad training rows and k32 32-feature stages"""
    masked_exists = npad <= MASK_MAX_K
    # the screen needs a masked variance kernel behind it (UT_VAR_SKIP=0 forbids one) and its planes in LDS
    allowed = masked_exists and k32 <= QS_MAX_K32 and env.var_skip != 0
    if env.screen == UNSET:
        screen, count = allowed and hints.screen, allowed and not hints.screen
    else:
        screen, count = allowed and env.screen == 1, False
    if screen:
        on_list = hints.list if env.strips == UNSET else env.strips == 1
        return Plan(True, True, False, LIST if on_list else MASKED)
    skip = hints.var_skip if env.var_skip == UNSET else env.var_skip == 1
    return Plan(True, False, count, MASKED if skip and masked_exists else UNMASKED)


def hints_next(hints, p, n):
    if not p.mask:
        return hints
    if p.screen:
        zero = 8 * n.cert           # a certified unit is 8 blocks that were never visited to be counted
        sparse = n.nsparse + zero
    else:
        zero = n.zero_bytes if p.count else 0
        sparse = n.nsparse
    screen, backoff = 2 * zero >= n.blocks, hints.backoff
    if p.screen:
        if not screen:
            backoff = 8             # a screen that cleared under half: held off for 8 unscreened calls
    elif backoff > 0:
        screen, backoff = False, backoff - 1
    return Hints(16 * sparse >= n.blocks, screen, 8 * zero >= 7 * n.blocks, backoff)
