"""The unit plan of a speed-field solve on fused passes (schedule.cpp plan_units, SpeedPlan::kFused), through its
binding: K = 1..12 x check cadence 1, 2, 4, 5. No GPU: the plan is host code.

A fused plan is the pass split of a stored start at n = 1: the units follow each other from n = 1 to K - 1 steps in all,
none is an analytic start (a speed solve has none), none leaves u^{K-1} out (drop_prev stays off with a coefficient), and
none is deeper than the coefficient passes are built. A pass checks any of its levels itself, so a fused unit may span
check steps, and every check step must fall on a level of exactly one unit; a single step checks its own level; where
the plan falls back to two-step pairs (temporal = 2, tb off) a pair must not span one, because k_leapfrog2 checks its
last level only."""
import pytest

from test_speed_cpu import speed_spec

KS = list(range(1, 13))
CADENCES = [1, 2, 4, 5]
FUSED, PAIRS = 3, 1


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _plan(K, every, speed=FUSED, **opts):
    C = _C()
    o = C.SolverOptions()
    o.check_every = every
    for k, v in opts.items():
        setattr(o, k, v)
    return C.plan_units(speed_spec(24, False, 2.0, K_=K, check_every=every).native(), o, start_n=1, analytic=False,
                        sources=False, speed=speed)


def _is_check(n, K, every):
    return n >= 1 and (n % every == 0 or n == K)


@pytest.mark.parametrize("temporal", [3, 4, 5])
@pytest.mark.parametrize("every", CADENCES)
@pytest.mark.parametrize("K", KS)
def test_fused_plan(K, every, temporal):
    C = _C()
    units = _plan(K, every, temporal=temporal)
    n = 1
    for u in units:
        assert u["n"] == n and u["steps"] >= 1
        assert u["steps"] <= min(temporal, C.p2_varc_max_stages)
        assert not u["drop_prev"] and not u["analytic"] and not u["exchange"]
        # a unit crosses a check step only if it is an LDS pass, which checks any of its levels; a single step checks
        # its own (last) level
        assert u["lds_pass"] == (u["steps"] >= 2)
        assert all(c == n + u["steps"] for c in u["checked"]) or u["lds_pass"]
        n += u["steps"]
    assert sum(u["steps"] for u in units) == K - 1 and n == max(K, 1)
    # every check step after the stored start falls on a level that one unit checks, exactly once
    got = [c for u in units for c in u["checked"]]
    assert got == [m for m in range(2, K + 1) if _is_check(m, K, every)]
    # deep passes wherever the steps allow one: at most one unit per `depth` steps, plus the tail
    depth = min(temporal, C.p2_varc_max_stages)
    assert len(units) <= (K - 1) // depth + 2
    if K - 1 >= 3:
        assert max(u["steps"] for u in units) > 2, "no fused pass of more than two steps was planned"


@pytest.mark.parametrize("opts", [dict(temporal=2), dict(tb=False), dict(temporal=1)], ids=["t2", "no-tb", "t1"])
@pytest.mark.parametrize("every", CADENCES)
@pytest.mark.parametrize("K", KS)
def test_fallback_is_the_pair_plan(K, every, opts):
    """temporal <= 2 or tb off: a fused request plans what the pair plan does, and no pair spans a check step."""
    units = _plan(K, every, **opts)
    assert units == _plan(K, every, speed=PAIRS, **opts)
    n = 1
    for u in units:
        assert u["n"] == n and u["steps"] in (1, 2) and not u["drop_prev"] and not u["analytic"]
        assert not u["lds_pass"] and all(c == n + u["steps"] for c in u["checked"])
        if u["steps"] == 2:
            assert not _is_check(n + 1, K, every), "a two-step pair crosses a check step"
        n += u["steps"]
    assert sum(u["steps"] for u in units) == K - 1
    assert [c for u in units for c in u["checked"]] == [m for m in range(2, K + 1) if _is_check(m, K, every)]
