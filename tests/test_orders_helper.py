"""CPU checks of the ranking comparison the planner tests use (tests/_util.order_mismatch)."""
import numpy as np

from tests._util import order_mismatch, orders_equivalent


def test_exact_ties_must_stay_tied_and_in_generation_order(golden):
    g = golden("planner")
    cost, order = g["cost"][0], g["order"][0]
    assert cost[0] == cost[18]                                    # an exact tie of the reference (heading 0)
    assert orders_equivalent(cost, order, cost, order)
    # the tie swapped in the ranking: rejected
    swapped = order.copy()
    i, j = list(order).index(0), list(order).index(18)
    swapped[i], swapped[j] = swapped[j], swapped[i]
    assert order_mismatch(cost, order, cost, swapped) is not None
    # the device split the tie by an ulp (its atan2 rounds differently) and ranks it by its own costs: accepted
    split = cost.copy()
    split[0] = np.nextafter(split[0], np.inf)
    assert orders_equivalent(cost, order, split, swapped)
    # ... but not by more than a near-tie
    split[0] = split[18] * (1 + 1e-6)
    assert "tie" in order_mismatch(cost, order, split, swapped)


def test_near_ties_may_swap_but_nothing_else():
    cost = np.array([3.0, 1.0, 1.0 + 4e-16, 2.0, 1.0 + 1e-6])
    order = np.argsort(cost, kind="stable")                        # [1, 2, 4, 3, 0]
    near = order.copy()
    near[[0, 1]] = near[[1, 0]]                                    # 1 and 2 differ by 4e-16: a near-tie
    assert orders_equivalent(cost, order, cost, near)
    far = order.copy()
    far[[1, 2]] = far[[2, 1]]                                      # 2 and 4 differ by 1e-6 relative
    assert not orders_equivalent(cost, order, cost, far)
    assert not orders_equivalent(cost, order, cost, order[:-1].tolist() + [order[0]])     # not a permutation
