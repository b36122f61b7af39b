"""Every training-episode route of dkt_amd.ops (tests/episode_routes.py) makes exactly the library launches it is known to make, in that order, once each:
the forward and the backward half separately, read from ops.kernel_timing (its keys come in order of first launch).  A route that grows a launch, loses one,
reorders two or launches for a gradient nobody asked for fails here."""
import pytest

import episode_routes as er

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", er.ROUTES, ids=lambda r: r.name)
def test_route_launches_exactly_these_kernels_in_this_order(route, cuda):
    got = er.run(route, cuda, launches=True)
    print(route.name, "forward", got["forward"], "backward", got["backward"])
    assert got["forward"] == [(k, 1) for k in route.forward]
    assert got["backward"] == [(k, 1) for k in route.backward]
    assert (got["outs"][route.e_index] is None) if route.e_is_none else all(o is not None for o in got["outs"])
    assert got["grads"] and all(g is not None for g in got["grads"].values())
