"""The two statements of the closed-loop routes agree, without a GPU: the C entries of include/dpilqr_policy.h (the limits of
csrc/launch.hpp's closed-loop section, tested by the launchers) answer DPILQR_OK for exactly the shapes batch.route_serves says
their route serves -- every family, every k in 1 .. 65, all eight entries.  The batch is empty and the pointers are fake: an entry
that accepts the shape returns before any HIP call, one that refuses it does so before it looks at B."""
import pytest

from tests import closed_loop_refusal_cases as rc

FAMILIES = ((3, 2), (4, 2), (5, 2), (6, 3), (12, 4))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def test_c_entries_serve_exactly_what_the_route_table_says(lib):
    from dpilqr_amd.batch import ProblemBatch, route_serves
    n, differ = 0, []
    for name in rc.METHODS:
        route = ProblemBatch.CLOSED_LOOP[name][0]
        for ns, nc in FAMILIES:
            for k in range(1, 66):
                kind, rcode, text = rc.c_call(lib, name, rc.empty_desc(lib, k, ns, nc), kc_max=k)
                n += 1
                if (rcode == lib.OK) != route_serves(route, k, ns, nc) or rcode not in (lib.OK, lib.EUNSUPPORTED):
                    differ.append((name, k, ns, nc, rcode, text))
    assert n == 8 * 5 * 65 == 2600
    assert not differ, differ[:10]


def test_the_route_table_is_the_documented_one():
    """include/dpilqr_policy.h's words: small n_x <= 60 and k <= 20; large 60 < n_x <= 240, k <= 20, three families; team k <= 64,
    twelve bikes."""
    from dpilqr_amd.batch import ProblemBatch, route_refusal, route_serves
    served = lambda route: {(k, ns, nc) for ns, nc in FAMILIES for k in range(1, 66) if route_serves(route, k, ns, nc)}
    assert served("small") == {(k, ns, nc) for ns, nc in FAMILIES for k in range(1, 21) if k * ns <= 60}
    assert served("large") == {(k, ns, nc) for ns, nc in ((4, 2), (6, 3), (12, 4)) for k in range(1, 21) if 60 < k * ns <= 240}
    assert served("team") == {(k, ns, nc) for ns, nc in FAMILIES for k in range(1, 65) if ns != 5 or k <= 12}
    assert not served("small") & served("large") and served("small") | served("large") <= served("team")
    assert route_refusal("large", 15, 4, 2) == "below" and route_refusal("large", 21, 4, 2) == "beyond"
    assert route_refusal("team", 65, 5, 2) == "beyond" and route_refusal("team", 13, 5, 2) == "family"
    assert sorted(ProblemBatch.CLOSED_LOOP) == sorted(rc.METHODS)
    assert {name: route for name, (route, _) in ProblemBatch.CLOSED_LOOP.items()} == {
        name: "large" if name.endswith("_large") else "team" if name.endswith("_team") else "small" for name in rc.METHODS}
