"""``hostprep.route`` and the classifiers built on it against the recorded answers in
tests/golden/method_routes.json (tests/golden/make_golden_routes.py: 7,865 method strings — the
prefix x name x suffix grid, all ordered pairs of names, every method string the suite, the golden
generators, bench.py and BASELINE.json mention — recorded from the classifiers as they were before
they were folded into one router): same value or same exception class for every string, both
``is2d``; and ``route`` puts every string into exactly the family those answers imply."""
import importlib.util
import json
import os

import pcgmix_amd  # noqa: F401
from pcgmix_amd import hostprep as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_routes", os.path.join(GOLDEN, "make_golden_routes.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(os.path.join(GOLDEN, "method_routes.json")) as _f:
    FIXTURE = json.load(_f)
RECORDED = G.decode(FIXTURE)


def test_fixture_covers_the_corpus():
    assert tuple(FIXTURE["functions"]) == G.FUNCTIONS and FIXTURE["recorded_from_commit"]
    assert [tuple(FIXTURE[k]) for k in ("prefixes", "names", "suffixes")] == [G.PREFIXES, G.NAMES, G.SUFFIXES]
    assert G.PREFIXES[0] == "" and set(FIXTURE["grid_changes"]) <= set(G.PREFIXES[1:])
    grid = {p + n + s for p in G.PREFIXES for n in G.NAMES for s in G.SUFFIXES}
    pairs = {a + " " + b for a in G.NAMES for b in G.NAMES}
    assert len(G.PREFIXES) * len(G.NAMES) * len(G.SUFFIXES) == 16 * 37 * 11 and len(pairs) == 37 * 37
    assert grid <= set(RECORDED) and pairs <= set(RECORDED)
    for text in ("durratiomixup", "durmixmagwarp(0.2,4)", "(saloptenv)durmixmagwarp(0.2,4)", "labelcutmix timewarp"):
        assert text in RECORDED
    # every chain name is a name of the grid
    for chain in (H._CHAIN_1D, H._CHAIN_2D):
        assert {name for name, _, _ in chain} <= set(G.NAMES)


def test_classifiers_reproduce_the_recorded_answers():
    wrong = [(m, G.answers(H, m), a) for m, a in RECORDED.items() if G.answers(H, m) != a]
    assert not wrong, f"{len(wrong)} of {len(RECORDED)} differ, first: {wrong[0]}"


def expected_family(answer, is2d):
    """The one family the recorded answers of the old classifiers imply."""
    sel = answer["select_method"]
    claims = []
    if answer["cutpaste_recipe"].get("v") is not None:
        claims.append("cutpaste")
    if not is2d and answer["latent_recipe"].get("v") is not None:
        claims.append("latent")
    if "v" in sel:
        if sel["v"] is None:
            claims.append("passthrough")
        elif sel["v"] in (H.PCGMIX_METHODS_2D if is2d else H.SPLICE_METHODS_1D):
            claims.append("splice")
        else:
            assert sel["v"] in (H.BASELINE_METHODS_2D if is2d else H.BASELINE_METHODS_1D)
            claims.append("baseline")
    else:
        assert sel["x"] == "NotImplementedError"
    assert len(claims) <= 1, claims                       # the old classifiers were a partition
    return claims[0] if claims else "refused"


def test_route_places_every_string_in_one_family():
    seen = set()
    for m, (one, two) in RECORDED.items():
        for is2d, answer in ((False, one), (True, two)):
            r = H.route(m, is2d)
            assert r.family == expected_family(answer, is2d), (m, is2d, r)
            seen.add((is2d, r.family))
            assert bool(r.refusal) == (r.family == "refused"), (m, is2d, r)
            if r.family in ("splice", "baseline"):
                assert r.branch == answer["select_method"]["v"]
            elif r.family == "cutpaste":
                assert r.branch == answer["cutpaste_recipe"]["v"]
            elif r.family == "passthrough":
                assert r.branch is None
            if r.family != "splice":
                assert r.plain is None and r.salopt is None
            if not is2d:
                assert r.soft_targets == answer["soft_targets"]["v"]
    families = {"passthrough", "splice", "baseline", "cutpaste", "refused"}
    assert seen == {(True, f) for f in families} | {(False, f) for f in families | {"latent"}}


def test_route_is_cached_and_never_raises():
    for m in ("durratiomixup", "(salopt)durmixmagwarp(smooth)", "cutmix", "mixup+0.5 timewarp"):
        assert H.route(m, False) is H.route(m, False)
    bad = H.route("(alpha=x)durmixmagwarp(smooth)", False)
    assert bad.family == "splice" and isinstance(bad.plain, ValueError)
    assert H.select_method("(alpha=x)durmixmagwarp(smooth)", False) == "durmixmagwarp"
    assert H.cutpaste_recipe("(alpha=x)durmixmagwarp(smooth)", False) is None
