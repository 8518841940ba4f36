#!/usr/bin/env python3
"""Recorded answers of the method classifiers in ``hostprep``, as ``tests/golden/method_routes.json``.

    python tests/golden/make_golden_routes.py [--out FILE] [--hostprep FILE --commit REV]

Pure Python: needs neither the reference nor the library nor a GPU.  For every method string of a
corpus and both ``is2d`` the outcome of ``select_method``, ``plain_recipe``, ``cutpaste_recipe``
and (1D only: they take no ``is2d``) ``salopt_recipe``, ``latent_recipe``, ``soft_targets`` is
recorded — ``{"v": value}`` or ``{"x": exception class name}``.  The file holds each distinct 1D
and 2D answer once (``answers_1d`` / ``answers_2d``: the outcomes in the order of ``functions``),
each distinct pair of them once (``answers``), and per method string only the index of its pair:
``grid[name][suffix]`` for the empty prefix, ``grid_changes[prefix][name][suffix]`` for the rows
another prefix changes, ``pairs[first][second]`` and ``others`` (string -> index);
``decode`` gives {string: [1D answer, 2D answer]} back.  tests/test_method_routes_cpu.py asserts
that the package still gives these answers.

``--hostprep FILE`` records the answers of another revision's ``hostprep.py`` (e.g. the output of
``git show REV:<package>/hostprep.py``), loaded next to the package's own module.

The corpus:
  * the grid prefix x name x suffix below (16 x 37 x 11 = 6,512 combinations, 6,373 distinct strings);
  * every ordered pair of two names joined by a space (37 x 37);
  * every string literal in tests/*.py, tests/golden/make_golden*.py and bench.py, and every string
    in BASELINE.json, that holds one of the names (at most 120 characters, one line).
"""
import argparse
import ast
import glob
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PREFIXES = ("", "(rand)", "(saloptenv)", "(saloptsum5)", "(salopt)", "(samePCG)", "(sameDataset)",
            "(mixAll)", "(alpha=0.4)", "(sameCVD)", "(closestbins=3)", "(UMC-subset)", "(plus)",
            "saliency-", "manifold-", "label")
# every name the reference's two dispatchers know (augmentations.py:700-729, augmentations2d.py:
# 269-281), and four strings that only look like one
NAMES = ("durratiocutmix", "lengthcutmix", "datasetcutmix", "wav-durratiocutmix", "wavcutmix",
         "lc-nointrusion", "labelcutmix", "swapsysdia", "s1s2mask", "cont-cutmix", "saliency-cutmix",
         "latentmixup", "manifold-cutmix(ch)", "manifold-cutmix", "manifold-cutout(ch)",
         "manifold-cutout", "cutmix(ch)", "cutmix", "cutout(ch)", "cutout", "gaussiannoise",
         "magnitudewarp", "timewarp", "mixup", "timemask", "durratiomixup", "durmixmagwarp",
         "respiratoryscale", "durmixrespscale",
         "freqmask", "durmixfreqmask", "durmixtimemask", "durmixcutout",
         "durratiowavcutmix", "(UMC-subset)durratiocutmix", "nothing", "fcn")
SUFFIXES = ("", "(same)", "(mix)", "(0.2,4)", "(smooth)", "cutout", "(ch)", "(12,20)", "(t,f)",
            "+0.5", "(smooth)(cutout)+0.3")
FUNCTIONS = ("select_method", "plain_recipe", "cutpaste_recipe", "salopt_recipe", "latent_recipe",
             "soft_targets")


def literal_strings():
    """Method strings named in the suite, the golden generators, bench.py and BASELINE.json."""
    found = set()
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))
                   + glob.glob(os.path.join(HERE, "make_golden*.py"))) + [os.path.join(ROOT, "bench.py")]
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        found.update(n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str))

    def walk(node):
        if isinstance(node, str):
            found.add(node)
        elif isinstance(node, dict):
            for k, v in node.items():
                walk(k)
                walk(v)
        elif isinstance(node, list):
            for v in node:
                walk(v)
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        walk(json.load(f))
    names = [n for n in NAMES if n not in ("nothing", "fcn")]
    return sorted(s for s in found if len(s) <= 120 and "\n" not in s and any(n in s for n in names))


def outcome(fn, *args):
    try:
        value = fn(*args)
    except Exception as exc:                               # the class is part of the answer
        return {"x": type(exc).__name__}
    return {"v": json.loads(json.dumps(value))}            # tuples as lists, as the file holds them


def answers(H, method):
    """[1D answer, 2D answer] of one method string."""
    one = {"select_method": outcome(H.select_method, method, False),
           "plain_recipe": outcome(H.plain_recipe, method, False),
           "cutpaste_recipe": outcome(H.cutpaste_recipe, method, False),
           "salopt_recipe": outcome(H.salopt_recipe, method),
           "latent_recipe": outcome(H.latent_recipe, method),
           "soft_targets": outcome(H.soft_targets, method)}
    two = {"select_method": outcome(H.select_method, method, True),
           "plain_recipe": outcome(H.plain_recipe, method, True),
           "cutpaste_recipe": outcome(H.cutpaste_recipe, method, True)}
    return [one, two]


def load_hostprep(path=None):
    import pcgmix_amd  # noqa: F401
    if path is None:
        from pcgmix_amd import hostprep
        return hostprep
    spec = importlib.util.spec_from_file_location(pcgmix_amd.__name__ + ".hostprep_recorded", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod                           # dataclasses look the module up
    spec.loader.exec_module(mod)
    return mod


def record(H):
    """The file's content for the classifiers of module ``H``."""
    tables = {"answers_1d": [], "answers_2d": [], "answers": []}

    def index(key, value):
        table = tables[key]
        if value not in table:
            table.append(value)
        return table.index(value)

    def pair(method):
        one, two = answers(H, method)
        return index("answers", [index("answers_1d", [one[f] for f in FUNCTIONS]),
                                 index("answers_2d", [two[f] for f in FUNCTIONS[:3]])])
    planes = {p: [[pair(p + n + s) for s in SUFFIXES] for n in NAMES] for p in PREFIXES}
    grid = planes[""]
    changes = {p: {n: row for n, row, base in zip(NAMES, plane, grid) if row != base}
               for p, plane in planes.items() if p}
    pairs = [[pair(a + " " + b) for b in NAMES] for a in NAMES]
    others = {m: pair(m) for m in literal_strings()}
    return dict(prefixes=PREFIXES, names=NAMES, suffixes=SUFFIXES, functions=FUNCTIONS, **tables,
                grid=grid, grid_changes=changes, pairs=pairs, others=others)


def decode(fixture):
    """{method string: [1D answer, 2D answer]} of a recorded file, answers as ``answers`` gives them."""
    fn = fixture["functions"]
    full = [[dict(zip(fn, fixture["answers_1d"][i])), dict(zip(fn[:3], fixture["answers_2d"][j]))]
            for i, j in fixture["answers"]]
    out = {m: full[k] for m, k in fixture["others"].items()}
    for a, row in zip(fixture["names"], fixture["pairs"]):
        out.update((a + " " + b, full[k]) for b, k in zip(fixture["names"], row))
    for p in fixture["prefixes"]:
        changed = fixture["grid_changes"].get(p, {})
        for n, row in zip(fixture["names"], fixture["grid"]):
            out.update((p + n + s, full[k]) for s, k in zip(fixture["suffixes"], changed.get(n, row)))
    return out


def dump(fixture, f):
    """JSON with one line per key, and one per answer and per row of the grid and the pairs."""
    def lines(rows):
        return "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "]"
    parts = []
    for key, value in fixture.items():
        many = key in ("answers_1d", "answers_2d", "grid", "pairs")
        parts.append(json.dumps(key) + ":" + (lines(value) if many else json.dumps(value, separators=(",", ":"))))
    f.write("{" + ",\n".join(parts) + "}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "method_routes.json"))
    ap.add_argument("--hostprep", default=None, help="record another revision's hostprep.py")
    ap.add_argument("--commit", default=None, help="the revision the answers come from (default: HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                        capture_output=True, text=True, check=True).stdout.strip()
    fixture = dict(recorded_from_commit=commit, **record(load_hostprep(a.hostprep)))
    with open(a.out, "w") as f:
        dump(fixture, f)
    print(f"{len(decode(json.load(open(a.out))))} method strings, {len(fixture['answers'])} distinct answers, "
          f"{os.path.getsize(a.out)} bytes -> {a.out}")


if __name__ == "__main__":
    main()
