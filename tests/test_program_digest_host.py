"""The programs the engine builds, op for op, against tests/golden/program_digest.json (tests/program_digest.py; no GPU, the
built libraries for ``conv3x3_gn_slots``).  A change that moves a route regenerates the fixture
(``python -m tests.program_digest --write``) and its review sees which programs moved."""
import json
import subprocess
import sys

from tests import program_digest as PD


def test_routes_imports_without_torch():
    # (the file itself: the package's __init__ imports the pipeline, and with it torch)
    code = "import runpy, sys; runpy.run_path('marigold_amd/routes.py'); assert not {'torch', 'marigold_amd'} & set(sys.modules)"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=PD.ROOT)


def test_programs_match_the_digest(tmp_path):
    with open(PD.FIXTURE) as f:
        want = json.load(f)["programs"]
    assert sorted(want) == sorted(PD.CONFIGS), "the fixture and program_digest.CONFIGS name different configurations"
    moved = []
    for name, text, kinds in PD.texts():
        got = PD.entry(text, kinds)
        if got != want[name]:
            (tmp_path / (name.replace("/", "__") + ".txt")).write_text(text)
            k, lines = PD.first_difference(text, want[name])
            kinds_moved = {kd: (got["kinds"].get(kd, 0), want[name]["kinds"].get(kd, 0)) for kd in set(got["kinds"]) | set(want[name]["kinds"])
                           if got["kinds"].get(kd, 0) != want[name]["kinds"].get(kd, 0)}
            moved.append(f"{name}: {got['ops']} ops (fixture {want[name]['ops']}), kind counts (now, fixture) {kinds_moved}; the first op "
                         f"that differs is among ops {k} ... {k + PD.BLOCK - 1}:\n  " + "\n  ".join(lines))
    assert not moved, ("programs differ from the fixture (their text is under " + str(tmp_path) + "; `python -m tests.program_digest --dump DIR`"
                       " on the fixture's commit gives the text to diff against):\n" + "\n".join(moved))
