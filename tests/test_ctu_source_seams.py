"""Two things the CTU search headers say in ONE place each (source text only; runs without a GPU):
  * the host emulation runs another wave's work in place by switching g_emul_wave -- only emul_on_wave (ctu_core.h) does that;
  * the reference's pruning test (search.c:1952-1956) and its factor 1.1 / 1.075 -- only split_pruned (ctu_core.h) spells it out."""
import os
import re

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uvg266_amd", "csrc")
HEADERS = ("ctu_core.h", "ctu_pb.h", "ctu_leaf4.h")


def body_of(text, name):
    """the braces' content of the first function definition called `name`"""
    at = text.index(name + "(")
    start = text.index("{", at)
    depth, i = 0, start
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return start, i + 1
        i += 1


def outside(name, pattern):
    core = open(os.path.join(SRC, "ctu_core.h")).read()
    a, b = body_of(core, name)
    assert re.search(pattern, core[a:b]), f"{name} does not hold what this test looks for"
    found = []
    for h in HEADERS:
        text = open(os.path.join(SRC, h)).read()
        if h == "ctu_core.h":
            text = text[:a] + "\n" * text[a:b].count("\n") + text[b:]
        found += [f"{h}:{i + 1}: {ln.strip()}" for i, ln in enumerate(text.splitlines()) if re.search(pattern, ln)]
    return found


def test_only_emul_on_wave_switches_the_emulations_wave():
    found = outside("emul_on_wave", r"\bg_emul_wave\s*(=(?!=)|[-+|&^]=|\+\+|--)|(\+\+|--)\s*g_emul_wave\b")
    assert [f for f in found if "static int g_emul_wave = 0;" not in f] == []          # (the declaration)


def test_only_split_pruned_spells_out_the_pruning_test():
    assert outside("split_pruned", r"1\.075") == []
