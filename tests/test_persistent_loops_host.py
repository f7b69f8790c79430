"""tests/persistent_loops.py held to the source: one entry per `persistent_grid(` call site of amcx.hip and amcx_launch.h, and
every test an entry names exists.  No GPU.  Only the word `persistent_grid` is read from the sources."""
import ast
import re
from pathlib import Path

from tests import persistent_loops as pl

REPO = Path(__file__).resolve().parents[1]


def _call_sites(path):
    """lines that call persistent_grid( -- not the line that defines it, and not a comment"""
    sites = []
    for number, line in enumerate((REPO / path).read_text().splitlines(), start=1):
        code = line.split("//")[0]
        if "persistent_grid(" in code and not re.match(r"\s*inline\b.*\bpersistent_grid\(", code):
            sites.append(number)
    return sites


def test_every_persistent_launch_has_an_entry():
    assert {entry[0] for entry in pl.TABLE} == set(pl.SOURCES)
    for path in pl.SOURCES:
        sites = _call_sites(path)
        entries = [entry for entry in pl.TABLE if entry[0] == path]
        assert len(sites) == len(entries), (f"{path} calls persistent_grid( on lines {sites}: {len(sites)} call sites, "
                                            f"tests/persistent_loops.py has {len(entries)} entries for it")
    assert sum(len(_call_sites(path)) for path in pl.SOURCES) == len(pl.TABLE)
    # the definition is the one line left out
    assert sum((REPO / path).read_text().count("persistent_grid(") for path in pl.SOURCES) >= len(pl.TABLE) + 1


def test_every_named_test_exists_and_needs_the_gpu():
    functions = {}
    for _, what, tests in pl.TABLE:
        assert what and tests, what
        for path, name in tests:
            if path not in functions:
                source = (REPO / path).read_text()
                functions[path] = ({node.name for node in ast.parse(source).body if isinstance(node, ast.FunctionDef)}, source)
            names, source = functions[path]
            assert name in names, f"{path} has no {name} ({what})"
            assert "pytestmark = pytest.mark.gpu" in source, path
            assert "three_trips" in name                       # the tests that assert units >= 2 grid + 1 are named for it


def test_the_named_tests_assert_their_units():
    """every named test, or a helper it calls, asserts `>= 2 * grid + 1`"""
    for path in sorted({path for _, _, tests in pl.TABLE for path, _ in tests}):
        assert "2 * grid + 1" in (REPO / path).read_text(), path
