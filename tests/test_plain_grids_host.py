"""tests/plain_grids.py held to the source: one entry per launch with `dim3((unsigned)gx, (unsigned)gy)` of amcx.hip, every
test an entry names exists, and each kernel decodes its item from both grid dimensions.  No GPU.  Only those words, the line
that sets `gx` and the decode `blockIdx.y * gridDim.x + blockIdx.x` are read from the sources."""
import ast
from pathlib import Path

import pytest

from tests import plain_grids as pg

REPO = Path(__file__).resolve().parents[1]
LAUNCH = "dim3((unsigned)gx, (unsigned)gy)"
DECODE = "blockIdx.y * gridDim.x + blockIdx.x"


def _code(line):
    return line.split("//")[0]


def _code_py(line):
    """a line of a test without its trailing comment (no `#` stands inside a string on the lines read here)"""
    return line.split("#")[0]


def _call_sites(path):
    """(line of the launch, line that sets gx) of every folded launch: code, not comment"""
    lines = Path(path).read_text().splitlines()
    sites = []
    for number, line in enumerate(lines, start=1):
        if LAUNCH in _code(line):
            gx = next((n for n in range(number, 0, -1) if "gx =" in _code(lines[n - 1])), None)
            sites.append((number, gx))
    return sites


def _check_sites(path):
    """the table against the folded launches of `path` (amcx.hip, or a copy of it)"""
    lines = Path(path).read_text().splitlines()
    sites = _call_sites(path)
    assert len(sites) == len(pg.TABLE), (f"{path} launches with {LAUNCH} on lines {[s[0] for s in sites]}: {len(sites)} call sites, "
                                         f"tests/plain_grids.py has {len(pg.TABLE)} entries")
    for launch, gx in sites:
        assert gx is not None and launch - gx <= 3, f"{path}:{launch}: no line that sets gx in front of the launch"
        assert _code(lines[gx - 1]).count(str(pg.LINE)) == 2, f"{path}:{gx}: gx is not cut at {pg.LINE}: {lines[gx - 1].strip()}"
    assert len({gx for _, gx in sites}) == len(sites)                    # every launch has a gx line of its own


def test_every_folded_launch_has_an_entry():
    assert pg.LINE == 65536 == 1 << 16
    _check_sites(REPO / pg.SOURCE)
    assert len(pg.HEADERS) == len(pg.TABLE)


def test_a_fourth_folded_launch_without_an_entry_is_named_by_file_and_line(tmp_path):
    source = (REPO / pg.SOURCE).read_text()
    copy = tmp_path / "amcx_with_a_fourth.hip"
    copy.write_text(source + "  const int64_t gx = n < 65536 ? n : 65536, gy = (n + gx - 1) / gx;\n"
                             "  launch(new_kernel, dim3((unsigned)gx, (unsigned)gy), 256, 0, stream, a);\n")
    with pytest.raises(AssertionError) as caught:
        _check_sites(copy)
    last = len(source.splitlines()) + 2
    assert str(copy) in str(caught.value) and str(last) in str(caught.value) and "4 call sites" in str(caught.value)
    # a launch in a comment is none, and one whose line is cut elsewhere is refused by its gx line
    copy.write_text(source + "  // dim3((unsigned)gx, (unsigned)gy)\n")
    _check_sites(copy)
    copy.write_text(source.replace("n_groups < 65536 ? n_groups : 65536", "n_groups < 65535 ? n_groups : 65535"))
    with pytest.raises(AssertionError, match="gx is not cut at 65536"):
        _check_sites(copy)


def test_every_named_test_exists_and_needs_the_gpu():
    functions = {}
    for what, tests in pg.TABLE:
        assert what and tests, what
        for path, name in tests:
            if path not in functions:
                source = (REPO / path).read_text()
                functions[path] = ({node.name for node in ast.parse(source).body if isinstance(node, ast.FunctionDef)}, source)
            names, source = functions[path]
            assert name in names, f"{path} has no {name} ({what})"
            assert "pytestmark = pytest.mark.gpu" in source, path
            assert "lines_of_the_grid" in name                 # the tests that assert items >= 2 LINE + 1 are named for it


def test_the_named_tests_assert_their_items():
    """every named test asserts `>= 2 * LINE + 1` in its own body -- the carrier's `>= LINE + 1`: a line of it is 2.1 GB of input"""
    named = sorted({path for _, tests in pg.TABLE for path, _ in tests})
    assert sorted(pg.BOUND) == named
    for _, tests in pg.TABLE:
        for path, name in tests:
            source = (REPO / path).read_text()
            assert "from tests.plain_grids import LINE" in source, path
            node = next(n for n in ast.parse(source).body if isinstance(n, ast.FunctionDef) and n.name == name)
            body = [_code_py(line) for line in source.splitlines()[node.lineno - 1:node.end_lineno]]
            assert any(line.strip().startswith("assert ") and pg.BOUND[path] in line for line in body), \
                f"{path}::{name} has no line `assert ... {pg.BOUND[path]}`"
    assert [bound for bound in pg.BOUND.values() if bound != ">= 2 * LINE + 1"] == [">= LINE + 1"]
    assert pg.BOUND["tests/test_gpu_carrier.py"] == ">= LINE + 1"


def test_every_kernel_decodes_its_item_from_both_dimensions():
    for (what, _), header in zip(pg.TABLE, pg.HEADERS):
        code = [_code(line) for line in (REPO / header).read_text().splitlines()]
        assert sum(DECODE in line for line in code) == 1, f"{header}: the item is not {DECODE} ({what})"
        kernel = what.split(": ")[1].split(",")[0]
        assert any("__global__" in line and kernel + "(" in line for line in code), f"{header} does not hold {kernel}"
