"""The door table of tests/doors.py, checked without a GPU: importing it builds the table and touches no device.  The committed
list of identifiers (tests/golden/doors_idents.txt, one per line) makes a door that was renamed or lost show up in a diff."""
import ast
from pathlib import Path

import doors

TESTS = Path(__file__).resolve().parent


def test_every_door_runs_on_a_known_config():
    for ident, (config, fn) in doors.DOORS.items():
        assert config in doors.CONFIGS and callable(fn), ident


def test_the_table_is_the_committed_list_of_identifiers(golden_dir):
    listed = (golden_dir / "doors_idents.txt").read_text().split("\n")
    assert listed.pop() == "" and len(set(listed)) == len(listed)
    table = set(doors.DOORS)
    assert table == set(listed), f"not listed: {sorted(table - set(listed))}; listed and gone: {sorted(set(listed) - table)}"


def test_no_file_here_imports_a_test_module():
    """helpers live in helper modules (doors.py, diag.py, gpu_engines.py, the models); a test module is nobody's library"""
    found = []
    for path in sorted(TESTS.glob("*.py")):
        for node in ast.walk(ast.parse(path.read_text(), str(path))):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + ([a.name for a in node.names] if not node.module or node.module == "tests" else [])
            found += [f"{path.name}:{node.lineno} imports {n}" for n in names if n.split(".")[-1].startswith("test_")]
    assert not found, found
