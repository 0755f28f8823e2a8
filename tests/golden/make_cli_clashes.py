"""Writes cli_clashes.json: what moni-hip-align answers to every cell of tests/test_cli_clashes.py (exit code, stderr, the stdout of a passing --dry-run).
Run it with the binary whose behaviour is to be kept:  python tests/golden/make_cli_clashes.py [path/to/moni-hip-align]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_cli_clashes as t  # noqa: E402

exe = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else t.EXE
with tempfile.TemporaryDirectory() as d:
    t.write_inputs(d)
    doc = {t.key(c): t.answer(exe, d, c) for c in t.cells()}
with open(os.path.join(HERE, "cli_clashes.json"), "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
