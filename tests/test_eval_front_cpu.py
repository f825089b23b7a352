"""The front records of the one-launch evaluation (fast-racing_amd/csrc/frx_eval_front.hpp: EvalFront, eval_front_fill) on the host: tests/hostcheck/eval_front_main.cpp
is compiled with the address and undefined-behaviour sanitizers as a program of its own and run.  It builds offset tables for the piece counts (64,), (64, 7, 9, 3, 2),
(2,), (3,) and nine candidates, with the soft and with the fixed total time, and compares every field of every record with the table expression the kernel uses
without the record; it checks the record's size and alignment (at compile time, and the address of every record of an array) and nT in both layers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_front_records_against_the_table_expressions(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++: the host check cannot be built")
    exe = str(tmp_path / "eval_front_san")
    src = os.path.join(ROOT, "tests", "hostcheck", "eval_front_main.cpp")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-1000:], r.stderr[-3000:])
    m = re.search(r"(\d+) records, (\d+) fields compared, (\d+) disagreements", r.stdout)
    assert m, r.stdout
    # five batches of 1 + 5 + 1 + 1 + 9 = 17 candidates, two layers, three task sizes
    assert int(m.group(1)) == 17 * 2 * 3 and int(m.group(2)) == 17 * 2 * 3 * 16 + 6 and int(m.group(3)) == 0
