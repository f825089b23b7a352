"""The decision of the one-launch evaluation's prelude switch (fast-racing_amd/csrc/frx_launch_forms.hpp: EvalSwitches::old_prelude, EvalClusterForm::old_prelude,
eval_form_has_prelude) on the host: tests/hostcheck/eval_prelude_main.cpp is compiled with the address and undefined-behaviour sanitizers as a program of its own and run.
It enumerates all eight switches with both inputs of eval_cluster_form: the shortened prelude exists behind the two-trip front with the value-major hand-off and nowhere
else, FRX_EVAL_PRELUDE=0 shows there and moves no other member of the form, and every form a launch can take is among those whose LDS limit is raised."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prelude_switch_over_every_form(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++: the host check cannot be built")
    exe = str(tmp_path / "eval_prelude_san")
    src = os.path.join(ROOT, "tests", "hostcheck", "eval_prelude_main.cpp")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-1000:], r.stderr[-3000:])
    m = re.search(r"(\d+) decisions enumerated, (\d+) with a prelude to choose, (\d+) of them take the shortened one, (\d+) disagreements", r.stdout)
    assert m, r.stdout
    # 256 settings of the eight switches x (geometry class, stamped) and the six-member form; a prelude to choose: the four switches it needs set, FRX_EVAL_FRONT not 0,
    # the other three free - 8 settings x 4; half of them with FRX_EVAL_PRELUDE=0
    assert [int(m.group(i)) for i in range(1, 5)] == [256 * 4 + 1, 32, 16, 0]
