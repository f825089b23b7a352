"""The decision of the one-launch evaluation's adjoint switch (fast-racing_amd/csrc/frx_launch_forms.hpp: EvalSwitches::old_adjoint, EvalClusterForm::old_adjoint,
eval_form_has_adjoint) on the host: tests/hostcheck/eval_adjoint_main.cpp is compiled with the address and undefined-behaviour sanitizers as a program of its own and run.
It enumerates all nine switches with both inputs of eval_cluster_form: the adjoint with its operands in front of the poll exists where the two-trip front, the value-major
hand-off and the shortened prelude are all on and nowhere else, FRX_EVAL_ADJOINT=0 shows there and moves no other member of the form, every form a launch can take is
among those whose LDS limit is raised, and initialisers written before the member existed mean the default."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adjoint_switch_over_every_form(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++: the host check cannot be built")
    exe = str(tmp_path / "eval_adjoint_san")
    src = os.path.join(ROOT, "tests", "hostcheck", "eval_adjoint_main.cpp")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-1000:], r.stderr[-3000:])
    m = re.search(r"(\d+) decisions enumerated, (\d+) with an adjoint to choose, (\d+) of them take the operands in front of the poll, (\d+) disagreements", r.stdout)
    assert m, r.stdout
    # 512 settings of the nine switches x (geometry class, stamped) and the forms written with fewer members; an adjoint to choose: the four switches it needs set,
    # FRX_EVAL_FRONT and FRX_EVAL_PRELUDE not 0, FRX_EVAL_CHAIN, FRX_EVAL_GEOM and FRX_EVAL_ADJOINT free - 8 settings x 4; half of them with FRX_EVAL_ADJOINT=0
    assert [int(m.group(i)) for i in range(1, 5)] == [512 * 4 + 1, 32, 16, 0]
