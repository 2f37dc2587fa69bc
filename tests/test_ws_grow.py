"""The workspace's grow-only reserve (akshar_amd/csrc/ak_ws_grow.h) on the host: ws_grow_host.cpp
compiles the header with recording stubs in place of the three runtime calls and checks its
contract; one program, one run per property."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "akshar_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ws_grow") / "ws_grow_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "ws_grow_host.cpp")])
    return exe


# noop: no runtime call when need <= cap; order: synchronize, free, allocate; fail: {null, 0} and the
# error code after a failed allocation, and a smaller need allocates again; rows: ws_reserve's three
# lists with the 1st / 2nd / 3rd allocation failing; policy: exact / x1.5 / x2 capacities. Every case
# ends with every allocation freed exactly once.
@pytest.mark.parametrize("case", ["noop", "order", "fail", "rows", "policy"])
def test_ws_grow(prog, case):
    r = subprocess.run([prog, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("%s: ok" % case)
