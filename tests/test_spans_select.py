"""The selection step of ak_ids_spans (akshar_amd/csrc/ak_spans.h spans_select) with equal keys: a
stand-alone host program (tests/emu/spans_select.cpp, its own main, one emulated wave of 64 threads)
draws the keys from a handful of values and holds the cuts to a stable sort by (key, index). Real
draws tie once in 2^32, so this is where the rule "equal keys go to the smaller j" is exercised."""
import os
import subprocess

from tests.conftest import ROOT


def test_select_breaks_ties_by_index(tmp_path):
    exe = str(tmp_path / "spans_select")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-pthread", "-DAK_HOST_EMU", "-I", os.path.join(ROOT, "akshar_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "spans_select.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
