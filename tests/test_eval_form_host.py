"""The host half of the quotient's evaluation form (masp_amd/csrc/host/eval_form.h: the column-compressed copy of C, the layout and offset
arithmetic of the merged base set) on the CPU: a stand-alone program, tests/native/eval_form_host.cpp, built with the address and
undefined-behaviour sanitizers and started as a child process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc")


def test_csc_and_layout(tmp_path):
    exe = str(tmp_path / "eval_form_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                           "-I", CSRC, os.path.join(HERE, "native", "eval_form_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout.splitlines() == ["csc ok", "layout ok", "all ok"]
