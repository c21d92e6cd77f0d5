"""The token step's short decimal fields (csrc/rec_digits.h) on the CPU: scratch/host_rec_digits_test.cpp built with the host compiler under the
address and undefined-behaviour sanitizers and run as a child process of its own -- every length 0 .. 10 at every byte offset against a
byte-wise statement of nw_tok's short path, in columns that end where the header says they may.  No GPU, nothing loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "scratch", "host_rec_digits_test.cpp")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_short_decimal_fields_convert_as_the_byte_loop_does(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "host_rec_digits_test")
    build = [cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             "-I" + os.path.join(ROOT, "scratch", "hoststub"), "-I" + os.path.join(ROOT, "slimfastq_amd", "csrc"), SRC, "-o", exe]
    with open(SRC) as f:                                    # the program's first line is its build command: the same flags
        first = f.readline()
    for flag in build[1:6]:
        assert flag in first, flag
    # the sanitizers' runtimes linked in where the compiler can (g++: its default is shared runtimes, which want to be the first library loaded)
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run(build + static, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(build, check=True, cwd=ROOT)
    out = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.rstrip().endswith("ok"), out.stdout[-2000:]
