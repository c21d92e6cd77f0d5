"""The -R option's argument errors (cli.cpp): no GPU is touched before they are found."""
import subprocess

import pytest

from test_gpu_parity import _cli


@pytest.mark.parametrize("arg", ("", "5", "5:", ":5", "5:0", "a:b", "5:3x", "-1:4", "3:4:5", "1 :2"))
def test_a_malformed_range_prints_the_usage(arg):
    p = subprocess.run([_cli(), "-d", "-R", arg, "-f", "nowhere.sfq"], capture_output=True)
    assert p.returncode == 0 and b"Usage" in p.stdout and b"-R first:count" in p.stdout


def test_a_range_with_a_compress_run_is_an_error(tmp_path):
    out = tmp_path / "x.sfq"
    p = subprocess.run([_cli(), "-R", "0:10", "-f", str(out)], input=b"@r\nACGT\n+\nIIII\n", capture_output=True)
    assert p.returncode == 1 and b"-R" in p.stderr and not out.exists()
