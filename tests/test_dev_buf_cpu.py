"""The owning buffer type and the grow protocol (csrc/dev_buf.h) as a stand-alone program under the address and undefined-behaviour
sanitizers (tools/dev_buf_check.cpp), with a counting fake policy in the place of the device's and the pinned allocator: a failed
allocation at every position of a list leaves every buffer of the list empty, no block live and an error answered -- a context that
its destruction and a later call can still handle; a second growth frees each old block exactly once; moves empty their source,
destruction frees each block once, reset() twice is harmless; the entries asked to be cleared, and only those, are cleared -- and no
run leaves a sanitizer report."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dev_buf_check") / "dev_buf_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "dev_buf_check.cpp"), "-o", exe], check=True)

    def run(what):
        r = subprocess.run([exe, what], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)   # a sanitizer report ends the program with a status and a text
        return r.stdout.strip()
    return run


@pytest.mark.parametrize("what", ["grow", "ownership", "clearing"])
def test_dev_buf(check, what):
    assert check(what) == "ok"
