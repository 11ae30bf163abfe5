"""The engine-file parser (csrc/engine_file.h) as a stand-alone program under the address and undefined-behaviour sanitizers
(tools/engine_file_check.cpp): the file-level rows of tests/engine_file_cases.py get the status and text the library gives them, a
good file is accepted, every prefix of a good file is refused -- and no run leaves a sanitizer report."""
import os
import shutil
import subprocess

import pytest

from tests import engine_file_cases as cases
from tests.conftest import ROOT

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("engine_file_check") / "engine_file_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "engine_file_check.cpp"), "-o", exe], check=True)

    def run(path, H=cases.NET_H):
        r = subprocess.run([exe, path, str(H)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)      # a sanitizer report ends the program with a status and a text
        status, _, text = r.stdout.rstrip("\n").partition(" ")
        return int(status), text
    return run


@pytest.mark.parametrize("case", cases.FILE_CASES, ids=[c.name for c in cases.FILE_CASES])
def test_file_level_refusals(check, case, tmp_path):
    path = str(tmp_path / "case.spvw")
    cases.write(case, path)
    status, text = check(path)
    assert status == case.code and text.endswith(case.text) and path in text, text


def test_level_must_divide_the_height(check, tmp_path):
    from spvo import weights
    path = str(tmp_path / "good.spvw")
    weights.save(cases.good(), path)
    with open(path, "rb") as fh:
        data = fh.read()
    accepted = f"8 7 {(len(data) - cases.records_end(data) - 8) // 4} 0"          # tensors, ops, payload floats, precision
    assert check(path, 64) == (0, accepted) and check(path, 360) == (0, accepted)
    assert check(path, 60) == (cases.IO, path + ": bad tensor level")          # 60 rows halve twice, not three times


def test_late_rows_pass_the_parser(check, tmp_path):
    """what the plan loader refuses is none of the parser's business: those files parse"""
    for case in cases.LATE_CASES:
        path = str(tmp_path / "case.spvw")
        cases.write(case, path)
        status, text = check(path)
        assert status == 0, (case.name, text)


def test_every_prefix_is_refused(check, tmp_path):
    from spvo import weights
    good = tmp_path / "good.spvw"
    weights.save(cases.good(), str(good))
    data = good.read_bytes()
    path = str(tmp_path / "prefix.spvw")
    header_end = cases.records_end(data) + 8
    for n in list(range(0, 201)) + [header_end - 1, header_end, header_end + 3, len(data) - 1]:
        with open(path, "wb") as fh:
            fh.write(data[:n])
        want = " is not a SPVW0003 weight file" if n < 48 else ": truncated" if n < header_end else ": truncated payload"
        assert check(path) == (cases.IO, path + want), n
