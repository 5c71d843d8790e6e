"""The launch ledger (gesture2vec_amd/csrc/launch_ledger.hpp: LDS high-water mark per kernel, residency per (kernel, block, bytes),
CU count, each per device) driven on the CPU by tests/launch_ledger_host.cpp with counting stubs for the runtime calls: built and
run plain, and again under ThreadSanitizer.  And the source rule that goes with it: the runtime calls the ledger guards occur in
misc.hip only.  Host code only, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gesture2vec_amd", "csrc")


def _host_cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in ("c++", os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        path = shutil.which(cand)
        if path:
            return path
    pytest.fail("no host C++ compiler (c++, or the clang++ that ships with ROCm): the launch ledger cannot be checked")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread", "-g"]], ids=["plain", "tsan"])
def test_ledger_contract(tmp_path, flags):
    exe = tmp_path / "launch_ledger_host"
    subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", *flags, "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "launch_ledger_host.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout == "launch ledger ok\n", run.stdout + run.stderr


def _csrc_lines():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(CSRC, name), errors="replace") as fh:
                for n, line in enumerate(fh, 1):
                    yield name, n, line


def test_reservation_and_occupancy_calls_live_in_misc_hip_only():
    pat = re.compile(r"hipFuncSetAttribute|hipOccupancyMaxActiveBlocksPerMultiprocessor")
    hits = [(name, n, m[0]) for name, n, line in _csrc_lines() for m in pat.finditer(line)]
    assert {m for _, _, m in hits} == {"hipFuncSetAttribute", "hipOccupancyMaxActiveBlocksPerMultiprocessor"}, hits
    assert not [h for h in hits if h[0] != "misc.hip"], hits


def test_the_no_reservation_limit_is_written_once():
    hits = [(name, line.strip()) for name, _, line in _csrc_lines() if re.search(r"48\s*\*\s*1024", line)]
    assert hits == [("launch_ledger.hpp", "constexpr size_t LDS_NO_RESERVE_LIMIT = 48 * 1024;")], hits
