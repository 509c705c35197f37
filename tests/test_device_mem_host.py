"""The owners of device and pinned memory (rmf_crowdsim_amd/csrc/cs_device_mem.hip.inc) without a GPU: the generic part of
that file compiles with plain g++ and no HIP header, and tests/cpp/test_device_mem.cpp, which drives it with a counting
malloc-backed policy that can fail the k-th allocation, passes under the address and undefined-behaviour sanitizers; and
the four allocation calls of the HIP runtime appear in no other part of the engine."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rmf_crowdsim_amd", "csrc")


def test_the_owners_hold_free_and_move_under_the_sanitizers(tmp_path):
    exe = tmp_path / "test_device_mem"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_device_mem.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    assert re.search(r"^\d+ allocations, \d+ frees, \d+ waits, 0 checks failed$", run.stdout, flags=re.M)


def test_only_the_owners_allocate_and_free():
    calls = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name == "cs_device_mem.hip.inc":
            continue
        for n, line in enumerate(open(os.path.join(CSRC, name)), 1):
            if calls.search(line.split("//")[0]):
                found.append(f"{name}:{n}: {line.strip()}")
    assert not found, "\n".join(found)
    own = open(os.path.join(CSRC, "cs_device_mem.hip.inc")).read()
    assert sorted(set(m.group(1) for m in calls.finditer(own))) == ["hipFree", "hipHostFree", "hipHostMalloc", "hipMalloc"]
