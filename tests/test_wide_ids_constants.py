"""CS_CFG_WIDE_IDS is one value in the C header, the Python ctypes layer and the Rust binding (no GPU needed)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_ids_flag_agrees_across_bindings():
    from rmf_crowdsim_amd import CS_CFG_WIDE_IDS, _abi
    header = open(os.path.join(ROOT, "include", "crowdstep.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "rmf_crowdsim_gpu", "src", "ffi.rs")).read()
    c = re.search(r"#define CS_CFG_WIDE_IDS (\d+)u", header)
    rs = re.search(r"pub const CS_CFG_WIDE_IDS: u32 = (\d+);", ffi)
    assert c and rs
    assert int(c.group(1)) == int(rs.group(1)) == _abi.CS_CFG_WIDE_IDS == CS_CFG_WIDE_IDS == 16
    others = [int(v) for v in re.findall(r"#define CS_CFG_\w+ (\d+)u", header)]
    assert others.count(16) == 1  # no other CS_CFG_ bit uses it


def test_ffi_layout_still_agrees():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_ffi_layout.py")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
