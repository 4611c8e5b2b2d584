"""The lean kernel's in-kernel closed loop (csrc/admm_lean.hip.h, MPC = true) in the compiler's own output, one unit each as
csrc/jit.cpp writes them (TMPC_DEFINE_LEAN_JIT_ENTRY_MPC, the Makefile's flags for the lean instantiations): the loop kernel
of (4, 1, 20) on the cartpole pattern — what mpc_rollout launches with TINYMPC_HIP_LEAN_WS=1 and TINYMPC_HIP_LEAN_LOOP=1 —
and its dense sibling with shared references.  From the kernel metadata: no spilled register, no scratch, and the LDS (the
staging and every lane's parked v, z, which the loop keeps between the steps) within the 160 KiB a gfx950 workgroup may have."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CARTPOLE_PATTERN = "0x1000a0021cc63ull"      # lean_pattern_rm of problems.cartpole's (A, B): csrc/linst_4_1_20.hip
EX, EU = 4 * 20, 1 * 19


def _metadata(tmp_path, tag, refs, pattern):
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    src, out = tmp_path / f"{tag}.hip", tmp_path / f"{tag}.s"
    src.write_text('#include "lean_entry.hip.h"\nTMPC_DEFINE_LEAN_JIT_ENTRY_MPC("lean<4,1,20>", 4, 1, 20, true, true, true, false, '
                   f'tmpc::{refs}, {pattern})\n')
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "-DTMPC_JIT_UNIT",
                    f"-I{csrc}", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    assert len(re.findall(r"^\s+\.name:\s+_ZN4tmpc16admm_lean_kernel", text, flags=re.M)) == 1      # one kernel per unit
    return {key: [int(m) for m in re.findall(r"\.%s:\s+(\d+)" % key, text)]
            for key in ("vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("tag,refs,pattern", [("loop_sparse", "REF_ZERO", CARTPOLE_PATTERN), ("loop_shared", "REF_SHARED", "0")])
def test_loop_kernel_resources(tmp_path, tag, refs, pattern):
    md = _metadata(tmp_path, tag, refs, pattern)
    assert md["vgpr_spill_count"] == [0], md
    assert md["private_segment_fixed_size"] == [0], md
    lds = md["group_segment_fixed_size"]
    assert len(lds) == 1 and 256 * (EX + EU) * 4 <= lds[0] <= 163840, md      # (the parked rows are there)
