"""The scaled sparse sweeps of the headline kernel in the compiler's own assembly (csrc/admm_lean.hip.h: SCL).

The unit is built as tests/test_lean_pk_asm.py builds its own, with cartpole's SCALED pattern (admm_params.h:
lean_pattern_scaled — A01, A12, A23 and B3 units beside A00 and A11): admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true,
XB=false, zero references, fp32 state, that pattern> — what bench.py's default launches.  Forward rows 2 and 3 start from a
free operand, 25 fp64 per knot for 27: the hot loop (99 of 100 iterations) has at most 582 - 2 x 19 = 544 vector
instructions, still packs the slack / dual update (27 v_pk_add_f32), spills nothing, and the status fold behind it keeps its
7 swaps.  The tolerance-terminated unit of the same pattern, which must agree with it bit for bit, compiles without a spill."""
import os
import re
import subprocess

import pytest

from tests.test_lean_pk_asm import _hot_loop, _ops, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CARTPOLE_SCALED_PATTERN = "0x4f000a0863cc63ull"   # lean_pattern_scaled of cartpole's pattern: csrc/linst_4_1_20_scaled.hip
N = 20

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _unit(tmp_path, tag, live):
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    src, out = tmp_path / f"{tag}.hip", tmp_path / f"{tag}.s"
    src.write_text(f'#include "lean_entry.hip.h"\nTMPC_DEFINE_LEAN_JIT_ENTRY_SP("lean<4,1,20>", 4, 1, 20, {live}, true, true, false, '
                   f"tmpc::REF_ZERO, float, {CARTPOLE_SCALED_PATTERN})\n"
                   f"static_assert(tmpc::kCartpolePatternScaled == {CARTPOLE_SCALED_PATTERN}, \"the built-in kernels' pattern\");\n")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "-DTMPC_JIT_UNIT",
                    f"-I{csrc}", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True, timeout=600)
    lines = out.read_text().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN4tmpc16admm_lean_kernel\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", "\n".join(lines))]
    return lines[start + 1:end], spills


def test_scaled_headline_loop(tmp_path):
    body, spills = _unit(tmp_path, "scaled", "false")
    loop, ops = _hot_loop(body), _ops(body)
    pk, valu = sum(o == "v_pk_add_f32" for o in loop), _valu(loop)
    f64 = sum(o.startswith(("v_fma_f64", "v_fmac_f64", "v_add_f64", "v_mul_f64")) for o in loop)
    swaps = sum(o.startswith("global_atomic_swap") for o in ops)
    print(f"scaled: {valu} VALU in the loop ({f64} fp64, {pk} v_pk_add_f32), spills {spills}, {swaps} global_atomic_swap")
    assert valu <= 582 - 2 * (N - 1)
    assert pk >= 27
    assert spills == [0] and not any(o.startswith("scratch_") for o in ops)
    assert swaps == 7


def test_scaled_live_unit_does_not_spill(tmp_path):
    body, spills = _unit(tmp_path, "scaled_live", "true")
    assert spills == [0] and not any(o.startswith("scratch_") for o in _ops(body))
