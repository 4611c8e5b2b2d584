"""The headline kernel's epilogue in the compiler's own assembly (csrc/admm_lean.hip.h): no scratch, the solution stores
are 16-byte stores (store_wave_wide, csrc/admm_quad.hip.h), the last workgroup's swaps of the status fold are issued
together.  One variant, as csrc/jit.cpp writes a unit (seconds; the whole linst_4_1_20.hip entry takes minutes):
admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true, XB=false, zero references, fp32 state, the cartpole pattern> — what
bench.py's default launches.

The status fold ahead of the store (-DTMPC_LEAN_FOLD_FIRST=1) measured slower than the fold behind it and is not the default
(profiles/r07_lean_ab.txt); what that order promises — no buffer_wbl2, no s_waitcnt vmcnt(0) and no atomic behind the first
solution store — is checked on a build with the macro on.  The unit with the wide store off shows what the store-width check
sees in the form it guards against."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CARTPOLE_PATTERN = "0x1000a0021cc63ull"      # lean_pattern_rm of problems.cartpole's (A, B): csrc/linst_4_1_20.hip
NX, NU, N = 4, 1, 20


def _kernel_body(tmp_path, tag, flags):
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    src, out = tmp_path / f"{tag}.hip", tmp_path / f"{tag}.s"
    src.write_text('#include "lean_entry.hip.h"\nTMPC_DEFINE_LEAN_JIT_ENTRY_SP("lean<4,1,20>", 4, 1, 20, false, true, true, false, '
                   f"tmpc::REF_ZERO, float, {CARTPOLE_PATTERN})\n")
    # the Makefile's flags for the lean instantiations
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "-DTMPC_JIT_UNIT",
                    *flags, f"-I{csrc}", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True, timeout=600)
    lines = out.read_text().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN4tmpc16admm_lean_kernel\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ops = [l.split()[0] + " " + " ".join(l.split()[1:]) for l in lines[start + 1:end] if l.startswith("\t") and not l.strip().startswith((";", "."))]
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", "\n".join(lines))]
    return ops, spills


def _epilogue(ops):
    """(index of the last status atomic, indices of the 16-byte stores behind the iteration loop, ... of the 4-byte ones)"""
    atomics = [i for i, o in enumerate(ops) if o.startswith("global_atomic_")]
    loop_end = max(i for i, o in enumerate(ops) if re.match(r"v_(fma|fmac|mul|add)_f64", o))
    wide = [i for i, o in enumerate(ops) if o.startswith("global_store_dwordx4") and i > loop_end]
    narrow = [i for i, o in enumerate(ops) if re.match(r"global_store_(dword|short|byte) ", o) and i > loop_end]
    return atomics, wide, narrow


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_headline_epilogue_in_the_compiled_kernel(tmp_path):
    ex, eu = NX * N, NU * (N - 1)
    # all-lanes and predicated copy of the states (nx N / 4 each), the controls' flat image (ceil(16 eu / 64)), the residuals,
    # the status block
    n_wide = 2 * (ex // 4) + (16 * eu + 63) // 64 + 2
    # 4-byte stores: the predicated controls (a float4 of their image may span two instances), iteration count, solved flag,
    # the fifth status word
    n_narrow = eu + 3

    ops, spills = _kernel_body(tmp_path, "default", [])
    assert spills == [0] and not any(o.startswith("scratch_") for o in ops)
    atomics, wide, narrow = _epilogue(ops)
    assert atomics, "status fold not found"
    assert len(wide) >= n_wide and len(narrow) <= n_narrow, (len(wide), len(narrow))
    # the last workgroup's five swaps are issued together: no wait between the first and the last of them
    swaps = [i for i, o in enumerate(ops) if o.startswith("global_atomic_swap")]
    assert len(swaps) == 7 and not any(o.startswith("s_waitcnt") and "vmcnt" in o for o in ops[swaps[0]:swaps[-1]])

    # fold first: behind the fold's last atomic come the two stores that publish the status block, then the solution's
    ops, spills = _kernel_body(tmp_path, "fold_first", ["-DTMPC_LEAN_FOLD_FIRST=1"])
    assert spills == [0] and not any(o.startswith("scratch_") for o in ops)
    atomics, wide, narrow = _epilogue(ops)
    sol_wide = [i for i in wide if i > atomics[-1]]
    sol_narrow = [i for i in narrow if i > atomics[-1]]
    assert len(sol_wide) >= n_wide and len(sol_narrow) <= n_narrow, (len(sol_wide), len(sol_narrow))
    assert min(wide + narrow) > atomics[-1]
    behind = ops[min(sol_wide + sol_narrow):]
    assert not any(o.startswith(("buffer_wbl2", "buffer_inv", "global_atomic_")) for o in behind)
    assert not any(o.startswith("s_waitcnt") and "vmcnt(0)" in o for o in behind)

    # the 4-byte form the store-width check guards against
    ops, spills = _kernel_body(tmp_path, "narrow", ["-DTMPC_LEAN_WIDE_STORE=0"])
    assert spills == [0]
    atomics, wide, narrow = _epilogue(ops)
    assert len(narrow) >= 2 * (ex + eu) and min(narrow) < atomics[0]
    assert any(o.startswith("buffer_wbl2") for o in ops[min(narrow):])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_long_horizon_unit_keeps_compiling(tmp_path):
    """(3, 2, 28): 54 controls per instance.  The predicated control store stages [64][nu (N-1) | 1] floats per wavefront —
    56 KB for the workgroup, more than the wide image's 48 KiB — and the unit must go on compiling within the 64 KiB of static
    LDS (a unit that fails to compile sends its solver to the run-time-shape kernels without an error)"""
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    src, out = tmp_path / "unit.hip", tmp_path / "unit.s"
    src.write_text('#include "lean_entry.hip.h"\nTMPC_DEFINE_LEAN_JIT_ENTRY("lean<3,2,28>", 3, 2, 28, false, true, true, false, '
                   "tmpc::REF_ZERO, float)\n")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "-DTMPC_JIT_UNIT",
                    f"-I{csrc}", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    lds = [int(m) for m in re.findall(r"LDSByteSize:\s+(\d+)", asm)]
    assert lds and 4 * 64 * 55 * 4 <= max(lds) <= 64 * 1024, lds
    # nx N = 84 takes the wide store at 28 floats a pass: 2 x 21 state stores and 14 of the controls' image at least
    assert asm.count("global_store_dwordx4") >= 2 * 21 + 14
