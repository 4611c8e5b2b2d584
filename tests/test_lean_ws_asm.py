"""The workspace-keeping lean kernels (csrc/admm_lean.hip.h, WS = true) in the compiler's own assembly, one unit each as
csrc/jit.cpp writes them (TMPC_DEFINE_LEAN_JIT_ENTRY_WS, the Makefile's flags for the lean instantiations): the
tolerance-terminated and the fixed-iteration kernel of (4, 1, 20) on the cartpole pattern — what bench.py's two
kept-workspace configs launch with TINYMPC_HIP_LEAN_WS=1.
 * no scratch: vgpr_spill_count 0, no scratch_ instruction;
 * LDS within the 160 KiB a gfx950 workgroup may have (the tolerance-terminated kernel parks every lane's previous v, z
   there: nx N + nu (N-1) floats per lane beside the staging);
 * the kept workspace comes in through the wavefront's LDS staging ahead of the iteration loop (load_wave_x / load_wave_u:
   every loaded float crosses LDS) and leaves through the staged stores: 16-byte stores for every array, 4-byte stores only
   where the shape needs them — the predicated controls-shaped arrays of a ragged wavefront (u, z, y, d: nu (N-1) each;
   a float4 of their flat image may span two instances), iteration count, solved flag, the fifth status word."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CARTPOLE_PATTERN = "0x1000a0021cc63ull"      # lean_pattern_rm of problems.cartpole's (A, B): csrc/linst_4_1_20.hip
NX, NU, N = 4, 1, 20
EX, EU = NX * N, NU * (N - 1)


def _unit(tmp_path, tag, live, xb=False):
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    src, out = tmp_path / f"{tag}.hip", tmp_path / f"{tag}.s"
    src.write_text('#include "lean_entry.hip.h"\nTMPC_DEFINE_LEAN_JIT_ENTRY_WS("lean<4,1,20>", 4, 1, 20, '
                   f'{"true" if live else "false"}, true, true, {"true" if xb else "false"}, tmpc::REF_ZERO, {CARTPOLE_PATTERN})\n')
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "-DTMPC_JIT_UNIT",
                    f"-I{csrc}", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN4tmpc16admm_lean_kernel\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ops = [l.split()[0] for l in lines[start + 1:end] if l.startswith("\t") and not l.strip().startswith((";", "."))]
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    lds = [int(m) for m in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    return ops, spills, lds


def _regions(ops):
    """(ops ahead of the iteration loop, ops of the loop, ops behind it): the loop is where the fp64 arithmetic is"""
    f64 = [i for i, o in enumerate(ops) if re.match(r"v_(fma|fmac|mul|add)_f64", o)]
    return ops[:f64[0]], ops[f64[0]:f64[-1] + 1], ops[f64[-1] + 1:]


def _lds_floats_written(ops):
    return (sum(o == "ds_write_b32" for o in ops) + 2 * sum(o in ("ds_write2_b32", "ds_write2st64_b32") for o in ops)
            + 2 * sum(o == "ds_write_b64" for o in ops) + 4 * sum(o == "ds_write_b128" for o in ops))


def _stores(ops):
    wide = sum(o == "global_store_dwordx4" for o in ops)
    narrow = sum(o in ("global_store_dword", "global_store_short", "global_store_byte") for o in ops)
    return wide, narrow


# one store site (all-lanes copy + predicated copy) without a state bound: 16-byte stores of the two states-shaped arrays
# (xout, v: nx N / 4 each, twice) and of the four controls-shaped arrays' flat images (all-lanes copy only), the residuals
N_WIDE_SITE = 2 * 2 * (EX // 4) + 4 * ((16 * EU + 63) // 64) + 1
# ... its 4-byte stores: the predicated controls-shaped arrays, iteration count, solved flag
N_NARROW_SITE = 4 * EU + 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_fixed_iteration_ws_kernel(tmp_path):
    ops, spills, lds = _unit(tmp_path, "ws_fixed", live=False)
    assert spills == [0] and not any(o.startswith("scratch_") for o in ops)
    assert lds and max(lds) <= 160 * 1024, lds
    pro, loop, epi = _regions(ops)
    # every float of v (knots 1.., fetched as whole 16-float pieces: ceil(nx N / 16) x 16), y, z, d crosses LDS on its way in
    assert _lds_floats_written(pro) >= EX + 3 * EU, _lds_floats_written(pro)
    assert sum(o.startswith("global_load_dword") for o in pro) >= EX + 3 * EU
    assert not any(o.startswith("global_store") for o in pro + loop)      # nothing is stored before the loop has run
    wide, narrow = _stores(epi)
    assert wide >= N_WIDE_SITE + 1 and narrow <= N_NARROW_SITE + 1, (wide, narrow)   # (+ the status block, + its fifth word)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("xb", [False, True], ids=["plain", "state_bound"])
def test_tolerance_terminated_ws_kernel(tmp_path, xb):
    ops, spills, lds = _unit(tmp_path, "ws_live", live=True, xb=xb)
    assert spills == [0] and not any(o.startswith("scratch_") for o in ops)
    # the parked previous slack: 256 lanes x (nx N (+ pad) + nu (N-1)) floats beside the staging
    assert lds and 256 * (EX + EU) * 4 <= max(lds) <= 160 * 1024, lds
    pro, loop, epi = _regions(ops)
    n_x = 2 if xb else 1                                                  # states-shaped arrays loaded: v (and g)
    assert _lds_floats_written(pro) >= n_x * EX + 3 * EU
    assert not any(o.startswith("global_store") for o in pro)
    # two store sites: the converged exit inside the loop and the exit at max_iter behind it; with a state bound each also
    # stores g (nx N / 4 more 16-byte stores, twice)
    site_wide = N_WIDE_SITE + (2 * (EX // 4) if xb else 0)
    wide, narrow = _stores(loop + epi)
    assert wide >= 2 * site_wide + 1 and narrow <= 2 * N_NARROW_SITE + 1, (wide, narrow)
    # (which instructions the compiler lays out between the first and the last fp64 instruction is its own business: the
    # converged exit's store is counted with the other one, above; the parked slack shows in the LDS size)
    # the parked v goes to LDS 16 bytes at a time (rows of an odd number of float4 are conflict-free for such writes only).
    # Behind the prologue the 4-byte LDS writes are the controls-shaped arrays' staging (u, z, y, d: two copies at each of the
    # two store sites) and the parked z; v parked element by element would add nx N of them — half of that is allowed
    n4 = sum(o == "ds_write_b32" for o in loop + epi) + 2 * sum(o in ("ds_write2_b32", "ds_write2st64_b32") for o in loop + epi)
    assert n4 <= 2 * 2 * 4 * EU + EU + EX // 2, n4
