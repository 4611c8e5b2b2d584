"""The stream kernel's closed loop (TINYMPC_HIP_STREAM_MPC / TINYMPC_HIP_STREAM_LOOP) without a GPU: the two switches, the
three units of the in-kernel loop, and the kernels of the tightest shape — (12, 4): three state rows per lane — in the
compiler's own assembly, compiled as the Makefile compiles csrc/sinst_mpc_12_4.hip.
 * both switches are members of Switches, read in read_switches (so reload_switches picks them up), off by default;
 * csrc/sinst_mpc_4_1.hip, sinst_mpc_6_3.hip, sinst_mpc_12_4.hip exist;
 * (12, 4) carries the fp64-state loop kernels, EXT in {0, 1, 2}, one family: vgpr_spill_count 0 and no scratch_ instruction
   in any of them, fp64 arithmetic, and the log's stores.
Forms left to the chain of launches (csrc/streamg_entry.hip.h, streamg_mpc_built), each because the compiler cannot hold it in
registers at the wavefronts per SIMD its plain twin is held to:
 * (12, 4), fp32 state, EXT 0 / 1 / 2, one family or one per instance: three wavefronts per SIMD leave 168 registers; the loop
   forms spill 28 / 116 / 161 (one family) and 48 / 109 / 157 (per instance) of them;
 * (6, 3), fp32 state, one family per instance, EXT 2: 2 spilled registers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_switches_are_declared_read_and_off_by_default():
    header = open(os.path.join(CSRC, "solver.h")).read()
    body = header[header.index("struct Switches {"):]
    body = body[:body.index("};")]
    assert re.search(r"\bstream_mpc = false\b", body) and re.search(r"\bstream_loop = false\b", body)
    solver = open(os.path.join(CSRC, "solver.hip")).read()
    reader = solver[solver.index("Switches read_switches() {"):]
    reader = reader[:reader.index("\n}")]
    assert 'w.stream_mpc = on("TINYMPC_HIP_STREAM_MPC");' in reader
    assert 'w.stream_loop = on("TINYMPC_HIP_STREAM_LOOP");' in reader
    # the chain asks the first switch, the loop is tried only inside the chain's branch (plan_rollout, the one place that reads
    # the two); a solver without the persistent workspace is refused before either route is taken
    plan = solver[solver.index("Solver::plan_rollout(int mpc_steps) {"):]
    plan = plan[:plan.index("\n}")]
    assert re.search(r"const bool stream = sw\.stream_mpc && !ke && !ce && !st\.adaptive_rho;", plan)
    assert re.search(r"\} else if \(stream\) \{\s*loop\.stream_loop = true;\s*route = \(sw\.stream_loop && ", plan)
    assert plan.index("if (!warm_start) return refuse(") < plan.index("} else if (stream) {")
    assert solver.count("sw.stream_loop") == 1 and plan.count("sw.stream_mpc") == solver.count("sw.stream_mpc") - 1   # (+ select_kernel's precision 2 gate)
    for shape in ("4_1", "6_3", "12_4"):
        assert os.path.isfile(os.path.join(CSRC, f"sinst_mpc_{shape}.hip"))


def test_forms_left_to_the_chain_are_the_listed_ones():
    """streamg_mpc_built, read as text: fp64 state is built for one family; (12, 4) fp32 state and (6, 3) per-instance EXT 2 are not"""
    entry = open(os.path.join(CSRC, "streamg_entry.hip.h")).read()
    fn = entry[entry.index("constexpr bool streamg_mpc_built("):]
    fn = fn[:fn.index("\n}")]
    assert "if (wide) return !het;" in fn
    assert "if (nx == 12 && nu == 4) return false;" in fn
    assert "if (nx == 6 && nu == 3 && het && ext == 2) return false;" in fn
    assert fn.count("return") == 4


@pytest.fixture(scope="module")
def mpc_kernels(tmp_path_factory):
    out = tmp_path_factory.mktemp("stream_mpc") / "sinst_mpc_12_4.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "sinst_mpc_12_4.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    lines = text.splitlines()
    kernels = {}
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN4tmpc23admm_streamg_mpc_kernelILi12ELi4ELi4ELi(\d)ELb([01])E([df])EEvNS_10AdmmParamsE):", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            kernels[(int(m.group(2)), m.group(3) == "1", m.group(4))] = [x.split()[0] for x in lines[i + 1:end]
                                                                        if x.startswith("\t") and not x.strip().startswith((";", "."))]
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    scratch = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    return kernels, spills, scratch


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_three_fp64_state_loop_kernels_without_scratch(mpc_kernels):
    kernels, spills, scratch = mpc_kernels
    assert sorted(kernels) == [(e, False, "d") for e in (0, 1, 2)]
    assert spills == [0] * 3 and scratch == [0] * 3
    for key, ops in kernels.items():
        assert not any(o.startswith("scratch_") for o in ops), key
        assert any(re.match(r"v_(fma|fmac|mul|add)_f64", o) for o in ops), key
        # the plant step's quad broadcasts are DPP moves, and the loop over steps is a backward branch beyond the iteration loop's
        assert any("dpp" in o for o in ops), key
        assert sum(o.startswith("s_cbranch") for o in ops) > 4, key
