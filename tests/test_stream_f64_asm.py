"""The stream kernel's fp64-state form (csrc/admm_streamg.hip.h, ST = double) without a GPU: the switch that routes precision 2
to it, and the six kernels of the tightest shape — (12, 4): three state rows per lane, every knot buffer twice as wide — in
the compiler's own assembly, compiled as the Makefile compiles csrc/sinst_f64_12_4.hip.
 * TINYMPC_HIP_STREAM_F64 is a member of Switches, read in read_switches (so reload_switches picks it up), off by default;
 * EXT in {0, 1, 2} x OS in {false, true}: six kernels, fp64 recurrences, one family, fixed rho;
 * no scratch: vgpr_spill_count 0 and no scratch_ instruction in any of them;
 * the state rows travel wide: a lane's three doubles are one 16-byte and one 8-byte access, never 4-byte ones."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_switch_is_declared_read_and_off_by_default():
    header = open(os.path.join(CSRC, "solver.h")).read()
    body = header[header.index("struct Switches {"):]
    body = body[:body.index("};")]
    assert re.search(r"\bstream_f64 = false\b", body)
    solver = open(os.path.join(CSRC, "solver.hip")).read()
    reader = solver[solver.index("Switches read_switches() {"):]
    reader = reader[:reader.index("\n}")]
    assert 'w.stream_f64 = on("TINYMPC_HIP_STREAM_F64");' in reader
    # the precision-2 branch asks the route, and the route asks the switch
    assert re.search(r"route_stream_f64\(\) const \{\s*if \(!sw\.stream_f64\b", solver)
    for shape in ("4_1", "6_3", "12_4"):
        assert os.path.isfile(os.path.join(CSRC, f"sinst_f64_{shape}.hip"))


@pytest.fixture(scope="module")
def f64_kernels(tmp_path_factory):
    out = tmp_path_factory.mktemp("stream_f64") / "sinst_f64_12_4.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "sinst_f64_12_4.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    lines = text.splitlines()
    kernels = {}
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN4tmpc19admm_streamg_kernelILi12ELi4ELi4EdLi(\d)ELb0ELb([01])ELb0EdEEvNS_10AdmmParamsE):", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            kernels[(int(m.group(2)), m.group(3) == "1")] = [x.split()[0] for x in lines[i + 1:end]
                                                             if x.startswith("\t") and not x.strip().startswith((";", "."))]
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    return kernels, spills


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_six_kernels_without_scratch(f64_kernels):
    kernels, spills = f64_kernels
    assert sorted(kernels) == [(e, o) for e in (0, 1, 2) for o in (False, True)]
    assert spills == [0] * 6
    for key, ops in kernels.items():
        assert not any(o.startswith("scratch_") for o in ops), key
        assert any(re.match(r"v_(fma|fmac|mul|add)_f64", o) for o in ops), key


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_state_rows_travel_wide(f64_kernels):
    kernels, _ = f64_kernels
    for key, ops in kernels.items():
        ld16, ld8 = sum(o == "global_load_dwordx4" for o in ops), sum(o == "global_load_dwordx2" for o in ops)
        st16, st8 = sum(o == "global_store_dwordx4" for o in ops), sum(o == "global_store_dwordx2" for o in ops)
        # every state-shaped array of the sweeps is one 16-byte + one 8-byte access per lane (RX = 3), the input-shaped
        # ones (RU = 1) one 8-byte access: as many 16-byte accesses as state-shaped transfers, at least the box set's
        # (forward: g, v in / g, w (+ fused) out; backward: w (and g) in)
        assert ld16 >= 3 and st16 >= 2 and ld8 >= ld16 and st8 >= st16, (key, ld16, ld8, st16, st8)
        # 4-byte stores are the fp32 ends only: the solution (3 + 1 rows), iteration count, solved flag, 4 residuals, the
        # status block; nothing of the iteration
        assert sum(o == "global_store_dword" for o in ops) <= 3 + 1 + 2 + 4 + 5, key
