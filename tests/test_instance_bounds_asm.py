"""Per-instance box bounds (tinympc_set_instance_bounds) without a GPU: the stream kernel's `ib` form (csrc/admm_streamg.hip.h,
admm_streamg_ib_kernel) of the tightest shape that must stay in registers — (6, 3): lane 3 owns no row, two rows per owning lane — in the
compiler's own assembly, compiled as the Makefile compiles csrc/sinst_ib_6_3.hip, and the new entry points from the header
down to the built library.
 * the three translation units csrc/sinst_ib_{4_1,6_3,12_4}.hip exist;
 * EXT in {0, 2} x {one family, one per instance} x OS: eight kernels, fp64 recurrences, fp32 state, fixed rho;
 * no scratch: vgpr_spill_count 0 and no scratch_ instruction in any of them;
 * the header declares tinympc_set_instance_bounds, tinympc_bounds_mode, tinympc_sharded_set_instance_bounds, the Python
   mirror binds them, and the built library exports them (this is the part that fails without the feature)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("tinympc_set_instance_bounds", "tinympc_bounds_mode", "tinympc_sharded_set_instance_bounds")


def test_units_exist_and_name_their_shape():
    for nx, nu in ((4, 1), (6, 3), (12, 4)):
        path = os.path.join(CSRC, f"sinst_ib_{nx}_{nu}.hip")
        assert os.path.isfile(path), path
        assert f"TMPC_DEFINE_STREAMG_IB({nx}, {nu}, 4)" in open(path).read()
    kernel = open(os.path.join(CSRC, "admm_streamg.hip.h")).read()
    # the form is a kernel of its own name, compiled from the stream kernel's text: the existing kernels keep their names
    assert "void admm_streamg_ib_kernel(const AdmmParams P)" in kernel
    assert re.search(r"bool ADP = false, class ST = float>\s*__global__", kernel)
    # the new kernel arguments sit behind everything the existing kernels read
    params = open(os.path.join(CSRC, "admm_params.h")).read()
    body = params[params.index("struct AdmmParams {"):]
    body = body[:body.index("\n};")]
    assert body.index("gslot_cap;") < body.index("*ibx, *ibu;") < body.index("ib_kx, ib_ku") < body.index("int ib_on;")


@pytest.fixture(scope="module")
def ib_kernels(tmp_path_factory):
    out = tmp_path_factory.mktemp("stream_ib") / "sinst_ib_6_3.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "sinst_ib_6_3.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    lines = text.splitlines()
    kernels = {}
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN4tmpc22admm_streamg_ib_kernelILi6ELi3ELi4ELi(\d)ELb([01])ELb([01])EEEvNS_10AdmmParamsE):", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            kernels[(int(m.group(2)), m.group(3) == "1", m.group(4) == "1")] = [
                x.split()[0] for x in lines[i + 1:end] if x.startswith("\t") and not x.strip().startswith((";", "."))]
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    return kernels, spills


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_eight_kernels_without_scratch(ib_kernels):
    kernels, spills = ib_kernels
    assert sorted(kernels) == [(e, h, o) for e in (0, 2) for h in (False, True) for o in (False, True)]
    assert spills == [0] * 8
    for key, ops in kernels.items():
        assert not any(o.startswith("scratch_") for o in ops), key
        assert any(re.match(r"v_(fma|fmac|mul|add)_f64", o) for o in ops), key    # fp64 recurrences
        # (6, 3): a lane's two state rows are one 8-byte access — the bound rows travel like the scratch rows
        assert sum(o == "global_load_dwordx2" for o in ops) >= 4, key


def test_header_declares_and_python_binds():
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
    from tinympc_julia_amd import tinympc
    for sym in SYMBOLS:
        assert sym in tinympc.SIGNATURES, sym
    assert hasattr(tinympc.BatchSolver, "set_instance_bounds") and hasattr(tinympc.BatchSolver, "bounds_mode")
    assert hasattr(tinympc.ShardedBatchSolver, "set_instance_bounds")
    julia = open(os.path.join(ROOT, "tinympc-julia_amd", "julia", "TinyMPC.jl")).read()
    assert "function set_instance_bounds(" in julia and "x_min::Array{Float64,3}" in julia


def test_built_library_exports_the_entry_points(hip_lib):
    import tinympc_julia_amd as t
    out = subprocess.run(["nm", "-D", "--defined-only", t.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for sym in SYMBOLS:
        assert sym in exported, sym
    for sym in SYMBOLS:      # ... and bound by load_library (AttributeError there if one were missing)
        assert getattr(hip_lib, sym).restype is not None
