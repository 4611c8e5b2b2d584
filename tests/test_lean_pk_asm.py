"""The packed slack / dual update of the headline kernel in the compiler's own assembly (csrc/admm_lean.hip.h: PK).

The unit is built as tests/test_lean_epilogue_asm.py builds it: admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true,
XB=false, zero references, fp32 state, the cartpole pattern> — what bench.py's default launches.  Its hot loop (the
iterations without residuals: 99 of 100) is the largest innermost backward-branch region with more than 100 v_fma_f64 and fewer
than 2 000 instructions.  Per iteration the 19 knots make 9 pairs and a single: two packed adds per pair in the forward sweep
(t = u + y, y = t - znew) and one in the backward sweep (r~ = znew - y), 27 v_pk_add_f32 for 54 scalar adds — 609 vector
instructions become 582 at most, without a spilled register.  With -DTMPC_LEAN_PK=0 the loop is the scalar one, 609
instructions exactly; the tolerance-terminated (LIVE) and state-bounded (XB) units never pack."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CARTPOLE_PATTERN = "0x1000a0021cc63ull"      # lean_pattern_rm of problems.cartpole's (A, B): csrc/linst_4_1_20.hip
N = 20
SCALAR_LOOP_VALU = 609                       # the scalar loop's vector instructions (profiles/r07_lean_fixed_cost.txt)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _unit(tmp_path, tag, flags, live="false", xb="false"):
    """(instructions of the kernel, its vgpr_spill_count) of the (4,1,20) cartpole-pattern unit with the given LIVE / XB"""
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    src, out = tmp_path / f"{tag}.hip", tmp_path / f"{tag}.s"
    src.write_text(f'#include "lean_entry.hip.h"\nTMPC_DEFINE_LEAN_JIT_ENTRY_SP("lean<4,1,20>", 4, 1, 20, {live}, true, true, {xb}, '
                   f"tmpc::REF_ZERO, float, {CARTPOLE_PATTERN})\n")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "-DTMPC_JIT_UNIT",
                    *flags, f"-I{csrc}", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True, timeout=600)
    lines = out.read_text().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN4tmpc16admm_lean_kernel\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    spills = [int(m) for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", "\n".join(lines))]
    return lines[start + 1:end], spills


def _ops(body):
    return [l.split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((";", "."))]


def _hot_loop(body):
    """opcodes of the largest backward-branch region with more than 100 v_fma_f64 and fewer than 2 000 instructions that
    holds no other such region (the loop over the iterations, which holds the residual iteration too, is one as well)"""
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    regions = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if not m or labels.get(m.group(1), i) >= i:
            continue
        ops = _ops(body[labels[m.group(1)]:i + 1])
        if sum(o == "v_fma_f64" for o in ops) > 100 and len(ops) < 2000:
            regions.append((labels[m.group(1)], i, ops))
    inner = [r for r in regions if not any(q is not r and r[0] <= q[0] and q[1] <= r[1] for q in regions)]
    assert inner, "hot loop not found"
    return max(inner, key=lambda r: len(r[2]))[2]


def _valu(ops):
    return sum(o.startswith("v_") for o in ops)


def test_headline_loop_packs_the_slack_and_dual_update(tmp_path):
    body, spills = _unit(tmp_path, "pk", [])
    loop = _hot_loop(body)
    pk, valu = sum(o == "v_pk_add_f32" for o in loop), _valu(loop)
    print(f"PK: {pk} v_pk_add_f32, {valu} VALU in the loop, spills {spills}")
    assert pk >= 3 * ((N - 1) // 2)
    assert valu <= 582
    assert spills == [0] and not any(o.startswith("scratch_") for o in _ops(body))


def test_switch_off_is_the_scalar_loop(tmp_path):
    body, spills = _unit(tmp_path, "pk0", ["-DTMPC_LEAN_PK=0"])
    loop = _hot_loop(body)
    print(f"PK=0: {_valu(loop)} VALU in the loop, spills {spills}")
    assert not any(o == "v_pk_add_f32" for o in _ops(body))
    assert _valu(loop) == SCALAR_LOOP_VALU


@pytest.mark.parametrize("live,xb", [("true", "false"), ("false", "true")], ids=["LIVE", "XB"])
def test_other_forms_never_pack(tmp_path, live, xb):
    body, _ = _unit(tmp_path, f"u_{live}_{xb}", [], live=live, xb=xb)
    assert not any(o == "v_pk_add_f32" for o in _ops(body))
