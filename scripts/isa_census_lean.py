"""Instruction census of the headline kernel's ADMM iteration from the compiler's own assembly (hipcc -S of csrc/linst_4_1_20.hip):
admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true, XB=false, REFS=zero> — the benchmark's instantiation (tolerances <= 0, bounds constant over
the knots, one wavefront per SIMD) — its innermost loop (the iterations that do not form residuals: 99 of 100), counted by class,
next to round 3's census of quad<4,1,20,g1>.  From r06 on the benchmark runs the sparse kernel of the cartpole pattern (SP != 0); the
dense (controller-Hessenberg, SP = 0) instantiation that TINYMPC_HIP_LEAN_DENSE=1 runs is counted beside it.  TMPC_CENSUS_ASM: an
existing hipcc -S output of the unit to count instead of compiling it.  From r21 on the benchmark runs the scaled sparse kernel
(csrc/linst_4_1_20_scaled.hip, the scaled cartpole pattern): that unit is compiled and counted, with the unscaled sparse kernel's
committed census (profiles/r16_cartpole_isa_census.json) beside it; from r22 on that kernel folds C into the costate's scale and
r21's census stands beside it too.  Output: profiles/<tag>_cartpole_isa_census.json"""
import collections, json, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r04"
asm = os.environ.get("TMPC_CENSUS_ASM") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "lean20_census.s")
if not os.environ.get("TMPC_CENSUS_ASM"):
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-honor-nans", "-fno-slp-vectorize", "--cuda-device-only",
                "-I" + os.path.join(ROOT, "tinympc-julia_amd/csrc"), "-S", os.path.join(ROOT, "tinympc-julia_amd/csrc", "linst_4_1_20_scaled.hip" if tag >= "r21" else "linst_4_1_20.hip"), "-o", asm], check=True,
               stderr=subprocess.DEVNULL)
lines = open(asm).read().splitlines()
# (the trailing template argument is the (A, B) pattern: 0x1000a0021cc63 = 281517928598627, the cartpole model's; 0 the dense form)
# (WS = MPC = false behind the pattern since the workspace-keeping forms exist)
KERNELS = {"sparse": "_ZN4tmpc16admm_lean_kernelILi4ELi1ELi20ELb0ELb1ELb1ELb0ELi0EfLm281517928598627ELb0ELb0EEEvNS_10AdmmParamsE:",
           "dense": "_ZN4tmpc16admm_lean_kernelILi4ELi1ELi20ELb0ELb1ELb1ELb0ELi0EfLm0ELb0ELb0EEEvNS_10AdmmParamsE:"}
if tag >= "r21":   # (0x4f000a0863cc63 = 22236566250572899: lean_pattern_scaled of the cartpole pattern)
    KERNELS = {"scaled": "_ZN4tmpc16admm_lean_kernelILi4ELi1ELi20ELb0ELb1ELb1ELb0ELi0EfLm22236566250572899ELb0ELb0EEEvNS_10AdmmParamsE:"}
if tag < "r08":
    KERNELS = {k: v.replace("ELb0ELb0EEEv", "EEEv") for k, v in KERNELS.items()}
if tag < "r06":
    KERNELS = {"dense": "_ZN4tmpc16admm_lean_kernelILi4ELi1ELi20ELb0ELb1ELb1ELb0ELi0EfEEvNS_10AdmmParamsE:"}


def census(want):
    return census_of(next(i for i, l in enumerate(lines) if l.startswith(want)))


def census_of(start):
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    lab = {}
    for n, b in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", b)
        if m and ("Inner Loop Header" in b or (n + 1 < len(body) and "Inner Loop Header" in body[n + 1])): lab[m.group(1)] = n
    loops = []
    for n, b in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", b)
        if m and m.group(1) in lab and lab[m.group(1)] < n: loops.append((lab[m.group(1)], n))
    def is_inst(l):
        s = l.strip()
        return bool(s) and not s.startswith((";", ".", "//")) and not s.endswith(":")
    lo, hi = max(loops, key=lambda lp: sum(1 for l in body[lp[0]:lp[1] + 1] if is_inst(l) and re.match(r"v_(fma|fmac|mul|add)_f64", l.strip())))
    classes = collections.OrderedDict([
        ("fp64 FMA / mul / add (the recurrences)", r"v_(fma|fmac|mul|add)_f64"),
        ("fp32 <-> fp64 conversions", r"v_cvt_f(32_f64|64_f32)"),
        ("AGPR moves (v_accvgpr_read / write)", r"v_accvgpr_"),
        ("fp32 packed add / sub (two knots per instruction)", r"v_pk_(add|mul|fma)_f32"),
        ("fp32 arithmetic (add / sub)", r"v_(add|sub|subrev|mul|fma|fmac)_f32"),
        ("fp32 med3 (the box projection)", r"v_(min|max|med3)_f32"),
        ("moves / selects / integer VALU", r"v_(mov|cndmask|readlane|readfirstlane|writelane|add_u32|lshl|and|or|cmp)"),
        ("other VALU", r"v_"),
        ("scalar memory", r"s_load|s_buffer_load"), ("scalar ALU / control", r"s_(?!waitcnt|nop|load|buffer_load)"), ("waits / nops", r"s_waitcnt|s_nop"),
        ("LDS", r"ds_"), ("global / scratch memory", r"global_|scratch_|buffer_|flat_")])
    counts = collections.OrderedDict((k, 0) for k in classes)
    for l in body[lo:hi + 1]:
        if not is_inst(l): continue
        op = l.strip().split()[0]
        for k, pat in classes.items():
            if re.match(pat, op): counts[k] += 1; break
    valu = sum(v for k, v in counts.items() if k.split()[0] in ("fp64", "fp32", "AGPR", "moves", "other"))
    meta = {}
    for l in lines:
        pass
    out = {"kernel": "lean<4,1,20> = admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true, XB=false, REFS=zero> (the benchmark's instantiation)",
           "instructions_per_iteration": sum(counts.values()), "by_class": counts, "valu_instructions": valu,
           "necessary_fp64_fma": counts["fp64 FMA / mul / add (the recurrences)"],
           "necessary_share_of_valu": counts["fp64 FMA / mul / add (the recurrences)"] / valu,
           "floor_ms_100_iterations_at_4_cycles_2.4GHz": 4 * valu * 100 / 2.4e9 * 1e3,
           "round3_quad_g1": {"valu_instructions": 1506, "fp64": 911, "conversions": 228, "agpr_moves": 268, "kernel_ms": 0.3537},
           "round4_lean_dense": {"instructions": 1029, "valu_instructions": 1025, "fp64": 911},
           "coordinates": "controller-Hessenberg (x = T x^, T orthogonal; HB = !LIVE && !XB && ONE): banded M^ = T'MT, trapezoidal b^ = T'B" if tag >= "r05" else "plain",
           "scratch_instructions_in_kernel": sum(1 for l in body if re.match(r"\s+scratch_", l)),
           "measured": "profiles/r04_lean_timeline.txt: 4.09 core cycles per loop instruction in-kernel (s_memtime), 2.08 GHz with every CU busy (2.35 GHz at 80 CUs)"}
    return out


res = {k: census(w) for k, w in KERNELS.items()}
out = res.get("scaled") or res.get("sparse", res["dense"])
if "scaled" in res:
    out["kernel"] = ("lean<4,1,20> = admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true, XB=false, REFS=zero, SP=scaled cartpole pattern> "
                     "(the benchmark's instantiation)")
    out["coordinates"] = ("diagonally scaled, x^ = S x: sparse sweeps on S A S^-1 and S B with units at A01, A12, A23, B3 "
                          "(u = -K^ x^ - d, x^+ = A^ x^ + B^ u; p^ = W x^ + A^' p^ - K^' t)")
    prev = json.load(open(os.path.join(ROOT, "profiles", "r16_cartpole_isa_census.json")))
    out["unscaled_sparse_r16"] = {k: prev[k] for k in ("instructions_per_iteration", "valu_instructions", "necessary_fp64_fma", "by_class")}
    for k in ("round3_quad_g1", "round4_lean_dense"):
        out.pop(k, None)
    if tag >= "r22":   # C folded into the costate's scale (admm_lean.hip.h: FOLD): the same kernel symbol, r21's census beside it
        out["coordinates"] = ("diagonally scaled, x^ = S x, the costate carried as pv = c p^ with the scalar c = C = -rho Quu_inv: "
                              "u = -K^ x^ - d, x^+ = A^ x^ + B^ u; d = c r~ + B^' pv (no product by C), pv = c W x^ + A^' pv - K^' d; "
                              "24 fp64 per knot for 25")
        prev = json.load(open(os.path.join(ROOT, "profiles", "r21_cartpole_isa_census.json")))
        out["scaled_unfolded_r21"] = {k: prev[k] for k in ("instructions_per_iteration", "valu_instructions", "necessary_fp64_fma", "by_class")}
        out["predicted_share_of_loop_removed"] = 1.0 - out["valu_instructions"] / prev["valu_instructions"]
if "sparse" in res:
    out["kernel"] = ("lean<4,1,20> = admm_lean_kernel<4,1,20, LIVE=false, UBK=true, ONE=true, XB=false, REFS=zero, SP=cartpole pattern> "
                     "(the benchmark's instantiation)")
    out["coordinates"] = "plain, sparse sweeps on the model's A and B (u = -Kinf x - d, x+ = A x + B u; p~ = x + A' p~ - Kinf' t)"
    out["dense_hessenberg_SP0"] = {k: res["dense"][k] for k in ("instructions_per_iteration", "valu_instructions", "necessary_fp64_fma",
                                                                 "scratch_instructions_in_kernel", "by_class")}
json.dump(out, open(os.path.join(ROOT, "profiles", f"{tag}_cartpole_isa_census.json"), "w"), indent=1)
print(json.dumps(out, indent=1))
