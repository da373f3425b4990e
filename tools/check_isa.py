#!/usr/bin/env python3
"""Static checks on the gfx950 code objects that correctness/performance depend on (no GPU needed).

  * no kernel may use scratch (private segment): a kernel with register spills returned wrong,
    run-to-run different results from a hipGraph replay / beside a second stream on this stack
    ("Compiler / runtime hazards")
  * the LDS-DMA GEMM (bf16, f16, pair, fp8- and int4-operand forms) must not wait vmcnt(0) in front of a tile's first
    ds_read (Makefile note on gemm.o)
  * the f16 decode GEMV (ANYREF_MODE_PERF_F16) must multiply on the packed f16 dot (v_dot2[c]_f32_f16), not fall back to
    unpack + FMA
  * the f16-pair GEMM (ANYREF_MODE_PARITY16_F16) must multiply on the f16 MFMA only (a bf16 MFMA there would read f16 terms as
    bf16 words), and its decode GEMV must exist

usage: python tools/check_isa.py    (compiles anyref_amd/csrc/*.hip to assembly under /tmp)
"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyref_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
         "--cuda-device-only", "-S"]


def asm_of(src, strict):
    out = os.path.join(tempfile.gettempdir(), "anyref_isa_" + os.path.basename(src) + ".s")
    flags = FLAGS + ([] if strict else ["-fno-strict-aliasing"])
    subprocess.run(["hipcc"] + flags + [os.path.join(CSRC, src), "-o", out], check=True)
    return open(out).read()


def main():
    bad = 0
    allowed_scratch = ()
    for src in ("gemm.hip", "gemm_f16.hip", "gemm_sp16.hip", "gemm_sp16h.hip", "gemv.hip", "gemv_int4.hip", "attention.hip", "ops.hip"):
        s = asm_of(src, strict=src in ("gemm.hip", "gemm_f16.hip", "gemm_sp16.hip", "gemm_sp16h.hip", "gemv.hip", "gemv_int4.hip"))
        for name, seg in re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", s):
            if int(seg) > 0 and not any(a in name for a in allowed_scratch):
                print(f"FAIL {src}: {name} uses {seg} bytes of scratch")
                bad += 1
        if src in ("gemm.hip", "gemm_f16.hip", "gemm_sp16.hip", "gemm_sp16h.hip"):
            for m in re.finditer(r"^(_ZN6anyref16gemm_glds_kernel\S*):[^\n]*\n(.*?)\.Lfunc_end", s, re.S | re.M):
                lines = m.group(2).split("\n")
                n = sum(1 for k, l in enumerate(lines)
                        if "s_waitcnt vmcnt(0)" in l and any("ds_read" in x for x in lines[k + 1:k + 4]))
                if n:
                    print(f"FAIL {src}: {m.group(1)} waits vmcnt(0) before {n} ds_read group(s)")
                    bad += 1
        if src == "gemm.hip":  # the int4-operand form (last template argument) is among the kernels checked above
            if not re.search(r"^_ZN6anyref16gemm_glds_kernelI\S*NS_4bf16ELb1EEEvNS_8GemmArgsE:", s, re.M):
                print("FAIL gemm.hip: no int4-operand LDS-DMA GEMM instantiation found")
                bad += 1
        if src == "gemm_sp16h.hip":
            kernels = re.findall(r"^(_ZN6anyref16gemm_glds_kernel\S*):[^\n]*\n(.*?)\.Lfunc_end", s, re.S | re.M)
            if not kernels:
                print("FAIL gemm_sp16h.hip: no LDS-DMA GEMM instantiation found")
                bad += 1
            for name, body in kernels:
                if "v_mfma_f32_16x16x32_f16" not in body or re.search(r"v_mfma_f32_16x16x\d+_bf16", body):
                    print(f"FAIL gemm_sp16h.hip: {name} does not multiply on the f16 MFMA alone")
                    bad += 1
        if src == "gemv.hip":
            if not re.search(r"^_ZN6anyref11gemv_kernelINS_5sp16hE\S*:", s, re.M):
                print("FAIL gemv.hip: no f16-pair decode GEMV instantiation found")
                bad += 1
            f16 = re.findall(r"^(_ZN6anyref11gemv_kernelINS_3f16E\S*):[^\n]*\n(.*?)\.Lfunc_end", s, re.S | re.M)
            if not f16:
                print("FAIL gemv.hip: no f16 decode GEMV instantiation found")
                bad += 1
            for name, body in f16:
                if not re.search(r"\bv_dot2c?_f32_f16(_e32|_e64)?\s", body):
                    print(f"FAIL gemv.hip: {name} has no v_dot2_f32_f16 / v_dot2c_f32_f16 (unpack + FMA fallback)")
                    bad += 1
    print("isa check:", "FAILED" if bad else "ok")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
