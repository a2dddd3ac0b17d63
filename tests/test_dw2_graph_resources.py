"""Static check of the dW1 + mask-product launch in csrc/gemm.hip (no GPU needed: hipcc cross-compiles for gfx950), in the
manner of tests/test_dw2_feed_resources.py.  gemm_f32_dw2g_kernel holds the fp32 tile bodies of dW1, the C-tile body (bf16 MFMA
passes over the three-way split of S2) and, in its <true> instance, the head body; the launch is tuned for four waves per SIMD
(at most 128 VGPRs + AGPRs) and four 256-thread workgroups per CU (at most 40 KiB of LDS each).  A compiler that allocates
differently would halve the occupancy with every functional test still green, so the compiler's own resource report is checked
(the report only, not the assembly)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_dw2g_kernels_keep_four_waves_per_simd_and_four_workgroups_per_cu(tmp_path):
    src = os.path.join(ROOT, "gcn-string_amd", "csrc", "gemm.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-Wno-unused-function", "-DGCNX_BUILD", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "gemm.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("spill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"),
                         ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                found[name][key] = int(m.group(1))
    dw2g = {n: v for n, v in found.items() if "gemm_f32_dw2g_kernel" in n}
    assert len(dw2g) == 2, sorted(found)                   # <true> with the head leaves, <false> without
    for n, v in dw2g.items():
        print(n, v)
        assert v["scratch"] == 0 and v.get("spill", 0) == 0 and v.get("sspill", 0) == 0, (n, v)
        assert v["waves"] >= 4 and v["lds"] <= 40960, (n, v)
        assert v["vgprs"] + v["agprs"] <= 128, (n, v)
    # the reduction launch that folds the scaled slabs: no scratch either, and all of its workgroups resident at config 2
    red = {n: v for n, v in found.items() if "reduce_sgd_kernel" in n}
    assert len(red) == 1
    for n, v in red.items():
        print(n, v)
        assert v["scratch"] == 0 and v["waves"] >= 4, (n, v)
