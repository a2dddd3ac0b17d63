"""Static check of the dW1 + dW2 launch in csrc/gemm.hip (no GPU needed: hipcc cross-compiles for gfx950).  The launch is tuned
for four waves per SIMD (at most 128 VGPRs + AGPRs) and four 256-thread workgroups per CU (at most 40 KiB of LDS each), and
gemm_f32_dw2_head_kernel shares its register budget with the head body: both kernels now hold two tile bodies (dw_tile_interior
and gemm_f32_tile) next to it.  A compiler that allocates differently would halve the occupancy with every functional test
still green, so the compiler's own resource report is checked here (the report only, not the assembly)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_dw2_kernels_keep_four_waves_per_simd_and_four_workgroups_per_cu(tmp_path):
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
                         ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                found[name][key] = int(m.group(1))
    dw2 = {n: v for n, v in found.items() if "gemm_f32_dw2_kernel" in n or "gemm_f32_dw2_head_kernel" in n}
    assert len(dw2) == 2, sorted(found)
    for n, v in dw2.items():
        print(n, v)
        assert v["scratch"] == 0 and v["waves"] >= 4 and v["lds"] <= 40960, (n, v)
        assert v["vgprs"] + v["agprs"] <= 128, (n, v)
