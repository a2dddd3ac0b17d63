"""Static check of csrc/fused.hip (no GPU needed: hipcc cross-compiles for gfx950).  Three 512-thread workgroups per CU --
what the one-launch GCNConv step is tuned for -- need every K = 128 instance at <= 80 VGPRs without scratch.  The byte-mask
gather loop of the backward holds that only because an empty ordering asm keeps hipcc from converting a whole trip of
bytes at once; a compiler that schedules differently would bring the spills back with every functional test still
green, so the compiler's own resource report is checked here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_fused_kernels_fit_three_workgroups_per_cu(tmp_path):
    src = os.path.join(ROOT, "gcn-string_amd", "csrc", "fused.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-Wno-unused-function", "-DGCNX_BUILD", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "fused.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                found[name][key] = int(m.group(1))
    k128 = {n: v for n, v in found.items() if "gcn_conv_fused_kernelILi128E" in n}
    # weighted / unweighted x forward / backward x f32 / bf16x3, plus the four byte-mask backward instances
    assert len(k128) == 12, sorted(found)
    for n, v in k128.items():
        assert v["scratch"] == 0 and v["vgprs"] <= 80 and v["waves"] >= 6, (n, v)
    for n, v in found.items():
        if "gcn_conv_fused_kernel" in n:
            assert v["scratch"] == 0, (n, v)
