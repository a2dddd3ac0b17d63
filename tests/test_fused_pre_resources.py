"""Static check of gcn_conv_pre_kernel in csrc/fused.hip (no GPU needed: hipcc cross-compiles for gfx950), next to
test_fused_resources.py: the forward on a stored A X is measured and kept at three 512-thread workgroups per CU for the
flagship width (K = 128: 6 waves per SIMD, at most 80 VGPRs) and at four for the narrower ones (8 waves per SIMD) -- the
compiler's own figures of the build LOG.md Round 6 records -- without scratch.  A compiler that allocates differently would
lose that with every functional test still green."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# waves / SIMD per (K, X3) instance in the kept build (LOG.md, Round 6: compiler resource table)
KEPT_WAVES = {(128, False): 6, (128, True): 6, (64, False): 8, (64, True): 8, (32, False): 8, (32, True): 8}


def test_pre_kernels_have_no_scratch_and_keep_their_occupancy(tmp_path):
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
    pre = {}
    for n, v in found.items():
        m = re.search(r"gcn_conv_pre_kernelILi(\d+)ELb([01])E", n)
        if m:
            pre[int(m.group(1)), m.group(2) == "1"] = v
        assert "gcn_conv_pre_kernel" not in n or "gcn_conv_fused_kernel" not in n      # a kernel of its own name
    assert sorted(pre) == sorted(KEPT_WAVES), sorted(found)
    for key, v in pre.items():
        assert v["scratch"] == 0 and v["waves"] >= KEPT_WAVES[key], (key, v)
