"""CPU: what the compiler makes of the Winograd-domain weight-gradient kernel (erd_amd/csrc/wgrad_wino.hip; hipcc cross-compiles without
a GPU).  The kernel runs 512 threads on one CU -- two waves per SIMD, 256 registers each -- with 128 of them accumulators and the raw
loads of the next K-step in flight under the MFMAs: a piece that does not fit becomes scratch memory, whose loads wait in the same
in-order counter as the operand loads.  So: no scratch, all LDS dynamic (the host sizes it), at most 256 registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wgrad_wino_kernel_uses_no_scratch_only_dynamic_lds_and_at_most_256_registers(tmp_path):
    mk = open(os.path.join(ROOT, "erd_amd", "csrc", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    gemm = re.search(r"^GEMM_FLAGS := (.*)$", mk, re.M).group(1).split()
    assert re.search(r"wgrad_wino\.o:[^\n]*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(GEMM_FLAGS\) -c", mk)      # the flags below are the Makefile's for this file
    assert re.search(r"^SRCS := [^\n]*\\\n[^\n]*wgrad_wino\.hip", mk, re.M) and "wgrad_wino.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1)
    out = tmp_path / "wgrad_wino.s"
    r = subprocess.run([HIPCC, *cxx, *gemm, "-S", "--cuda-device-only", "-o", str(out), "wgrad_wino.hip"],
                       cwd=os.path.join(ROOT, "erd_amd", "csrc"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(out).read()
    seen = 0
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", s, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if "conv_wgrad_wino_kernel" not in name:
            continue
        seen += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name
        code = [t.strip() for t in body.split("\n") if t.strip() and not t.strip().startswith(";")]
        assert not any(t.startswith("scratch_") for t in code), name
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))      # (the unified file: architectural + accumulation registers)
        print(f"{name}: {vgprs} registers, {sum(t.startswith('v_mfma') for t in code)} MFMAs in {len(code)} instructions")
        assert vgprs <= 256, (name, vgprs)
    assert seen == 1, seen
