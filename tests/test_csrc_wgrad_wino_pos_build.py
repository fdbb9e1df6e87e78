"""CPU: what the compiler makes of the one-position-per-workgroup kernel of the Winograd-domain weight gradient (wgrad_wino_pos_kernel,
erd_amd/csrc/wgrad_wino.hip; hipcc cross-compiles without a GPU).  Like the row kernel (tests/test_csrc_wgrad_wino_build.py) it runs 512
threads on one CU -- two waves per SIMD, 256 registers each -- with 128 of them accumulators; its raw loads of the next K-step are up to
64 registers (16 eight-byte pieces of x, 16 of dz at the positions whose row and column both combine two entries) in flight under the
MFMAs, which is why the x fragments are read one column block at a time.  So: no scratch, all LDS dynamic, at most 256 registers, and one
K loop: 48 MFMAs (2 x 4 blocks x 6 limb products)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wgrad_wino_pos_kernel_uses_no_scratch_only_dynamic_lds_and_at_most_256_registers(tmp_path):
    mk = open(os.path.join(ROOT, "erd_amd", "csrc", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    gemm = re.search(r"^GEMM_FLAGS := (.*)$", mk, re.M).group(1).split()
    assert re.search(r"wgrad_wino\.o:[^\n]*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(GEMM_FLAGS\) -c", mk)      # the flags below are the Makefile's for this file
    out = tmp_path / "wgrad_wino.s"
    r = subprocess.run([HIPCC, *cxx, *gemm, "-S", "--cuda-device-only", "-o", str(out), "wgrad_wino.hip"],
                       cwd=os.path.join(ROOT, "erd_amd", "csrc"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(out).read()
    seen = 0
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", s, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if "wgrad_wino_pos_kernel" not in name:
            continue
        seen += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name
        code = [t for t in (t.split(";")[0].strip() for t in body.split("\n")) if t]      # (labels carry trailing comments)
        assert not any(t.startswith("scratch_") for t in code), name
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))      # (the unified file: architectural + accumulation registers)
        # the K loop: from the label the last backward branch across the MFMAs jumps to, up to that branch (loads, MFMAs, barrier, staging)
        first = next(i for i, t in enumerate(code) if t.startswith("v_mfma"))
        labels = {t[:-1]: i for i, t in enumerate(code) if t.endswith(":")}
        back = [i for i, t in enumerate(code) if i > first and re.match(r"s_c?branch", t) and labels.get(t.split()[-1], len(code)) <= first]
        loop = code[labels[code[back[-1]].split()[-1]]:back[-1] + 1] if back else code[first:]
        mfmas = sum(t.startswith("v_mfma") for t in loop)
        print(f"{name}: {vgprs} registers; K loop: {mfmas} MFMAs in {len(loop)} instructions, {sum(t.startswith('v_') for t in loop) - mfmas} other "
              f"vector instructions, {sum(t.startswith('buffer_load') for t in loop)} loads, {sum(t.startswith('ds_write') for t in loop)} LDS stores, "
              f"{sum(t.startswith('ds_read') for t in loop)} LDS reads")
        assert vgprs <= 256, (name, vgprs)
        assert sum(t.startswith("v_mfma") for t in code) == 48 and mfmas == 48, name
    assert seen == 1, seen
