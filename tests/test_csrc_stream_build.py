"""CPU: what the compiler makes of the streaming kernels of elementwise.hip that keep four rows in flight per thread (GroupNorm apply,
GroupNorm backward statistics and apply, the float4 column sum, the per-level scale; hipcc cross-compiles without a GPU), read from
tools/kernel_resources.py: no scratch, no spills, and few enough registers for four waves per SIMD (128) -- eight 16-byte loads in flight
per thread are 32 registers, and a launch of these kernels wants its workgroups resident together.  Resource numbers only.  The
constants that tests/test_gpu_stream_exact.py restates are held to the source here."""
import os
import re
import shutil
import subprocess
import sys

import pytest

import reduce_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "erd_amd", "csrc", "elementwise.hip")

TOUCHED = ["gn_apply_kernel<256, 32, float>", "gn_apply_kernel<256, 32, erd::bf16s>",
           "gn_bwd_stats_kernel<256, 32, float>", "gn_bwd_stats_kernel<256, 32, erd::bf16s>",
           "gn_bwd_apply_kernel<256, 32, float>", "gn_bwd_apply_kernel<256, 32, erd::bf16s>",
           "colsum_vec_kernel<float>", "colsum_vec_kernel<erd::bf16s>", "colsum_kernel<float>", "colsum_kernel<erd::bf16s>",
           "level_scale_kernel", "level_scale_bwd_kernel<true>", "level_scale_bwd_kernel<false>"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_streaming_kernels_use_no_scratch_and_allow_four_waves_per_simd():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(?:void )?(.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) spill\s+(\d+)/(\d+)\s+occ (\d+) scratch (\d+)$", line)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    assert len(rows) > 30, r.stdout[-2000:]
    for name in TOUCHED:
        assert name in rows, (name, sorted(rows))
        vgpr, agpr, vspill, sspill, occ, scratch = rows[name]
        print(f"{name}: {vgpr} VGPRs, {occ} waves per SIMD")
        assert (scratch, vspill, sspill, agpr) == (0, 0, 0, 0), (name, rows[name])
        assert vgpr <= 128 and occ >= 4, (name, rows[name])


def test_stream_test_constants_match_the_source():
    src = open(SRC).read()
    for needle in ("GN_FLIGHT = 4;", "GN_ROWS = 128;", "GN_STAT_ROWS = 512;", "#define COLSUM_WGS 128", "r + 4 * (GN_FLIGHT - 1) < r1; r += 4 * GN_FLIGHT",
                   "r + 48 < r1; r += 64", "C4 < 64 ? C4 : 64", "unit = 4 * lanes", "i + 3 * 256 < cnt4; i += 4 * 256", "for (int64_t i = threadIdx.x; i < cnt; i += 256) y[base + i] = x[base + i] * a;",
                   "threadIdx.x & 63, rl = threadIdx.x >> 6"):
        assert needle in src, needle
    assert (R.GN_ROWS, R.GN_STAT_ROWS, R.GN_STAT_LANES, R.COLSUM_RPB) == (128, 512, 16, 64)
    # the 16-byte paths are taken on alignment, the 4-byte ones otherwise
    assert "C % 4 == 0 && aligned16(x, dy) && aligned16(dx, dx)" in src
    assert "map_type == ERD_BF16 ? 7 : 15" in src
