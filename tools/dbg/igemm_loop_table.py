#!/usr/bin/env python3
"""Where do the LDS-DMA requests, LDS reads, waits and MFMAs of a conv_igemm_kernel instantiation stand in its device assembly?
    hipcc <the Makefile's flags for conv_mfma.hip> -S --cuda-device-only -o conv_mfma.s conv_mfma.hip
    python tools/dbg/igemm_loop_table.py conv_mfma.s [substring of the mangled name, default: 128 x 128, GL, no residual / mask / tap sets]
Prints the kernel's instruction stream from the first LDS-DMA request to the last one's slice barrier, run-length coded: labels and
branches, `DMA` (buffer_load ... lds), ds_read_*, s_waitcnt, s_barrier, `MFMA`, and `valu` / `salu` for everything between them."""
import re
import sys

DEFAULT = "conv_igemm_kernelILi128ELi128ELi4ELi1ELi32ELi2ELb0ELb0ELb0ELb0ELb1ELb0ELb0ELb1EEE"


def table(path, key=DEFAULT):
    s = open(path).read()
    m = re.search(r"^(_Z\S*" + re.escape(key) + r"\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", s, re.S | re.M)
    assert m, "no such kernel"
    ev = []
    for line in m.group(2).split("\n"):
        t = line.strip()
        if not t or t.startswith(";") or t.startswith(".") and not t.startswith(".LBB"):
            continue
        op = t.split()[0]
        if t.startswith(".LBB"):
            k = t.split(":")[0] + ":"
        elif "offen lds" in t:
            k = "DMA"
        elif op.startswith("v_mfma"):
            k = "MFMA"
        elif op.startswith("ds_read") or op in ("s_barrier",) or op.startswith("s_cbranch") or op == "s_branch":
            k = t if op.startswith("s_") and op != "s_barrier" else op
        elif op == "s_waitcnt":
            k = t
        elif op.startswith("s_mov_b32") and "m0" in t or op == "s_nop":
            continue      # the request's own scalar part / hazard padding
        elif op.startswith("v_") or op.startswith("buffer_") or op.startswith("global_"):
            k = "valu" if op.startswith("v_") else op
        elif op.startswith("s_"):
            k = "salu"
        else:
            continue
        ev.append(k)
    first = ev.index("DMA")
    last = len(ev) - 1 - ev[::-1].index("DMA")
    end = next(i for i in range(last, len(ev)) if ev[i] == "s_barrier")
    # skip the prologue's requests: start at the first label behind the prologue's barrier
    out, prev, n = [], None, 0
    for k in ev[first:end + 40]:
        if k == prev:
            n += 1
        else:
            if prev is not None:
                out.append(prev + (" x%d" % n if n > 1 else ""))
            prev, n = k, 1
    out.append(prev + (" x%d" % n if n > 1 else ""))
    return out


if __name__ == "__main__":
    print("\n".join(table(sys.argv[1], *(sys.argv[2:3]))))
