#!/usr/bin/env python3
"""Per-launch times of the streaming kernels of elementwise.hip at the step's shapes, set against a copy of the same bytes.

  tools/bench_stream.py [--json OUT]                 time the library that ERD_HIP_LIB selects (default: the built one)
  tools/bench_stream.py --compare PARENT.json NEW.json [...]   one table of several such runs (taken in one session on one box)

GroupNorm on the head's [4, 22400, 256] fp32 maps, the column sum on 89 600 x 68 and x 80, the level scale on [4, 22400, 68].
Each entry point is launched 10 times between HIP events of its own (after 3 warm-up launches): median, min, max in microseconds.
The yardstick is measured in the same process: torch's copy_ of a tensor with the same read + write bytes.  gn_bwd is
erd_gn_relu_bwd whole (workspace fill, statistics, apply); `rocprofv3 --kernel-trace --stats` on this script separates its kernels.
The sha256 of every stored output is printed, so that two libraries can be told to compute the same bits."""
import argparse
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure():
    import torch
    from erd_amd import _lib, kernels as K

    sizes, h, w = [], 100, 168
    for _ in range(5):
        sizes.append((h, w)); h, w = (h + 1) // 2, (w + 1) // 2
    N, A = 4, sum(a * b for a, b in sizes)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    c, dy = rnd(N, A, 256) * 2 + 0.3, rnd(N, A, 256)
    gamma, beta = torch.rand(256, device="cuda", generator=g) + 0.5, rnd(256) * 0.3
    x68, d68, x80 = rnd(N, A, 68), rnd(N, A, 68), rnd(N, A, 80)
    alphas = torch.rand(5, device="cuda", generator=g) + 0.5
    _, mr = K.gn_relu_forward(c, gamma, beta, sizes)
    outs = {}

    def apply():
        import ctypes as C
        y = torch.empty_like(c)
        lv = K.make_levels(sizes)
        K.call("erd_gn_relu_apply", K._p(c), K._p(y), K._p(gamma), K._p(beta), K._p(mr), N, A, 256, 32, C.byref(lv), 0, K._stream())
        outs["gn_apply y"] = y

    def bwd():
        outs["gn_bwd dc"], outs["gn_bwd dgamma (atomic)"], outs["gn_bwd dbeta (atomic)"] = K.gn_relu_backward(c, dy, gamma, beta, mr, sizes)

    def cs(x, name):
        def f():
            outs[name + " (atomic)"] = K.colsum(x.view(-1, x.shape[-1]))
        return f

    def ls():
        outs["level_scale y"] = K.level_scale(x68, alphas, sizes)

    def lsb():
        outs["level_scale_bwd dx"], outs["level_scale_bwd dalphas (atomic)"] = K.level_scale_bwd(x68, d68, alphas, sizes)

    mb = lambda t: t.numel() * t.element_size() / 1e6
    cases = [("gn_apply", apply, 2 * mb(c)), ("gn_bwd", bwd, 5 * mb(c)), ("colsum_68", cs(x68, "colsum_68"), mb(x68)),
             ("colsum_80", cs(x80, "colsum_80"), mb(x80)), ("level_scale", ls, 2 * mb(x68)), ("level_scale_bwd", lsb, 3 * mb(x68))]

    def times(fn, n=10, warm=3):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for _ in range(warm):                       # the timed launches queue behind these: no launch starts on an idle GPU
            fn()
        for s, e in ev:
            s.record(); fn(); e.record()
        torch.cuda.synchronize()
        t = [s.elapsed_time(e) * 1e3 for s, e in ev]
        return dict(median=statistics.median(t), min=min(t), max=max(t))

    res = {"lib": _lib.LIB_PATH, "csrc_sha": _lib.load().erd_csrc_sha().decode(), "kernels": {}}
    for name, fn, mbytes in cases:
        src = torch.empty(int(mbytes * 1e6 / 2 / 4), device="cuda").normal_()
        dst = torch.empty_like(src)
        t, tc = times(fn), times(lambda: dst.copy_(src))
        res["kernels"][name] = dict(mb=mbytes, **t, copy=tc)
        del src, dst
    torch.cuda.synchronize()
    res["sha"] = {k: hashlib.sha256(v.detach().cpu().numpy().tobytes()).hexdigest()[:16] for k, v in sorted(outs.items())}
    return res


def show(res):
    print(f"library {res['lib']}")
    print(f"{'entry point':<16} {'MB':>6} {'median us':>10} {'min':>8} {'max':>8} {'TB/s':>6} | {'copy us':>8} {'copy TB/s':>9} | copy/kernel")
    for k, v in res["kernels"].items():
        print(f"{k:<16} {v['mb']:6.1f} {v['median']:10.1f} {v['min']:8.1f} {v['max']:8.1f} {v['mb'] / v['median']:6.2f} | "
              f"{v['copy']['median']:8.1f} {v['mb'] / v['copy']['median']:9.2f} | {v['copy']['median'] / v['median']:.2f}")
    for k, v in res["sha"].items():
        print(f"  sha256 {k:<34} {v}")


def compare(paths):
    runs = [json.load(open(p)) for p in paths]
    base = runs[0]
    print("median us per launch (fraction of the same run's copy rate); verdict against the first run: faster when its median is below the")
    print("first run's median by more than the first run's max - min")
    print(f"{'entry point':<16}" + "".join(f" {os.path.basename(p)[:-5]:>22}" for p in paths))
    for k in base["kernels"]:
        line = f"{k:<16}"
        b = base["kernels"][k]
        for r in runs:
            v = r["kernels"][k]
            tag = "" if r is base else (" faster" if b["median"] - v["median"] > b["max"] - b["min"] else " same")
            line += f" {v['median']:8.1f} ({v['copy']['median'] / v['median']:.2f}){tag:>7}"
        print(line + f"   parent max - min {b['max'] - b['min']:.1f}")
    for k in base["sha"]:
        same = ["=" if r["sha"].get(k) == base["sha"][k] else "differs" for r in runs[1:]]
        print(f"  bits of {k:<34} {' '.join(same)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--compare", nargs="+")
    a = ap.parse_args()
    if a.compare:
        compare(a.compare)
    else:
        r = measure()
        show(r)
        if a.json:
            json.dump(r, open(a.json, "w"), indent=1)
