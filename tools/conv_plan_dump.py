"""Every answer of the conv host layer's introspection entry points over a sweep of problems, one line each: the return code and
result of et_conv2d_kernel_name (ops 0..4, every parity class), et_conv2d_stem_kernel_name, et_conv2d_stats_rows_for and
et_conv2d_stats_adds_for (ops 0..2).  Host only (no GPU needed: device_cus() falls back to 256 compute units, the MI355X's count).

A change of the conv host layer (csrc/conv_host.hip; csrc/conv_host.h holds the row lists it selects from) that is meant to leave the kernel selection alone is checked by dumping before and after and
diffing the two files:
    python tools/conv_plan_dump.py --lib <old libet_hip.so> > old.txt;  python tools/conv_plan_dump.py > new.txt;  diff old.txt new.txt

The sweep: every tests/test_conv.py SELECT case, every conv of the three bench workloads at their batch sizes, the stream kernel's
16 + 1 layer shapes, rejected arguments; for the three dtypes, with and without a zero page, and with the persistent-grid test
hooks (ET_CONV_S1_WGS, ET_CONV_STEM_WGS) and ET_STEM_U8 unset and set."""
import argparse
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problems():
    """(N, H, W, Cin, Cout, k, stride, pad), in a fixed order, without repeats"""
    from tests import test_conv as tc
    out = [c[0] for c in tc.SELECT]
    for wl, batches in (("v5l-ssod", (16, 32, 64)), ("v5s-sup", (64,)), ("v8-sup", (32,))):
        shapes = tc._workload_conv_shapes(wl)
        for B in batches:
            for (h, w, ci, co, k, s, p) in shapes:
                out.append((B, h, w, 8 if k == 6 else (ci + 7) // 8 * 8, (co + 7) // 8 * 8, k, s, p))
    out += [(1, 8, 8, 64 * kc, co, 1, 1, 0) for kc in (1, 2, 4) for co in (64, 128, 256)]
    out += [
        (1, 16, 16, 16, 16, 7, 1, 3),      # more than 36 taps
        (1, 16, 16, 16, 16, 3, 0, 1),      # stride 0
        (0, 16, 16, 16, 16, 3, 1, 1),      # N = 0
        (1, 16, 16, 12, 16, 3, 1, 1),      # Cin % 8 != 0 (16-bit types)
        (1, 16, 16, 16, 12, 3, 1, 1),      # Cout % 8 != 0: no dgrad
        (1, 16, 16, 16, 16, 3, 3, 1),      # dgrad stride 3
        (1, 1, 1, 16, 16, 1, 2, 0),        # stride 2 on one pixel: three parity classes are empty
    ]
    return list(dict.fromkeys(out))


def dump(dll, out):
    buf = ctypes.create_string_buffer(256)

    def name(fn, *a):
        buf.value = b""
        rc = fn(*a, buf, 256)
        return f"{rc}:{buf.value.decode() if rc == 0 else ''}"

    probs = problems()
    knobs = ("ET_CONV_S1_WGS", "3"), ("ET_CONV_STEM_WGS", "3"), ("ET_STEM_U8", "0")
    for on in itertools.product((False, True), repeat=len(knobs)):
        for (k, v), o in zip(knobs, on):
            os.environ.pop(k, None)
            if o:
                os.environ[k] = v
        env = ",".join(f"{k}={v}" for (k, v), o in zip(knobs, on) if o) or "-"
        for dt, zp, (N, H, W, ci, co, k, s, p) in itertools.product((0, 1, 2), (1, 0), probs):
            head = f"env {env} dtype {dt} zp {zp} conv {N} {H} {W} {ci} {co} {k} {s} {p}"
            for op in range(-1, 6):                      # -1 and 5: out of range
                for pc in range(4):
                    out.write(f"{head} name op {op} class {pc} -> {name(dll.et_conv2d_kernel_name, op, dt, N, H, W, ci, co, k, k, s, p, zp, pc)}\n")
            for op, u8 in itertools.product((0, 2), (0, 1)):
                out.write(f"{head} stem_name op {op} u8 {u8} -> {name(dll.et_conv2d_stem_kernel_name, op, dt, u8, 3, N, H, W, co, k, k, s, p)}\n")
            for op in range(-1, 4):
                rows = dll.et_conv2d_stats_rows_for(op, dt, N, H, W, ci, co, k, k, s, p, zp)
                adds = dll.et_conv2d_stats_adds_for(op, dt, N, H, W, ci, co, k, k, s, p, zp)
                out.write(f"{head} stats op {op} -> rows {rows} adds {adds}\n")
    for k, _ in knobs:
        os.environ.pop(k, None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=None, help="the libet_hip.so to ask (default: this tree's build)")
    args = ap.parse_args()
    from efficientteacher_amd import _lib
    dump(_lib.load(args.lib), sys.stdout)
