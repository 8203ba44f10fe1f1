"""Timing of the Thomas-Middlecoff evaluation (tm_smoother_update_control_function: k_tm_edges + k_tm_blend, K10) on the 4096^2 bench block
beside K1 (TFI, tm_dev_tfi_block on device pointers) in the same process and run -- the yardstick: both write 16 B/node and read edges only.
An event pair per repeat around each call, repeats interleaved; median and min - max.

    python tools/control_field_timing.py [--repeats 7] [--size 4096] [--out profiles/control_field_timing.txt]      (needs the MI355X)"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from turbomesh_amd import _capi, configs  # noqa: E402
from turbomesh_amd.smoothing import smooth, solver, wall_control_function as wcf  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return f"median {np.median(v):8.4f}  min {v.min():8.4f}  max {v.max():8.4f}"


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join("profiles", "control_field_timing.txt"))
    args = ap.parse_args()
    n = args.size
    L = _capi.lib()
    edges = configs.single_block_edges(n, n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    pts, cl = [dev(x.points) for x in edges], [dev(x.clustering) for x in edges]
    out = torch.empty(n * n * 2, dtype=torch.float64, device="cuda")
    p = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_double))   # noqa: E731

    def tfi():
        _capi.check(L.tm_dev_tfi_block(p(out), n, n, p(pts[0]), p(pts[1]), p(pts[2]), p(pts[3]), p(cl[0]), p(cl[1]), p(cl[2]), p(cl[3]), None))

    mesh = configs.single_block(n, n, perturb=0.25)
    with smooth.Smoother(mesh, solver.Option.hip(inner=solver.Inner.relax), wcf.Algorithm.thomas_middlecoff()) as sm:
        for _ in range(3):   # warm both code objects
            tfi()
            sm.update_control_function()
        t_tfi, t_tm = [], []
        for _ in range(args.repeats):
            t_tfi.append(timed(tfi))
            t_tm.append(timed(sm.update_control_function))
        pq = sm.control_function()
    gbs = lambda ms: 16.0 * n * n / (1e-3 * ms) / 1e9   # noqa: E731
    lines = [f"Thomas-Middlecoff evaluation (k_tm_edges + k_tm_blend) beside K1 (TFI) on a {n}^2 block, ms per call, event pairs, {args.repeats} repeats "
             "interleaved after a warm-up (tools/control_field_timing.py)",
             f"  K1 TFI (tm_dev_tfi_block)                      {spread(t_tfi)}   {gbs(np.median(t_tfi)):8.1f} GB/s of 16 B/node written",
             f"  field (tm_smoother_update_control_function)    {spread(t_tm)}   {gbs(np.median(t_tm)):8.1f} GB/s of 16 B/node written",
             f"  field / TFI (medians) {np.median(t_tm) / np.median(t_tfi):.2f}   (aim: parity, up to 1.5 x allowed); max |P| {np.abs(pq[:, 0]).max():.3e} max |Q| {np.abs(pq[:, 1]).max():.3e}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
