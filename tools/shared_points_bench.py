#!/usr/bin/env python3
"""Shared points (ECGPU_SHARED_POINTS) against the per-element calls: what the defaults of the size rule rest on.

    python tools/shared_points_bench.py [--parent-lib lib_exp/libecgpu_parent.so] [--out profiles/shared_points.txt] [--reps 7] [--max-log2 22]

Device-resident and warmed; the two sides of every comparison alternate in ONE process, `reps` times each, and every figure is the
median with its range, so a difference can be read against the spread.  The baseline side - the same call with the point replicated n
times, without the flag - runs on `--parent-lib` (a build of the parent commit: `ECGPU_LIB`-style second library in the same
process) where given, otherwise on the tree's own library, and the report says which.  Needs a GPU: there is no fallback.

Sections: table builds (a call that misses against the same call hitting), one point at n = 2^10 .. 2^max by the rule and pinned,
two-term combinations, verification under one key."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rustcrypto-elliptic-curves_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ecgpu  # noqa: E402
from oracle import ecmodel as M  # noqa: E402
from oracle import synth  # noqa: E402


class OtherContext(ecgpu.Context):
    """a context of another build of the library, loaded beside the tree's own"""

    def __init__(self, path, device=0):
        self.lib = ecgpu.load_library(path)
        self.handle = ctypes.c_void_p()
        rc = self.lib.ecgpu_create(ctypes.byref(self.handle), device)
        if rc != 0:
            raise ecgpu.EcgpuError("ecgpu_create on %s failed with %d" % (path, rc))
        self.device, self._pinned = device, []


def fmt(ts):
    return "%8.3f ms (%.3f .. %.3f)" % (statistics.median(ts), min(ts), max(ts))


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def alternate(sides, reps):
    """sides: [(label, ctx, fn)] -> {label: [ms]}; one warm-up each, then reps rounds in which the sides take turns"""
    for _, ctx, fn in sides:
        fn()
        ctx.synchronize()
    out = {label: [] for label, _, _ in sides}
    for _ in range(reps):
        for label, ctx, fn in sides:
            out[label].append(timed(ctx, fn))
    return out


def point_rows(c, pts):
    return np.frombuffer(b"".join(M.i2b(c, x) + M.i2b(c, y) for x, y in pts), dtype=np.uint8).reshape(len(pts), 2 * c.nbytes).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_points.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-log2", type=int, default=22)
    ap.add_argument("--curves", default="k256,p256,p384")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shared_points_bench: no GPU - nothing is measured without one")
    ctx = ecgpu.Context(0)
    base_ctx = OtherContext(a.parent_lib) if a.parent_lib else ctx
    base_name = "parent commit's library" if a.parent_lib else "this tree's library, replicated points, no flag"
    S, D = ecgpu.SHARED_POINTS, ecgpu.DEVICE
    lines = ["shared points against per-element points: %s; baseline = %s; %d alternating repetitions, median (min .. max)"
             % (torch.cuda.get_device_name(0), base_name, a.reps), ""]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for cn in a.curves.split(","):
        c, cv, bcv = M.CURVES[cn], ctx.curve(cn), base_ctx.curve(cn)
        nb = c.nbytes
        nmax = 1 << a.max_log2
        pts = synth.points(c, 64, start=500)
        d_sc = torch.empty((2 * nmax, nb), dtype=torch.uint8, device="cuda")
        cv.synth_scalars_device(d_sc, 2 * nmax, seed=11)
        d_out = torch.empty((nmax, 2 * nb), dtype=torch.uint8, device="cuda")
        d_out2 = torch.empty((nmax, 2 * nb), dtype=torch.uint8, device="cuda")
        d_inf = torch.empty((nmax,), dtype=torch.uint8, device="cuda")
        h = point_rows(c, pts[:1])
        d_rep = torch.from_numpy(np.tile(h, (nmax, 1))).cuda()
        h2 = point_rows(c, pts[1:3])
        d_rep2 = torch.from_numpy(np.tile(h2, (nmax // 2, 1))).cuda()

        emit("== %s: table builds (host clock around a 64-element call that misses, against the same call hitting) ==" % cn)
        ctx.set_option(ecgpu.OPT_SHARED_MIN, 1)
        fresh = 3
        for wb in (8, 16, 20):
            ctx.set_option(ecgpu.OPT_SHARED_WINDOW, wb)
            miss, hit = [], []
            for r in range(3):
                p = point_rows(c, pts[fresh:fresh + 1])
                fresh += 1
                for dest in (miss, hit):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    cv.mul_device(d_sc, p, d_out, 64, d_out_inf=d_inf, flags=S)
                    ctx.synchronize()
                    dest.append((time.perf_counter() - t0) * 1e3)
            emit("  %2d-bit windows: miss %s   hit %s" % (wb, fmt(miss), fmt(hit)))
        ctx.set_option(ecgpu.OPT_SHARED_WINDOW, 0)

        emit("== %s: one point, n results: replicated (baseline) | by the rule after a hit | pinned 8 | 16 | 20 ==" % cn)
        for lg in range(10, a.max_log2 + 1, 2):
            n = 1 << lg
            sides = [("base", base_ctx, lambda: bcv.mul_device(d_sc, d_rep, d_out2, n, d_out_inf=d_inf))]
            for label, wb in (("rule", 0), ("w8", 8), ("w16", 16), ("w20", 20)):
                def run(wb=wb):
                    ctx.set_option(ecgpu.OPT_SHARED_WINDOW, wb)
                    cv.mul_device(d_sc, h, d_out, n, d_out_inf=d_inf, flags=S)
                sides.append((label, ctx, run))
            t = alternate(sides, a.reps)
            assert torch.equal(d_out[:n], d_out2[:n]), "the two sides differ"
            emit("  2^%-2d  base %s | rule %s | w8 %s | w16 %s | w20 %s" % (lg, fmt(t["base"]), fmt(t["rule"]), fmt(t["w8"]), fmt(t["w16"]), fmt(t["w20"])))
        ctx.set_option(ecgpu.OPT_SHARED_WINDOW, 0)

        emit("== %s: two terms, n combinations: replicated (baseline) | shared, by the rule ==" % cn)
        for lg in (12, 16, 20):
            n = 1 << min(lg, a.max_log2 - 1)
            base = lambda: base_ctx.curve(cn)._call("ecgpu_lincomb_batch", d_sc, d_rep2, ecgpu.AFFINE, 2, d_out2, ecgpu.AFFINE, d_inf, n, D, 0)
            mine = lambda: cv._call("ecgpu_lincomb_batch", d_sc, h2, ecgpu.AFFINE, 2, d_out, ecgpu.AFFINE, d_inf, n, D, S)
            t = alternate([("base", base_ctx, base), ("mine", ctx, mine)], a.reps)
            assert torch.equal(d_out[:n], d_out2[:n]), "the two sides differ"
            emit("  2^%-2d  base %s | shared %s" % (lg, fmt(t["base"]), fmt(t["mine"])))

        emit("== %s: verification under one key, n signatures: per-element keys (baseline) | shared key ==" % cn)
        d = 0x1234567 % c.n
        q = M.affine_mul(c, d, (c.gx, c.gy))
        key = point_rows(c, [q])
        for lg in (12, 16, 20):
            n = 1 << min(lg, a.max_log2)
            dz = d_sc[:n]
            d_sig = torch.empty((n, 2 * nb), dtype=torch.uint8, device="cuda")
            d_rec = torch.empty((n,), dtype=torch.uint8, device="cuda")
            d_ok = torch.empty((n,), dtype=torch.uint8, device="cuda")
            d_ok2 = torch.empty((n,), dtype=torch.uint8, device="cuda")
            d_key = torch.from_numpy(np.tile(key, (n, 1))).cuda()
            d_d = torch.from_numpy(np.tile(np.frombuffer(M.i2b(c, d), dtype=np.uint8), (n, 1))).cuda()
            cv.ecdsa_sign_prehash_device(d_d, dz, None, d_sig, d_rec, d_ok, n, flags=0)
            base = lambda: bcv.ecdsa_verify_device(dz, d_sig, d_key, d_ok2, n, flags=0)
            mine = lambda: cv.ecdsa_verify_device(dz, d_sig, key, d_ok, n, flags=S)
            t = alternate([("base", base_ctx, base), ("mine", ctx, mine)], a.reps)
            assert torch.equal(d_ok, d_ok2) and bool(d_ok.all()), "the two sides differ"
            emit("  2^%-2d  base %s | shared %s" % (lg, fmt(t["base"]), fmt(t["mine"])))
        ctx.set_option(ecgpu.OPT_SHARED_MIN, 0)
        emit()
        del d_sc, d_out, d_out2, d_inf, d_rep, d_rep2
        torch.cuda.empty_cache()

    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()
    if base_ctx is not ctx:
        base_ctx.close()


if __name__ == "__main__":
    main()
