#!/usr/bin/env python3
"""Timings of deterministic signing, device-resident, 2^20 signatures per call (profiles/deterministic_signing.txt):

    python tools/signing_bench.py [log2 of the batch] [repeats]

Per curve: the RFC 6979 nonce kernel alone, ecgpu_ecdsa_sign_prehash_batch against ecgpu_ecdsa_sign_batch with caller-supplied
nonces; for secp256k1 ecgpu_schnorr_sign_prehash_batch against two constant-time generator multiplications.  The calls of a
comparison alternate within every repeat; the figure is the median of the repeats after one warm-up round, timed with the
context's events (ecgpu_timer_start / stop)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rustcrypto-elliptic-curves_amd"))


def main():
    import torch
    import ecgpu
    n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 20)
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    ctx = ecgpu.Context(0)
    print("batch %d, %d repeats, median ms (min .. max)" % (n, reps))
    for name in ("k256", "p256", "p384"):
        cv = ctx.curve(name)
        nb = cv.nb
        buf = lambda w: torch.zeros((n, w), dtype=torch.uint8, device="cuda")
        d, z, x, k, sig, rec, ok, pt = buf(nb), buf(nb), buf(nb), buf(nb), buf(2 * nb), buf(1), buf(1), buf(2 * nb)
        cv.synth_scalars_device(d, n, 11)
        cv.synth_scalars_device(z, n, 12)
        cv.synth_scalars_device(x, n, 13)
        torch.cuda.synchronize()
        calls = {
            "rfc6979 nonce kernel": lambda: cv.rfc6979_nonce_device(d, z, None, k, n),
            "rfc6979 nonce kernel, additional data": lambda: cv.rfc6979_nonce_device(d, z, x, k, n),
            "ecdsa_sign (caller's nonces)": lambda: cv.ecdsa_sign_device(d, k, z, sig, rec, ok, n),
            "ecdsa_sign_prehash": lambda: cv.ecdsa_sign_prehash_device(d, z, None, sig, rec, ok, n),
        }
        if name == "k256":
            calls["two mul_gen_ct launches"] = lambda: (cv.mul_device(d, None, pt, n, flags=ecgpu.SECRET_SCALARS), cv.mul_device(k, None, pt, n, flags=ecgpu.SECRET_SCALARS))
            calls["schnorr_sign_prehash"] = lambda: cv.schnorr_sign_prehash_device(d, z, x, sig, k, ok, n)
        times = {c: [] for c in calls}
        for r in range(reps + 1):
            for c, fn in calls.items():
                ctx.timer_start()
                fn()
                ms = ctx.timer_stop()
                if r:
                    times[c].append(ms)
        for c, t in times.items():
            print("%-5s %-40s %8.3f  (%.3f .. %.3f)" % (name, c, statistics.median(t), min(t), max(t)))
        base, full = statistics.median(times["ecdsa_sign (caller's nonces)"]), statistics.median(times["ecdsa_sign_prehash"])
        print("%-5s sign_prehash / sign = %.3f; %.1f x 10^6 signatures/s" % (name, full / base, n / full / 1e3))
        if name == "k256":
            print("k256  schnorr_sign_prehash / two mul_gen_ct = %.3f" % (statistics.median(times["schnorr_sign_prehash"]) / statistics.median(times["two mul_gen_ct launches"])))
    ctx.close()


if __name__ == "__main__":
    main()
