#!/usr/bin/env python3
"""Timings of the message-level calls, device-resident, 2^20 messages per call (profiles/message_signing.txt):

    python tools/digest_bench.py [log2 of the batch] [rounds] [digest|calls|all|keccak]

digest: ecgpu_digest_batch on SHA-256 and SHA-384 for messages of 32, 200, 1024 and 4096 bytes in records of the length rounded up
to 16, each shape twice: the records aligned (whole blocks read by words, csrc/sha2.hpp update_aligned) and the same buffer
entered one byte into its allocation (every byte through `update`, the only path there was before the word path).
calls: ecgpu_ecdsa_sign_msg_batch and ecgpu_ecdsa_verify_msg_batch on 32- and 200-byte messages against the prehash calls on
digests computed beforehand, per curve.
keccak (profiles/keccak_digest.txt): ecgpu_digest_batch on Keccak-256, SHA3-256 and SHA3-384 next to SHA-256 for messages of 32, 64
and 1024 bytes, aligned and one byte in as above; then ecgpu_ecdsa_recover_digest_batch and ecgpu_ecdsa_sign_digest_batch with
Keccak-256 on secp256k1 against ecgpu_ecdsa_recover_batch and ecgpu_ecdsa_sign_prehash_batch on the same digests.
The calls of a comparison alternate within every round; the figure is the median of the rounds after one warm-up round, timed
with the context's events (ecgpu_timer_start / stop)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rustcrypto-elliptic-curves_amd"))

LENGTHS = (32, 200, 1024, 4096)
HASHES = ((0, "sha256", 64, 9), (1, "sha384", 128, 17))          # id, name, block bytes, padding bytes at least
SPONGES = ((16, "keccak256", 136, 1), (17, "sha3_256", 136, 1), (18, "sha3_384", 104, 1))
KECCAK_LENGTHS = (32, 64, 1024)


def run_rounds(ctx, calls, rounds):
    times = {c: [] for c in calls}
    for r in range(rounds + 1):
        for c, fn in calls.items():
            ctx.timer_start()
            fn()
            ms = ctx.timer_stop()
            if r:
                times[c].append(ms)
    return times


def bench_digest(ctx, n, rounds, hashes=HASHES, lengths=LENGTHS):
    import torch
    import ecgpu
    print("== ecgpu_digest_batch: batch %d, %d rounds, median ms [min .. max]; 10^6 messages/s, 10^6 compressions/s, GB/s of message bytes" % (n, rounds))
    for length in lengths:
        stride = (length + 15) // 16 * 16
        big = torch.randint(0, 256, (n * stride + 16,), dtype=torch.uint8, device="cuda")
        out = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert big.data_ptr() % 16 == 0
        views = {"aligned (words)": big[:n * stride], "1 byte in (bytes)": big[1:1 + n * stride]}
        lens = torch.full((n,), length, dtype=torch.int32, device="cuda")         # the ragged form: 200 bytes lie in records of 208
        torch.cuda.synchronize()
        calls = {}
        for h, hname, _, _ in hashes:
            for vname, v in views.items():
                calls[(hname, vname)] = (lambda h=h, v=v: ecgpu.digest_device(ctx, h, v, stride, lens, out, n))
        times = run_rounds(ctx, calls, rounds)
        for h, hname, bb, pad in hashes:
            blocks = (length + pad + bb - 1) // bb
            med = {}
            for vname in views:
                t = times[(hname, vname)]
                med[vname] = statistics.median(t)
                print("%-9s %5d B  %-18s %9.3f [%9.3f .. %9.3f]  %9.1f Mmsg/s %9.1f Mcompr/s %8.2f GB/s" %
                      (hname, length, vname, med[vname], min(t), max(t), n / med[vname] / 1e3, n * blocks / med[vname] / 1e3, n * length / med[vname] / 1e6))
            a, b = times[(hname, "aligned (words)")], times[(hname, "1 byte in (bytes)")]
            print("%-9s %5d B  bytes / words = %.2f; gap of the medians %.3f ms, spread of the rounds %.3f ms (words) %.3f ms (bytes)" %
                  (hname, length, med["1 byte in (bytes)"] / med["aligned (words)"], med["1 byte in (bytes)"] - med["aligned (words)"], max(a) - min(a), max(b) - min(b)))
        del big, out, views, calls


def bench_calls(ctx, n, rounds):
    import torch
    import ecgpu
    print("== message-level calls against the prehash calls on precomputed digests: batch %d, %d rounds, median ms [min .. max]" % (n, rounds))
    for name in ("k256", "p256", "p384"):
        cv = ctx.curve(name)
        nb = cv.nb
        buf = lambda w: torch.zeros((n, w), dtype=torch.uint8, device="cuda")
        d, z, sig, rid, ok, pub = buf(nb), buf(nb), buf(2 * nb), buf(1), buf(1), buf(2 * nb)
        cv.synth_scalars_device(d, n, 11)
        cv.mul_device(d, None, pub, n, flags=ecgpu.SECRET_SCALARS)
        for length in (32, 200):
            stride = (length + 15) // 16 * 16
            msgs = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device="cuda")
            lens = torch.full((n,), length, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ecgpu.digest_device(ctx, ecgpu.CURVE_HASH[cv.id], msgs, stride, lens, z, n)
            cv.ecdsa_sign_msg_device(d, msgs, stride, lens, None, sig, rid, ok, n)          # valid signatures for the verifications
            ctx.synchronize()
            assert bool(ok.all())
            calls = {
                "digest alone": lambda: ecgpu.digest_device(ctx, ecgpu.CURVE_HASH[cv.id], msgs, stride, lens, z, n),
                "sign_prehash": lambda: cv.ecdsa_sign_prehash_device(d, z, None, sig, rid, ok, n),
                "sign_msg": lambda: cv.ecdsa_sign_msg_device(d, msgs, stride, lens, None, sig, rid, ok, n),
                "verify (prehash)": lambda: cv.ecdsa_verify_device(z, sig, pub, ok, n),
                "verify_msg": lambda: cv.ecdsa_verify_msg_device(msgs, stride, lens, sig, pub, ok, n),
            }
            times = run_rounds(ctx, calls, rounds)
            ctx.synchronize()
            assert bool(ok.all())
            med = {c: statistics.median(t) for c, t in times.items()}
            for c, t in times.items():
                print("%-5s %4d B  %-18s %9.3f [%9.3f .. %9.3f]" % (name, length, c, med[c], min(t), max(t)))
            print("%-5s %4d B  sign_msg - sign_prehash = %+.3f ms (%.2f %%); verify_msg - verify = %+.3f ms (%.2f %%)" %
                  (name, length, med["sign_msg"] - med["sign_prehash"], 100 * (med["sign_msg"] / med["sign_prehash"] - 1),
                   med["verify_msg"] - med["verify (prehash)"], 100 * (med["verify_msg"] / med["verify (prehash)"] - 1)))


def bench_keccak_calls(ctx, n, rounds):
    """recover_digest / sign_digest with Keccak-256 on secp256k1 against the prehash calls on the same digests"""
    import torch
    import ecgpu
    print("== Keccak-256 message-level calls on secp256k1 against the prehash calls on the same digests: batch %d, %d rounds, median ms [min .. max]" % (n, rounds))
    cv = ctx.curve("k256")
    buf = lambda w: torch.zeros((n, w), dtype=torch.uint8, device="cuda")
    d, z, sig, rid, ok, pub = buf(32), buf(32), buf(64), buf(1), buf(1), buf(64)
    cv.synth_scalars_device(d, n, 11)
    for length in (32, 64, 200):
        stride = (length + 15) // 16 * 16
        msgs = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device="cuda")
        lens = torch.full((n,), length, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ecgpu.digest_device(ctx, ecgpu.KECCAK256, msgs, stride, lens, z, n)
        cv.ecdsa_sign_digest_device(ecgpu.KECCAK256, d, msgs, stride, lens, None, sig, rid, ok, n)       # valid signatures for the recoveries
        ctx.synchronize()
        assert bool(ok.all())
        calls = {
            "digest alone": lambda: ecgpu.digest_device(ctx, ecgpu.KECCAK256, msgs, stride, lens, z, n),
            "sign_prehash": lambda: cv.ecdsa_sign_prehash_device(d, z, None, sig, rid, ok, n),
            "sign_digest": lambda: cv.ecdsa_sign_digest_device(ecgpu.KECCAK256, d, msgs, stride, lens, None, sig, rid, ok, n),
            "recover (prehash)": lambda: cv.ecdsa_recover_device(z, sig, rid, pub, ok, n),
            "recover_digest": lambda: cv.ecdsa_recover_digest_device(ecgpu.KECCAK256, msgs, stride, lens, sig, rid, pub, ok, n),
        }
        times = run_rounds(ctx, calls, rounds)
        ctx.synchronize()
        assert bool(ok.all())
        med = {c: statistics.median(t) for c, t in times.items()}
        for c, t in times.items():
            print("k256 %4d B  %-18s %9.3f [%9.3f .. %9.3f]" % (length, c, med[c], min(t), max(t)))
        print("k256 %4d B  sign_digest - sign_prehash = %+.3f ms (%.2f %%); recover_digest - recover = %+.3f ms (%.2f %%)" %
              (length, med["sign_digest"] - med["sign_prehash"], 100 * (med["sign_digest"] / med["sign_prehash"] - 1),
               med["recover_digest"] - med["recover (prehash)"], 100 * (med["recover_digest"] / med["recover (prehash)"] - 1)))


def main():
    import ecgpu
    n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 20)
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    what = sys.argv[3] if len(sys.argv) > 3 else "all"
    ctx = ecgpu.Context(0)
    if what in ("digest", "all"):
        bench_digest(ctx, n, rounds)
    if what in ("calls", "all"):
        bench_calls(ctx, n, rounds)
    if what == "keccak":
        bench_digest(ctx, n, rounds, HASHES[:1] + SPONGES, KECCAK_LENGTHS)
        bench_keccak_calls(ctx, n, rounds)
    ctx.close()


if __name__ == "__main__":
    main()
