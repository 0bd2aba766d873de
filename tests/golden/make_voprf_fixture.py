#!/usr/bin/env python3
"""Scrape the VOPRF DeriveKeyPair vectors of the reference's hash_to_scalar tests into a JSON fixture.

    python tests/golden/make_voprf_fixture.py <path of the reference checkout>

Sources (relative to the reference checkout): {p256,p384}/src/arithmetic/hash2curve.rs, test `hash_to_scalar_voprf` (three
vectors per curve, from draft-irtf-cfrg-voprf appendix A).  Only DATA is extracted - dst, key_info, seed and the expected secret
key, each as hex - no reference source text is kept.  The message of a vector is seed || I2OSP(len(key_info), 2) || key_info ||
I2OSP(counter, 1) with the first counter (from 0) whose scalar is not zero.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

FIELD = re.compile(r'(dst|key_info|seed|sk_sm):\s*(?:&hex!\(\s*"([0-9A-Fa-f]+)"\s*\)|b"((?:[^"\\]|\\.)*)")', re.S)


def unescape(lit: str) -> bytes:
    """the bytes of a Rust byte-string literal (printable characters and \\xNN escapes are all these vectors use)"""
    out, i = bytearray(), 0
    while i < len(lit):
        if lit[i] == "\\":
            assert lit[i + 1] == "x", lit
            out.append(int(lit[i + 2:i + 4], 16))
            i += 4
        else:
            out.append(ord(lit[i]))
            i += 1
    return bytes(out)


def scrape(ref: str, curve: str):
    with open(os.path.join(ref, curve, "src", "arithmetic", "hash2curve.rs")) as f:
        text = f.read()
    text = text[text.index("fn hash_to_scalar_voprf"):]
    text = text[text.index("const TEST_VECTORS"):]
    text = text[:text.index("];")]
    vectors, cur = [], {}
    for name, hexlit, bytelit in FIELD.findall(text):
        cur[name] = hexlit.lower() if hexlit else unescape(bytelit).hex()
        if len(cur) == 4:
            vectors.append(cur)
            cur = {}
    assert len(vectors) == 3 and not cur, (curve, len(vectors))
    return vectors


def main():
    ref = sys.argv[1]
    out = {curve: scrape(ref, curve) for curve in ("p256", "p384")}
    with open(os.path.join(HERE, "voprf_hash_to_scalar.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
