#!/usr/bin/env python3
"""Scrape the deterministic-signing vectors of the reference's ECDSA tests into a JSON fixture.

    python tests/golden/make_signing_fixture.py <path of the reference checkout>

Sources (relative to the reference checkout): p256/src/ecdsa.rs, tests `rfc6979` and `prehash_signer_signing_with_sha384`;
p384/src/ecdsa.rs, tests `rfc6979` and `prehash_signer_signing_with_sha256`.  Only DATA is extracted - the secret key, each
message, the hash that produced the prehash and the expected signature, as hex or names - no reference source text is kept.
`Signer::sign` hashes with the curve's own digest (SHA-256 for P-256, SHA-384 for P-384); the prehash tests name theirs.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

CURVE_HASH = {"p256": "sha256", "p384": "sha384"}
TESTS = {"p256": ("rfc6979", "prehash_signer_signing_with_sha384"), "p384": ("rfc6979", "prehash_signer_signing_with_sha256")}

KEY = re.compile(r'let x = hex!\(\s*"([0-9A-Fa-f]+)"\s*\)')
SIGN = re.compile(r'signer\.sign\(b"([^"]*)"\)')
DIGEST = re.compile(r'sha2::(Sha\d+)::digest\(b"([^"]*)"\)')
SIG = re.compile(r'&hex!\(\s*((?:"[0-9A-Fa-f\s]+"\s*)+)\)', re.S)


def test_body(text: str, name: str) -> str:
    body = text[text.index("fn %s()" % name):]
    return body[:body.index("\n    }\n")]


def scrape(ref: str, curve: str):
    with open(os.path.join(ref, curve, "src", "ecdsa.rs")) as f:
        text = f.read()
    key, vectors = None, []
    for name in TESTS[curve]:
        body = test_body(text, name)
        k = KEY.search(body).group(1).lower()
        assert key in (None, k), curve
        key = k
        sigs = ["".join(re.findall(r"[0-9A-Fa-f]+", s)).lower() for s in SIG.findall(body)]
        if name == "rfc6979":
            msgs = [(m, CURVE_HASH[curve]) for m in SIGN.findall(body)]
        else:
            msgs = [(m, h.lower()) for h, m in DIGEST.findall(body)]
        assert len(msgs) == len(sigs) and msgs, (curve, name)
        vectors += [{"test": name, "message": m.encode().hex(), "hash": h, "signature": s} for (m, h), s in zip(msgs, sigs)]
    assert len(vectors) == 3, (curve, len(vectors))
    return {"secret_key": key, "vectors": vectors}


def main():
    ref = sys.argv[1]
    out = {curve: scrape(ref, curve) for curve in ("p256", "p384")}
    with open(os.path.join(HERE, "rfc6979_sign.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
