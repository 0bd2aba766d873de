"""The layer between the field primitives and the whole kernels, on the device: the point formulas of csrc/jacobian.hpp, msm.hpp and
mulfast_k256.hpp, the masked additions of the constant-time kernels and the RFC 6979 nonce generator, built for gfx950 with the
product's flags (tests/devtwin: devtwin_group.hip in the throughput and the ECGPU_K256_BRANCHFREE configuration, devtwin_rfc6979.hip)
and run one pair of operands per lane.

The vectors (tests/group_edge_vectors.py) put every exceptional branch of every formula - accumulator at infinity, the same point,
opposite points, each with denominators 1, 2, p - 1 and random, infinity given as raw p on secp256k1, coordinates given as t + p,
values of H that pass the top-word prefilter of is_zero_fast and are not zero - into three lane layouts: whole waves of one class,
neighbouring lanes of different classes, and a single exceptional lane at 0, 31, 32 or 63 of an ordinary wave.
tests/test_hosttwin_group_edges.py shows on the CPU, by the ECGPU_EXC_NOTE counters, that each class enters the branch it names.

- every result equals oracle.ecmodel.affine_add / affine_neg on Python integers, infinity exactly where the model says, Z3 = Z1 zr
- every output word equals the host twin's (raw secp256k1 words are bit-identical by the contract of test_gpu_field_primitives.py,
  Montgomery outputs are canonical); Montgomery outputs are below the modulus
- a row gives the same words in all three layouts
- rfc6979::generate_k with q = 2^255 + 0x1D / 2^383 + 0x1D: k and the rejection count equal tests/rfc6979_model.py and the host twin
  on every lane of streams in which one wave holds lanes with 0, 1, 2 and >= 3 rejections; zero rejections on the real orders"""
import random

import numpy as np
import pytest

import devtwin_util as D
import group_edge_vectors as V
from hosttwin_util import buf, lib as hostlib, outbuf
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu

# the branch-free build: the secp256k1 ops and every masked form (the configuration ops_k256_ct.hip ships them in)
CASES = [("group", cn, op) for cn in M.CURVES for op in V.ops_of(cn)]
CASES += [("group_bf", cn, op) for cn in M.CURVES for op in V.ops_of(cn) if cn == "k256" or op in V.MASKED]
_HOST = {}


def host_rows(cn, op):
    if (cn, op) not in _HOST:
        _HOST[cn, op] = V.run(D.host_pt_op(), M.CURVES[cn], op, V.rows(cn, op))
    return _HOST[cn, op]


@pytest.mark.parametrize("build,cn,op", CASES)
def test_formula_on_device(build, cn, op):
    c = M.CURVES[cn]
    rs = V.rows(cn, op)
    host = host_rows(cn, op)
    fn = D.device_pt_op(build)
    seen = {}
    for name, order in V.layouts(rs).items():
        out = V.run(fn, c, op, [rs[i] for i in order])
        bad = np.nonzero((out != host[order]).any(axis=1))[0]               # word for word the host twin's, in every layout
        if bad.size:
            i = order[bad[0]]
            raise AssertionError((build, cn, op, name, "lane %d" % bad[0], rs[i].cls, V.check(c, op, rs[i], out[bad[0]]),
                                  out[bad[0]].tolist(), host[i].tolist()))
        for lane, i in enumerate(order):
            if i not in seen:                                               # equal words: one check against the integers per row
                seen[i] = True
                err = V.check(c, op, rs[i], out[lane])
                assert err is None, (build, cn, op, name, lane, rs[i].cls, err, [hex(x) for x in rs[i].p], [hex(x) for x in rs[i].q], rs[i].aux)
    assert len(seen) == len(rs)


@pytest.mark.parametrize("build", ["group", "group_bf"])
def test_k256_jac_add_mixed_with_and_without_zr(build):
    """the form the kernels call (zr = nullptr; exact and equal to the host twin by test_formula_on_device) against the form with the
    ratio, lane by lane in the interleaved layout: the same X, Y, Z words, except where the accumulator is doubled with a denominator
    that is not one (two triples of one point: see tests/test_hosttwin_group_edges.py)"""
    c = M.CURVES["k256"]
    rs = V.rows("k256", "k_jac_add_mixed")
    order = V.layouts(rs)["interleaved"]
    part = [rs[i] for i in order]
    with_zr = V.run(D.device_pt_op(build), c, "k_jac_add_mixed", part)
    without = V.run(D.device_pt_op(build), c, "k_jac_add_mixed_nozr", part)
    doubled = np.array([r.branch == "same" and not r.z1 for r in part])
    minus_one = np.array([r.p[2] % c.p == c.p - 1 for r in part])             # (x, -y, -1) doubles to the triple that (x, y, 1) doubles to
    same_words = (with_zr[:, :24] == without[:, :24]).all(axis=1)
    judged = ~(doubled & minus_one)
    assert (doubled & judged).sum() >= 30 and (same_words == ~doubled)[judged].all(), np.nonzero((same_words == doubled) & judged)[0][:8].tolist()
    assert not without[:, 32:40].any()


# ---- RFC 6979: the rejection loop ---------------------------------------------------------------------------------------------
def host_generate_k(hid, q, ins):
    nb = 32 if hid == 0 else 48
    out = outbuf(nb)
    res = []
    for x, h1, extra in ins:
        rej = hostlib().ht_rfc6979_generate_k(hid, buf(x), buf(h1), buf(extra) if extra else None, buf(q.to_bytes(nb, "big")), out)
        res.append((int.from_bytes(bytes(out), "big"), rej))
    return res


@pytest.mark.parametrize("name", sorted(V.RFC_STREAMS))
def test_rfc6979_rejection_loop(name):
    hid, q, ins, want = V.rfc6979_stream(name)
    assert V.wave_mixes_rounds([r for _, r in want]) and max(r for _, r in want) >= 3
    ks, rej = D.rfc6979_generate_k(hid, [x for x, _, _ in ins], [h for _, h, _ in ins], [e for _, _, e in ins], q)
    got = list(zip(ks, rej))
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (name, len(bad), bad[0], got[bad[0]], want[bad[0]])
    assert got == host_generate_k(hid, q, ins)


@pytest.mark.parametrize("cn", sorted(M.CURVES))
def test_rfc6979_real_orders_reject_nothing(cn):
    import rfc6979_model as R
    c = M.CURVES[cn]
    hid = 1 if cn == "p384" else 0
    rng = random.Random("rfc6979/" + cn)
    ins = [(rng.randrange(1, c.n).to_bytes(c.nbytes, "big"), rng.randrange(c.n).to_bytes(c.nbytes, "big"), rng.randbytes(c.nbytes) if i % 3 == 2 else b"")
           for i in range(320)]
    want = [R.generate_k(c.n, R.CURVE_HASH[cn], x, h1, extra) for x, h1, extra in ins]
    ks, rej = D.rfc6979_generate_k(hid, [x for x, _, _ in ins], [h for _, h, _ in ins], [e for _, _, e in ins], c.n)
    assert list(zip(ks, rej)) == want
    assert not any(rej)
    assert list(zip(ks, rej)) == host_generate_k(hid, c.n, ins)
