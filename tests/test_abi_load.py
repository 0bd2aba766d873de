"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol that
include/ecgpu.h declares (no compute calls without a GPU), and the product has no CPU fallback.
The header is also the yardstick for the two hand-written mirrors of it - the prototype table of the Python binding and the
extern block of the Rust shim - and for the package's constants: names, arity and the class of type at every position."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import ecgpu


def declared_symbols():
    with open(os.path.join(ROOT, "include", "ecgpu.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ecgpu_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = ctypes.CDLL(ecgpu.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ecgpu.h but not exported"
    assert set(names) == set(ecgpu.EXPORTED_SYMBOLS)
    # and nothing else leaves the library (csrc/ecgpu.map): the boundary is the C ABI only
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", ecgpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == set(names)


def test_python_binding_declares_all_prototypes():
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    lib = ecgpu.load_library()
    assert lib.ecgpu_version().startswith(b"ecgpu")
    assert [lib.ecgpu_field_bytes(c) for c in (0, 1, 2, 9)] == [32, 32, 48, 0]


def test_load_library_applies_the_table():
    """every row of the prototype table is on the loaded library; the default library is cached, an explicit path is loaded afresh"""
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    lib = ecgpu.load_library()
    for name, (restype, argtypes) in ecgpu._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert ecgpu.load_library() is lib
    other = ecgpu.load_library(ecgpu.LIB_PATH)
    assert other is not lib and ecgpu.load_library() is lib
    assert other.ecgpu_field_bytes.restype is ctypes.c_size_t


# ---- the boundary against the header, without the library -----------------------------------------------------------------
# A parameter or return type is classed as: "ptr" (pointer to context or group, or a data pointer: void*, uint8_t*, uint32_t*,
# const or not), "pp" (pointer to pointer), "size_t*", "int*", "float*", "int64_t*", "char*", or one of the scalars "size_t",
# "int", "unsigned", "int64_t", "uint64_t"; "void" for a function that returns nothing.
_DATA = {"ecgpu_ctx", "ecgpu_group", "void", "uint8_t", "uint32_t"}
_TYPED_POINTEE = {"size_t", "int", "float", "int64_t", "char"}
_SCALARS = {"size_t", "int", "unsigned", "int64_t", "uint64_t"}


def _c_class(decl, is_return=False):
    """class of one C parameter declaration (type and name) or of a return type"""
    t = re.sub(r"\bconst\b", " ", decl)
    stars = t.count("*")
    words = t.replace("*", " ").split()
    if not is_return:
        words = words[:-1]                  # the parameter's name
    base = " ".join(words)
    if stars == 2 and base in _DATA:
        return "pp"
    if stars == 1 and base in _DATA:
        return "ptr"
    if stars == 1 and base in _TYPED_POINTEE:
        return base + "*"
    if stars == 0 and (base in _SCALARS or (is_return and base == "void")):
        return base
    raise AssertionError("include/ecgpu.h: cannot class %r" % decl)


def header_prototypes():
    """name -> (class of the return type, [class of each parameter]) for every prototype of include/ecgpu.h, in its order"""
    with open(os.path.join(ROOT, "include", "ecgpu.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ecgpu_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", text):
        params = m.group(3).strip()
        out[m.group(2)] = (_c_class(m.group(1), True), [] if params in ("", "void") else [_c_class(p) for p in params.split(",")])
    return out, text


def _ctypes_class(t):
    # on LP64 ctypes has one type object for size_t and uint64_t (c_ulong), and one for int64_t and long: the table cannot
    # tell them apart, so test_prototype_table_matches_header merges uint64_t into size_t on the header's side
    P = ctypes.POINTER
    return {None: "void", ctypes.c_void_p: "ptr", P(ctypes.c_void_p): "pp", P(ctypes.c_size_t): "size_t*", P(ctypes.c_int): "int*",
            P(ctypes.c_float): "float*", P(ctypes.c_int64): "int64_t*", ctypes.c_char_p: "char*", ctypes.c_size_t: "size_t", ctypes.c_int: "int",
            ctypes.c_uint: "unsigned", ctypes.c_int64: "int64_t"}[t]


def test_prototype_table_matches_header():
    """_PROTOTYPES has exactly the header's names, in the header's order, each with the header's arity and the same class of type at
    every position and for the return value"""
    header, _ = header_prototypes()
    assert len(header) == len(declared_symbols()) >= 80
    assert list(ecgpu._PROTOTYPES) == list(header)
    assert ecgpu.EXPORTED_SYMBOLS == tuple(header)

    def merged(c):
        return "size_t" if c == "uint64_t" and ctypes.c_size_t is ctypes.c_uint64 else c
    for name, (ret, params) in header.items():
        restype, argtypes = ecgpu._PROTOTYPES[name]
        assert _ctypes_class(restype) == merged(ret), name
        assert [_ctypes_class(a) for a in argtypes] == [merged(p) for p in params], name
    assert ecgpu._PROTOTYPES["ecgpu_version"][1] == ()


def _rust_class(t):
    t = " ".join(t.split())
    if re.fullmatch(r"\*(mut|const) \*(mut|const) (ecgpu_ctx|ecgpu_group|c_void|u8)", t):
        return "pp"
    m = re.fullmatch(r"\*(mut|const) (\w+)", t)
    if m:
        pointee = {"usize": "size_t*", "c_int": "int*", "f32": "float*", "i64": "int64_t*", "c_char": "char*",
                   "ecgpu_ctx": "ptr", "ecgpu_group": "ptr", "c_void": "ptr", "u8": "ptr", "u32": "ptr"}
        return pointee[m.group(2)]
    return {"usize": "size_t", "c_int": "int", "c_uint": "unsigned", "i64": "int64_t", "u64": "uint64_t"}[t]


def test_rust_extern_block_matches_header():
    """the hand-written extern block of rust/ecgpu-sys (no compiler here to check it) declares the header's functions with the
    header's arity and, per position, a type of the same class (usize, c_int, c_uint, u64, i64, raw pointers by pointee)"""
    header, _ = header_prototypes()
    with open(os.path.join(ROOT, "rustcrypto-elliptic-curves_amd", "rust", "ecgpu-sys", "src", "lib.rs")) as f:
        text = f.read()
    block = text[text.index('extern "C" {'):]
    block = re.sub(r"//[^\n]*", "", block[:block.index("\n}\n")])
    rust = {}
    for m in re.finditer(r"pub fn (ecgpu_[a-z0-9_]+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+?))?\s*;", block):
        params = [p.split(":", 1)[1] for p in m.group(2).split(",") if p.strip()]
        rust[m.group(1)] = ("void" if m.group(3) is None else _rust_class(m.group(3)), [_rust_class(p) for p in params])
    assert set(rust) == set(header), sorted(set(rust) ^ set(header))
    for name in header:
        assert rust[name] == header[name], name


# header enumerator -> the package's constant of the same meaning: the name without its ECGPU_ prefix, except for these
_RENAMED = {"ECGPU_PT_AFFINE": "AFFINE", "ECGPU_PT_PROJECTIVE": "PROJECTIVE", "ECGPU_MEM_HOST": "HOST", "ECGPU_MEM_DEVICE": "DEVICE"}
# the statuses have no constants of their own (Context.check raises EcgpuError with the number and the library's text)
_NOT_MIRRORED = {"ECGPU_OK", "ECGPU_ERR_ARG", "ECGPU_ERR_NO_DEVICE", "ECGPU_ERR_RUNTIME", "ECGPU_ERR_UNSUPPORTED"}


def test_constants_have_the_headers_values():
    _, text = header_prototypes()
    enumerators = dict((n, int(v)) for n, v in re.findall(r"\b(ECGPU_[A-Z0-9_]+)\s*=\s*(-?\d+)u?\b", text))
    for family, least in (("ECGPU_FE_", 7), ("ECGPU_SC_", 7), ("ECGPU_OPT_", 10), ("ECGPU_MEM_", 2), ("ECGPU_PT_", 2), ("ECGPU_H2C_", 2),
                          ("ECGPU_SHA", 4), ("ECGPU_BATCH_", 2)):
        assert sum(n.startswith(family) for n in enumerators) >= least, family
    for n in ("ECGPU_K256", "ECGPU_P256", "ECGPU_P384", "ECGPU_KECCAK256", "ECGPU_EXACT_REFERENCE", "ECGPU_ECDSA_LOW_S", "ECGPU_PUBLIC_SCALARS",
              "ECGPU_SECRET_SCALARS", "ECGPU_REDUCE_NONZERO", "ECGPU_GROUP_NO_RCCL"):
        assert n in enumerators, n
    options = 0
    for name, value in enumerators.items():
        if name in _NOT_MIRRORED:
            continue
        if name == "ECGPU_OPT_COUNT_":
            continue
        py = _RENAMED.get(name, name[len("ECGPU_"):])
        assert getattr(ecgpu, py) == value, (name, py)
        options += name.startswith("ECGPU_OPT_")
    mine = sorted(getattr(ecgpu, n) for n in dir(ecgpu) if n.startswith("OPT_"))
    assert enumerators["ECGPU_OPT_COUNT_"] == options == len(mine) and mine == list(range(options))
    assert ecgpu.CURVE_IDS == {"k256": enumerators["ECGPU_K256"], "p256": enumerators["ECGPU_P256"], "p384": enumerators["ECGPU_P384"]}


def test_no_cpu_fallback_without_gpu():
    """Without a gfx950 device the product must fail loudly, never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    with pytest.raises(ecgpu.EcgpuError):
        ecgpu.Context(0)


def test_product_does_not_reference_oracle():
    """oracle/ is test infrastructure: nothing under the package may import, link or open it."""
    pkg = os.path.join(ROOT, "rustcrypto-elliptic-curves_amd")
    for d, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hpp", ".hip", ".h", ".cpp", "Makefile")):
                with open(os.path.join(d, fn), errors="ignore") as f:
                    for ln in f:
                        code = ln.split("//")[0].split("#")[0] if not fn.endswith(".py") else ln.split("#")[0]
                        assert "oracle/" not in code and "import oracle" not in code and "from oracle" not in code, (fn, ln)


def _example_binary():
    import subprocess
    d = os.path.join(ROOT, "examples")
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "abi_example")


def test_c_caller_links_and_fails_loudly_without_gpu():
    """examples/abi_example.c is a plain-C caller of include/ecgpu.h (gcc, no HIP headers): it must compile and link
    against the library, and without a gfx950 device stop with the no-device status instead of computing anything."""
    import subprocess
    import torch
    exe = _example_binary()
    if torch.cuda.is_available():
        pytest.skip("a GPU is present (test_gpu_api.py runs the example)")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "no usable gfx950 device" in r.stderr


def test_host_chunk_schedule():
    """The chunking of host-buffer batches (csrc/host_pipe.hpp) is host logic and needs no device: sizes add up, grow from an eighth
    of a pass to a whole pass, end small (short drain), and leave no crumbs."""
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    P = 1 << 23
    assert ecgpu.host_chunk_schedule(1 << 24, P) == [1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 20]
    assert ecgpu.host_chunk_schedule(1 << 25, P) == [1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 23, 1 << 23, 1 << 20]
    assert ecgpu.host_chunk_schedule((1 << 21) + 12345, P) == [1 << 20, (1 << 20) + 12345]
    assert ecgpu.host_chunk_schedule((1 << 22) + (1 << 20) + 4321, P) == [1 << 20, 1 << 21, (1 << 20) + 4321, 1 << 20]
    import random
    rng = random.Random(5)
    for _ in range(300):
        n = rng.randrange(1, 1 << 27)
        pass_units = 1 << rng.randrange(18, 26)
        p = min(max(pass_units, 1 << 20), 1 << 23)
        s = ecgpu.host_chunk_schedule(n, pass_units)
        assert sum(s) == n and all(x > 0 for x in s)
        assert all(x <= p + p // 16 for x in s), (n, pass_units, s)              # a chunk is at most a pass (plus an absorbed crumb)
        if len(s) > 1:
            assert s[-1] <= max(p // 8, 0) + p // 16 or s[-1] < 2 * (p // 8), (n, pass_units, s)   # short drain
            assert all(x >= p // 16 for x in s), (n, pass_units, s)             # no crumbs


def test_shard_range_arithmetic():
    """ecgpu_shard_range (the index ranges a device group hands its members): balanced, contiguous, disjoint,
    covering - including n < parts and n = 0 - and the same as the Python launcher's parallel.shard_range for equal shares."""
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    import random
    rng = random.Random(11)
    cases = [(0, 1), (0, 8), (5, 8), (8, 8), (9, 8), ((1 << 26), 8), ((1 << 23) + 777, 2), ((1 << 22) + 12345, 2), (1, 64)]
    cases += [(rng.randrange(0, 1 << 40), rng.randrange(1, 65)) for _ in range(200)]
    for n, k in cases:
        nxt, sizes = 0, []
        for i in range(k):
            lo, cnt = ecgpu.shard_range(n, k, i)
            assert lo == nxt
            nxt = lo + cnt
            sizes.append(cnt)
        assert nxt == n and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    with pytest.raises(ValueError):
        ecgpu.shard_range(10, 0, 0)
    with pytest.raises(ValueError):
        ecgpu.shard_range(10, 4, 4)
    from ecgpu import parallel
    for world in (1, 2, 4, 8):
        for rank in range(world):
            lo, hi = parallel.shard_range((1 << 24) + 5, rank, world)
            assert (lo, hi - lo) == ecgpu.shard_range((1 << 24) + 5, world, rank)
