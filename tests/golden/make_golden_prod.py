#!/usr/bin/env python3
"""Regenerate the PROD / BAND / BOR / BXOR fixtures:
tests/golden/reduce_prod_<kind>.npz (and .partN.npz), reduce_prod_int.npz and
tests/golden/manifest_prod.json.

    python tests/golden/make_golden_prod.py [reference-root]

Expected outputs come from the reference's OWN CPU reduction, reduce_kernel<T>
(source/compute.h:14-23), instantiated with this project's wrapper types
HiCCL::prodof<U>, bandof<U>, borof<U> and bxorof<U> (include/hiccl/ops.h) --
the types whose `T acc = 0` is the operator's identity and whose `+=` is the
operator.  As make_golden_ops.py does, the function is read out of the
reference header and piped to ROCm's clang++ on stdin; the shared object goes
to a temporary directory that is removed afterwards, so no reference text or
binary enters this repository.

Nothing is written unless the NumPy restatement (tests/prod_expected.py fold:
an in-order multiply in the kind's type; bf16 as widen, f32 multiply, round to
nearest even on the bits; integers with wrap-around) gives the same word on
every element, a NaN compared by NaN-ness -- tests/test_prod_cpu.py pins the
restatement to the stored outputs again, without the reference.

Files and cases (keys <case>/in, <case>/<op>, read by tests/conftest.py
load_golden, which joins <name>.npz and its <name>.partN.npz):
  reduce_prod_f32 / _f64 / _bf16 / _f16
      hostile_n<N>   product-hostile inputs (tests/hostile_prod.py),
                     (N, 17 * 241 + 5), shift = seed = N, N in 1, 2, 3, 8, 9, 17;
                     <case>/prod
  reduce_prod_int
      i32_n<N>, u64_n<N>   prod_expected.int_cases(kind, N, 17 * 61 + 5, seed=N);
                     <case>/prod, /band, /bor, /bxor
The every-pattern check (all 65,536 f16 / bf16 patterns times each of the 16
multipliers ops_expected.ADDENDS, the last a NaN) stores no words: 2 MiB per
kind do not compress under the size limit.  The manifest holds the sha256 of
the reference's output words, NaNs canonicalised (prod_expected.patterns_hash),
per kind; the tests recompute the words with prod_expected and check the hash.

Conditions asserted here, shares recorded in the manifest: only the classes
`one_nan` and `inf_times_zero` yield NaN, at most 1/8 of any case (2/17 by
construction); every `near_one` output is finite, normal and nonzero.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import hostile_prod as HP  # noqa: E402
import prod_expected as E  # noqa: E402
from make_golden_ops import CLANG, CTYPES, fragment  # noqa: E402

COUNT = 17 * 241 + 5
INT_COUNT = 17 * 61 + 5  # random words do not compress: a shorter case keeps the file small
NS = (1, 2, 3, 8, 9, 17)
MAX_BYTES = 1 << 20
PART_BYTES = 900 << 10  # uncompressed bytes per file: random mantissas do not compress
NAN_CAP = 1.0 / 8


def functions():
    """(op name, kind) of every instantiation."""
    return [(op, kind) for kind in CTYPES for op in E.ops_of(kind)]


def wrappers():
    out = ['static_assert(sizeof(HiCCL::prodof<HiCCL::bf16>) == 2 && sizeof(HiCCL::bxorof<uint64_t>) == 8, "storage");']
    for op, kind in functions():
        t = f"HiCCL::{op}of<{CTYPES[kind]}>"
        out.append(f'extern "C" void ref_{op}_{kind}(void *o, size_t c, void **in, int n) {{\n'
                   f"  HiCCL::reduce_kernel<{t}>(reinterpret_cast<{t} *>(o), c, reinterpret_cast<{t} **>(in), n); }}")
    return "\n".join(out) + "\n"


def build(ref_root, tmp):
    src = os.path.join(ref_root, "source", "compute.h")
    unit = ('#include <cstddef>\n#include <cstdint>\n#include "hiccl/ops.h"\nnamespace HiCCL {\n' + fragment(src) +
            "\n}\n" + wrappers())
    so = os.path.join(tmp, "libref_prod.so")
    subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-fPIC", "-shared",
                    "-I", os.path.join(ROOT, "include"), "-o", so, "-"], input=unit, text=True, check=True)
    lib = ctypes.CDLL(so)
    for op, kind in functions():
        f = getattr(lib, f"ref_{op}_{kind}")
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    return lib


def reference_fold(lib, kind, op, x):
    rows = [np.ascontiguousarray(r) for r in x]
    out = np.empty(x.shape[1], E.carrier(kind))
    tab = (ctypes.c_void_p * max(1, len(rows)))(*[r.ctypes.data for r in rows])
    getattr(lib, f"ref_{op}_{kind}")(out.ctypes.data, x.shape[1], tab, len(rows))
    return out


def pinned(lib, kind, x, what):
    """{op name: the reference's output}, after the restatement agreed."""
    outs = {}
    for op, code in E.ops_of(kind).items():
        ref = reference_fold(lib, kind, op, x)
        mine = E.fold(kind, code, x)
        if not E.bits_equal(kind, mine, ref):
            raise SystemExit(f"make_golden_prod: {what} {op}: the NumPy restatement differs from reduce_kernel<{op}of<"
                             f"{CTYPES[kind]}>>: {E.first_mismatch(kind, mine, ref)} -- nothing written")
        outs[op] = ref
    return outs


def check_hostile(kind, n, x, y):
    """The fixture conditions of one hostile case; returns its NaN share."""
    K = HP.KINDS[kind]
    cls = HP.class_of(COUNT, n)
    nan = E.is_nan(kind, y)
    allowed = np.isin(cls, [HP.CLASSES.index(c) for c in HP.NAN_CLASSES])
    assert not nan[~allowed].any(), f"{kind} n={n}: a NaN output outside {HP.NAN_CLASSES}"
    share = float(nan.mean())
    assert share <= NAN_CAP, f"{kind} n={n}: NaN share {share:.4f}"
    u = E.bits_of(kind, y[cls == HP.CLASSES.index("near_one")]).astype(np.uint64)
    e = (u >> np.uint64(K["mant"])) & np.uint64((1 << (K["bits"] - 1 - K["mant"])) - 1)
    assert ((e != 0) & (e != (1 << (K["bits"] - 1 - K["mant"])) - 1)).all(), \
        f"{kind} n={n}: a near_one output that is not finite, normal and nonzero"
    return share


def sha(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def split(name, cases):
    """[(file name, {key: array})]: cases in order, a new .partN file when the next case would not fit."""
    parts, size = [{}], 0
    for case, arrs in cases.items():
        nbytes = sum(a.nbytes for a in arrs.values())
        if parts[-1] and size + nbytes > PART_BYTES:
            parts.append({})
            size = 0
        for part, a in arrs.items():
            parts[-1][f"{case}/{part}"] = a
        size += nbytes
    return [(f"{name}.npz" if i == 0 else f"{name}.part{i + 1}.npz", arrs) for i, arrs in enumerate(parts)]


def main(argv):
    ref_root = argv[1] if len(argv) > 1 else "/root/reference"
    files, shares, hashes = [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref_root, tmp)
        for kind in E.FLOATS:
            cases, worst = {}, 0.0
            for n in NS:
                x = HP.hostile(kind, n, COUNT, shift=n, seed=n)
                y = pinned(lib, kind, x, f"{kind} hostile_n{n}")["prod"]
                worst = max(worst, check_hostile(kind, n, x, y))
                cases[f"hostile_n{n}"] = {"in": np.ascontiguousarray(x), "prod": y}
            for fname, arrs in split(f"reduce_prod_{kind}", cases):
                files.append((fname, arrs))
                shares[fname] = worst
        cases = {}
        for kind in E.INTS:
            for n in NS:
                x = E.int_cases(kind, n, INT_COUNT, seed=n)
                cases[f"{kind}_n{n}"] = dict({"in": np.ascontiguousarray(x)}, **pinned(lib, kind, x, f"{kind}_n{n}"))
        for fname, arrs in split("reduce_prod_int", cases):
            files.append((fname, arrs))
            shares[fname] = 0.0
        for kind in ("f16", "bf16"):
            assert E.is_nan(kind, E.ADDENDS[kind]).tolist() == [False] * 15 + [True]
            rows = []
            for a in range(16):
                rows.append(pinned(lib, kind, E.patterns_input(kind, a), f"{kind} patterns, multiplier {a}")["prod"])
            words = np.stack(rows)
            assert E.is_nan(kind, words[15]).all(), "the NaN multiplier's outputs are all NaN"
            hashes[kind] = {"sha256": E.patterns_hash(kind, words),
                            "nan_share": E.nan_share(kind, words[:15])}
        del lib
    stale = [f for f in os.listdir(HERE) if f.startswith("reduce_prod_") and f.endswith(".npz")]
    for f in stale:  # a set written again may take fewer files
        os.remove(os.path.join(HERE, f))
    info = {}
    for fname, arrs in files:
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_prod: {fname} would be {size} bytes (limit {MAX_BYTES})")
        info[fname] = {"cases": len({k.rsplit('/', 1)[0] for k in arrs}), "pinned_by": "reference", "sha256": sha(path),
                       "bytes": size, "nan_share_max": shares[fname]}
    manifest = {
        "files": info,
        "patterns": hashes,
        "generator": "tests/golden/make_golden_prod.py",
        "reference": "source/compute.h:14-23 reduce_kernel<T> with T = HiCCL::prodof<U> / bandof<U> / borof<U> / "
                     "bxorof<U> (include/hiccl/ops.h; clang++, built into a temporary directory); every output "
                     "equals tests/prod_expected.py fold (NaN by NaN-ness)",
        "inputs": "tests/hostile_prod.py hostile(kind, N, 4102, shift=N, seed=N); "
                  "prod_expected.int_cases(kind, N, 1042, seed=N); every 16-bit pattern times 16 multipliers",
        "nan_share": "nan_share_max: the largest NaN share of any expected output of the file (cap 1/8; only the "
                     "classes one_nan and inf_times_zero yield NaN).  patterns: sha256 of the reference's (16, 65536) "
                     "product words per kind, NaNs canonicalised, and the NaN share of the 15 non-NaN multipliers' rows",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_prod.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"files": info, "patterns": hashes}, indent=1))


if __name__ == "__main__":
    main(sys.argv)
