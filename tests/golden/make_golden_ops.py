#!/usr/bin/env python3
"""Regenerate the MAX / MIN fixtures: tests/golden/reduce_ops_<kind>.npz,
reduce_ops_patterns.npz and tests/golden/manifest_ops.json.

    python tests/golden/make_golden_ops.py [reference-root]

Expected outputs come from the reference's OWN CPU reduction, reduce_kernel<T>
(source/compute.h:14-23), instantiated with this project's wrapper types
HiCCL::maxof<U> and HiCCL::minof<U> (include/hiccl/ops.h) -- the types whose
`T acc = 0` is the operator's identity and whose `+=` is the operator.  As
make_golden_f16.py does, the function is read out of the reference header
(the lines between its first `#else` and the `#endif` after it) and piped to
ROCm's clang++ on stdin; the shared object goes to a temporary directory that
is removed afterwards, so no reference text or binary enters this repository.

Nothing is written unless the NumPy restatement (tests/ops_expected.py fold:
explicit NaN and signed-zero handling on the bit patterns) gives the same
word on every element, a NaN compared by NaN-ness -- tests/test_ops_cpu.py
pins the restatement to the stored outputs again, without the reference.

Files and cases (keys <case>/in, <case>/max, <case>/min, read by
tests/conftest.py load_golden):
  reduce_ops_f32 / _f64 / _bf16 / _f16 .npz
      hostile_n<N>   hostile inputs (tests/hostile.py, tests/hostile_f16.py)
                     (N, 17 * 241 + 5), shift = seed = N, N in 1, 2, 3, 8, 9, 17
  reduce_ops_int.npz
      i32_n<N>, u64_n<N>   ops_expected.int_cases(kind, N, 17 * 61 + 5, seed=N)
  reduce_ops_patterns.npz
      f16, bf16      <case>/addends (16,), and <case>/max_sel, <case>/min_sel
                     (16, 65536) uint8: every 16-bit pattern folded with each
                     addend (input 0 the patterns, input 1 the addend); the last
                     addend is a NaN and its rows are all NaN.  A maximum of two
                     values is one of them, so the reference's output is stored
                     as WHICH one (0 the pattern, 1 the addend, 2 a NaN;
                     ops_expected.pattern_selector checks that it is, and
                     patterns_expected turns it back into words): 2 MiB of
                     words per array do not compress under the size limit.

NaN share: only the `one_nan` class of the hostile inputs has a NaN input, so
at most 242 of a case's 4,102 expected outputs (1/17 of the columns) may be
NaN; the generator asserts at most 1/16 and the manifest records the share.
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
import hostile as H32  # noqa: E402
import hostile_f16 as H16  # noqa: E402
import ops_expected as E  # noqa: E402

CLANG = os.environ.get("HICCL_CLANGXX", "/opt/rocm/llvm/bin/clang++")
COUNT = 17 * 241 + 5
INT_COUNT = 17 * 61 + 5  # random words do not compress: a shorter case keeps the file small
NS = (1, 2, 3, 8, 9, 17)
MAX_BYTES = 1 << 20
NAN_CAP = 1.0 / 16

CTYPES = {"f32": "float", "f64": "double", "bf16": "HiCCL::bf16", "f16": "HiCCL::f16", "i32": "int32_t",
          "u64": "uint64_t"}


def wrappers():
    out = ['static_assert(sizeof(HiCCL::maxof<HiCCL::bf16>) == 2 && sizeof(HiCCL::minof<double>) == 8, "storage");']
    for kind, ct in CTYPES.items():
        for op in ("max", "min"):
            t = f"HiCCL::{op}of<{ct}>"
            out.append(f'extern "C" void ref_{op}_{kind}(void *o, size_t c, void **in, int n) {{\n'
                       f"  HiCCL::reduce_kernel<{t}>(reinterpret_cast<{t} *>(o), c, reinterpret_cast<{t} **>(in), n); }}")
    return "\n".join(out) + "\n"


def fragment(src):
    """The CPU branch of the reference header: after its first `#else`, up to the next `#endif`."""
    out, on = [], False
    for ln in open(src).read().splitlines():
        if ln.startswith("#else") and not on:
            on = True
            continue
        if ln.startswith("#endif") and on:
            break
        if on:
            out.append(ln)
    text = "\n".join(out)
    if "void reduce_kernel" not in text:
        raise SystemExit(f"make_golden_ops: reduce_kernel not found in {src}")
    return text


def build(ref_root, tmp):
    src = os.path.join(ref_root, "source", "compute.h")
    unit = ('#include <cstddef>\n#include <cstdint>\n#include "hiccl/ops.h"\nnamespace HiCCL {\n' + fragment(src) +
            "\n}\n" + wrappers())
    so = os.path.join(tmp, "libref_ops.so")
    subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-fPIC", "-shared",
                    "-I", os.path.join(ROOT, "include"), "-o", so, "-"], input=unit, text=True, check=True)
    lib = ctypes.CDLL(so)
    for kind in CTYPES:
        for op in ("max", "min"):
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


def hostile(kind, n):
    return H16.hostile(n, COUNT, shift=n, seed=n) if kind == "f16" else H32.hostile(kind, n, COUNT, shift=n, seed=n)


def pinned(lib, kind, x, what):
    """{op name: the reference's output}, after the restatement agreed."""
    outs = {}
    for op, code in E.OPS.items():
        ref = reference_fold(lib, kind, op, x)
        mine = E.fold(kind, code, x)
        if not E.bits_equal(kind, mine, ref):
            raise SystemExit(f"make_golden_ops: {what} {op}: the NumPy restatement differs from reduce_kernel<{op}of<"
                             f"{CTYPES[kind]}>>: {E.first_mismatch(kind, mine, ref)} -- nothing written")
        outs[op] = ref
    return outs


def sha(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def main(argv):
    ref_root = argv[1] if len(argv) > 1 else "/root/reference"
    files = {}  # file name -> {key: array}
    shares = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref_root, tmp)
        for kind in E.FLOATS:
            arrs, worst = {}, 0.0
            for n in NS:
                x = hostile(kind, n)
                cls = H32.class_of(COUNT, n)
                nan_in = E.is_nan(kind, x).any(axis=0)
                assert not nan_in[cls != H32.CLASSES.index("one_nan")].any(), "a NaN input outside the one_nan class"
                outs = pinned(lib, kind, x, f"{kind} hostile_n{n}")
                arrs[f"hostile_n{n}/in"] = np.ascontiguousarray(x)
                for op, y in outs.items():
                    s = E.nan_share(kind, y)
                    assert s <= NAN_CAP and E.is_nan(kind, y).sum() <= 242, f"{kind} n={n} {op}: NaN share {s:.4f}"
                    worst = max(worst, s)
                    arrs[f"hostile_n{n}/{op}"] = y
            files[f"reduce_ops_{kind}.npz"] = arrs
            shares[f"reduce_ops_{kind}.npz"] = worst
        arrs = {}
        for kind in E.INTS:
            for n in NS:
                x = E.int_cases(kind, n, INT_COUNT, seed=n)
                outs = pinned(lib, kind, x, f"{kind}_n{n}")
                arrs[f"{kind}_n{n}/in"] = np.ascontiguousarray(x)
                for op, y in outs.items():
                    arrs[f"{kind}_n{n}/{op}"] = y
        files["reduce_ops_int.npz"] = arrs
        shares["reduce_ops_int.npz"] = 0.0
        arrs, worst = {}, 0.0
        for kind in ("f16", "bf16"):
            adds = E.ADDENDS[kind]
            assert E.is_nan(kind, adds).tolist() == [False] * 15 + [True]
            arrs[f"{kind}/addends"] = adds
            res = {op: np.empty((16, 1 << 16), np.uint8) for op in E.OPS}
            for a, addend in enumerate(adds):
                x = np.stack([E.ALL_PATTERNS, np.full(1 << 16, addend, np.uint16)])
                outs = pinned(lib, kind, x, f"{kind} patterns, addend {a}")
                for op, y in outs.items():
                    s = E.nan_share(kind, y)
                    if a == 15:
                        assert s == 1.0, "the NaN addend's outputs are all NaN"
                    else:
                        assert s <= NAN_CAP
                        worst = max(worst, s)
                    res[op][a] = E.pattern_selector(kind, x, y)
            for op in E.OPS:
                arrs[f"{kind}/{op}_sel"] = res[op]
        files["reduce_ops_patterns.npz"] = arrs
        shares["reduce_ops_patterns.npz"] = worst
        del lib
    info = {}
    for fname, arrs in files.items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_ops: {fname} would be {size} bytes (limit {MAX_BYTES})")
        info[fname] = {"cases": len({k.rsplit('/', 1)[0] for k in arrs}), "pinned_by": "reference", "sha256": sha(path),
                       "bytes": size, "nan_share_max": shares[fname]}
    manifest = {
        "files": info,
        "generator": "tests/golden/make_golden_ops.py",
        "reference": "source/compute.h:14-23 reduce_kernel<T> with T = HiCCL::maxof<U> / HiCCL::minof<U> "
                     "(include/hiccl/ops.h; clang++, built into a temporary directory); every output equals "
                     "tests/ops_expected.py fold (NaN by NaN-ness)",
        "inputs": "tests/hostile.py / tests/hostile_f16.py hostile(N, 4102, shift=N, seed=N); "
                  "ops_expected.int_cases(kind, N, 1042, seed=N); every 16-bit pattern against 16 addends",
        "nan_share": "nan_share_max: the largest NaN share of any expected output of the file (cap 1/16; the "
                     "pattern rows of the NaN addend, all NaN by construction, are not counted)",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_ops.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(info, indent=1))


if __name__ == "__main__":
    main(sys.argv)
