#!/usr/bin/env python3
"""Regenerate the fp16 fixture: tests/golden/reduce_f16.npz (+ .part2.npz)
and tests/golden/manifest_f16.json.

    python tests/golden/make_golden_f16.py [reference-root]

Expected outputs come from the reference's OWN CPU reduction, reduce_kernel<T>
(source/compute.h:14-23), instantiated for the compiler's half type
(T = _Float16).  As oracle/build_ref.sh does, the function is read out of the
reference header (the lines between its first `#else` and the `#endif` after
it) and piped to ROCm's clang++ on stdin; the shared object goes to a
temporary directory that is removed afterwards, so no reference text or
binary enters this repository.  ROCm's __half does not compile on the host
through that fragment (it has no `+=`); _Float16 is the type `T acc = 0;
acc += x` works with.

The files are written only if NumPy's in-order float16 sum
(tests/hostile_f16.py native_sum) gives the same word on every element, a
NaN compared by NaN-ness -- tests/test_f16_cpu.py pins the restatement to the
stored outputs again, without the reference.

Cases (keys <case>/in (n, count) uint16 and <case>/out (count,) uint16, as
tests/conftest.py load_golden reads them):
  hostile_n<N>       hostile_f16.hostile(N, 17 * 241 + 5, shift=N, seed=N), N in 1, 2, 3, 8, 9, 17
  every_pattern      all 65,536 patterns as a single input
  tamed_n<N>[_near]  hostile_f16.tamed_bits(N, 17 * 241 + 5, seed=N), N in 2, 9, 17  (second file)
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
sys.path.insert(0, os.path.dirname(HERE))
import hostile_f16 as H  # noqa: E402

CLANG = os.environ.get("HICCL_CLANGXX", "/opt/rocm/llvm/bin/clang++")
COUNT = 17 * 241 + 5
MAX_BYTES = 1 << 20

WRAPPER = """
static_assert(sizeof(_Float16) == 2, "half storage");
extern "C" void ref_reduce_f16(uint16_t *o, size_t c, uint16_t **in, int n) {
  HiCCL::reduce_kernel<_Float16>(reinterpret_cast<_Float16 *>(o), c, reinterpret_cast<_Float16 **>(in), n); }
"""


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
        raise SystemExit(f"make_golden_f16: reduce_kernel not found in {src}")
    return text


def build(ref_root, tmp):
    src = os.path.join(ref_root, "source", "compute.h")
    unit = "#include <cstddef>\n#include <cstdint>\nnamespace HiCCL {\n" + fragment(src) + "\n}\n" + WRAPPER
    so = os.path.join(tmp, "libref_f16.so")
    subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-o", so, "-"],
                   input=unit, text=True, check=True)
    lib = ctypes.CDLL(so)
    lib.ref_reduce_f16.restype = None
    lib.ref_reduce_f16.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    return lib


def reference_sum(lib, x):
    rows = [np.ascontiguousarray(r) for r in x]
    out = np.empty(x.shape[1], np.uint16)
    tab = (ctypes.c_void_p * max(1, len(rows)))(*[r.ctypes.data for r in rows])
    lib.ref_reduce_f16(out.ctypes.data, x.shape[1], tab, len(rows))
    return out


def sha(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def main(argv):
    ref_root = argv[1] if len(argv) > 1 else "/root/reference"
    first, second = {}, {}
    for n in (1, 2, 3, 8, 9, 17):
        first[f"hostile_n{n}"] = H.hostile(n, COUNT, shift=n, seed=n)
    first["every_pattern"] = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)[None, :]
    for n in (2, 9, 17):
        second[f"tamed_n{n}"] = H.tamed_bits(n, COUNT, seed=n)
        second[f"tamed_n{n}_near"] = H.tamed_bits(n, COUNT, seed=n, near=True)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref_root, tmp)
        outs = {}
        for case, x in {**first, **second}.items():
            ref = reference_sum(lib, x)
            mine = H.native_sum(x)
            if not H.bits_equal(mine, ref):
                raise SystemExit(f"make_golden_f16: {case}: NumPy's float16 sum differs from reduce_kernel<_Float16>: "
                                 f"{H.first_mismatch(mine, ref)} -- nothing written")
            outs[case] = ref
            del ref
        del lib
    files = {}
    for fname, cases in (("reduce_f16.npz", first), ("reduce_f16.part2.npz", second)):
        arrs = {}
        for case, x in cases.items():
            arrs[f"{case}/in"] = np.ascontiguousarray(x)
            arrs[f"{case}/out"] = outs[case]
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_f16: {fname} would be {size} bytes (limit {MAX_BYTES})")
        files[fname] = {"cases": len(cases), "pinned_by": "reference", "sha256": sha(path), "bytes": size,
                        "nan_share_max": max(float(H.is_nan(outs[c]).mean()) for c in cases)}
    manifest = {
        "files": files,
        "generator": "tests/golden/make_golden_f16.py",
        "reference": "source/compute.h:14-23 reduce_kernel<T> with T = _Float16 (clang++, built into a temporary "
                     "directory); every output equals NumPy's in-order float16 sum (NaN by NaN-ness)",
        "inputs": "tests/hostile_f16.py: hostile(N, 4102, shift=N, seed=N); every 16-bit pattern; "
                  "tamed_bits(N, 4102, seed=N[, near=True])",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_f16.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(files, indent=1))


if __name__ == "__main__":
    main(sys.argv)
