#!/usr/bin/env python3
"""Regenerate the scaled-sum fixtures: tests/golden/reduce_scale_<kind>.npz
(and .partN.npz) and tests/golden/manifest_scale.json.

    python tests/golden/make_golden_scale.py [reference-root]

out[i] = finish(s[i], alpha) (include/hiccl_reduce.h, hiccl_reduce_scaled).
The sum s comes from the reference's OWN CPU reduction, reduce_kernel<T>
(source/compute.h:14-23), for T = float, double, HiCCL::bf16 and _Float16 (the
half add itself; HiCCL::f16 where the compiler has no _Float16).  As
make_golden_prod.py does, the function is read out of the reference header and
piped to ROCm's clang++ on stdin; the shared object goes to a temporary
directory that is removed afterwards, so no reference text or binary enters
this repository.  `finish` is this generator's own C++, compiled into the same
object: one multiply for double and float, and for the 2-byte types a float
product stored to a volatile float (rounded to f32) and then converted to T.
The f32 accumulator of HICCL_ACC_WIDE is not the reference's arithmetic: its
sum is the generator's own in-order float loop, finished the same way.

Nothing is written unless the NumPy restatement (tests/scale_expected.py)
gives the same word on every element, a NaN compared by NaN-ness --
tests/test_scale_cpu.py pins the restatement to the stored outputs again,
without the reference.

Files and cases (read by tests/conftest.py load_golden, which joins <name>.npz
and its <name>.partN.npz; an array's key is <case>/<part>):
  reduce_scale_f32 / _f64 / _bf16 / _f16
      hostile_n<N>/a<i>   the scaled sum under scale_expected.ALPHAS[i], N in
                          1, 2, 3, 8, 9, 17, count 17 * 241 + 5
      hostile_n<N>/w<i>   bf16 and f16: the same under HICCL_ACC_WIDE
The inputs are not stored: they are scale_expected.hostile(kind, N) -- the
existing hostile generators (tests/hostile.py, tests/hostile_f16.py) at shift =
seed = N -- and the manifest holds the sha256 of each input array.
The every-pattern check (all 65,536 bf16 / f16 patterns as a single input,
n = 1, times every alpha, both accumulators) stores no words either: the
manifest holds the sha256 of the generator's output words, NaNs canonicalised,
per kind and accumulator.

Conditions asserted here: for a finite nonzero alpha an output is NaN exactly
where the plain sum is; for alpha = 0 exactly where the sum is NaN or infinite.
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
import scale_expected as E  # noqa: E402
from make_golden_ops import CLANG, fragment  # noqa: E402

MAX_BYTES = 1 << 20
PART_BYTES = 700 << 10  # uncompressed bytes per file: random mantissas do not compress

# kind -> the sum's C++ type
CTYPES = {"f32": "float", "f64": "double", "bf16": "HiCCL::bf16", "f16": "half_t"}

OWN = r"""
#ifdef __FLT16_MANT_DIG__
typedef _Float16 half_t;
#else
typedef HiCCL::f16 half_t;
#endif
// finish(s, alpha): double and float one multiply; the 2-byte types an f32
// product ROUNDED TO F32 (the volatile store), then rounded to T
template <class T> static T finish(T s, double alpha) { return s * (T)alpha; }
template <class T> static T finish2(float s, double alpha) {
  volatile float p = s * (float)alpha;
  return (T)(float)p;
}
template <> HiCCL::bf16 finish<HiCCL::bf16>(HiCCL::bf16 s, double alpha) { return finish2<HiCCL::bf16>((float)s, alpha); }
template <> half_t finish<half_t>(half_t s, double alpha) { return finish2<half_t>((float)s, alpha); }

template <class T> static void scaled(void *o, size_t c, void **in, int n, double alpha) {
  T *out = reinterpret_cast<T *>(o);
  HiCCL::reduce_kernel<T>(out, c, reinterpret_cast<T **>(in), n);
  for (size_t i = 0; i < c; i++) out[i] = finish<T>(out[i], alpha);
}
// HICCL_ACC_WIDE: an in-order float accumulator from +0, finished once
template <class T> static void scaled_wide(void *o, size_t c, void **in, int n, double alpha) {
  T *out = reinterpret_cast<T *>(o);
  for (size_t i = 0; i < c; i++) {
    volatile float acc = 0.0f;
    for (int k = 0; k < n; k++) acc = acc + (float)reinterpret_cast<T **>(in)[k][i];
    out[i] = finish2<T>(acc, alpha);
  }
}
"""


def wrappers():
    out = [OWN]
    for kind, t in CTYPES.items():
        out.append(f'extern "C" void ref_scaled_{kind}(void *o, size_t c, void **in, int n, double a) '
                   f"{{ scaled<{t}>(o, c, in, n, a); }}")
        out.append(f'extern "C" void ref_sum_{kind}(void *o, size_t c, void **in, int n, double) {{\n'
                   f"  HiCCL::reduce_kernel<{t}>(reinterpret_cast<{t} *>(o), c, reinterpret_cast<{t} **>(in), n); }}")
        if kind in E.HALVES:
            out.append(f'extern "C" void ref_wide_{kind}(void *o, size_t c, void **in, int n, double a) '
                       f"{{ scaled_wide<{t}>(o, c, in, n, a); }}")
    return "\n".join(out) + "\n"


def build(ref_root, tmp):
    src = os.path.join(ref_root, "source", "compute.h")
    unit = ('#include <cstddef>\n#include <cstdint>\n#include "hiccl/elem_types.h"\nnamespace HiCCL {\n' + fragment(src) +
            "\n}\n" + wrappers())
    so = os.path.join(tmp, "libref_scale.so")
    # no contraction: an add must not fuse with the multiply that follows it, as in the library
    subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC",
                    "-shared", "-I", os.path.join(ROOT, "include"), "-o", so, "-"], input=unit, text=True, check=True)
    lib = ctypes.CDLL(so)
    for kind in CTYPES:
        for what in ("scaled", "sum") + (("wide",) if kind in E.HALVES else ()):
            f = getattr(lib, f"ref_{what}_{kind}")
            f.restype = None
            f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    return lib


def reference(lib, what, kind, x, alpha=1.0):
    rows = [np.ascontiguousarray(r) for r in x]
    out = np.empty(x.shape[1], E.carrier(kind))
    tab = (ctypes.c_void_p * max(1, len(rows)))(*[r.ctypes.data for r in rows])
    getattr(lib, f"ref_{what}_{kind}")(out.ctypes.data, x.shape[1], tab, len(rows), float(alpha))
    return out


def pinned(lib, kind, x, alpha, wide, what):
    """The generator's output, after the restatement agreed."""
    ref = reference(lib, "wide" if wide else "scaled", kind, x, alpha)
    mine = E.scaled(kind, x, alpha, wide)
    if not E.bits_equal(kind, mine, ref):
        raise SystemExit(f"make_golden_scale: {what}: the NumPy restatement differs from the generator's C++: "
                         f"{E.first_mismatch(kind, mine, ref)} -- nothing written")
    return ref


def check_nan(kind, y, acc, alpha, wide, what):
    """The NaN conditions; `acc`: the plain sum in the accumulator type."""
    acc = acc if kind in ("f32", "f64") or wide else E.widen(kind, acc)
    nan = E.is_nan(kind, y)
    if alpha == 0.0:
        assert np.array_equal(nan, ~np.isfinite(acc)), f"{what}: alpha 0 is NaN exactly where the sum is NaN or infinite"
    else:
        assert np.array_equal(nan, np.isnan(acc)), f"{what}: a NaN output where the plain sum has none (or the reverse)"


def sha(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def split(name, arrays):
    """[(file name, {key: array})]: arrays in order, a new .partN file when the next would not fit."""
    parts, size = [{}], 0
    for key, a in arrays.items():
        if parts[-1] and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += a.nbytes
    return [(f"{name}.npz" if i == 0 else f"{name}.part{i + 1}.npz", arrs) for i, arrs in enumerate(parts)]


def main(argv):
    ref_root = argv[1] if len(argv) > 1 else "/root/reference"
    files, inputs, hashes = [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref_root, tmp)
        for kind in E.KINDS:
            arrays = {}
            for n in E.NS:
                x = E.hostile(kind, n)
                inputs[f"{kind}/hostile_n{n}"] = E.array_hash(x)
                s = reference(lib, "sum", kind, x)
                assert E.bits_equal(kind, E.plain_sum(kind, x), s), f"{kind} n={n}: the restated plain sum"
                for wide in (False, True) if kind in E.HALVES else (False,):
                    acc = E.acc_sum(kind, x, wide) if wide else s
                    for i, (name, alpha) in enumerate(E.ALPHAS):
                        what = f"{kind} hostile_n{n} alpha {name}{' wide' if wide else ''}"
                        y = pinned(lib, kind, x, alpha, wide, what)
                        check_nan(kind, y, acc, alpha, wide, what)
                        arrays[f"hostile_n{n}/{'w' if wide else 'a'}{i}"] = y
            files += split(f"reduce_scale_{kind}", arrays)
        for kind in E.HALVES:
            x = E.ALL_PATTERNS[None, :]
            for wide in (False, True):
                rows = [pinned(lib, kind, x, a, wide, f"{kind} every pattern alpha {name}") for name, a in E.ALPHAS]
                hashes[f"{kind}{'_wide' if wide else ''}"] = E.words_hash(kind, np.stack(rows))
        del lib
    stale = [f for f in os.listdir(HERE) if f.startswith("reduce_scale_") and f.endswith(".npz")]
    for f in stale:  # a set written again may take fewer files
        os.remove(os.path.join(HERE, f))
    info = {}
    for fname, arrs in files:
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_scale: {fname} would be {size} bytes (limit {MAX_BYTES})")
        info[fname] = {"arrays": len(arrs), "pinned_by": "reference sum + generator finish", "sha256": sha(path),
                       "bytes": size}
    manifest = {
        "files": info,
        "inputs": inputs,
        "patterns": hashes,
        "alphas": [[name, float(a).hex()] for name, a in E.ALPHAS],
        "generator": "tests/golden/make_golden_scale.py",
        "reference": "source/compute.h:14-23 reduce_kernel<T>, T = float, double, HiCCL::bf16, _Float16 (clang++, built "
                     "into a temporary directory), finished by the generator's own C++; every output equals "
                     "tests/scale_expected.py scaled (NaN by NaN-ness)",
        "inputs_from": "scale_expected.hostile(kind, N): tests/hostile.py / hostile_f16.py hostile(N, 4102, shift=N, "
                       "seed=N); `inputs` holds the sha256 of each array's bytes",
        "patterns_of": "sha256 of the (11, 65536) output words of every 16-bit pattern as a single input times every "
                       "alpha, NaNs canonicalised, per kind and accumulator",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_scale.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"files": info, "patterns": hashes}, indent=1))


if __name__ == "__main__":
    main(sys.argv)
