#!/usr/bin/env python3
"""Regenerate the widened-sum fixtures: tests/golden/reduce_widen_<kind>.npz
(and .partN.npz) and tests/golden/manifest_widen.json.

    python tests/golden/make_golden_widen.py

out[i] = s32[i], or fl32(s32[i] * (float)alpha) (include/hiccl_reduce.h,
hiccl_reduce_widened).  widen is exact, so s32 is the reference's OWN CPU
reduction in f32, reduce_kernel<float> (source/compute.h:14-23), applied to the
widened inputs: it is called from oracle/_ref/libhiccl_ref.so (ref_reduce_f32,
built by oracle/build_ref.sh where the reference is present; this generator
stops without it).  The widening handed to it is tests/widen_expected.py's
(the bf16 shift, NumPy's float16, torch's float8 conversions).  `finish` is
this generator's own C: a float product stored to a volatile float, compiled
into a temporary directory that is removed afterwards.

Nothing is written unless the restatement (tests/widen_expected.py: an explicit
in-order f32 loop, then the f32 multiply) gives the same word on every element,
a NaN compared by NaN-ness -- tests/test_widen_cpu.py pins the restatement to
the stored outputs again, without the reference.

Files and cases (read by tests/conftest.py load_golden; a key is <case>/<part>):
  reduce_widen_bf16 / _f16 / _e4m3 / _e5m2
      n<N>/s      the unscaled sum, N in 1, 2, 3, 8, 9, 17, count 4,102
      n<N>/a<i>   the scaled sum under widen_expected.ALPHAS[i], i >= 1
                  (ALPHAS[0] is 1.0: its words are checked against n<N>/s here
                  and in the tests, not stored twice)
The inputs are not stored: they are widen_expected.inputs(kind, N), and the
manifest holds the sha256 of each input array.  The every-pattern tables (every
16-bit pattern of bf16 / f16 and every byte of FP8 as input 0, against each of
16 addends as input 1) store no words either: the manifest holds the sha256 of
the reference's (16, 2^bits) output words, NaNs canonicalised, per kind.

Asserted here: at most hostile.NAN_CAP of every stored array is NaN (under
alpha = 0 not counting the NaNs that stand where the stored sum is infinite:
widen_expected.assert_nan_cap); for a finite nonzero alpha an output is NaN
exactly where the sum is, for alpha = 0 exactly where the sum is NaN or
infinite.
"""
import ctypes
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
import widen_expected as E  # noqa: E402
from make_golden_ops import CLANG  # noqa: E402
from make_golden_scale import MAX_BYTES, sha, split  # noqa: E402

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libhiccl_ref.so")

OWN = r"""
#include <stddef.h>
void finish_f32(float *out, const float *s, size_t c, double alpha) {
  for (size_t i = 0; i < c; i++) {
    volatile float p = s[i] * (float)alpha;
    out[i] = p;
  }
}
"""


def load_reference():
    if not os.path.exists(REF_SO):
        raise SystemExit(f"make_golden_widen: {REF_SO} not built (oracle/build_ref.sh needs the reference) -- "
                         "nothing written")
    ref = ctypes.CDLL(REF_SO)
    ref.ref_reduce_f32.restype = None
    ref.ref_reduce_f32.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    return ref


def build_finish(tmp):
    so = os.path.join(tmp, "libfinish.so")
    subprocess.run([CLANG, "-x", "c", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, "-"], input=OWN,
                   text=True, check=True)
    lib = ctypes.CDLL(so)
    lib.finish_f32.restype = None
    lib.finish_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double]
    return lib


def reference_sum(ref, kind, x):
    """reduce_kernel<float> on the widened rows of x."""
    rows = [np.ascontiguousarray(E.widen(kind, r), np.float32) for r in x]
    out = np.empty(x.shape[1], np.float32)
    tab = (ctypes.c_void_p * max(1, len(rows)))(*[r.ctypes.data for r in rows])
    ref.ref_reduce_f32(out.ctypes.data, x.shape[1], tab, len(rows))
    return out


def own_finish(fin, s, alpha):
    s = np.ascontiguousarray(s, np.float32)
    out = np.empty_like(s)
    fin.finish_f32(out.ctypes.data, s.ctypes.data, s.size, float(alpha))
    return out


def pinned(got, mine, what, inf_of=None):
    if not E.bits_equal(mine, got):
        bad = E.mismatches(mine, got)
        raise SystemExit(f"make_golden_widen: {what}: the restatement differs from the reference on {len(bad)} words, "
                         f"first at {int(bad[0])} -- nothing written")
    E.assert_nan_cap(got, inf_of)
    return got


def main():
    ref = load_reference()
    files, inputs, hashes, shares = [], {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        fin = build_finish(tmp)
        for kind in E.KINDS:
            arrays = {}
            for n in E.NS:
                x = E.inputs(kind, n)
                inputs[f"{kind}/n{n}"] = E.array_hash(x)
                s = pinned(reference_sum(ref, kind, x), E.widened(kind, x), f"{kind} n={n}")
                arrays[f"n{n}/s"] = s
                shares[f"{kind}/n{n}"] = {"nan": round(float(np.isnan(s).mean()), 4),
                                          "inf": round(float(np.isinf(s).mean()), 4)}
                for i, (name, alpha) in enumerate(E.ALPHAS):
                    what = f"{kind} n={n} alpha {name}"
                    y = pinned(own_finish(fin, s, alpha), E.widened(kind, x, alpha), what, s if alpha == 0.0 else None)
                    if alpha == 0.0:
                        assert np.array_equal(np.isnan(y), ~np.isfinite(s)), f"{what}: NaN exactly where s is not finite"
                    else:
                        assert np.array_equal(np.isnan(y), np.isnan(s)), f"{what}: NaN exactly where the sum is"
                    if i == 0:
                        assert alpha == 1.0 and E.bits_equal(y, s), f"{what}: alpha 1.0 gives the sum's words"
                    else:
                        arrays[f"n{n}/a{i}"] = y
            files += split(f"reduce_widen_{kind}", arrays)
        for kind in E.KINDS:
            rows = [reference_sum(ref, kind, E.pattern_inputs(kind, i)) for i in range(16)]
            got = np.stack(rows)
            if not E.bits_equal(E.patterns_expected(kind), got):
                raise SystemExit(f"make_golden_widen: {kind} every pattern: the restatement differs -- nothing written")
            hashes[kind] = E.words_hash(got)
        del fin
    stale = [f for f in os.listdir(HERE) if f.startswith("reduce_widen_") and f.endswith(".npz")]
    for f in stale:  # a set written again may take fewer files
        os.remove(os.path.join(HERE, f))
    info = {}
    for fname, arrs in files:
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_widen: {fname} would be {size} bytes (limit {MAX_BYTES})")
        info[fname] = {"arrays": len(arrs), "pinned_by": "reference f32 sum + generator finish", "sha256": sha(path),
                       "bytes": size}
    manifest = {
        "files": info,
        "inputs": inputs,
        "shares": shares,
        "patterns": hashes,
        "alphas": [[name, float(a).hex()] for name, a in E.ALPHAS],
        "generator": "tests/golden/make_golden_widen.py",
        "reference": "source/compute.h:14-23 reduce_kernel<float> (oracle/_ref/libhiccl_ref.so, ref_reduce_f32) on the "
                     "widened inputs, finished by the generator's own C; every output equals tests/widen_expected.py "
                     "widened (NaN by NaN-ness)",
        "inputs_from": "widen_expected.inputs(kind, N, 4102): hostile.hostile('bf16', N, 4102), hostile_f16.hostile(N, "
                       "4102), FP8: f8_expected.tame_bytes with hostile_bytes mixed in at 1 / (2N) per input; `inputs` "
                       "holds the sha256 of each array's bytes, `shares` the NaN / Inf share of each unscaled sum",
        "patterns_of": "sha256 of the (16, 2^bits) f32 output words of every pattern of the type as input 0 against "
                       "widen_expected.ADDENDS[kind][i] as input 1, NaNs canonicalised, per kind",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_widen.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"files": info, "patterns": hashes, "shares": shares}, indent=1))


if __name__ == "__main__":
    main()
