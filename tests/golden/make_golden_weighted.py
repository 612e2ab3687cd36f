#!/usr/bin/env python3
"""Regenerate the weighted-widened-sum fixtures:
tests/golden/reduce_weighted_<kind>.npz (and .partN.npz) and
tests/golden/manifest_weighted.json.

    python tests/golden/make_golden_weighted.py

t[k] = fl32(w[k] * widen(x[k])), s32 the in-order f32 sum of the rows t[k] from
+0, r = s32 or fl32(s32 * (float)alpha), out = r or fl32(p + r)
(include/hiccl_reduce.h, hiccl_reduce_weighted).  s32 is the reference's OWN
CPU reduction in f32, reduce_kernel<float> (source/compute.h:14-23), applied to
the PRE-MULTIPLIED rows t[k], called from oracle/_ref/libhiccl_ref.so as
tests/golden/make_golden_widen.py calls it (this generator stops without it).
The rows are made by this generator's own C -- a product stored to a volatile
float, built with -ffp-contract=off into a temporary directory -- and so are
the finishing multiply and the add of the prior (make_golden_accum.py's).

Nothing is written unless the restatement (tests/weighted_expected.py, on
tests/widen_expected.py and tests/accum_expected.py) gives the same word on
every element, a NaN compared by NaN-ness -- tests/test_weighted_cpu.py pins
the restatement to the stored outputs again, without the reference.

Files and cases (read by tests/conftest.py load_golden; a key is <case>/<part>):
  reduce_weighted_bf16 / _f16 / _e4m3 / _e5m2, N in 1, 2, 3, 8, 9, 17, count 4,102
      n<N>/<set>.<alpha>       overwriting: every weight set unscaled (alpha
                               `none`), dequant and signs also under 1/3 (`third`)
      n<N>/acc.<set>.<alpha>   accumulating on accum_expected.prior(kind, N):
                               dequant, signs and extreme, unscaled and under 1/3
The inputs, the weights and the priors are not stored: they are
widen_expected.inputs(kind, N), weighted_expected.weights(set, N) and
accum_expected.prior(kind, N); the manifest holds the weights as hex floats.

Asserted here and recorded in the manifest (`conditions`):
  ones        the `ones` words equal the stored reduce_widen_<kind> n<N>/s;
  NaN cap     widen_expected.assert_nan_cap on every expected array (`shares`
              holds each case's worst share);
  fusion      dequant and signs, N >= 2: acc = fma(w, x, acc) rounded once
              differs from the contract on at least one word;
  weighted    every set but `ones` differs from the unweighted sum;
  rotation    dequant, N >= 2: the weights permuted by one place differ.
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
import accum_expected as A  # noqa: E402
import weighted_expected as X  # noqa: E402
import widen_expected as E  # noqa: E402
from make_golden_accum import build_own, own_add, own_contribution  # noqa: E402
from make_golden_ops import CLANG  # noqa: E402
from make_golden_scale import MAX_BYTES, sha, split  # noqa: E402
from make_golden_widen import load_reference  # noqa: E402

OWN = r"""
#include <stddef.h>
void premul_f32(float *out, const float *x, size_t c, float w) {
  for (size_t i = 0; i < c; i++) {
    volatile float t = w * x[i];
    out[i] = t;
  }
}
"""


def build_premul(tmp):
    so = os.path.join(tmp, "libpremul.so")
    subprocess.run([CLANG, "-x", "c", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, "-"], input=OWN,
                   text=True, check=True)
    lib = ctypes.CDLL(so)
    lib.premul_f32.restype = None
    lib.premul_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float]
    return lib


def stop(msg):
    raise SystemExit(f"make_golden_weighted: {msg} -- nothing written")


def reference_sum(ref, pre, kind, x, w):
    """reduce_kernel<float> on the pre-multiplied rows of x."""
    rows = []
    for k in range(x.shape[0]):
        wide = np.ascontiguousarray(E.widen(kind, x[k]), np.float32)
        t = np.empty_like(wide)
        pre.premul_f32(t.ctypes.data, wide.ctypes.data, wide.size, float(w[k]))
        rows.append(t)
    out = np.empty(x.shape[1], np.float32)
    tab = (ctypes.c_void_p * len(rows))(*[a.ctypes.data for a in rows])
    ref.ref_reduce_f32(out.ctypes.data, x.shape[1], tab, len(rows))
    return out


def one_case(ref, pre, own, kind, x, w, alpha, p, what):
    s = reference_sum(ref, pre, kind, x, w)
    out = own_contribution(own, s, alpha)
    if p is not None:
        out = own_add(own, p, out)
    mine = X.expected(kind, x, w, alpha, p)
    if not E.bits_equal(mine, out):
        bad = E.mismatches(mine, out)
        stop(f"{what}: the restatement differs on {len(bad)} words, first at {int(bad[0])}")
    E.assert_nan_cap(out)
    return out


def main():
    ref = load_reference()
    files, shares = [], {}
    cond = {"ones": {}, "fusion": {}, "weighted": {}, "rotation": {}}
    with tempfile.TemporaryDirectory() as tmp:
        pre, own = build_premul(tmp), build_own(tmp)
        for kind in X.KINDS:
            arrays = {}
            stored = np.load(os.path.join(HERE, f"reduce_widen_{kind}.npz"), allow_pickle=False)
            for n in X.NS:
                x, p = E.inputs(kind, n), A.prior(kind, n)
                tag = f"{kind}/n{n}"
                plain = E.widened(kind, x)
                worst_over = worst_acc = 0.0
                for name, alpha in X.OVER_CASES:
                    w = X.weights(name, n)
                    what = f"{kind} n={n} {name} alpha {X.alpha_name(alpha)}"
                    out = one_case(ref, pre, own, kind, x, w, alpha, None, what)
                    arrays[f"n{n}/{name}.{X.alpha_name(alpha)}"] = out
                    worst_over = max(worst_over, float(np.isnan(out).mean()))
                    if alpha is not None:
                        continue
                    if name == "ones":
                        assert E.bits_equal(out, stored[f"n{n}/s"]), f"{what}: not the stored widened sum's words"
                        cond["ones"][tag] = int(out.size)
                    else:
                        d = len(E.mismatches(plain, out))
                        assert d >= 1, f"{what}: the unweighted sum's words"
                        cond["weighted"][f"{tag}/{name}"] = d
                    if name in ("dequant", "signs") and n >= 2:
                        d = len(E.mismatches(X.fused(kind, x, w), out))
                        assert d >= 1, f"{what}: a fused multiply-add gives the same words"
                        cond["fusion"][f"{tag}/{name}"] = d
                    if name == "dequant" and n >= 2:
                        d = len(E.mismatches(X.weighted(kind, x, X.rotated(w)), out))
                        assert d >= 1, f"{what}: the weights permuted by one place give the same words"
                        cond["rotation"][tag] = d
                for name, alpha in X.ACCUM_CASES:
                    w = X.weights(name, n)
                    what = f"{kind} n={n} accumulating {name} alpha {X.alpha_name(alpha)}"
                    out = one_case(ref, pre, own, kind, x, w, alpha, p, what)
                    arrays[f"n{n}/acc.{name}.{X.alpha_name(alpha)}"] = out
                    worst_acc = max(worst_acc, float(np.isnan(out).mean()))
                shares[tag] = {"nan_worst_over": round(worst_over, 4), "nan_worst_accum": round(worst_acc, 4)}
            files += split(f"reduce_weighted_{kind}", arrays)
        del pre, own
    stale = [f for f in os.listdir(HERE) if f.startswith("reduce_weighted_") and f.endswith(".npz")]
    for f in stale:  # a set written again may take fewer files
        os.remove(os.path.join(HERE, f))
    info = {}
    for fname, arrs in files:
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_weighted: {fname} would be {size} bytes (limit {MAX_BYTES})")
        info[fname] = {"arrays": len(arrs), "pinned_by": "reference f32 sum of the generator's pre-multiplied rows",
                       "sha256": sha(path), "bytes": size}
    manifest = {
        "files": info,
        "shares": shares,
        "conditions": cond,
        "weights": {f"{name}/n{n}": [float(v).hex() for v in X.weights(name, n)] for name in X.WEIGHT_SETS for n in X.NS},
        "generator": "tests/golden/make_golden_weighted.py",
        "reference": "source/compute.h:14-23 reduce_kernel<float> (oracle/_ref/libhiccl_ref.so, ref_reduce_f32) on the "
                     "rows fl32(w[k] * widen(x[k])), which the generator's own C makes (a product stored to a volatile "
                     "float, -ffp-contract=off), scaled and added to the prior by make_golden_accum.py's C; every output "
                     "equals tests/weighted_expected.py (NaN by NaN-ness)",
        "inputs_from": "widen_expected.inputs(kind, N, 4102), weighted_expected.weights(set, N), "
                       "accum_expected.prior(kind, N)",
        "conditions_of": "`ones`: words equal to the stored reduce_widen_<kind> n<N>/s; words on which a wrong result "
                         "differs from the contract's: `fusion` fma(w, x, acc) rounded once, `weighted` the unweighted "
                         "sum, `rotation` the weights permuted by one place",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_weighted.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"files": info, "shares": shares}, indent=1))


if __name__ == "__main__":
    main()
