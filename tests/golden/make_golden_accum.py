#!/usr/bin/env python3
"""Regenerate the accumulating-widened-sum fixtures:
tests/golden/reduce_accum_<kind>.npz (and .partN.npz) and
tests/golden/manifest_accum.json.

    python tests/golden/make_golden_accum.py

out[i] = fl32(p + r), r = s32[i] or fl32(s32[i] * (float)alpha), p the output
before the launch (include/hiccl_reduce.h, hiccl_reduce_accumulate).  s32 is
the reference's OWN CPU reduction in f32, reduce_kernel<float>
(source/compute.h:14-23), on the widened inputs, called from
oracle/_ref/libhiccl_ref.so exactly as tests/golden/make_golden_widen.py calls
it (this generator stops without it).  The two finishing steps -- the product
and the add of the old output, each stored to a volatile float -- are this
generator's own C, built with -ffp-contract=off into a temporary directory.
The last add is pinned to the reference as well: reduce_kernel<float> over the
two rows {p, r} gives the same word wherever p is not -0 (+0 + p is p there).

Nothing is written unless the restatement (tests/accum_expected.py, on
tests/widen_expected.py) gives the same word on every element, a NaN compared by
NaN-ness -- tests/test_accum_cpu.py pins the restatement to the stored outputs
again, without the reference.

Files and cases (read by tests/conftest.py load_golden; a key is <case>/<part>):
  reduce_accum_bf16 / _f16 / _e4m3 / _e5m2
      n<N>/p      the prior, accum_expected.prior(kind, N): N in 0, 1, 2, 3, 8, 9,
                  17, count 4,102
      n<N>/a<i>   the output under accum_expected.ALPHAS[i]: i = 0 the unscaled
                  form; i = 1 (alpha 1.0) is checked against it here and in the
                  tests, not stored twice
      zero/p, zero/x, zero/a0, zero/a4
                  the hand-written zero case: p = -0 and three all--0 inputs
                  give +0 unscaled and -0 under alpha = -1/1024
The inputs are not stored: they are widen_expected.inputs(kind, N); the manifest
holds the sha256 of each input array and of each prior.

Asserted here and recorded in the manifest (`conditions`):
  NaN cap     widen_expected.assert_nan_cap on every expected array (under
              alpha = 0 not counting the NaNs that stand where the unscaled
              widened sum is infinite);
  fusion      alpha = 1/3 and 0.7, N >= 1: fma(s32, a32, p) rounded once differs
              from the contract on at least one word;
  order       unscaled, N >= 2: p folded in as addend 0 differs on at least one;
  repeat      three accumulations differ from p + 3r on at least one word.
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
import widen_expected as E  # noqa: E402
from make_golden_ops import CLANG  # noqa: E402
from make_golden_scale import MAX_BYTES, sha, split  # noqa: E402
from make_golden_widen import load_reference, reference_sum  # noqa: E402

OWN = r"""
#include <stddef.h>
void finish_f32(float *out, const float *s, size_t c, double alpha) {
  for (size_t i = 0; i < c; i++) {
    volatile float r = s[i] * (float)alpha;
    out[i] = r;
  }
}
void add_prior_f32(float *out, const float *p, const float *r, size_t c) {
  for (size_t i = 0; i < c; i++) {
    volatile float v = p[i] + r[i];
    out[i] = v;
  }
}
"""


def build_own(tmp):
    so = os.path.join(tmp, "libaccum.so")
    subprocess.run([CLANG, "-x", "c", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, "-"], input=OWN,
                   text=True, check=True)
    lib = ctypes.CDLL(so)
    lib.finish_f32.restype = None
    lib.finish_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double]
    lib.add_prior_f32.restype = None
    lib.add_prior_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def own_contribution(own, s, alpha):
    s = np.ascontiguousarray(s, np.float32)
    if alpha is None:
        return s
    out = np.empty_like(s)
    own.finish_f32(out.ctypes.data, s.ctypes.data, s.size, float(alpha))
    return out


def own_add(own, p, r):
    p, r = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(r, np.float32)
    out = np.empty_like(p)
    own.add_prior_f32(out.ctypes.data, p.ctypes.data, r.ctypes.data, p.size)
    return out


def reference_pair(ref, p, r):
    """reduce_kernel<float> over the two rows {p, r}."""
    rows = [np.ascontiguousarray(p, np.float32), np.ascontiguousarray(r, np.float32)]
    out = np.empty(rows[0].size, np.float32)
    tab = (ctypes.c_void_p * 2)(*[a.ctypes.data for a in rows])
    ref.ref_reduce_f32(out.ctypes.data, out.size, tab, 2)
    return out


def stop(msg):
    raise SystemExit(f"make_golden_accum: {msg} -- nothing written")


def one_case(ref, own, kind, x, p, alpha, what, inf_of):
    """The expected words of one case, pinned three ways."""
    s = reference_sum(ref, kind, x)
    r = own_contribution(own, s, alpha)
    out = own_add(own, p, r)
    mine = A.accumulated(kind, x, p, alpha)
    if not E.bits_equal(mine, out):
        bad = E.mismatches(mine, out)
        stop(f"{what}: the restatement differs on {len(bad)} words, first at {int(bad[0])}")
    pair = reference_pair(ref, p, r)
    keep = A.not_neg_zero(p)
    if not E.bits_equal(pair[keep], out[keep]):
        stop(f"{what}: the reference's reduce_kernel<float> over {{p, r}} differs where p is not -0")
    E.assert_nan_cap(out, inf_of)
    return out


def main():
    ref = load_reference()
    files, inputs, priors, shares = [], {}, {}, {}
    cond = {"fusion": {}, "order": {}, "repeat": {}}
    alpha_of = dict(A.ALPHAS)
    with tempfile.TemporaryDirectory() as tmp:
        own = build_own(tmp)
        for kind in A.KINDS:
            arrays = {}
            for n in A.NS:
                x, p = E.inputs(kind, n), A.prior(kind, n)
                tag = f"{kind}/n{n}"
                inputs[tag], priors[tag] = E.array_hash(x), E.array_hash(p)
                arrays[f"n{n}/p"] = p
                s = E.widened(kind, x, count=p.size)  # (pinned by make_golden_widen.py; the NaN-cap exception's sum)
                worst = 0.0
                for i, (name, alpha) in enumerate(A.ALPHAS):
                    what = f"{kind} n={n} alpha {name}"
                    out = one_case(ref, own, kind, x, p, alpha, what, s if alpha == 0.0 else None)
                    worst = max(worst, float(np.isnan(out).mean()))
                    if i == 1:
                        assert alpha == 1.0 and E.bits_equal(out, arrays[f"n{n}/a0"]), f"{what}: the unscaled words"
                    else:
                        arrays[f"n{n}/a{i}"] = out
                    if n >= 1 and name in ("third", "0.7"):
                        d = len(E.mismatches(A.fused(kind, x, p, alpha), out))
                        assert d >= 1, f"{what}: a fused multiply-add gives the same words"
                        cond["fusion"][f"{tag}/{name}"] = d
                    if n >= 2 and alpha is None:
                        d = len(E.mismatches(A.prior_first(kind, x, p), out))
                        assert d >= 1, f"{what}: the prior as addend 0 gives the same words"
                        cond["order"][tag] = d
                shares[tag] = {"nan_worst": round(worst, 4)}
            x, p = E.inputs(kind, 8), A.prior(kind, 8)
            three = A.accumulated(kind, x, p, alpha_of["third"], times=3)
            d = len(E.mismatches(A.thrice_at_once(kind, x, p, alpha_of["third"]), three))
            assert d >= 1, f"{kind}: three accumulations equal p + 3r"
            cond["repeat"][f"{kind}/n8/third"] = d
            # the zero rules, by hand
            zx, zp = A.zero_case(kind)
            arrays["zero/x"], arrays["zero/p"] = zx, zp
            for i in (0, 4):
                name, alpha = A.ALPHAS[i]
                out = one_case(ref, own, kind, zx, zp, alpha, f"{kind} zero case alpha {name}", None)
                want = 0x00000000 if alpha is None else 0x80000000
                assert alpha is None or alpha == -1.0 / 1024.0
                assert (out.view(np.uint32) == want).all(), f"{kind} zero case alpha {name}: {out.view(np.uint32)}"
                arrays[f"zero/a{i}"] = out
            files += split(f"reduce_accum_{kind}", arrays)
        del own
    stale = [f for f in os.listdir(HERE) if f.startswith("reduce_accum_") and f.endswith(".npz")]
    for f in stale:  # a set written again may take fewer files
        os.remove(os.path.join(HERE, f))
    info = {}
    for fname, arrs in files:
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        if size >= MAX_BYTES:
            os.remove(path)
            raise SystemExit(f"make_golden_accum: {fname} would be {size} bytes (limit {MAX_BYTES})")
        info[fname] = {"arrays": len(arrs), "pinned_by": "reference f32 sum + generator finish and add", "sha256": sha(path),
                       "bytes": size}
    manifest = {
        "files": info,
        "inputs": inputs,
        "priors": priors,
        "shares": shares,
        "conditions": cond,
        "alphas": [[name, None if a is None else float(a).hex()] for name, a in A.ALPHAS],
        "generator": "tests/golden/make_golden_accum.py",
        "reference": "source/compute.h:14-23 reduce_kernel<float> (oracle/_ref/libhiccl_ref.so, ref_reduce_f32) on the "
                     "widened inputs, scaled and added to the prior by the generator's own C (-ffp-contract=off); every "
                     "output equals tests/accum_expected.py accumulated (NaN by NaN-ness) and, wherever the prior is "
                     "not -0, reduce_kernel<float> over the rows {prior, contribution}",
        "inputs_from": "widen_expected.inputs(kind, N, 4102); the prior accum_expected.prior(kind, N): `inputs` and "
                       "`priors` hold the sha256 of each array's bytes, `shares` the worst NaN share of a case's outputs",
        "conditions_of": "words on which a wrong kernel's result differs from the contract's: `fusion` fma(s32, a32, p) "
                         "rounded once; `order` the prior as addend 0 of the unscaled fold; `repeat` p + 3r against "
                         "three launches",
        "numpy": np.__version__,
    }
    with open(os.path.join(HERE, "manifest_accum.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"files": info, "shares": shares, "conditions": cond}, indent=1))


if __name__ == "__main__":
    main()
