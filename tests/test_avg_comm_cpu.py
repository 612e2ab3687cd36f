"""CPU tier: averaging Comm<T> (Comm<T>::set_scale) end to end on the host port
(build/avg_comm_host, tests/cpp/avg_comm.cpp).

One launch per (topology, alpha): the seven element types set_scale takes,
counts 1, 5 and 4099 per rank, reduce (4), reduce-scatter (7), all-reduce (8)
and the ordered all-reduce (8o); on the ringnodes = 2 row also token `r`, a
reduce whose senders all sit on the other ring node.  The topologies are
tests/test_types_comm_cpu.py's.  Every rank's whole receive allocation is
compared with tests/avg_expected.py: what the collective defines is
finish(s, alpha) of the unscaled communicator's word s -- the multiply once per
element, in the compute that completes the sum, whatever the schedule (tree
levels, ring, stripes, pipeline stages) -- and everything else is still the
0xA5 prefill.  Alphas 0.7 (a missing and a doubled multiply both show, and so
do the halves' two roundings) and 1 / np.

Also: a scatter under set_scale and a second alpha die at init() with their
messages, and a scale cleared before add_reduce leaves the unscaled words.
"""
import os
import shutil
import subprocess

import pytest

import avg_expected as AE
from conftest import make
from test_types_comm_cpu import TOPOLOGIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPIRUN = shutil.which("mpirun") or "/opt/conda/bin/mpirun"
HOST = os.path.join(ROOT, "build", "avg_comm_host")
COUNTS = (1, 5, 4099)
TOKENS = ["4", "7", "8", AE.ORDERED]

pytestmark = pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")


@pytest.fixture(scope="module", autouse=True)
def built():
    make(ROOT, "build/avg_comm_host")


@pytest.fixture(scope="module")
def types(built):
    """The seven types; six where the host compiler has no _Float16."""
    return AE.driver_types(MPIRUN, HOST)


def run(np_, types, counts, tokens, topo, inp, out, alpha):
    hier, libs, stripe, ring, depth = topo
    cmd = [MPIRUN, "-np", np_, HOST, "+".join(types), ",".join(map(str, counts)), ",".join(tokens), stripe, ring, depth,
           hier, libs, inp, out, repr(float(alpha))]
    return subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=240,
                          env=dict(os.environ, OMP_NUM_THREADS="1"), cwd="/tmp")


@pytest.mark.parametrize("which", ["0.7", "1/np"])
@pytest.mark.parametrize("np_,hier,libs,stripe,ring,depth", TOPOLOGIES,
                         ids=[f"np{t[0]}-{t[1]}-{t[2]}-s{t[3]}r{t[4]}d{t[5]}" for t in TOPOLOGIES])
def test_scaled_collectives(tmp_path, oracle, types, np_, hier, libs, stripe, ring, depth, which):
    alpha = 0.7 if which == "0.7" else 1.0 / np_
    topo = (hier, libs, stripe, ring, depth)
    tokens = TOKENS + ([AE.RING] if ring == 2 else [])
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    want = {t: AE.prepare(inp, t, np_, COUNTS, tokens, oracle, topo, alpha) for t in types}
    p = run(np_, types, COUNTS, tokens, topo, inp, out, alpha)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "final)" in p.stdout, "Coll::report names no final compute:\n" + p.stdout[-2000:]
    try:
        for t in types:
            AE.judge(out, t, np_, want[t])
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)


def test_cleared_scale_gives_the_unscaled_words(tmp_path, oracle):
    np_, hier, libs, stripe, ring, depth = TOPOLOGIES[1]
    topo = (hier, libs, stripe, ring, depth)
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    types = ("float", "bf16", "f8e5m2")
    want = {t: AE.prepare(inp, t, np_, (5, 4099), [AE.CLEARED], oracle, topo, 0.7) for t in types}
    p = run(np_, types, (5, 4099), [AE.CLEARED], topo, inp, out, 0.7)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "final)" not in p.stdout
    for t in types:
        AE.judge(out, t, np_, want[t])


def test_scaled_scatter_dies_at_init(tmp_path, oracle):
    """A scatter is a reduction of one sender: no compute to scale in."""
    np_, hier, libs, stripe, ring, depth = TOPOLOGIES[1]
    inp = str(tmp_path / "in")
    send, _ = AE.CE.reduce_inputs("sum", "f32", np_, 5 * np_, 2)
    for r in range(np_):
        send[r].tofile(AE._file(inp, "float", 5, "2", r))
    p = run(np_, ["float"], (5,), ["2"], (hier, libs, stripe, ring, depth), inp, str(tmp_path / "out"), 0.7)
    log = p.stdout + p.stderr
    assert p.returncode != 0, log[-2000:]
    assert "scaled REDUCE #0" in log and "no compute to scale in" in log, log[-2000:]
    assert not os.path.exists(AE._file(str(tmp_path / "out"), "float", 5, "2", 0))


def test_second_alpha_dies_at_init(tmp_path, oracle):
    np_, hier, libs, stripe, ring, depth = TOPOLOGIES[0]
    inp = str(tmp_path / "in")
    send, _ = AE.CE.reduce_inputs("sum", "f64", np_, 5 * np_, 3)
    for r in range(np_):
        send[r].tofile(AE._file(inp, "double", 5, "x", r))
    p = run(np_, ["double"], (5,), ["x"], (hier, libs, stripe, ring, depth), inp, str(tmp_path / "out"), 0.7)
    log = p.stdout + p.stderr
    assert p.returncode != 0, log[-2000:]
    assert "different alphas" in log and "one alpha per communicator" in log, log[-2000:]


def test_set_scale_rejects_other_types_at_compile_time(tmp_path):
    """An integer T or an operator wrapper fails to compile with a message, as
    Compute<T>::set_scale does; the seven floating types compile (and an
    integer Comm<T> that never asks for a scale still does)."""
    from test_widen_cpu import _mpi
    inc = ["-I", os.path.join(ROOT, "include"), "-I", _mpi()[0], "-DHICCL_PORT_HOST"]
    ok = tmp_path / "ok.cpp"
    ok.write_text('#include "hiccl.h"\nusing namespace HiCCL;\n'
                  "template <class T> void g() { Comm<T> c; c.set_scale(0.5); c.clear_scale(); }\n"
                  "void f() { g<float>(); g<double>(); g<bf16>(); g<f16>(); g<f8e4m3>(); g<f8e5m2>();\n"
                  "#ifdef __FLT16_MANT_DIG__\n           g<_Float16>();\n#endif\n"
                  "           Comm<int32_t> i; i.init(); Comm<maxof<float>> m; m.init(); }\n"
                  "int main() { return 0; }\n")
    cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(ok)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    for t, why in (("int32_t", "floating element types only"), ("size_t", "floating element types only"),
                   ("maxof<float>", "only sums are scaled"), ("prodof<bf16>", "only sums are scaled")):
        bad = tmp_path / "bad.cpp"
        bad.write_text(f'#include "hiccl.h"\nusing namespace HiCCL;\nvoid f() {{ Comm<{t}> c; c.set_scale(0.5); }}\n'
                       "int main() { return 0; }\n")
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only"] + inc + [str(bad)], capture_output=True, text=True)
        assert cc.returncode != 0 and "static assertion failed" in cc.stderr and "Comm::set_scale" in cc.stderr \
            and why in cc.stderr, t + cc.stderr[-2000:]
