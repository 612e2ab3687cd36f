"""CPU tier: Comm<T> end to end on the host port for every element type and
operator wrapper (build/types_comm_host, tests/cpp/types_comm.cpp).

One launch per (type, topology): counts 1, 5 and 4099 per rank, all eight
collectives, and for the SUM types the ordered all-reduce.  With pipeline
stages and stripes, counts 1 and 5 leave zero-length pieces and 4099 puts
pieces of every 1- and 2-byte type at odd byte offsets.  The topologies are
those of tests/test_mpi_host.py (its known-answer rows and its all-reduce
rows).  Every rank's whole receive allocation is compared with
tests/comm_expected.py: what the collective defines bit for bit (a reduction's
NaN by NaN-ness), everything else -- non-root ranks, the buffer past `count`,
the guards -- still the 0xA5 prefill; and the ordered all-reduce against
oracle/schedule.py's simulation with the type's own add.
"""
import os
import shutil
import subprocess

import pytest

import comm_expected as CE
from conftest import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPIRUN = shutil.which("mpirun") or "/opt/conda/bin/mpirun"
HOST = os.path.join(ROOT, "build", "types_comm_host")
COUNTS = (1, 5, 4099)

pytestmark = pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")

# np, hierarchy, libs, numstripe, ringnodes, pipedepth
TOPOLOGIES = [
    (2, "2", "mpi", 1, 1, 3),
    (4, "2,2", "mpi,ipc", 1, 1, 3),
    (8, "1,4,2", "mpi,ipc,ipc", 1, 1, 3),
    (6, "3,2", "mpi,mpi", 1, 1, 3),
    (2, "2", "mpi", 1, 1, 4),
    (8, "8", "mpi", 1, 1, 1),
    (8, "2,4", "mpi,ipc", 1, 2, 2),
    (8, "2,4", "mpi,ipc", 2, 1, 2),
]


@pytest.fixture(scope="module", autouse=True)
def built():
    make(ROOT, "build/types_comm_host")


@pytest.mark.parametrize("np_,hier,libs,stripe,ring,depth", TOPOLOGIES,
                         ids=[f"np{t[0]}-{t[1]}-{t[2]}-s{t[3]}r{t[4]}d{t[5]}" for t in TOPOLOGIES])
@pytest.mark.parametrize("tname", list(CE.TYPES))
def test_every_collective(tmp_path, oracle, tname, np_, hier, libs, stripe, ring, depth):
    tokens = CE.tokens_of(tname)
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    want = CE.prepare(inp, tname, np_, COUNTS, tokens, oracle, (hier, libs, stripe, ring, depth))
    cmd = [MPIRUN, "-np", str(np_), HOST, tname, ",".join(map(str, COUNTS)), ",".join(tokens), stripe, ring, depth, hier,
           libs, inp, out]
    p = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, OMP_NUM_THREADS="1"), cwd="/tmp")
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    try:
        CE.judge(out, tname, np_, want)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)  # the allocations of 8 ranks x 27 collectives
